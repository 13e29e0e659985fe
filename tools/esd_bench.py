"""Time per ESD iteration (SD/train_scripts.train_esd) on the full-size SD v1 U-Net (random weights) at a FIXED t_enc,
split into its four parts — the guided DDIM chain on the trained model, the batched frozen pass, the differentiated
trained pass (forward + loss + backward), the optimizer step — and the chain's time per DDIM step with the fused K21
step (`salun_ldm_ddim_step`) against the same step written as the reference's torch expression (chunk, four torch.full,
the elementwise operations, the sigma = 0 noise draw), alternated in ONE process.  Prints one JSON line.

    python tools/esd_bench.py [--ddim_steps 50] [--t_enc 25] [--reps 5] [--bf16] [--tiny]

The parts are separated by device synchronisations, so their sum is an upper bound of an unsplit iteration, which is
timed as well (`iteration_ms`).  `step_only_us`: the step alone on a resident eps, 200 calls per timing, host-side
launch cost included (that is what the step costs between two U-Net passes).
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_step(x, eps2, scale, smp, index):
    """p_sample_ddim's tensor expression (ldm/models/diffusion/ddim.py:326-372), operation for operation."""
    import torch
    b, device = x.shape[0], x.device
    e_t_uncond, e_t = eps2.chunk(2)
    e_t = e_t_uncond + scale * (e_t - e_t_uncond)
    a_t = torch.full((b, 1, 1, 1), float(smp.ddim_alphas[index]), device=device)
    a_prev = torch.full((b, 1, 1, 1), float(smp.ddim_alphas_prev[index]), device=device)
    sigma_t = torch.full((b, 1, 1, 1), float(smp.ddim_sigmas[index]), device=device)
    sqrt_one_minus_at = torch.full((b, 1, 1, 1), float(smp.ddim_sqrt_one_minus_alphas[index]), device=device)
    pred_x0 = (x - sqrt_one_minus_at * e_t) / a_t.sqrt()
    dir_xt = (1.0 - a_prev - sigma_t ** 2).sqrt() * e_t
    noise = sigma_t * torch.randn(x.shape, device=device) * 1.0
    return a_prev.sqrt() * pred_x0 + dir_xt + noise


def chain_torch(smp, cond, uncond, scale, x_T, till):
    import torch
    total = smp.ddim_timesteps[:-1].shape[0]
    ts = smp._timestep_rows(2 * x_T.shape[0], x_T.device)
    c_in = torch.cat([uncond, cond])
    x = x_T
    with torch.no_grad():
        for i in range(total):
            index = total - i - 1
            eps2 = smp.model.apply_model(torch.cat([x] * 2), ts[i], c_in)
            x = torch_step(x, eps2, scale, smp, index)
            if index + 1 == till:
                break
    return x


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--ddim_steps", type=int, default=50)
    ap.add_argument("--t_enc", type=int, default=25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--tiny", action="store_true", help="a small U-Net (checks the tool, measures nothing of interest)")
    a = ap.parse_args()
    import torch
    from unlearn_saliency_amd import ops, ops_sampler
    from unlearn_saliency_amd.optim import FusedMaskedAdam
    from unlearn_saliency_amd.SD import train_scripts as TS
    from unlearn_saliency_amd.SD.ddim import DDIMSampler
    from unlearn_saliency_amd.SD.ldm_lite import LatentDiffusionLite
    from unlearn_saliency_amd.SD.unet import V1_UNET_CONFIG
    torch.manual_seed(0)
    cfg = dict(V1_UNET_CONFIG)
    if a.tiny:
        cfg.update(image_size=8, model_channels=32, attention_resolutions=(2, 1), num_res_blocks=1, channel_mult=(1, 2),
                   num_heads=4, context_dim=24)
    hw = 8 if a.tiny else 64
    model = LatentDiffusionLite(cfg, bf16=a.bf16).cuda()
    model.use_mfma_convs()
    model.fill_zero_initialised()
    frozen = model.frozen_copy()
    arena = TS._unet_arena(model)
    opt = FusedMaskedAdam(arena, lr=1e-5)
    smp = DDIMSampler(model).make_schedule(a.ddim_steps, 0.0)
    ctx = cfg["context_dim"]
    emb_0, emb_p = torch.randn(1, 77, ctx, device="cuda"), torch.randn(1, 77, ctx, device="cuda")
    x_T = torch.randn(1, 4, hw, hw, device="cuda")
    t = torch.tensor([round((a.t_enc + 0.5) / a.ddim_steps * 1000)], device="cuda")
    model.train()
    sync = torch.cuda.synchronize

    def chain():
        return smp.sample(emb_p, emb_0, 3.0, x_T, till_T=a.t_enc)

    def frozen_pass(z):
        with torch.no_grad():
            return frozen.apply_model(torch.cat([z, z]), torch.cat([t, t]), torch.cat([emb_0, emb_p]))

    def trained_pass(z, e_0p):
        opt.zero_grad()
        ops.esd_loss(model.apply_model(z, t, emb_p), e_0p, 1.0).backward()

    def timed(fn, *args):
        sync()
        t0 = time.perf_counter()
        r = fn(*args)
        sync()
        return r, (time.perf_counter() - t0) * 1e3

    def iteration():
        z = chain()
        trained_pass(z, frozen_pass(z))
        opt.step()

    for _ in range(2):   # warm-up: kernel selection, workspaces, weight images
        iteration()
        chain_torch(smp, emb_p, emb_0, 3.0, x_T, a.t_enc)
    steps = smp.last_steps
    parts = {k: [] for k in ("chain_ms", "chain_torch_step_ms", "frozen_pass_ms", "trained_pass_ms", "optimizer_ms",
                             "iteration_ms")}
    for _ in range(a.reps):
        z, ms = timed(chain)
        parts["chain_ms"].append(ms)
        _, ms = timed(chain_torch, smp, emb_p, emb_0, 3.0, x_T, a.t_enc)
        parts["chain_torch_step_ms"].append(ms)
        e_0p, ms = timed(frozen_pass, z)
        parts["frozen_pass_ms"].append(ms)
        _, ms = timed(trained_pass, z, e_0p)
        parts["trained_pass_ms"].append(ms)
        _, ms = timed(opt.step)
        parts["optimizer_ms"].append(ms)
        _, ms = timed(iteration)
        parts["iteration_ms"].append(ms)
    # the step alone, on a resident eps
    eps2 = torch.randn(2, 4, hw, hw, device="cuda")
    coef = smp.coefficients(3)
    only = {"fused": [], "torch": []}
    with torch.no_grad():
        for _ in range(a.reps + 1):
            for k, fn in (("fused", lambda: ops_sampler.ldm_ddim_step(x_T, eps2, 3.0, *coef)),
                          ("torch", lambda: torch_step(x_T, eps2, 3.0, smp, 3))):
                sync()
                t0 = time.perf_counter()
                for _ in range(200):
                    fn()
                sync()
                only[k].append((time.perf_counter() - t0) / 200 * 1e6)
    med = lambda v: round(statistics.median(v), 3)
    out = {"workload": "sd_esd_iteration", "unet": "tiny" if a.tiny else "v1", "bf16": a.bf16, "ddim_steps": a.ddim_steps,
           "t_enc": a.t_enc, "chain_steps": steps, "reps": a.reps}
    for k, v in parts.items():
        out[k] = {"median": med(v), "min": round(min(v), 3), "max": round(max(v), 3)}
    out["chain_ms_per_step_fused"] = round(out["chain_ms"]["median"] / steps, 3)
    out["chain_ms_per_step_torch"] = round(out["chain_torch_step_ms"]["median"] / steps, 3)
    out["step_only_us"] = {k: {"median": med(v[1:]), "min": round(min(v[1:]), 3), "max": round(max(v[1:]), 3)}
                           for k, v in only.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
