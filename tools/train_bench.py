"""Training from scratch (`train.py --mode train`): the parameter tail and the whole step, on one GPU.

  tail   at N_D = 38,632,323 (the CFG-DDPM U-Net): (a) `salun_masked_adam_step` followed by `shadow.lerp_(p, 1 - mu)` —
         what a step ran before K20, 28 + 12 = 40 B / element in two launches — against (b) `salun_adam_ema_step`,
         36 B / element in one.  HIP events around `--group` back-to-back calls, (a) and (b) alternated in ONE process,
         median and range over `--reps`; achieved bytes/s are the algorithmic bytes over that time, against the 8 TB/s
         of MI355X_MICROARCH.md.
  step   steps/s of `Diffusion.train_step` at the config's batch (cifar10_train.yml: 128) on the synthetic set, the EMA
         folded into the Adam launch (`attach_ema`, what `--mode train` runs) and on `EMAHelper.update`'s own pass,
         alternated in blocks of `--steps`.

    python tools/train_bench.py [--reps 21] [--group 10] [--steps 10] [--blocks 3] [--batch 128] [--skip-step]

Prints one JSON line."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_D = 38_632_323
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec


def tail(a):
    import torch
    from unlearn_saliency_amd import ops
    n = a.n
    p, g = ops.fill_normal(n, 1, 0.0, 0.05), ops.fill_normal(n, 2, 0.0, 1e-3)
    m1, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    shadow = p.clone()
    sq = ops.grad_sqnorm(g)
    mu, hp = 0.9999, (2e-4, 0.9, 0.999, 1e-8, 0.0)
    step = [0]

    def two_pass():
        step[0] += 1
        ops.masked_adam_step(p, g, m1, v, None, *hp, step[0], sqnorm=sq, max_norm=1.0)
        shadow.lerp_(p, 1.0 - mu)

    def fused():
        step[0] += 1
        ops.adam_ema_step(p, g, m1, v, shadow, None, *hp, mu, step[0], sqnorm=sq, max_norm=1.0)

    run = {"adam_then_lerp": (two_pass, 40), "adam_ema_k20": (fused, 36)}
    for fn, _ in run.values():  # warm-up: code objects, clocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(a.reps):
        for k, (fn, _) in run.items():  # alternated: both see the same clocks and the same neighbours
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.group):
                fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) * 1e-3 / a.group)
    out = {"n": n, "reps": a.reps, "calls_per_rep": a.group}
    for k, (_, bpe) in run.items():
        ts = sorted(times[k])
        med = statistics.median(ts)
        gbs = bpe * n / med / 1e9
        out[k] = {"us_median": round(med * 1e6, 1), "us_min": round(ts[0] * 1e6, 1), "us_max": round(ts[-1] * 1e6, 1),
                  "alg_bytes_per_elem": bpe, "GBps": round(gbs, 1), "frac_of_8TBps": round(gbs / HBM_PEAK_GBS, 3)}
    out["k20_over_two_pass"] = round(out["adam_ema_k20"]["us_median"] / out["adam_then_lerp"]["us_median"], 4)
    out["expected_from_bytes"] = 0.9
    return out


def step(a):
    import torch
    from types import SimpleNamespace
    from unlearn_saliency_amd.DDPM.datasets import get_dataset
    from unlearn_saliency_amd.DDPM.functions import cycle, get_optimizer, load_config
    from unlearn_saliency_amd.DDPM.models.diffusion import Conditional_Model
    from unlearn_saliency_amd.DDPM.runners.diffusion import Diffusion
    from unlearn_saliency_amd.conv import use_salun_convs
    from unlearn_saliency_amd.flat import arena_of
    cfg = load_config(os.path.join(ROOT, "unlearn_saliency_amd", "DDPM", "configs", "cifar10_train.yml"))
    if a.batch:
        cfg.training.batch_size = a.batch
    args = SimpleNamespace(synthetic=True, label_to_forget=0, cond_scale=2.0, library_conv=False)
    torch.manual_seed(0)
    r = Diffusion(args, cfg)
    loader = get_dataset(args, cfg, device=r.device, synthetic=True)
    it = cycle(loader)
    model = Conditional_Model(cfg).to(r.device)
    use_salun_convs(model)
    opt = get_optimizer(cfg, arena=arena_of(model))
    ema = r._ema(model)
    model.train()

    def block(folded):
        if folded:
            assert ema.attach_to(opt, model)
        else:
            opt.detach_ema()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            r.train_step(model, opt, next(it), loader)
            ema.update(model)
        torch.cuda.synchronize()
        return a.steps / (time.perf_counter() - t0)

    for folded in (True, False):  # warm-up of both paths
        block(folded)
    rates = {True: [], False: []}
    for _ in range(a.blocks):
        for folded in (True, False):
            rates[folded].append(block(folded))
    fmt = lambda xs: {"steps_per_s_median": round(statistics.median(xs), 3), "steps_per_s_min": round(min(xs), 3),
                      "steps_per_s_max": round(max(xs), 3)}
    return {"batch": cfg.training.batch_size, "steps_per_block": a.steps, "blocks": a.blocks,
            "ema_folded": fmt(rates[True]), "ema_own_pass": fmt(rates[False])}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--n", type=int, default=N_D)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--group", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--steps", type=int, default=10, help="training steps per timed block")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None, help="default: the config's training.batch_size")
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("train_bench needs a ROCm device: a timing taken anywhere else says nothing")
    out = {"workload": "ddpm_train", "tail": tail(a)}
    if not a.skip_step:
        out["train_step"] = step(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
