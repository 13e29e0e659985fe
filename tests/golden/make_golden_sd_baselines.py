"""Reference-run goldens for the SD baselines: Erased Stable Diffusion and gradient ascent.

    python tests/golden/make_golden_sd_baselines.py   ->  tests/golden/sd_baselines.npz, tests/golden/cli_sd_baselines.json

EXECUTES the reference's own functions (build container only):

    train-esd.train_esd                   (SD/train-scripts/train-esd.py:129-342)
    gradient_ascent.gradient_ascent       (SD/train-scripts/gradient_ascent.py:14-121)

on the reference's `LatentDiffusion` around its `UNetModel` at the tiny configuration (`fixtures.sd_tiny_config`,
4 x 8 x 8 latents), sampled by the reference's REAL `ldm.models.diffusion.ddim.DDIMSampler`.  The lightning / stage
stand-ins are those of make_golden_sd_glue.py.  What is replaced here is plumbing only: `get_models` (returns the two
models built here and their samplers), `dataset` / `diffusers` / `convertModels`, and `DDIMSampler.register_buffer`,
which moves every table to "cuda" (no GPU in the build container).

ESD runs with `ddim_steps = 5`, `image_size = 64` (8 x 8 latents): 3 iterations of `full` with a saliency mask, 3 of
`xattn` without, 1 of `noxattn`.  `torch.randint` is patched so that the t_enc draws are 0, S - 1, 2 (and 3 for the
single iteration): the sampler's exit rule is pinned at both ends.  The other draws are the generator's; all are
recorded.  Every run is repeated with the reference in float64 (`model.double()`, default dtype float64, `.float()`
mapped to `.double()` so that the reference's GroupNorm32 / timestep embedding stay in float64) replaying the recorded
draws.  Stored per run: draws, DDIM steps taken per iteration, z, e_0, e_p, losses, Adam moments and final weights
(strided samples + float64 sums), for both precisions; the reference's OWN fp32-vs-float64 gap per quantity
(`rel_max`: max |a - b| / max |b|) and 4x that gap as the device's bound.  For iteration 0 of the first run the chain
itself: x, the batched eps, x_prev of every step.  Also the DDIM tables, and for each `train_method` the indices of
the parameters the reference hands to its optimizer (an empty selection makes torch.optim.Adam raise: recorded as
empty).  GA: 2 epochs, masked and unmasked, the same recordings.  Data only, no reference source.
"""
from __future__ import annotations

import ast
import importlib.util
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
from fixtures import fill_params, sd_glue_batches, sd_glue_contexts, sd_tiny_config, SD_GLUE_PROMPTS  # noqa: E402
from make_golden import _stub  # noqa: E402
from make_golden_sd_glue import REF_SD, _stub_lightning_and_stages  # noqa: E402
from unlearn_saliency_amd import rng  # noqa: E402

sys.dont_write_bytecode = True
torch.set_num_threads(8)
STRIDE = 499      # strided samples of N-sized vectors kept in the fixture
S = 5             # ddim_steps
LR = 1e-4
PROMPT, SEP = ", ".join(SD_GLUE_PROMPTS[:2]), ","
ESD_RUNS = (("esd_full_mask", "full", True, (0, S - 1, 2)), ("esd_xattn", "xattn", False, (0, S - 1, 2)),
            ("esd_noxattn", "noxattn", False, (3,)))
METHODS = ("noxattn", "selfattn", "xattn", "full", "notime", "xlayer", "selflayer")
DESCRIPTIONS = [f"class {i}" for i in range(10)]


def rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def build_ldm(double=False):
    _stub_lightning_and_stages()
    from ldm.models.diffusion.ddpm import LatentDiffusion
    model = LatentDiffusion(
        first_stage_config={"target": "salun_golden_stages.LatentsAsImages"},
        cond_stage_config={"target": "salun_golden_stages.PromptTable"},
        unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": sd_tiny_config()},
        conditioning_key="crossattn", cond_stage_key="txt", first_stage_key="jpg", cond_stage_trainable=False,
        scale_factor=1.0, timesteps=1000, linear_start=0.00085, linear_end=0.0120, image_size=8, channels=4,
        use_ema=False, monitor=None)
    fill_params(model.model.diffusion_model, 9000)
    ctx = model.cond_stage_model.contexts
    base = ctx[SD_GLUE_PROMPTS[0]]
    ctx.update({d: base + 0.01 * i for i, d in enumerate(DESCRIPTIONS)})
    if double:
        model = model.double()
        model.model.diffusion_model.dtype = torch.float64
        for k in list(ctx):
            ctx[k] = ctx[k].double()
    return model


def import_scripts():
    _stub("omegaconf")
    _stub("omegaconf.listconfig")
    sys.modules["omegaconf.listconfig"].ListConfig = type("ListConfig", (), {})
    for m in ("diffusers", "convertModels", "dataset", "torchvision", "torchvision.utils", "ldm.models.diffusion.ddim"):
        sys.modules.pop(m, None)
    sys.path.insert(0, REF_SD)
    df = types.ModuleType("diffusers")
    df.LMSDiscreteScheduler = lambda **k: None
    sys.modules["diffusers"] = df
    cm = types.ModuleType("convertModels")
    cm.savemodelDiffusers = lambda *a, **k: None
    sys.modules["convertModels"] = cm
    tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tvu = types.ModuleType("torchvision.utils")
    tvu.make_grid = lambda *a, **k: None
    tv.transforms, tv.utils = tvt, tvu
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.utils": tvu})
    ds = types.ModuleType("dataset")
    for name in ("setup_model", "setup_forget_data", "setup_remain_data"):
        setattr(ds, name, None)
    sys.modules["dataset"] = ds
    import matplotlib
    matplotlib.use("Agg")
    from ldm.models.diffusion.ddim import DDIMSampler   # the real one
    DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)   # the reference's moves to "cuda"
    mods = {}
    for name in ("train-esd", "gradient_ascent"):
        sp = importlib.util.spec_from_file_location("ref_sd_" + name.replace("-", "_"), f"{REF_SD}/train-scripts/{name}.py")
        m = importlib.util.module_from_spec(sp)
        sp.loader.exec_module(m)
        if hasattr(m, "sleep"):
            m.sleep = lambda s: None
        mods[name] = m
    return mods, DDIMSampler


class Patches:
    """Patch / restore a list of (object, attribute, replacement)."""

    def __init__(self, items):
        self.items = items

    def __enter__(self):
        self.saved = [(o, a, getattr(o, a)) for o, a, _ in self.items]
        for o, a, v in self.items:
            setattr(o, a, v)
        return self

    def __exit__(self, *exc):
        for o, a, v in reversed(self.saved):
            setattr(o, a, v)


def adam_state(opt, unet, dtype):
    n = sum(p.numel() for p in unet.parameters())
    m1, m2 = np.zeros(n, dtype), np.zeros(n, dtype)
    off = 0
    for p in unet.parameters():
        st = opt.state.get(p)
        if st:
            m1[off:off + p.numel()] = st["exp_avg"].reshape(-1).numpy()
            m2[off:off + p.numel()] = st["exp_avg_sq"].reshape(-1).numpy()
        off += p.numel()
    return m1, m2


def flat(unet):
    return torch.cat([p.detach().reshape(-1) for p in unet.parameters()]).numpy()


def store_state(out, tag, opt, unet, dtype):
    m1, m2 = adam_state(opt, unet, dtype)
    for name, v in (("exp_avg", m1), ("exp_avg_sq", m2), ("weights", flat(unet))):
        out[f"{tag}__{name}_s"] = v[::STRIDE].copy()
        out[f"{tag}__{name}_sum"] = np.float64(v.astype(np.float64).sum())


def float64_mode():
    """The reference's code casts to float32 by name in three places (GroupNorm32, the timestep embedding, softmax):
    under this context `.float()` keeps float64 and new tensors default to float64."""
    class Ctx:
        def __enter__(self):
            self.p = Patches([(torch.Tensor, "float", lambda t: t.double())]).__enter__()
            torch.set_default_dtype(torch.float64)

        def __exit__(self, *exc):
            torch.set_default_dtype(torch.float32)
            self.p.__exit__()
    return Ctx()


# ---------------------------------------------------------------------------------------------- ESD
def run_esd(E, DDIMSampler, method, mask_file, t_encs, replay=None, chain=None):
    """One execution of the reference's train_esd.  `replay` None: fp32, draws taken and recorded; else float64 on the
    recorded draws.  Returns the record."""
    double = replay is not None
    model, model_orig = build_ldm(double), build_ldm(double)
    rec = dict(words=[], randint=[], start=[], steps=[], z=[], e_0=[], e_p=[], losses=[], opt=[])
    real_randint, real_randn, real_sample, real_adam = torch.randint, torch.randn, random.sample, torch.optim.Adam
    dt = torch.float64 if double else torch.float32

    def randint(*a, **k):
        i = len(rec["randint"])
        if double:
            v = torch.tensor([int(replay["randint"][i])])
        elif i % 2 == 0:
            v = torch.tensor([int(t_encs[i // 2])])          # t_enc: forced
        else:
            v = real_randint(*a, **{kk: vv for kk, vv in k.items() if kk != "device"})
        rec["randint"].append(int(v))
        return v

    def randn(*a, **k):
        if "device" in k:                                     # the sampler's noise_like: multiplied by sigma = 0
            return real_randn(*a, **k)
        v = torch.from_numpy(replay["start"][len(rec["start"])]).to(dt) if double else real_randn(*a, **k)
        rec["start"].append(v.numpy().astype(np.float32))
        return v

    def sample(pop, k):
        w = [replay["words"][len(rec["words"])]] if double else real_sample(pop, k)
        rec["words"].append(w[0])
        return w

    class Adam(real_adam):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            rec["opt"].append(self)

    real_p = DDIMSampler.p_sample_ddim
    real_sampling = DDIMSampler.ddim_sampling

    def p_sample_ddim(self, x, c, t, index, **k):
        outs = real_p(self, x, c, t, index, **k)
        rec["steps"][-1] += 1
        if chain is not None and len(rec["steps"]) == 1 and not double:
            chain["x"].append(x.numpy().copy())
            chain["x_prev"].append(outs[0].numpy().copy())
            chain["index"].append(index)
        return outs

    def ddim_sampling(self, *a, **k):
        rec["steps"].append(0)
        return real_sampling(self, *a, **k)

    real_apply = type(model).apply_model

    def apply_model(self, x, t, c, *a, **k):
        o = real_apply(self, x, t, c, *a, **k)
        if self is model_orig:
            key = "e_0" if len(rec["e_0"]) == len(rec["e_p"]) else "e_p"
            rec[key].append(o.detach().numpy().copy())
            if key == "e_0":
                rec["z"].append(x.detach().numpy().copy())
        elif chain is not None and len(rec["steps"]) == 1 and not double and not torch.is_grad_enabled():
            chain["eps2"].append(o.detach().numpy().copy())
        return o

    real_mse = torch.nn.MSELoss.forward

    def mse(self, a, b):
        o = real_mse(self, a, b)
        rec["losses"].append(float(o.detach()))
        return o

    E.get_models = lambda *a, **k: (model_orig, DDIMSampler(model_orig), model, DDIMSampler(model))
    patches = [(torch, "randint", randint), (torch, "randn", randn), (random, "sample", sample),
               (torch.optim, "Adam", Adam), (DDIMSampler, "p_sample_ddim", p_sample_ddim),
               (DDIMSampler, "ddim_sampling", ddim_sampling), (type(model), "apply_model", apply_model),
               (torch.nn.MSELoss, "forward", mse)]
    torch.manual_seed(51)
    random.seed(52)
    with Patches(patches):
        run = lambda: E.train_esd(PROMPT, method, 3.0, 1.0, len(t_encs), LR, None, None, mask_file, None,
                                  ["cpu", "cpu"], seperator=SEP, image_size=64, ddim_steps=S)
        if double:
            with float64_mode():
                run()
        else:
            run()
    rec["model"], rec["sampler_tables"] = model, None
    return rec


def esd_selection(E, DDIMSampler, method, names):
    """The parameters the reference hands to its optimizer under `method`: train_esd with zero iterations."""
    model = build_ldm()
    E.get_models = lambda *a, **k: (model, None, model, None)
    got = []
    real_adam = torch.optim.Adam

    class Adam(real_adam):
        def __init__(self, params, *a, **k):
            params = list(params)
            got.append(params)
            super().__init__(params, *a, **k)

    with Patches([(torch.optim, "Adam", Adam)]):
        try:
            E.train_esd("x", method, 3.0, 1.0, 0, LR, None, None, None, None, ["cpu", "cpu"], image_size=64, ddim_steps=S)
        except ValueError as e:   # "optimizer got an empty parameter list"
            assert "empty parameter list" in str(e), e
    ids = {id(p): i for i, (_, p) in enumerate(model.model.diffusion_model.named_parameters())}
    return np.array(sorted(ids[id(p)] for p in got[0]), np.int64)


# ---------------------------------------------------------------------------------------------- GA
def run_ga(G, mask_file, fdl, rdl, replay=None):
    double = replay is not None
    model = build_ldm(double)
    rec = dict(randint=[], randn=[], losses=[], opt=[])
    real_randint, real_randn_like, real_adam = torch.randint, torch.randn_like, torch.optim.Adam

    def randint(*a, **k):
        v = torch.from_numpy(replay["randint"][len(rec["randint"])]) if double else real_randint(*a, **k)
        rec["randint"].append(v.numpy().copy())
        return v

    def randn_like(x, **k):
        v = torch.from_numpy(replay["randn"][len(rec["randn"])]).to(x.dtype) if double else real_randn_like(x, **k)
        rec["randn"].append(v.numpy().astype(np.float32))
        return v

    class Adam(real_adam):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            rec["opt"].append(self)

    real_item = torch.Tensor.item

    def item(self):
        v = real_item(self)
        if self.requires_grad:
            rec["losses"].append(v)
        return v

    G.setup_model = lambda *a, **k: model
    G.setup_remain_data = lambda c, bs, size: (rdl, DESCRIPTIONS)
    G.setup_forget_data = lambda c, bs, size: (fdl, DESCRIPTIONS)
    torch.manual_seed(61)
    ended = ""
    with Patches([(torch, "randint", randint), (torch, "randn_like", randn_like), (torch.optim, "Adam", Adam),
                  (torch.Tensor, "item", item)]):
        def run():
            G.gradient_ascent(3, "full", 0.5, 4, 2, LR, None, None, mask_file, None, "cpu", image_size=8)
        try:
            if double:
                with float64_mode():
                    run()
            else:
                run()
        except NameError as e:   # gradient_ascent.py:121 `save_history(losses, name, classes)`: undefined name, raised
            ended = repr(e)      # after training and after the model was saved
    rec["losses"] = rec["losses"][0::2]   # raw loss.item(): called twice per step (:96, :107)
    rec["model"], rec["ended"] = model, ended
    return rec


def flags_of(path):
    tree = ast.parse(open(path).read())
    table = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument" and node.args:
            name = ast.literal_eval(node.args[0])
            kw = {}
            for k in node.keywords:
                if k.arg in ("default", "required"):
                    kw[k.arg] = ast.literal_eval(k.value)
                elif k.arg == "type":
                    kw["type"] = getattr(k.value, "id", None)
            table[name.lstrip("-")] = kw
    return table


def main():
    with open(os.path.join(HERE, "cli_sd_baselines.json"), "w") as f:
        json.dump({"sd": {nm: flags_of(f"{REF_SD}/train-scripts/{nm}.py") for nm in ("train-esd", "gradient_ascent")}},
                  f, indent=1, sort_keys=True)
    mods, DDIMSampler = import_scripts()
    E, G = mods["train-esd"], mods["gradient_ascent"]
    out = {}
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp())
    try:
        model = build_ldm()
        unet = model.model.diffusion_model
        names = [n for n, _ in unet.named_parameters()]
        n = sum(p.numel() for p in unet.parameters())
        out["param_names"], out["n_params"], out["stride"] = np.array(names), np.int64(n), np.int64(STRIDE)
        out["ddim_steps"], out["lr"] = np.int64(S), np.float64(LR)
        out["prompt"], out["seperator"] = np.array(PROMPT), np.array(SEP)
        # the saliency mask of the masked runs: the low bit of the counter-based byte stream
        bits = (rng.u8(n, 77) & 1).astype(np.uint8)
        out["mask_seed"] = np.int64(77)      # (the bits themselves are regenerated by the tests: rng.u8(n, 77) & 1)
        off, mask = 0, {}
        for name, p in unet.named_parameters():
            mask[name] = torch.from_numpy(bits[off:off + p.numel()].astype(np.int64)).view_as(p)
            off += p.numel()
        torch.save(mask, "mask.pt")
        # the DDIM tables of the reference's sampler
        smp = DDIMSampler(model)
        smp.make_schedule(ddim_num_steps=S, ddim_eta=0.0, verbose=False)
        out["ddim_timesteps"] = np.asarray(smp.ddim_timesteps, np.int64)
        out["ddim_alphas"] = np.asarray(smp.ddim_alphas, np.float32)
        out["ddim_alphas_prev"] = np.asarray(smp.ddim_alphas_prev, np.float64)
        out["ddim_sigmas"] = np.asarray(smp.ddim_sigmas, np.float64)
        out["ddim_sqrt_one_minus_alphas"] = np.asarray(smp.ddim_sqrt_one_minus_alphas, np.float32)
        out["alphas_cumprod"] = model.alphas_cumprod.numpy().astype(np.float32)
        for method in METHODS:
            out[f"esd_selected__{method}"] = esd_selection(E, DDIMSampler, method, names)
            print("selection", method, len(out[f"esd_selected__{method}"]), "of", len(names))

        for tag, method, masked, t_encs in ESD_RUNS:
            chain = dict(x=[], eps2=[], x_prev=[], index=[]) if tag == ESD_RUNS[0][0] else None
            r32 = run_esd(E, DDIMSampler, method, "mask.pt" if masked else None, t_encs, chain=chain)
            r64 = run_esd(E, DDIMSampler, method, "mask.pt" if masked else None, t_encs, replay=r32)
            assert r32["steps"] == r64["steps"] and r32["randint"] == r64["randint"], (r32["steps"], r64["steps"])
            out[f"{tag}__words"] = np.array(r32["words"])
            out[f"{tag}__randint"] = np.array(r32["randint"], np.int64)
            out[f"{tag}__start"] = np.stack(r32["start"]).astype(np.float32)
            out[f"{tag}__steps"] = np.array(r32["steps"], np.int64)
            for sfx, r, dt in (("", r32, np.float32), ("__f64", r64, np.float64)):
                out[f"{tag}__losses{sfx}"] = np.array(r["losses"], np.float64)
                for q in ("z", "e_0", "e_p"):
                    out[f"{tag}__{q}{sfx}"] = np.stack(r[q]).astype(dt)
                store_state(out, tag + sfx.replace("__f64", "_f64"), r["opt"][-1], r["model"].model.diffusion_model, dt)
            for q in ("losses", "z", "e_0", "e_p"):
                gap = rel_max(out[f"{tag}__{q}"], out[f"{tag}__{q}__f64"])
                out[f"{tag}__gap_{q}"], out[f"{tag}__bound_{q}"] = np.float64(gap), np.float64(4 * gap)
            for q in ("exp_avg", "exp_avg_sq", "weights"):
                gap = rel_max(out[f"{tag}__{q}_s"], out[f"{tag}_f64__{q}_s"])
                out[f"{tag}__gap_{q}"], out[f"{tag}__bound_{q}"] = np.float64(gap), np.float64(4 * gap)
            if chain is not None:
                out["chain__x"], out["chain__eps2"] = np.stack(chain["x"]), np.stack(chain["eps2"])
                out["chain__x_prev"], out["chain__index"] = np.stack(chain["x_prev"]), np.array(chain["index"], np.int64)
            print(tag, "t_enc/t", r32["randint"], "steps", r32["steps"], "losses", r32["losses"], "f64", r64["losses"])
            print("   gaps", {q: float(out[f"{tag}__gap_{q}"]) for q in
                              ("losses", "z", "e_0", "e_p", "exp_avg", "exp_avg_sq", "weights")})

        _, _, forget, remain = sd_glue_batches()
        fdl = [(z, torch.tensor([3] * z.shape[0])) for z in forget]
        rdl = [(z, torch.tensor([(5 + i) % 10 if (5 + i) % 10 != 3 else 4 for i in range(z.shape[0])])) for z in remain]
        out["ga__remain_labels"] = np.stack([l.numpy() for _, l in rdl])
        for tag, masked in (("ga_masked", True), ("ga_unmasked", False)):
            r32 = run_ga(G, "mask.pt" if masked else None, fdl, rdl)
            r64 = run_ga(G, "mask.pt" if masked else None, fdl, rdl, replay=r32)
            out[f"{tag}__randint"] = np.stack(r32["randint"]).astype(np.int64)
            out[f"{tag}__randn"] = np.stack(r32["randn"]).astype(np.float32)
            out[f"{tag}__ended_with"] = np.array(r32["ended"])
            for sfx, r, dt in (("", r32, np.float32), ("__f64", r64, np.float64)):
                out[f"{tag}__losses{sfx}"] = np.array(r["losses"], np.float64) / 4   # as appended: loss.item() / batch_size
                store_state(out, tag + sfx.replace("__f64", "_f64"), r["opt"][-1], r["model"].model.diffusion_model, dt)
            gap = rel_max(out[f"{tag}__losses"], out[f"{tag}__losses__f64"])
            out[f"{tag}__gap_losses"], out[f"{tag}__bound_losses"] = np.float64(gap), np.float64(4 * gap)
            for q in ("exp_avg", "exp_avg_sq", "weights"):
                gap = rel_max(out[f"{tag}__{q}_s"], out[f"{tag}_f64__{q}_s"])
                out[f"{tag}__gap_{q}"], out[f"{tag}__bound_{q}"] = np.float64(gap), np.float64(4 * gap)
            print(tag, "losses", out[f"{tag}__losses"], "ended:", r32["ended"])
            print("   gaps", {q: float(out[f"{tag}__gap_{q}"]) for q in ("losses", "exp_avg", "exp_avg_sq", "weights")})
    finally:
        os.chdir(cwd)
    path = os.path.join(HERE, "sd_baselines.npz")
    np.savez_compressed(path, **out)
    print("wrote sd_baselines.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
