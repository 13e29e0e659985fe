"""Golden vectors for the STL-10 diffusion runs: calls the REFERENCE's DDPM code (the checkout make_golden_ddpm.py
imports from, build container only) on the inputs of tests/stl10_fixture.py.  Written after make_golden_ddpm.py.

ddpm_stl10.npz holds
  state_names / state_shapes   `state_dict()` of the reference's Conditional_Model under each of its STL-10 configs
                               (they share one model block) — what every shipped stl10_*.yml must build;
  fwd_test_s2                  the reduced U-Net's `mode="test"`, cond_scale 2 forward;
  rl_* / train_*               one `saliency_unlearn` step (method rl, no mask, alpha 1e-3) and one `train` step of the
                               reference's runner: the step's loss and the per-tensor sums after it;
  e32_*                        how far the reference's own fp32 run is from its fp64 run on the same inputs, over the
                               scale of the quantity (max |fp32 - fp64| / max |fp64|; for the loss, relative) — the
                               yardstick of the device test's bounds.
Every golden is the fp64 run.  The draws are not recorded: both runs and the test take them from stl10_fixture (the
i-th randn_like / randint / label-drop call gets the i-th draw); the counts of each run are stored.

    python tests/golden/make_golden_ddpm_stl10.py
"""
from __future__ import annotations

import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ddpm as MD  # noqa: E402
import stl10_fixture as SF  # noqa: E402
from fixtures import fill_params  # noqa: E402
from unlearn_saliency_amd.DDPM.functions import dict2namespace  # noqa: E402

REF_CONFIGS = ("stl10_train.yml", "stl10_forget.yml", "stl10_fim.yml", "stl10_sample.yml")
ALPHA = 1e-3


def run(RD, RM, kind, dtype):
    """One step of the reference's runner in `dtype` -> (loss, per-tensor sums, (n_randn, n_randint, n_keep))."""
    real = (torch.randn_like, torch.randint, RM.prob_mask_like, RM.get_timestep_embedding, RD.get_optimizer,
            RD.get_dataset, RD.get_forget_dataset, RD.Conditional_Model, torch.Tensor.backward)
    n = dict(randn=0, randint=0, keep=0)
    cap, losses = {}, []

    def randn_like(x, **k):
        n["randn"] += 1
        return torch.from_numpy(SF.randn_draw(n["randn"] - 1)).to(x.dtype).reshape(x.shape)

    def randint(*a, **k):
        n["randint"] += 1
        return torch.from_numpy(SF.randint_draw(n["randint"] - 1))

    def pml(shape, prob, device):
        if prob in (0, 1):
            return real[2](shape, prob, device)
        n["keep"] += 1
        return torch.from_numpy(SF.keep_draw(n["keep"] - 1))

    def temb(t, dim):  # the reference builds the embedding in fp32 whatever the model's dtype
        return real[3](t, dim).to(dtype)

    def get_opt(config, params):
        cap["params"] = list(params)
        return real[4](config, cap["params"])

    def backward(self, *a, **k):
        if self.dim() == 0:
            losses.append(float(self.item()))
        return real[8](self, *a, **k)

    as_loader = lambda bs: MD.Loader([(torch.from_numpy(x).to(dtype), torch.from_numpy(c)) for x, c in bs])
    cfg = SF.config(n_iters=1)
    old_dtype = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with tempfile.TemporaryDirectory() as d:
            os.makedirs(os.path.join(d, "ckpts"))
            cfg.ckpt_dir, cfg.log_dir = os.path.join(d, "out_ckpts"), os.path.join(d, "logs")
            os.makedirs(cfg.ckpt_dir)
            init = fill_params(real[7](cfg), SF.PARAM_SEED)
            torch.save([torch.nn.DataParallel(init).state_dict(), None, 0], os.path.join(d, "ckpts/ckpt.pth"))
            args = SimpleNamespace(ckpt_folder=d, label_to_forget=0, cond_scale=2.0, mask_path=None, method="rl",
                                   alpha=ALPHA)
            RD.get_dataset = lambda a, c: as_loader(SF.remain_batches())
            RD.get_forget_dataset = lambda a, c, l: (as_loader(SF.remain_batches()), as_loader(SF.forget_batches()))
            RD.Conditional_Model = lambda c: fill_params(real[7](c), SF.PARAM_SEED)
            RD.get_optimizer = get_opt
            torch.randn_like, torch.randint, RM.prob_mask_like, RM.get_timestep_embedding = randn_like, randint, pml, temb
            torch.Tensor.backward = backward
            try:
                torch.manual_seed(99)
                getattr(RD.Diffusion(args, cfg), kind)()
            finally:
                (torch.randn_like, torch.randint, RM.prob_mask_like, RM.get_timestep_embedding, RD.get_optimizer,
                 RD.get_dataset, RD.get_forget_dataset, RD.Conditional_Model, torch.Tensor.backward) = real
    finally:
        torch.set_default_dtype(old_dtype)
    assert len(losses) == 1 and all(p.dtype == dtype for p in cap["params"])
    sums = np.array([float(p.detach().double().sum()) for p in cap["params"]])
    return losses[0], sums, (n["randn"], n["randint"], n["keep"])


def forward(RM, dtype):
    old_dtype = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    real = RM.get_timestep_embedding
    RM.get_timestep_embedding = lambda t, dim: real(t, dim).to(dtype)
    try:
        model = fill_params(RM.Conditional_Model(SF.config()), SF.PARAM_SEED).eval()
        xb, cb = SF.batch(200)
        with torch.no_grad():
            out = model(torch.from_numpy(2 * xb - 1).to(dtype), torch.tensor(SF.FWD_T), torch.from_numpy(cb), mode="test",
                        cond_scale=2.0)
        return out.double().numpy()
    finally:
        RM.get_timestep_embedding = real
        torch.set_default_dtype(old_dtype)


def main():
    RD, _, RM = MD.import_reference_ddpm()
    out = {}
    tables = []
    for name in REF_CONFIGS:
        cfg = dict2namespace(yaml.safe_load(open(os.path.join(MD.REF, "configs", name))))
        sd = RM.Conditional_Model(cfg).state_dict()
        tables.append(([k for k in sd], [str(tuple(v.shape)) for v in sd.values()]))
    assert all(t == tables[0] for t in tables)  # the four files carry the same model block
    shipped = os.path.join(MD.ROOT, "unlearn_saliency_amd", "DDPM", "configs")
    for name in REF_CONFIGS:  # the shipped files hold the reference's values, key for key
        assert yaml.safe_load(open(os.path.join(shipped, name))) == yaml.safe_load(open(os.path.join(MD.REF, "configs", name)))
    out["state_names"], out["state_shapes"] = np.array(tables[0][0]), np.array(tables[0][1])

    scale = lambda a: float(np.abs(a).max())
    f32, f64 = forward(RM, torch.float32), forward(RM, torch.float64)
    out["fwd_test_s2"] = f64
    out["e32_fwd"] = np.float64(np.abs(f32 - f64).max() / scale(f64))
    for tag, kind in (("rl", "saliency_unlearn"), ("train", "train")):
        l32, s32, n32 = run(RD, RM, kind, torch.float32)
        l64, s64, n64 = run(RD, RM, kind, torch.float64)
        assert n32 == n64
        out[f"{tag}_loss"], out[f"{tag}_tensor_sums"] = np.float64(l64), s64
        out[f"{tag}_draw_counts"] = np.array(n64)
        out[f"e32_{tag}_loss"] = np.float64(abs(l32 - l64) / abs(l64))
        out[f"e32_{tag}_sums"] = np.float64(np.abs(s32 - s64).max() / scale(s64))
        print(tag, "loss", l64, "draws", n64, "e32 loss", out[f"e32_{tag}_loss"], "e32 sums", out[f"e32_{tag}_sums"],
              "max |sum32 - sum64|", np.abs(s32 - s64).max())
    out["alpha"] = np.float64(ALPHA)
    print("forward e32", out["e32_fwd"])
    np.savez_compressed(os.path.join(HERE, "ddpm_stl10.npz"), **out)
    print("ddpm_stl10.npz written:", os.path.getsize(os.path.join(HERE, "ddpm_stl10.npz")), "bytes")


if __name__ == "__main__":
    main()
