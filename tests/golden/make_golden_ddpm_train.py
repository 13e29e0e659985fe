"""Golden vectors for training from scratch: runs the REFERENCE's `Diffusion.train()` (DDPM/runners/diffusion.py:194-270,
imported from /root/reference/DDPM, build container only) on the reduced U-Net for 2 iterations with the EMA on,
recording every random draw (noise, timesteps, label drop).  `retrain()` (:399-480) has the same loop body over another
loader, so one capture pins both.

The EMA rate of the capture is 0.9 and not the 0.9999 of cifar10_train.yml: after two steps of lr 1e-4 a shadow at
0.9999 has moved by ~2e-8, a handful of fp32 ulps of a weight, and would pin nothing.  1 - 0.9 is still below 0.5, the
branch of lerp the training runs take.

    python tests/golden/make_golden_ddpm_train.py
"""
from __future__ import annotations

import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ddpm as MD  # noqa: E402
from fixtures import ddpm_batch, ddpm_small_config, fill_params  # noqa: E402

EMA_RATE = 0.9


def main():
    RD, RLoss, RM = MD.import_reference_ddpm()
    cfg = ddpm_small_config()
    cfg.training.n_iters = 2
    cfg.model.ema, cfg.model.ema_rate = True, EMA_RATE
    batches = MD.Loader([tuple(map(torch.from_numpy, ddpm_batch(4, 300 + i))) for i in range(2)])
    rec = dict(randn=[], randint=[], keep=[], loss=[])
    real = (torch.randn_like, torch.randint, RM.prob_mask_like, RD.get_optimizer, RD.get_dataset, RD.Conditional_Model,
            RD.EMAHelper, torch.Tensor.backward)
    cap = {}

    def randn_like(x, **k):
        r = real[0](x, **k)
        rec["randn"].append(r.clone())
        return r

    def randint(*a, **k):
        r = real[1](*a, **k)
        rec["randint"].append(r.clone())
        return r

    def pml(shape, prob, device):
        r = real[2](shape, prob, device)
        if prob not in (0, 1):
            rec["keep"].append(r.clone())
        return r

    def get_opt(config, params):
        cap["params"] = list(params)
        cap["opt"] = real[3](config, cap["params"])
        return cap["opt"]

    def backward(self, *a, **k):  # `loss.backward()` of the loop body: the step's loss
        if self.dim() == 0:
            rec["loss"].append(float(self.item()))
        return real[7](self, *a, **k)

    class RecordingEMA(real[6]):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            cap["ema"] = self

    with tempfile.TemporaryDirectory() as d:
        cfg.ckpt_dir, cfg.log_dir = os.path.join(d, "out_ckpts"), os.path.join(d, "logs")
        os.makedirs(cfg.ckpt_dir)
        args = SimpleNamespace(ckpt_folder=d, label_to_forget=0, cond_scale=2.0, mask_path=None)
        RD.get_dataset = lambda a, c: batches
        RD.Conditional_Model = lambda c: fill_params(real[5](c), 7000)  # the run starts from generator-filled weights
        RD.get_optimizer, RD.EMAHelper = get_opt, RecordingEMA
        torch.randn_like, torch.randint, RM.prob_mask_like = randn_like, randint, pml
        torch.Tensor.backward = backward
        try:
            torch.manual_seed(99)
            RD.Diffusion(args, cfg).train()
        finally:
            (torch.randn_like, torch.randint, RM.prob_mask_like, RD.get_optimizer, RD.get_dataset, RD.Conditional_Model,
             RD.EMAHelper, torch.Tensor.backward) = real
    s = MD.summarize(SimpleNamespace(parameters=lambda: cap["params"]))
    st = cap["opt"].state
    m1 = np.concatenate([st[p]["exp_avg"].reshape(-1).numpy() for p in cap["params"]])
    m2 = np.concatenate([st[p]["exp_avg_sq"].reshape(-1).numpy() for p in cap["params"]])
    shadow = cap["ema"].shadow
    assert not any(k.startswith("module.") for k in shadow)  # the reference registers the unwrapped module's names
    sh = np.concatenate([v.reshape(-1).numpy() for v in shadow.values()])
    assert sh.size == m1.size
    np.savez_compressed(os.path.join(HERE, "ddpm_train_step.npz"), param_sample=s["sample"],
                        tensor_sums=s["tensor_sums"], randn=np.stack([t.numpy() for t in rec["randn"]]),
                        randint=np.stack([t.numpy() for t in rec["randint"]]),
                        keep=np.stack([t.numpy() for t in rec["keep"]]), step_loss=np.array(rec["loss"], np.float64),
                        exp_avg_sample=m1[::MD.SAMPLE_STRIDE], exp_avg_sq_sample=m2[::MD.SAMPLE_STRIDE],
                        exp_avg_norm=np.float64(np.linalg.norm(m1.astype(np.float64))),
                        exp_avg_sq_sum=np.float64(m2.astype(np.float64).sum()),
                        shadow_sample=sh[::MD.SAMPLE_STRIDE], shadow_sum=np.float64(sh.astype(np.float64).sum()),
                        shadow_keys=np.array(list(shadow.keys())), n_iters=2, ema_rate=EMA_RATE)
    print("ddpm_train_step.npz written:", len(rec["randn"]), "randn,", len(rec["randint"]), "randint,",
          len(rec["keep"]), "keep draws; losses", rec["loss"])


if __name__ == "__main__":
    main()
