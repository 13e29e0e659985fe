"""CPU restatement of salun_adam_ema_step (K20) — TEST INFRASTRUCTURE ONLY.

The Adam part is the oracle's `masked_adam_step` (oracle/salun_oracle.c, the restatement salun_masked_adam_step is
pinned to); the EMA part is written here in numpy:

    w      = float32(1 - mu)                     1 - mu in double, then one rounding
    shadow = fma(w, p_new - shadow, shadow)      Tensor.lerp_(p_new, 1 - mu) for a weight below 0.5

numpy has no fused multiply-add.  The product of two fp32 numbers is exact in double (48 bits), so the fma is the sum
`shadow + w * d` evaluated in double and rounded to fp32 — exact except where the double sum itself had to round AND
landed on an fp32 tie (double rounding), which costs at most one fp32 ulp; the GPU tests that compare against this
restatement allow that one ulp on the shadow and nothing on p / m1 / v.

`install()` puts it behind `ops.adam_ema_step` the way tests/cpu_standins.py does for the other kernels, so the host
logic around the kernel (FusedMaskedAdam.attach_ema, EMAHelper's handshake, Diffusion.train) runs on the CPU.
"""
from __future__ import annotations

import numpy as np
import torch

import oracle


def ema_lerp(shadow: np.ndarray, p: np.ndarray, mu: float) -> None:
    """In place: shadow <- fma(w, p - shadow, shadow), w = float32(1 - mu)."""
    w = np.float32(1.0 - mu)
    d = (p - shadow).astype(np.float32)  # fp32 subtraction, one rounding
    shadow[...] = (shadow.astype(np.float64) + np.float64(w) * d.astype(np.float64)).astype(np.float32)


def adam_ema_step(p, g, m1, v, shadow, mask, gscale, lr, b1, b2, eps, wd, mu, step) -> None:
    """numpy arrays, all updated in place."""
    oracle.masked_adam_step(p, g, m1, v, mask, gscale, lr, b1, b2, eps, wd, step)
    ema_lerp(shadow, p, mu)


CALLS = {"adam_ema_step": 0, "masked_adam_step": 0}


def _np(t: torch.Tensor) -> np.ndarray:
    assert t.device.type == "cpu" and t.is_contiguous()
    return t.detach().numpy()


def install() -> None:
    """cpu_standins.install() + the stand-in of K20; both Adam entry points count their calls in CALLS."""
    import cpu_standins
    from unlearn_saliency_amd import ops
    cpu_standins.install()
    plain = ops.masked_adam_step

    def masked_adam_step(*a, **k):
        CALLS["masked_adam_step"] += 1
        return plain(*a, **k)

    def adam_ema_step_(p, g, m1, v, shadow, mask, lr, beta1, beta2, eps, weight_decay, mu, step, sqnorm=None,
                       max_norm=1.0, gscale=1.0):
        CALLS["adam_ema_step"] += 1
        ops.PARAM_EPOCH[0] += 1
        if sqnorm is not None:  # the kernel's rule: the clip coefficient replaces gscale
            gscale = oracle.clip_coef(float(sqnorm.item()), max_norm)
        adam_ema_step(_np(p), _np(g), _np(m1), _np(v), _np(shadow), None if mask is None else _np(mask), gscale, lr,
                      beta1, beta2, eps, weight_decay, mu, step)

    ops.masked_adam_step = masked_adam_step
    ops.adam_ema_step = adam_ema_step_
