"""Tensor-level wrappers of the sampler kernels (K19, csrc/salun_sampler.hip; include/salun.h).

Same conventions as ops.py / ops_ff.py: device tensors only, raw pointers and the current stream handed to
libsalun.so, a failing call raises `SalunError`.  Images are (B, C, H, W) fp32 in the model's range; `image_ids` is a
(B,) int64 device vector of GLOBAL image ids: every draw is keyed by (seed, step, image id), never by the batch.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib, ops
from ._lib import c_double, c_int64, c_size_t, c_uint64, check
from .draws import _M64, _splitmix64
from .ops import _dev, _stream

ANCESTRAL, GENERALIZED = 0, 1  # SALUN_SAMPLER_ANCESTRAL / SALUN_SAMPLER_GENERALIZED
VARIANTS = {"ancestral": ANCESTRAL, "ddpm_noisy": ANCESTRAL, "generalized": GENERALIZED}
START_STEP = 0  # the step index of the start noise x_T; reverse step k (0-based, in the order it is taken) draws at k + 1
IMAGES_U8_MAX_CHW = 16000


def sampler_key(seed: int, step: int, image_id: int) -> int:
    """The `salun_fill_normal` seed of one image's noise at one step (the kernels derive the same key on the device)."""
    return _splitmix64((_splitmix64((_splitmix64(int(seed) & _M64) + int(step)) & _M64) + int(image_id)) & _M64)


def _rows(t: torch.Tensor) -> Tuple[int, int]:
    if t.dim() < 1:
        raise ValueError("expected a batch of images")
    B = t.shape[0]
    return B, (t.numel() // B if B else 0)


def sampler_noise(image_ids: torch.Tensor, shape, seed: int, step: int = START_STEP) -> torch.Tensor:
    """(B, *shape) fp32: row b is fill_normal(prod(shape), sampler_key(seed, step, image_ids[b]))."""
    B = image_ids.numel()
    out = torch.empty((B,) + tuple(shape), dtype=torch.float32, device=image_ids.device)
    check(_lib.lib().salun_sampler_noise(_dev(out, torch.float32, "out"), c_uint64(int(seed) & _M64),
                                         _dev(image_ids, torch.int64, "image_ids"), c_int64(step), c_int64(B),
                                         c_int64(_rows(out)[1]), _stream()), "salun_sampler_noise")
    return out


def sampler_step(x: torch.Tensor, eps_cond: torch.Tensor, eps_null: Optional[torch.Tensor], cond_scale: float,
                 abar: torch.Tensor, idx_t: int, idx_next: int, variant: int, eta: float = 0.0,
                 noise: Optional[torch.Tensor] = None, seed: int = 0, image_ids: Optional[torch.Tensor] = None,
                 step: int = 0, out: Optional[torch.Tensor] = None, x0: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One reverse step (see salun_sampler_step).  `abar`: the device table of `alpha_bar_table`; `idx_t` / `idx_next`
    are i + 1 / j + 1 of the loop.  `noise` given: used as the step's z; else drawn on (seed, step, image_ids).
    `out` defaults to a new tensor (pass `x` for in place); `x0`, when given, receives the x0 estimate."""
    B, chw = _rows(x)
    if out is None:
        out = torch.empty_like(x)
    for nm, t in (("eps_cond", eps_cond), ("eps_null", eps_null), ("noise", noise), ("out", out), ("x0", x0)):
        if t is not None and t.shape != x.shape:
            raise ValueError(f"{nm} {tuple(t.shape)} does not match x {tuple(x.shape)}")
    if image_ids is not None and image_ids.numel() != B:
        raise ValueError(f"image_ids has {image_ids.numel()} entries for a batch of {B}")
    f = lambda t, nm: _dev(t, torch.float32, nm, True)
    check(_lib.lib().salun_sampler_step(_dev(x, torch.float32, "x"), _dev(eps_cond, torch.float32, "eps_cond"),
                                        f(eps_null, "eps_null"), c_double(cond_scale), _dev(abar, torch.float32, "abar"),
                                        abar.numel(), int(idx_t), int(idx_next), int(variant), c_double(eta),
                                        f(noise, "noise"), c_uint64(int(seed) & _M64),
                                        _dev(image_ids, torch.int64, "image_ids", True), c_int64(step),
                                        _dev(out, torch.float32, "out"), f(x0, "x0"), c_int64(B), c_int64(chw),
                                        _stream()), "salun_sampler_step")
    return out


def minmax(x: torch.Tensor) -> torch.Tensor:
    """Device tensor [min x, max x] (fixed reduction order)."""
    L = _lib.lib()
    n = x.numel()
    nbytes = int(L.salun_minmax_workspace_bytes(c_int64(n)))
    ws = ops.workspace(nbytes, x.device)
    lohi = torch.empty(2, dtype=torch.float32, device=x.device)
    check(L.salun_minmax(_dev(x, torch.float32, "x"), c_int64(n), _dev(lohi, torch.float32, "lohi"),
                         _dev(ws, torch.uint8, "ws"), c_size_t(nbytes), _stream()), "salun_minmax")
    return lohi


def images_to_u8(x: torch.Tensor, rescaled: bool = True, value_range: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, C, H, W) fp32 in the model's range -> (B, H, W, C) uint8: the reference's `inverse_data_transform` followed
    by torchvision's `save_image(normalize=True)`, per image, or over `value_range` = `minmax(x)` of a whole grid."""
    if x.dim() != 4:
        raise ValueError(f"x {tuple(x.shape)} must be (B, C, H, W)")
    B, C, H, W = x.shape
    if C * H * W > IMAGES_U8_MAX_CHW:
        raise NotImplementedError(f"images_to_u8: an image of {C}x{H}x{W} floats does not fit the workgroup's LDS "
                                  f"({IMAGES_U8_MAX_CHW} floats)")
    out = torch.empty((B, H, W, C), dtype=torch.uint8, device=x.device)
    check(_lib.lib().salun_images_to_u8(_dev(x, torch.float32, "x"), _dev(out, torch.uint8, "out"), c_int64(B), C,
                                        H * W, 1 if rescaled else 0, _dev(value_range, torch.float32, "value_range", True),
                                        _stream()), "salun_images_to_u8")
    return out


def ldm_ddim_step(x: torch.Tensor, eps: torch.Tensor, scale: float, c_s1m: float, c_sqrt_at: float, c_dir: float,
                  c_sqrt_aprev: float, c_sigma: float = 0.0, z: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, x0: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One reverse step of the LDM DDIM sampler on latents (K21, salun_ldm_ddim_step).  `eps` with 2B rows is the output
    of one batched U-Net pass over cat([x, x]) (rows [0, B) unconditional, [B, 2B) conditional, read in place); with B
    rows it is the no-guidance branch and `scale` must be 1.  The coefficients are the host's fp32 values
    (SD/ddim.py: DDIMSchedule.coefficients).  `out` defaults to a new tensor (pass `x` for in place)."""
    B, chw = _rows(x)
    if eps.shape[0] not in (B, 2 * B) or eps.shape[1:] != x.shape[1:]:
        raise ValueError(f"eps {tuple(eps.shape)} is neither x {tuple(x.shape)} nor its two-fold batch")
    guided = B > 0 and eps.shape[0] == 2 * B
    if out is None:
        out = torch.empty_like(x)
    for nm, t in (("z", z), ("out", out), ("x0", x0)):
        if t is not None and t.shape != x.shape:
            raise ValueError(f"{nm} {tuple(t.shape)} does not match x {tuple(x.shape)}")
    f = lambda t, nm: _dev(t, torch.float32, nm, True)
    check(_lib.lib().salun_ldm_ddim_step(_dev(x, torch.float32, "x"), _dev(eps, torch.float32, "eps"), int(guided),
                                         c_double(scale), c_double(c_s1m), c_double(c_sqrt_at), c_double(c_dir),
                                         c_double(c_sqrt_aprev), c_double(c_sigma), f(z, "z"),
                                         _dev(out, torch.float32, "out"), f(x0, "x0"), c_int64(B), c_int64(chw),
                                         _stream()), "salun_ldm_ddim_step")
    return out


LMS_ORDER = _lib.SALUN_LMS_ORDER


def lms_step(x: torch.Tensor, eps: torch.Tensor, scale: float, hist: torch.Tensor, slot: int, coeffs, den: float,
             out: Optional[torch.Tensor] = None, x_in: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One step of the linear multistep sampler (salun_lms_step; SD/lms.py).  `eps` with 2B rows is the output of one
    batched U-Net pass (rows [0, B) unconditional, [B, 2B) conditional, read in place); with B rows there is no guidance
    and `scale` must be 1.  `hist` [LMS_ORDER, *x.shape] is the ring of derivatives: this step's goes to `slot`, and
    `coeffs` (1 to LMS_ORDER host floats, newest derivative first) weigh slot, slot - 1, ...  `x_in`, when given, receives
    x_new / den in each of its eps.shape[0] / B row blocks: the input of the next pass.  `out` may be `x`."""
    B, chw = _rows(x)
    if eps.shape[0] not in (B, 2 * B) or eps.shape[1:] != x.shape[1:]:
        raise ValueError(f"eps {tuple(eps.shape)} is neither x {tuple(x.shape)} nor its two-fold batch")
    guided = B > 0 and eps.shape[0] == 2 * B
    c = [float(v) for v in coeffs]
    if not 1 <= len(c) <= LMS_ORDER:
        raise ValueError(f"lms_step: {len(c)} coefficients, the order is 1 to {LMS_ORDER}")
    if tuple(hist.shape) != (LMS_ORDER,) + tuple(x.shape):
        raise ValueError(f"hist {tuple(hist.shape)} must be {(LMS_ORDER,) + tuple(x.shape)}")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape:
        raise ValueError(f"out {tuple(out.shape)} does not match x {tuple(x.shape)}")
    if x_in is not None and x_in.shape != eps.shape:
        raise ValueError(f"x_in {tuple(x_in.shape)} does not match eps {tuple(eps.shape)}")
    c4 = c + [0.0] * (LMS_ORDER - len(c))
    check(_lib.lib().salun_lms_step(_dev(x, torch.float32, "x"), _dev(eps, torch.float32, "eps"), int(guided),
                                    c_double(scale), _dev(hist, torch.float32, "hist"), int(slot), len(c),
                                    c_double(c4[0]), c_double(c4[1]), c_double(c4[2]), c_double(c4[3]), c_double(den),
                                    _dev(out, torch.float32, "out"), _dev(x_in, torch.float32, "x_in", True),
                                    c_int64(B), c_int64(chw), _stream()), "salun_lms_step")
    return out
