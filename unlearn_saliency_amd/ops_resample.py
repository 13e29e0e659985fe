"""Tensor-level wrapper of K26 (csrc/salun_resample.hip; include/salun.h): the antialiased bilinear resample of uint8
images that `PIL.Image.resize(size, Image.BILINEAR)` — torchvision's `transforms.Resize` on a PIL image — computes,
bit for bit, on the device.

Same conventions as ops.py: device tensors only, raw pointers and the current stream handed to libsalun.so, a failing
call raises `SalunError`.  The source may start at any byte (a slice of a larger uint8 buffer is fine) but must be
contiguous.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _lib
from ._lib import c_int64, c_void_p, check
from .ops import _dev, _stream

CHANNELS = (1, 3, 4)


def lds_bytes(H: int, W: int, C: int, OH: int, OW: int) -> int:
    """LDS bytes of the launch for this size pair; 0 when the kernel refuses it (outside the limits, or a band of one
    output row would not fit SALUN_RESAMPLE_MAX_LDS).  Host arithmetic only."""
    return int(_lib.lib().salun_resample_u8_lds_bytes(int(H), int(W), int(C), int(OH), int(OW)))


def axis_table(n_in: int, n_out: int):
    """The library's coefficient table of one axis as host arrays (first tap [n_out], tap count [n_out],
    weights [n_out, ksize], all int32).  Host arithmetic only."""
    import ctypes

    import numpy as np
    ksize = ctypes.c_int(0)
    L = _lib.lib()
    check(L.salun_resample_u8_table(int(n_in), int(n_out), None, 0, ctypes.byref(ksize)), "salun_resample_u8_table")
    buf = np.empty(n_out * (2 + ksize.value), np.int32)
    check(L.salun_resample_u8_table(int(n_in), int(n_out), c_void_p(buf.ctypes.data), buf.size, ctypes.byref(ksize)),
          "salun_resample_u8_table")
    return buf[:n_out], buf[n_out:2 * n_out], buf[2 * n_out:].reshape(n_out, ksize.value)


def resize_u8(x: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """x uint8 [B, H, W, C] on the device -> uint8 [B, OH, OW, C], size = (OH, OW).  One launch."""
    if x.dim() != 4:
        raise ValueError(f"resize_u8: x {tuple(x.shape)} must be (B, H, W, C)")
    B, H, W, C = (int(v) for v in x.shape)
    OH, OW = (int(v) for v in size)
    src = _dev(x, torch.uint8, "x")
    if B < 1 or lds_bytes(H, W, C, OH, OW) == 0:
        raise ValueError(f"resize_u8: {B} x {H} x {W} x {C} -> {OH} x {OW} is outside the kernel's domain (B >= 1, C in "
                         f"{CHANNELS}, sides in [1, {_lib.SALUN_RESAMPLE_MAX_SIDE}], a one-row band within "
                         f"{_lib.SALUN_RESAMPLE_MAX_LDS} bytes of LDS)")
    out = torch.empty((B, OH, OW, C), dtype=torch.uint8, device=x.device)
    check(_lib.lib().salun_resample_u8(src, c_void_p(out.data_ptr()), c_int64(B), H, W, C, OH, OW, _stream()),
          "salun_resample_u8")
    return out
