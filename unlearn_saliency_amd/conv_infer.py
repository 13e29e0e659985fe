"""Inference convolution, pool and image normalisation on K27, K30 and their companions (csrc/salun_conv_infer.hip,
salun_conv1x1_infer.hip, salun_pool.hip, salun_imgnorm.hip).

Thin callers in the pattern of pool.py: inside the kernels' domain a call is one launch; outside it (a dtype or device
the kernels do not take, autocast, a filter or stride K27 refuses) the library op runs — LOUDLY: every such call is
counted in `LIBRARY_INFER_CALLS`, by reason, as `conv.LIBRARY_CONV_CALLS` counts the training convolutions that went
to the library.  Nothing here records an autograd graph: the kernels are forward only, and a tensor that requires grad
is one of the reasons a call goes to the library.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import _lib, ops_infer

# calls that went to the library instead of K27 / the pool / the normalise kernel, by reason
LIBRARY_INFER_CALLS = {"conv_shape": 0, "conv_dtype_or_autocast": 0, "conv_requires_grad": 0, "pool_dtype_or_autocast": 0,
                       "norm_shape": 0, "conv_up2": 0, "resize_host": 0}


def library_infer_calls() -> int:
    return sum(LIBRARY_INFER_CALLS.values())


def reset_library_infer_calls() -> None:
    for k in LIBRARY_INFER_CALLS:
        LIBRARY_INFER_CALLS[k] = 0


def _library_conv(x, w, scale, shift, addend, relu, stride, pad, out_size=None):
    if out_size is not None:       # low-side padding `pad`, zeros on the high side up to the last tap of the asked size
        R = int(w.shape[2])
        hi = [max((n - 1) * stride + R - pad - int(s), 0) for n, s in zip(out_size, x.shape[2:])]
        x, pad = F.pad(x, (pad, hi[1], pad, hi[0])), 0
    y = F.conv2d(x, w, None, stride, pad)
    if out_size is not None:
        y = y[:, :, :out_size[0], :out_size[1]]
    if scale is not None:
        y = y * scale.view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.view(1, -1, 1, 1)
    if addend is not None:
        y = y + addend
    return F.relu(y) if relu else y


def conv_bn_act(x: torch.Tensor, w: torch.Tensor, scale: Optional[torch.Tensor] = None,
                shift: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None, relu: bool = False,
                stride: int = 1, pad: int = 0, out: Optional[torch.Tensor] = None,
                tile: int = _lib.SALUN_INFER_TILE_AUTO, out_size: Optional[tuple] = None) -> torch.Tensor:
    """act(conv2d(x, w, stride, pad) * scale[k] + shift[k] + addend), forward only.  `out_size` = (P, Q): see
    ops_infer.conv2d_infer."""
    ts = [t for t in (x, w, scale, shift, addend) if t is not None]
    if not all(t.is_cuda and t.dtype == torch.float32 for t in ts) or torch.is_autocast_enabled():
        LIBRARY_INFER_CALLS["conv_dtype_or_autocast"] += 1
        return _library_conv(x, w, scale, shift, addend, relu, stride, pad, out_size)
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        LIBRARY_INFER_CALLS["conv_requires_grad"] += 1
        return _library_conv(x, w, scale, shift, addend, relu, stride, pad, out_size)
    ok = x.dim() == 4 and w.dim() == 4 and w.shape[2] == w.shape[3] and w.shape[1] == x.shape[1]
    if ok:
        N, C, H, W = (int(v) for v in x.shape)
        K, R = int(w.shape[0]), int(w.shape[2])
        P, Q = out_size if out_size is not None else \
            (ops_infer.conv_out_size(H, R, stride, pad), ops_infer.conv_out_size(W, R, stride, pad))
        ok = N >= 1 and P >= 1 and Q >= 1 and ops_infer.conv2d_infer_route(N, C, H, W, K, R, stride, pad, P, Q, tile) is not None
    if not ok:
        LIBRARY_INFER_CALLS["conv_shape"] += 1
        return _library_conv(x, w, scale, shift, addend, relu, stride, pad, out_size)
    return ops_infer.conv2d_infer(x.contiguous(), w.contiguous(), scale, shift,
                                  None if addend is None else addend.contiguous(), relu, stride, pad, out, tile, out_size)


def conv1x1_bn_act(x: torch.Tensor, w: torch.Tensor, scale: Optional[torch.Tensor] = None,
                   shift: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None, relu: bool = False,
                   out: Optional[torch.Tensor] = None, tile: int = _lib.SALUN_INFER_TILE_AUTO) -> torch.Tensor:
    """act(conv2d(x, w) * scale[k] + shift[k] + addend) of a 1 x 1 / stride-1 / unpadded w [K, C, 1, 1] on K30, forward
    only.  Outside K30's domain the call is `conv_bn_act`'s (K27, which returns the same bits, or - counted there - the
    library); nothing is counted here."""
    ts = [t for t in (x, w, scale, shift, addend) if t is not None]
    ok = all(t.is_cuda and t.dtype == torch.float32 for t in ts) and not torch.is_autocast_enabled() and \
        not (torch.is_grad_enabled() and any(t.requires_grad for t in ts)) and x.dim() == 4 and w.dim() == 4 and \
        w.shape[2] == 1 and w.shape[3] == 1 and w.shape[1] == x.shape[1] and x.shape[0] >= 1 and \
        x.shape[2] * x.shape[3] >= 1
    if ok:
        N, C, H, W = (int(v) for v in x.shape)
        ok = ops_infer.conv1x1_infer_route(N, C, H * W, int(w.shape[0]), tile) is not None
    if not ok:
        return conv_bn_act(x, w, scale, shift, addend, relu, 1, 0, out, tile)
    return ops_infer.conv1x1_infer(x.contiguous(), w.contiguous(), scale, shift,
                                   None if addend is None else addend.contiguous(), relu, out, tile)


def u8_crop_to_chw_norm(src: torch.Tensor, table: torch.Tensor, top: int, left: int, OH: int, OW: int,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Normalize(ToTensor(src[:, top:top+OH, left:left+OW])) of uint8 [B, H, W, C] device images; a window outside the
    image is an error, not a library call."""
    if not (src.is_cuda and src.dtype == torch.uint8 and src.dim() == 4 and 1 <= src.shape[3] <= _lib.SALUN_U8_NORM_MAX_C):
        LIBRARY_INFER_CALLS["norm_shape"] += 1
        return u8_to_chw_norm(src[:, top:top + OH, left:left + OW].contiguous(), table, out)
    return ops_infer.u8_crop_to_chw_norm(src.contiguous(), table, top, left, OH, OW, out)


def maxpool3x3s2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """max_pool2d(x, kernel_size=3, stride=2, padding=1) with the library's selection rule."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4) or torch.is_autocast_enabled() or \
            (torch.is_grad_enabled() and x.requires_grad):
        LIBRARY_INFER_CALLS["pool_dtype_or_autocast"] += 1
        return F.max_pool2d(x, 3, 2, 1)
    return ops_infer.maxpool3x3s2(x.contiguous(), out)


def u8_to_chw_norm(src: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Normalize(ToTensor(src)) of uint8 [B, H, W, C] device images through the [C, 256] table of ops_infer.u8_norm_table."""
    if not (src.is_cuda and src.dtype == torch.uint8 and src.dim() == 4 and 1 <= src.shape[3] <= _lib.SALUN_U8_NORM_MAX_C):
        LIBRARY_INFER_CALLS["norm_shape"] += 1
        idx = src.long().permute(0, 3, 1, 2)
        return torch.stack([table.to(src.device)[c][idx[:, c]] for c in range(idx.shape[1])], 1)
    return ops_infer.u8_to_chw_norm(src.contiguous(), table, out)


def conv_up2_bn_act(x: torch.Tensor, w: torch.Tensor, scale: Optional[torch.Tensor] = None,
                    shift: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None, relu: bool = False,
                    out: Optional[torch.Tensor] = None, tile: int = _lib.SALUN_INFER_TILE_AUTO) -> torch.Tensor:
    """act(conv2d(interpolate(x, scale_factor=2, mode="nearest"), w, padding=1) * scale[k] + shift[k] + addend), forward
    only: one K27 launch that gathers x[ih >> 1][iw >> 1]; the up-sampled tensor is never written."""
    def library(reason):
        LIBRARY_INFER_CALLS[reason] += 1
        return _library_conv(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, scale, shift, addend, relu, 1, 1)
    ts = [t for t in (x, w, scale, shift, addend) if t is not None]
    if not all(t.is_cuda and t.dtype == torch.float32 for t in ts) or torch.is_autocast_enabled() or \
            (torch.is_grad_enabled() and any(t.requires_grad for t in ts)):
        return library("conv_up2")
    ok = x.dim() == 4 and w.dim() == 4 and w.shape[2] == w.shape[3] and w.shape[1] == x.shape[1] and x.shape[0] >= 1
    if ok:
        N, C, H, W = (int(v) for v in x.shape)
        ok = ops_infer.conv2d_infer_up2_route(N, C, H, W, int(w.shape[0]), int(w.shape[2]), 1, 1, tile=tile) is not None
    if not ok:
        return library("conv_up2")
    return ops_infer.conv2d_infer_up2(x.contiguous(), w.contiguous(), scale, shift,
                                      None if addend is None else addend.contiguous(), relu, out, tile)
