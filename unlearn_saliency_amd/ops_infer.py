"""Tensor-level wrappers of K27, K30 and the kernels around them (csrc/salun_conv_infer.hip, salun_conv1x1_infer.hip,
salun_pool.hip, salun_imgnorm.hip, salun_cls_head.hip, salun_row_topk.hip; include/salun.h): the forward-only
convolutions with a folded-BatchNorm epilogue, the 3 x 3 / stride-2 max-pool, uint8 HWC -> normalised fp32 CHW (whole or
a window), the evaluation head and the row top-k.

Same conventions as ops.py: device tensors only, raw pointers and the current stream handed to libsalun.so, a failing
call raises `SalunError`.  Every function takes an optional `out` so that a caller with its own activation buffers
(DDPM/models/resnet34.InferencePlan) allocates nothing per call.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import c_int64, c_size_t, c_void_p, check
from .ops import _dev, _stream, workspace


def conv_out_size(size: int, R: int, stride: int, pad: int) -> int:
    return (size + 2 * pad - R) // stride + 1


def conv2d_infer_route(N, C, H, W, K, R, stride, pad, P, Q, tile: int = _lib.SALUN_INFER_TILE_AUTO) -> Optional[str]:
    """The label of the plan a call would run, or None where K27 refuses the shape.  Host arithmetic only."""
    buf = ctypes.create_string_buffer(96)
    rc = _lib.lib().salun_conv2d_infer_route(N, C, H, W, K, R, stride, pad, P, Q, tile, buf, 96)
    if rc == _lib.SALUN_EINVAL:
        return None
    check(rc, "salun_conv2d_infer_route")
    return buf.value.decode()


def conv2d_infer(x: torch.Tensor, w: torch.Tensor, scale: Optional[torch.Tensor] = None,
                 shift: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None, relu: bool = False,
                 stride: int = 1, pad: int = 0, out: Optional[torch.Tensor] = None,
                 tile: int = _lib.SALUN_INFER_TILE_AUTO, out_size: Optional[tuple] = None) -> torch.Tensor:
    """act(conv(x, w) * scale[k] + shift[k] + addend): x [N, C, H, W], w [K, C, R, R] -> [N, K, P, Q].  One launch.
    `pad` is the low-side padding; `out_size` = (P, Q) asks for more rows / columns than the symmetric formula gives:
    taps past the high edge read zero (F.pad(x, (0, 1, 0, 1)) + a stride-2 convolution is pad = 0 with P = H / 2)."""
    N, C, H, W = (int(v) for v in x.shape)
    K, Cw, R, S = (int(v) for v in w.shape)
    if Cw != C or R != S:
        raise ValueError(f"conv2d_infer: weight {tuple(w.shape)} does not fit x {tuple(x.shape)}")
    P, Q = out_size if out_size is not None else (conv_out_size(H, R, stride, pad), conv_out_size(W, R, stride, pad))
    if out is None:
        out = torch.empty((N, K, P, Q), dtype=torch.float32, device=x.device)
    elif out.numel() != N * K * P * Q:
        raise ValueError("conv2d_infer: out has the wrong size")
    if addend is not None and addend.numel() != out.numel():
        raise ValueError("conv2d_infer: addend has the wrong size")
    check(_lib.lib().salun_conv2d_infer(_dev(x, torch.float32, "x"), _dev(w, torch.float32, "w"),
                                        _dev(scale, torch.float32, "scale", True),
                                        _dev(shift, torch.float32, "shift", True),
                                        _dev(addend, torch.float32, "addend", True), _dev(out, torch.float32, "out"),
                                        N, C, H, W, K, R, stride, pad, P, Q, int(bool(relu)), tile, _stream()),
          "salun_conv2d_infer")
    return out.view(N, K, P, Q)


def conv2d_infer_up2_route(N, C, H, W, K, R=3, stride=1, pad=1, P=None, Q=None,
                           tile: int = _lib.SALUN_INFER_TILE_AUTO) -> Optional[str]:
    """The label of the plan conv2d_infer_up2 would run on a STORED [N, C, H, W] input, or None where it refuses."""
    P = conv_out_size(2 * H, R, stride, pad) if P is None else P
    Q = conv_out_size(2 * W, R, stride, pad) if Q is None else Q
    buf = ctypes.create_string_buffer(96)
    rc = _lib.lib().salun_conv2d_infer_up2_route(N, C, H, W, K, R, stride, pad, P, Q, tile, buf, 96)
    if rc == _lib.SALUN_EINVAL:
        return None
    check(rc, "salun_conv2d_infer_up2_route")
    return buf.value.decode()


def conv2d_infer_up2(x: torch.Tensor, w: torch.Tensor, scale: Optional[torch.Tensor] = None,
                     shift: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None, relu: bool = False,
                     out: Optional[torch.Tensor] = None, tile: int = _lib.SALUN_INFER_TILE_AUTO, stride: int = 1,
                     pad: int = 1) -> torch.Tensor:
    """act(conv(up2(x), w) * scale[k] + shift[k] + addend) with up2 = nearest-neighbour 2x, which is never written:
    x [N, C, H, W], w [K, C, 3, 3] -> [N, K, 2H, 2W].  One launch.  (stride and pad exist so that a refusal can be asked
    for; the kernel serves stride 1.)"""
    N, C, H, W = (int(v) for v in x.shape)
    K, Cw, R, S = (int(v) for v in w.shape)
    if Cw != C or R != S:
        raise ValueError(f"conv2d_infer_up2: weight {tuple(w.shape)} does not fit x {tuple(x.shape)}")
    P, Q = conv_out_size(2 * H, R, stride, pad), conv_out_size(2 * W, R, stride, pad)
    if out is None:
        out = torch.empty((N, K, P, Q), dtype=torch.float32, device=x.device)
    elif out.numel() != N * K * P * Q:
        raise ValueError("conv2d_infer_up2: out has the wrong size")
    if addend is not None and addend.numel() != out.numel():
        raise ValueError("conv2d_infer_up2: addend has the wrong size")
    check(_lib.lib().salun_conv2d_infer_up2(_dev(x, torch.float32, "x"), _dev(w, torch.float32, "w"),
                                            _dev(scale, torch.float32, "scale", True),
                                            _dev(shift, torch.float32, "shift", True),
                                            _dev(addend, torch.float32, "addend", True), _dev(out, torch.float32, "out"),
                                            N, C, H, W, K, R, stride, pad, P, Q, int(bool(relu)), tile, _stream()),
          "salun_conv2d_infer_up2")
    return out.view(N, K, P, Q)


def conv1x1_infer_route(N, C, HW, K, tile: int = _lib.SALUN_INFER_TILE_AUTO, aligned16: bool = True,
                        w_aligned16: bool = True) -> Optional[str]:
    """The label of the plan a K30 call would run, or None where K30 refuses the shape.  Host arithmetic only.
    `aligned16`: x and y are 16-byte aligned; `w_aligned16`: w is."""
    buf = ctypes.create_string_buffer(96)
    rc = _lib.lib().salun_conv1x1_infer_route(N, C, c_int64(HW), K, tile, int(bool(aligned16)), int(bool(w_aligned16)),
                                              buf, 96)
    if rc == _lib.SALUN_EINVAL:
        return None
    check(rc, "salun_conv1x1_infer_route")
    return buf.value.decode()


def conv1x1_infer(x: torch.Tensor, w: torch.Tensor, scale: Optional[torch.Tensor] = None,
                  shift: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None, relu: bool = False,
                  out: Optional[torch.Tensor] = None, tile: int = _lib.SALUN_INFER_TILE_AUTO) -> torch.Tensor:
    """K30: act(conv1x1(x, w) * scale[k] + shift[k] + addend): x [N, C, H, W], w [K, C] or [K, C, 1, 1] ->
    [N, K, H, W].  One launch; the bits of conv2d_infer with R = 1."""
    N, C, H, W = (int(v) for v in x.shape)
    K = int(w.shape[0])
    if w.numel() != K * C:
        raise ValueError(f"conv1x1_infer: weight {tuple(w.shape)} does not fit x {tuple(x.shape)}")
    if out is None:
        out = torch.empty((N, K, H, W), dtype=torch.float32, device=x.device)
    elif out.numel() != N * K * H * W:
        raise ValueError("conv1x1_infer: out has the wrong size")
    if addend is not None and addend.numel() != out.numel():
        raise ValueError("conv1x1_infer: addend has the wrong size")
    check(_lib.lib().salun_conv1x1_infer(_dev(x, torch.float32, "x"), _dev(w, torch.float32, "w"),
                                         _dev(scale, torch.float32, "scale", True),
                                         _dev(shift, torch.float32, "shift", True),
                                         _dev(addend, torch.float32, "addend", True), _dev(out, torch.float32, "out"),
                                         N, C, c_int64(H * W), K, int(bool(relu)), tile, _stream()),
          "salun_conv1x1_infer")
    return out.view(N, K, H, W)


def u8_crop_to_chw_norm(src: torch.Tensor, table: torch.Tensor, top: int, left: int, OH: int, OW: int,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Normalize(ToTensor(src[:, top:top+OH, left:left+OW])) of uint8 [B, H, W, C] -> fp32 [B, C, OH, OW]; the crop is
    never copied."""
    B, H, W, C = (int(v) for v in src.shape)
    if tuple(table.shape) != (C, 256):
        raise ValueError(f"u8_crop_to_chw_norm: table {tuple(table.shape)} must be ({C}, 256)")
    if out is None:
        out = torch.empty((B, C, max(OH, 0), max(OW, 0)), dtype=torch.float32, device=src.device)
    elif out.numel() != B * C * OH * OW:
        raise ValueError("u8_crop_to_chw_norm: out has the wrong size")
    check(_lib.lib().salun_u8_crop_to_chw_norm(_dev(src, torch.uint8, "src"), _dev(table, torch.float32, "table"),
                                               _dev(out, torch.float32, "out"), c_int64(B), H, W, C, int(top), int(left),
                                               int(OH), int(OW), _stream()), "salun_u8_crop_to_chw_norm")
    return out.view(B, C, OH, OW)


def row_topk(p: torch.Tensor, k: int, values: Optional[torch.Tensor] = None, indices: Optional[torch.Tensor] = None):
    """p [B, K] fp32 -> (values [B, k] fp32, indices [B, k] int64), sorted: larger first, NaN above every number, equal
    values by ascending index (include/salun.h)."""
    B, K = (int(v) for v in p.shape)
    if values is None:
        values = torch.empty((B, k), dtype=torch.float32, device=p.device)
    if indices is None:
        indices = torch.empty((B, k), dtype=torch.int64, device=p.device)
    if values.numel() != B * k or indices.numel() != B * k:
        raise ValueError("row_topk: values / indices have the wrong size")
    check(_lib.lib().salun_row_topk(_dev(p, torch.float32, "p"), _dev(values, torch.float32, "values"),
                                    _dev(indices, torch.int64, "indices"), c_int64(B), K, int(k), _stream()),
          "salun_row_topk")
    return values.view(B, k), indices.view(B, k)


def decoded_to_u8(x: torch.Tensor, C: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x fp32 [B, Cp, H, W] in [-1, 1] -> uint8 [B, H, W, C] = round(clamp(x / 2 + 0.5, 0, 1) * 255) of its first C
    channels (default: all), half to even, NaN -> 0."""
    B, Cp, H, W = (int(v) for v in x.shape)
    C = Cp if C is None else int(C)
    if out is None:
        out = torch.empty((B, H, W, C), dtype=torch.uint8, device=x.device)
    elif out.numel() != B * H * W * C:
        raise ValueError("decoded_to_u8: out has the wrong size")
    check(_lib.lib().salun_decoded_to_u8(_dev(x, torch.float32, "x"), Cp, C, c_int64(H * W), c_int64(B),
                                         _dev(out, torch.uint8, "out"), _stream()), "salun_decoded_to_u8")
    return out.view(B, H, W, C)


def maxpool3x3s2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.max_pool2d(x, 3, 2, 1) of x [N, C, H, W] -> [N, C, (H+1)/2, (W+1)/2]."""
    N, C, H, W = (int(v) for v in x.shape)
    OH, OW = (H + 1) // 2, (W + 1) // 2
    if out is None:
        out = torch.empty((N, C, OH, OW), dtype=torch.float32, device=x.device)
    elif out.numel() != N * C * OH * OW:
        raise ValueError("maxpool3x3s2: out has the wrong size")
    check(_lib.lib().salun_maxpool3x3s2_forward(_dev(x, torch.float32, "x"), _dev(out, torch.float32, "out"),
                                                c_int64(N * C), H, W, _stream()), "salun_maxpool3x3s2_forward")
    return out.view(N, C, OH, OW)


def u8_norm_table(mean, std) -> torch.Tensor:
    """The 256 x C table of ((u / 255) - mean[c]) / std[c] in fp32 steps, as a HOST tensor [C, 256]."""
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    if m.ndim != 1 or m.shape != s.shape:
        raise ValueError("u8_norm_table: mean and std are two vectors of one length")
    table = np.empty((m.size, 256), np.float32)
    check(_lib.lib().salun_u8_norm_table(c_void_p(m.ctypes.data), c_void_p(s.ctypes.data), int(m.size),
                                         c_void_p(table.ctypes.data)), "salun_u8_norm_table")
    return torch.from_numpy(table)


def u8_to_chw_norm(src: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src uint8 [B, H, W, C], table fp32 [C, 256] on the device -> fp32 [B, C, H, W] = Normalize(ToTensor(src))."""
    B, H, W, C = (int(v) for v in src.shape)
    if tuple(table.shape) != (C, 256):
        raise ValueError(f"u8_to_chw_norm: table {tuple(table.shape)} must be ({C}, 256)")
    if out is None:
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=src.device)
    elif out.numel() != B * C * H * W:
        raise ValueError("u8_to_chw_norm: out has the wrong size")
    check(_lib.lib().salun_u8_to_chw_norm(_dev(src, torch.uint8, "src"), _dev(table, torch.float32, "table"),
                                          _dev(out, torch.float32, "out"), c_int64(B), H, W, C, _stream()),
          "salun_u8_to_chw_norm")
    return out.view(B, C, H, W)


def gn_split_slabs(C: int, HW: int, G: int, slab_vec4: int = 0) -> int:
    """Slabs per group of K28 for the shape (0 where it refuses it).  Host arithmetic only."""
    return int(_lib.lib().salun_gn_split_slabs(C, c_int64(HW), G, slab_vec4))


def gn_split_forward(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, silu: bool,
                     out: Optional[torch.Tensor] = None, slab_vec4: int = 0, want_stats: bool = False):
    """K28: [silu](group_norm(x)) of x [N, C, H, W] in two launches; `out` may be `x`.  -> y, or (y, mean, rstd)."""
    N, C = int(x.shape[0]), int(x.shape[1])
    HW = int(x.numel() // (N * C))
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape:
        raise ValueError("gn_split_forward: out has the wrong shape")
    L = _lib.lib()
    nbytes = int(L.salun_gn_split_workspace_bytes(N, C, c_int64(HW), int(groups), slab_vec4))
    ws = workspace(nbytes, x.device)
    stats = torch.empty(2 * N * int(groups), dtype=torch.float32, device=x.device)
    mean, rstd = stats[:N * int(groups)], stats[N * int(groups):]
    check(L.salun_gn_split_forward(_dev(x, torch.float32, "x"), _dev(out, torch.float32, "out"),
                                   _dev(gamma, torch.float32, "weight"), _dev(beta, torch.float32, "bias"),
                                   c_void_p(mean.data_ptr()), c_void_p(rstd.data_ptr()), N, C, c_int64(HW), int(groups),
                                   ctypes.c_double(eps), int(bool(silu)), slab_vec4, c_void_p(ws.data_ptr()),
                                   c_size_t(nbytes), _stream()), "salun_gn_split_forward")
    return (out, mean, rstd) if want_stats else out


def vae_posterior_sample(moments: torch.Tensor, zc: int, image_ids: Optional[torch.Tensor], seed: int, draw: int,
                         scale: float, deterministic: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """moments [B, Cm, h, w] (Cm >= 2 zc; further channels ignored) -> z [B, zc, h, w] =
    scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * e), e = ops_sampler.sampler_noise(image_ids, (zc, h, w), seed,
    step=draw); with `deterministic` scale * mean."""
    B, Cm, h, w = (int(v) for v in moments.shape)
    if out is None:
        out = torch.empty((B, zc, h, w), dtype=torch.float32, device=moments.device)
    elif out.numel() != B * zc * h * w:
        raise ValueError("vae_posterior_sample: out has the wrong size")
    check(_lib.lib().salun_vae_posterior_sample(_dev(moments, torch.float32, "moments"), Cm, int(zc), c_int64(h * w),
                                                c_int64(B), _dev(image_ids, torch.int64, "image_ids", bool(deterministic)),
                                                ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), c_int64(int(draw)),
                                                ctypes.c_double(scale), int(bool(deterministic)),
                                                _dev(out, torch.float32, "out"), _stream()),
          "salun_vae_posterior_sample")
    return out.view(B, zc, h, w)


class EvalMeters:
    """The device-side running sums of the evaluation head: no host synchronisation until `read()`."""

    def __init__(self, device):
        self.f = torch.zeros(2, dtype=torch.float64, device=device)   # entropy_sum, prob_sum
        self.i = torch.zeros(2, dtype=torch.int64, device=device)     # hits, count

    def read(self) -> dict:
        f, i = self.f.cpu(), self.i.cpu()
        return {"entropy_sum": float(f[0]), "prob_sum": float(f[1]), "hits": int(i[0]), "count": int(i[1])}


def cls_head_eval(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, label: int, meters: Optional[EvalMeters],
                  zero_safe: bool = False):
    """pool -> fc -> softmax of x [B, C, H, W]; adds the batch's entropy, p[:, label], hits and count to `meters`.
    -> (logits [B, K], p [B, K])."""
    B, C = int(x.shape[0]), int(x.shape[1])
    HW = int(x.numel() // (B * C))
    K = int(weight.shape[0])
    L = _lib.lib()
    logits = torch.empty((B, K), dtype=torch.float32, device=x.device)
    p = torch.empty((B, K), dtype=torch.float32, device=x.device)
    nbytes = L.salun_cls_head_eval_workspace_bytes(c_int64(B), C, K)
    ws = workspace(nbytes, x.device, "cls_eval")
    f = c_void_p(meters.f.data_ptr()) if meters is not None else c_void_p(None)
    f1 = c_void_p(meters.f.data_ptr() + 8) if meters is not None else c_void_p(None)
    i0 = c_void_p(meters.i.data_ptr()) if meters is not None else c_void_p(None)
    i1 = c_void_p(meters.i.data_ptr() + 8) if meters is not None else c_void_p(None)
    check(L.salun_cls_head_eval(_dev(x, torch.float32, "x"), _dev(weight, torch.float32, "weight"),
                                _dev(bias, torch.float32, "bias"), int(label), c_void_p(logits.data_ptr()),
                                c_void_p(p.data_ptr()), f, f1, i0, i1, c_int64(B), C, HW, K, int(bool(zero_safe)),
                                c_void_p(ws.data_ptr()), c_size_t(ws.numel()), _stream()), "salun_cls_head_eval")
    return logits, p
