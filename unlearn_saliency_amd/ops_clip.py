"""Tensor-level wrappers of K29 (csrc/salun_clip_text.hip; include/salun.h): the four fp32 forward kernels of the CLIP
text encoder beside the K15 GEMM — embedding gather + add, LayerNorm, causal self-attention over a fused qkv buffer,
quick-GELU.

Same conventions as ops.py: device tensors only, raw pointers and the current stream handed to libsalun.so, a failing
call raises `SalunError`, nothing falls back to the library's ops.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib
from ._lib import c_int64, check
from .ops import _dev, _stream

ATTN_MAX_T = _lib.SALUN_CLIP_ATTN_MAX_T
ATTN_D = _lib.SALUN_CLIP_ATTN_D


def check_ids(ids: torch.Tensor, vocab: int) -> None:
    """The host-side validation `clip_embed` runs before it launches: an id outside [0, vocab) is a ValueError that names
    it."""
    if ids.dtype != torch.int64:
        raise TypeError(f"clip_embed: ids must be int64, got {ids.dtype}")
    if ids.numel():
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= vocab:
            raise ValueError(f"clip_embed: token id {hi if hi >= vocab else lo} is outside the vocabulary of {vocab} entries")


def clip_embed(ids: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x[b, t, :] = tok[ids[b, t], :] + pos[t, :].  ids: int64 [B, T] on the HOST (the tokenizer's output; validated
    here, then copied) or on the device (the caller has validated them with `check_ids`)."""
    B, T = (int(v) for v in ids.shape)
    V, W = (int(v) for v in tok.shape)
    if int(pos.shape[0]) < T or int(pos.shape[1]) != W:
        raise ValueError(f"clip_embed: {T} tokens of width {W} do not fit the position table {tuple(pos.shape)}")
    if not ids.is_cuda:
        check_ids(ids, V)
        ids = ids.to(tok.device)
    if out is None:
        out = torch.empty((B, T, W), dtype=torch.float32, device=tok.device)
    elif out.numel() != B * T * W:
        raise ValueError("clip_embed: out has the wrong size")
    check(_lib.lib().salun_clip_embed(_dev(ids, torch.int64, "ids"), _dev(tok, torch.float32, "tok"),
                                      _dev(pos, torch.float32, "pos"), _dev(out, torch.float32, "out"), c_int64(B), T, W,
                                      c_int64(V), _stream()), "salun_clip_embed")
    return out.view(B, T, W)


def ln_f32_forward(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm over the last dimension of a contiguous fp32 tensor."""
    W = int(x.shape[-1])
    rows = int(x.numel() // W)
    if int(gamma.numel()) != W or int(beta.numel()) != W:
        raise ValueError("ln_f32_forward: gamma and beta have the row's width")
    if out is None:
        out = torch.empty_like(x)
    elif out.numel() != x.numel():
        raise ValueError("ln_f32_forward: out has the wrong size")
    check(_lib.lib().salun_ln_f32_forward(_dev(x, torch.float32, "x"), _dev(gamma, torch.float32, "gamma"),
                                          _dev(beta, torch.float32, "beta"), _dev(out, torch.float32, "out"),
                                          c_int64(rows), W, ctypes.c_double(eps), _stream()), "salun_ln_f32_forward")
    return out


def attn_causal_f32(qkv: torch.Tensor, B: int, T: int, H: int, scale: float, out: Optional[torch.Tensor] = None,
                    D: int = ATTN_D) -> torch.Tensor:
    """softmax(scale q k^T + causal) v per (batch, head) of the fused projection buffer qkv [B T, 3 H D] (columns: q, k,
    v; a head's D channels contiguous) -> [B T, H D], heads concatenated.  One launch; no transposing copy."""
    W = H * D
    if tuple(qkv.shape) != (B * T, 3 * W):
        raise ValueError(f"attn_causal_f32: qkv {tuple(qkv.shape)} is not [{B * T}, {3 * W}]")
    if out is None:
        out = torch.empty((B * T, W), dtype=torch.float32, device=qkv.device)
    elif tuple(out.shape) != (B * T, W):
        raise ValueError("attn_causal_f32: out has the wrong shape")
    check(_lib.lib().salun_attn_causal_f32(_dev(qkv, torch.float32, "qkv"), _dev(out, torch.float32, "out"), B, H, T, D,
                                           c_int64(3 * W), 0, W, 2 * W, c_int64(W), ctypes.c_double(scale), _stream()),
          "salun_attn_causal_f32")
    return out


def quick_gelu_(x: torch.Tensor) -> torch.Tensor:
    """x * sigmoid(1.702 x), in place."""
    check(_lib.lib().salun_quick_gelu(_dev(x, torch.float32, "x"), c_int64(x.numel()), _stream()), "salun_quick_gelu")
    return x
