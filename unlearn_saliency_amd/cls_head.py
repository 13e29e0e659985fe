"""Host side of K23 (csrc/salun_cls_head.hip): the classifier head of the CIFAR ResNets as one autograd node.

  fused_cls_head(x4d, fc, target, meters=None)   (mean cross-entropy, logits.detach()) from layer4's [B, C, H, W] output:
                                                 average pool -> fc -> log-softmax -> NLL -> argmax == target in ONE
                                                 forward launch and two backward launches (reference: ResNet.py:317-320
                                                 + CrossEntropyLoss + utils.accuracy, about a dozen library launches)
  HeadMeters(device)                             the running loss sum / hit count / sample count of an epoch ON the
                                                 device; the kernel adds to them, `read()` is the only host sync
  use_fused_head(model)                          switches a model's `forward_loss(x, target, meters)` to K23;
                                                 `model(x)` is unchanged

The backward honours the incoming scalar gradient (loss sign, data-parallel shard scale) and adds the fc gradients
straight into the flat arena when `gradsink.dest` says they can go there, exactly as `gemm._Linear.backward` does.
fp32 device tensors only: anything else is an error, not a fall-back.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, gradsink, ops
from ._lib import c_int, c_int64, c_size_t, c_void_p, check
from .fastfn import FastFunction


def _ptr(t: Optional[torch.Tensor]) -> c_void_p:
    return c_void_p(t.data_ptr() if t is not None else None)


class HeadMeters:
    """loss_sum (float64), hits (int64), count (int64): one 3 x 8-byte device block that K23 adds to."""

    def __init__(self, device: torch.device):
        self.block = torch.zeros(3, dtype=torch.int64, device=device)
        self.loss_sum = self.block[0:1].view(torch.float64)
        self.hits = self.block[1:2]
        self.count = self.block[2:3]

    def reset(self) -> None:
        self.block.zero_()

    @torch.no_grad()
    def add_library(self, loss: torch.Tensor, output: torch.Tensor, target: torch.Tensor) -> None:
        """The same three sums from a library head's outputs (the `--library_conv` path), still without a host sync."""
        n = output.shape[0]
        self.loss_sum += loss.detach().double() * n
        self.hits += (output.detach().argmax(dim=1) == target).sum()
        self.count += n

    def read(self) -> Tuple[float, float, int]:
        """-> (mean loss, top-1 in percent, samples); synchronises the host."""
        raw = self.block.cpu()
        n = int(raw[2])
        if n == 0:
            return 0.0, 0.0, 0
        return float(raw[0:1].view(torch.float64)) / n, float(raw[1]) * 100.0 / n, n


def _check_inputs(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], target: torch.Tensor) -> None:
    if x.dim() != 4 or not x.is_cuda or x.dtype != torch.float32:
        raise TypeError(f"fused_cls_head: expected an fp32 device tensor [B, C, H, W], got {x.dtype} {tuple(x.shape)} on "
                        f"{x.device} (no CPU fallback)")
    if bias is None or weight.dtype != torch.float32 or not weight.is_cuda or weight.dim() != 2:
        raise TypeError("fused_cls_head: the classifier must be an fp32 device nn.Linear with a bias")
    B, C = x.shape[0], x.shape[1]
    K = weight.shape[0]
    if weight.shape[1] != C or target.shape != (B,):
        raise ValueError(f"fused_cls_head: x {tuple(x.shape)}, weight {tuple(weight.shape)}, target {tuple(target.shape)}")
    if B < 1 or C > _lib.SALUN_CLS_HEAD_MAX_C or K > _lib.SALUN_CLS_HEAD_MAX_K:
        raise ValueError(f"fused_cls_head: B = {B}, C = {C}, K = {K} outside K23's domain (C <= "
                         f"{_lib.SALUN_CLS_HEAD_MAX_C}, K <= {_lib.SALUN_CLS_HEAD_MAX_K})")


def head_forward(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, target: torch.Tensor,
                 meters: Optional[HeadMeters] = None):
    """One `salun_cls_head_forward` call -> pooled [B, C], logits [B, K], p [B, K], loss [B], loss_mean [1]."""
    B, C, H, W = x.shape
    K = weight.shape[0]
    dev = x.device
    pooled = torch.empty((B, C), dtype=torch.float32, device=dev)
    logits = torch.empty((B, K), dtype=torch.float32, device=dev)
    p = torch.empty((B, K), dtype=torch.float32, device=dev)
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    mean = torch.empty(1, dtype=torch.float32, device=dev)
    L = _lib.lib()
    nbytes = L.salun_cls_head_workspace_bytes(c_int64(B), C, K)
    ws = ops.workspace(nbytes, dev, "cls_head")
    check(L.salun_cls_head_forward(_ptr(x), _ptr(weight), _ptr(bias), _ptr(target), _ptr(pooled), _ptr(logits), _ptr(p),
                                   _ptr(loss), _ptr(mean), _ptr(meters.loss_sum if meters else None),
                                   _ptr(meters.hits if meters else None), _ptr(meters.count if meters else None),
                                   c_int64(B), C, H * W, K, _ptr(ws), c_size_t(ws.numel()),
                                   c_void_p(torch.cuda.current_stream().cuda_stream)), "salun_cls_head_forward")
    return pooled, logits, p, loss, mean


def head_backward(p: torch.Tensor, pooled: torch.Tensor, weight: torch.Tensor, target: torch.Tensor,
                  grad_out: Optional[torch.Tensor], HW: int, dx: Optional[torch.Tensor], dw: Optional[torch.Tensor],
                  db: Optional[torch.Tensor], accumulate_w: bool = False, accumulate_b: bool = False) -> torch.Tensor:
    """One `salun_cls_head_backward` call; returns dlogits [B, K]."""
    B, K = p.shape
    C = pooled.shape[1]
    dlogits = torch.empty_like(p)
    check(_lib.lib().salun_cls_head_backward(_ptr(p), _ptr(pooled), _ptr(weight), _ptr(target), _ptr(grad_out),
                                             _ptr(dlogits), _ptr(dx), _ptr(dw), _ptr(db), int(bool(accumulate_w)),
                                             int(bool(accumulate_b)), c_int64(B), C, HW, K,
                                             c_void_p(torch.cuda.current_stream().cuda_stream)),
          "salun_cls_head_backward")
    return dlogits


_NO_GRAD = gradsink.Dest(None, False)  # a parameter that needs no gradient: the kernel skips it, autograd gets None


class _ClsHead(FastFunction):
    @staticmethod
    def forward(ctx, x, weight, bias, target, meters):
        pooled, logits, p, _, mean = head_forward(x, weight, bias, target, meters)
        ctx.save_for_backward(p, pooled, weight, target)
        ctx.params = (weight, bias)  # the Parameter objects (gradient destinations)
        ctx.xshape = x.shape
        ctx.mark_non_differentiable(logits)
        return mean.view(()), logits

    @staticmethod
    def backward(ctx, gloss, _glogits):
        p, pooled, weight, target = ctx.saved_tensors
        B, C, H, W = ctx.xshape
        g = gloss.detach().reshape(1)
        if g.dtype != torch.float32 or not g.is_cuda:
            g = g.to(device=p.device, dtype=torch.float32)
        dx = torch.empty(ctx.xshape, dtype=torch.float32, device=p.device) if ctx.needs_input_grad[0] else None
        dw = gradsink.dest(ctx.params[0], torch.empty) if ctx.needs_input_grad[1] else _NO_GRAD
        db = gradsink.dest(ctx.params[1], torch.empty) if ctx.needs_input_grad[2] else _NO_GRAD
        head_backward(p, pooled, weight, target, g, H * W, dx, dw.out, db.out, dw.accumulate, db.accumulate)
        return dx, dw.returned(), db.returned(), None, None


def fused_cls_head(x4d: torch.Tensor, fc: nn.Linear, target: torch.Tensor, meters: Optional[HeadMeters] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean cross-entropy of fc(avgpool(x4d)) against `target`, the logits detached).  `meters`, when given, receives
    the batch's loss sum, hits and sample count on the device."""
    _check_inputs(x4d, fc.weight, fc.bias, target)
    if torch.is_autocast_enabled():
        raise RuntimeError("fused_cls_head is fp32: call it outside autocast regions")
    if not x4d.is_contiguous():
        x4d = x4d.contiguous()
    if target.dtype != torch.int64 or not target.is_cuda or not target.is_contiguous():
        target = target.to(device=x4d.device, dtype=torch.int64).contiguous()
    return _ClsHead.apply(x4d, fc.weight, fc.bias, target, meters)


def library_head_loss(model: nn.Module, x: torch.Tensor, target: torch.Tensor, meters: Optional[HeadMeters] = None,
                      criterion=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The same pair from the model's own forward and the library's cross-entropy (`--library_conv`, models without
    a fused head)."""
    output = model(x)
    loss = criterion(output, target) if criterion is not None else F.cross_entropy(output, target)
    if meters is not None:
        meters.add_library(loss, output, target)
    return loss, output.detach()


def head_parts(model: nn.Module):
    """(function x -> the [B, C, H, W] input of the model's average pool, its last nn.Linear), or None.  Two layouts:
    a `features(x)` method with an `fc` layer (ResNetCifar), and an nn.Sequential named `features` behind the model's
    `normalize` layer with a `classifier` layer (VGG); a model of the second kind may bring its own `feature_maps(x)`
    (VGG's runs the fused BN / K24 path when that is switched on)."""
    feats = getattr(model, "features", None)
    if isinstance(feats, nn.Module):
        linear = getattr(model, "classifier", None)
        maps = getattr(model, "feature_maps", None)
        if maps is None:
            norm = getattr(model, "normalize", None)
            maps = feats if norm is None else (lambda x: feats(norm(x)))
    else:
        linear, maps = getattr(model, "fc", None), feats
    return (maps, linear) if callable(maps) and isinstance(linear, nn.Linear) else None


def use_fused_head(model: nn.Module, flag: bool = True) -> nn.Module:
    """Route `model.forward_loss(x, target, meters)` through K23.  The model needs `features(x)` (the [B, C, H, W]
    input of its average pool) and an `fc` nn.Linear, as ResNetCifar has, or a `features` nn.Sequential and a
    `classifier` nn.Linear, as VGG has."""
    if flag and head_parts(model) is None:
        raise TypeError(f"use_fused_head: {type(model).__name__} has no features() / fc pair")
    model.fused_head = bool(flag)
    return model


def forward_loss(model: nn.Module, x: torch.Tensor, target: torch.Tensor, meters: Optional[HeadMeters] = None,
                 criterion=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss, logits.detach()) of one batch: K23 when `use_fused_head(model)` was called, else the library head."""
    if getattr(model, "fused_head", False):
        maps, linear = head_parts(model)
        return fused_cls_head(maps(x), linear, target, meters)
    return library_head_loss(model, x, target, meters, criterion)
