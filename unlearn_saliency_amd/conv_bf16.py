"""`nn.Conv2d` on the bf16 MFMA convolution kernels (csrc/salun_conv_bf16.hip, K11) — the convolution path of the
Stable-Diffusion U-Net in its bf16 configuration (BASELINE.json configs[4]; reference: autocast over the `conv_nd`
modules of SD/ldm/modules/diffusionmodules/openaimodel.py and SD/ldm/modules/attention.py:230-247).

`use_salun_convs_bf16(model)` re-classes every eligible `nn.Conv2d` in place (parameters, names, state_dict untouched:
the fp32 master weights stay views of the flat arena).  Such a module

  * takes any 4-D device tensor, views it as bf16 NHWC (`channels_last` — a no-op for tensors these modules produced),
  * reads a bf16 image of its weight that is re-packed only when the master weights changed (weightimg.py: the
    parameter epoch the fused optimizer kernels bump, torch's version counters, the parameter's address),
  * returns a bf16 `channels_last` tensor (logical NCHW shape, so the surrounding model code is unchanged),
  * in backward writes dX in bf16 and adds dW / db in fp32 straight into the parameters' `.grad` views (gradsink.py).

Shapes outside the kernels' domain (C or K not a multiple of 32: the 4-channel latent head and tail of the U-Net)
run on the fp32 MFMA kernels of conv.py; nothing here calls the library convolution.
"""
from __future__ import annotations

import os
import weakref as _weakref

import torch

from .fastfn import FastFunction
import torch.nn as nn

from . import gradsink, ops, weightimg, wgrad_side
from .conv import SalunConv2d, _eligible


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """Logical NCHW tensor -> contiguous [N, H, W, C] bf16 view/copy."""
    return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)


def _can_overlap() -> bool:
    """Weight / bias gradients that go straight into `.grad` (gradsink) are consumed by nothing before the end of the
    backward pass: they are issued on the backward-weight side stream (wgrad_side.beside), next to the input-gradient
    kernels of this and the following layers — at batch 8 most of the SD U-Net's kernels leave CUs idle."""
    return wgrad_side.OVERLAP and not torch.cuda.is_current_stream_capturing()


def _weight_bias_grad(mod, has_bias, xn, dyn, wshape, s, p, dnb=None):
    """ONE backward-weight call for dW, db and (`dnb`, fp32 [N, K]) the per-image channel sums of dy, over NHWC bf16 views
    (a Linear layer's tokens included); returns (dw, db) as autograd gets them: None for what was added into `.grad`."""
    to_w = gradsink.dest(mod.weight)
    # the kernel has ONE accumulate flag for dw and db: without a weight sink it overwrites both outputs, so the bias
    # gradient must not target bias.grad then (it would be overwritten, not accumulated) — it goes through autograd
    # like dw; with a weight sink but no bias sink, db accumulates into fresh zeros
    to_b = gradsink.dest(mod.bias, torch.zeros, when=to_w.accumulate) if has_bias else None
    all_in_grad = to_w.accumulate and (to_b is None or to_b.accumulate)
    bias_out = to_b.out if has_bias else None
    if all_in_grad and _can_overlap():
        # everything the backward-weight call writes lands in .grad storage: side stream; dnb is read by autograd on THIS
        # stream right away, so its (small) sums are a launch of their own here
        if dnb is not None:
            ops.colsum_bf16(dyn, dyn.shape[0], nbias_out=dnb)
        wgrad_side.beside(dyn.device, (xn, dyn), lambda side: ops.conv2d_bf16_backward_weight(
            xn, dyn, wshape, s, p, out=to_w.out, accumulate=True, bias_out=bias_out, stream=side))
        return None, None
    got = ops.conv2d_bf16_backward_weight(xn, dyn, wshape, s, p, out=to_w.out, accumulate=to_w.accumulate,
                                          bias_out=bias_out, nbias_out=dnb)
    return to_w.returned(got), (to_b.returned() if has_bias else None)


class _ConvBF16Fn(FastFunction):
    @staticmethod
    def forward(ctx, x, w, bias, mod, nbias, addend):
        R, s, p = mod.kernel_size[0], mod.stride[0], mod.padding[0]
        xn = _nhwc(x)
        wp = mod.packed_weight()
        an = _nhwc(addend) if addend is not None else None
        y = ops.conv2d_bf16_forward(xn, wp, R, s, p, bias=bias, nbias=nbias, addend=an)
        ctx.save_for_backward(xn)  # (the weight is reached through `mod`: no saved-tensor hook for it, norm._FusedGN16)
        ctx.w_shape = tuple(w.shape)
        ctx.mod, ctx.has_bias, ctx.x_dtype = mod, bias is not None, x.dtype
        ctx.nbias, ctx.addend_dtype = nbias is not None, (addend.dtype if addend is not None else None)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy):
        xn, = ctx.saved_tensors
        mod, wshape = ctx.mod, ctx.w_shape
        R, s, p = mod.kernel_size[0], mod.stride[0], mod.padding[0]
        dyn = _nhwc(dy)
        dx = dw = db = dnb = dadd = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            if ctx.nbias and ctx.needs_input_grad[4] and dyn.shape[0] <= 128:
                # per-image channel sums of dy out of the bias gradient's partial sums (one kernel pair for both)
                dnb = torch.empty((dyn.shape[0], wshape[0]), dtype=torch.float32, device=dyn.device)
            dw, db = _weight_bias_grad(mod, ctx.has_bias, xn, dyn, wshape, s, p, dnb)
        if ctx.needs_input_grad[0]:
            dx = ops.conv2d_bf16_backward_data(dyn, mod.packed_weight(), tuple(xn.shape), R, s, p).permute(0, 3, 1, 2)
            if dx.dtype != ctx.x_dtype:
                dx = dx.to(ctx.x_dtype)
        if ctx.nbias and ctx.needs_input_grad[4] and dnb is None:  # (frozen weights: no backward-weight launch to ride on)
            dnb = dyn.float().sum(dim=(1, 2))
        if ctx.addend_dtype is not None and ctx.needs_input_grad[5]:
            dadd = dy if dy.dtype == ctx.addend_dtype else dy.to(ctx.addend_dtype)
        return dx, dw, db, None, dnb, dadd


# ------------------------------------------------------------------------------------------- weight images
# After an optimizer step EVERY bf16 weight image of a model is stale.  One pack launch per layer at its first use was
# 256 launches of ~13 us per SD step (round 5 profile: 1.4 % of the device time, most launches far too small to fill the
# chip); the images of the modules `use_salun_convs_bf16` / `use_salun_linears_bf16` re-classed are therefore REGISTERED
# (weightimg.py: the staleness rule and the batch), and the first stale one any of them asks for re-packs all stale
# images of that device in ceil(n / 64) launches (csrc: k_pack_jobs).  A module that was never registered (built by hand
# in a test) packs alone, as before.  No event orders a pack against other streams: SD/train_scripts.forget_and_target
# watches PACK_LAUNCHES instead and keeps the target pass on the main stream when the forget pass packed anything.
BATCH_PACKS = [os.environ.get("SALUN_BF16_BATCH_PACK", "1") != "0"]  # A/B switch: False = one launch per image at its first use
PACK_LAUNCHES = weightimg.BF16_LAUNCHES
# (the ops.* seams are looked up per call: host tests replace them)
_IMAGES = weightimg.Registry(lambda jobs: ops.bf16_pack_batch(jobs), PACK_LAUNCHES, per_device=True, batching=BATCH_PACKS)


def _kcr(w):
    """(K, C, R) of a convolution's OIHW or a Linear layer's [K, C] weight."""
    return w.shape[0], w.shape[1], (w.shape[2] if w.dim() == 4 else 1)


def _alloc(w):
    K, C, R = _kcr(w)
    return torch.empty((K, R * R, C), dtype=torch.bfloat16, device=w.device)


def _alone(w, buf):
    K, C, R = _kcr(w)
    return ops.conv2d_bf16_pack(w.detach().view(K, C, R, R), buf)


# attribute of the module -> kind: the [K, R*R, C] image, and the transposed [C, K] one of a Linear layer
_KINDS = {
    "_img": weightimg.Kind(_alloc, lambda w, buf: (w.detach(), buf, *_kcr(w), False), _alone),
    "_img_t": weightimg.Kind(lambda w: torch.empty((w.shape[1], w.shape[0]), dtype=torch.bfloat16, device=w.device),
                             lambda w, buf: (w.detach(), buf, w.shape[0], w.shape[1], 1, True),
                             lambda w, buf: ops.pack_bf16(w.detach(), True, buf)),
}


def _slot(mod, attr: str, registered: bool = False) -> weightimg.Image:
    """The image `attr` of `mod`, made at its first use (re-classed modules never ran an __init__ of ours)."""
    img = weightimg.Image(_KINDS[attr], _IMAGES, lambda ref=_weakref.ref(mod): getattr(ref(), "weight", None), registered)
    setattr(mod, attr, img)
    return img


class SalunConv2dBF16(nn.Conv2d):
    """Same parameters / state_dict as nn.Conv2d; device tensors go through the bf16 MFMA kernels."""

    _img = None

    def packed_weight(self) -> torch.Tensor:
        return weightimg.image(self._img or _slot(self, "_img"), self.weight)

    def forward(self, x, nbias=None, addend=None):
        """`nbias` ([N, K] fp32, e.g. a ResBlock's time-embedding term) and `addend` (a tensor of the output's shape,
        e.g. the residual branch) are added in the kernel's epilogue."""
        if not x.is_cuda or x.dim() != 4:
            raise RuntimeError("SalunConv2dBF16 needs a 4-D device tensor (the HIP kernels have no CPU path)")
        return _ConvBF16Fn.apply(x, self.weight, self.bias, self, nbias, addend)


# ----------------------------------------------------------------------------------------------- Linear layers
# A Linear layer on a token tensor [.., M tokens, C] IS a 1x1 convolution over an NHWC image whose pixels are the
# tokens — the layout the K11 kernels already read — so the transformer blocks' projections (to_q / to_k / to_v /
# to_out, the GEGLU and output projections of the feed-forward; SD/ldm/modules/attention.py:37-75,168-247) run on
# conv_bf16_igemm / conv_bf16_wgrad instead of the library GEMM: the bf16 weight image is packed once per optimizer
# step (not cast on every forward, recompute and backward), the bias (and, where the caller passes one, the residual)
# rides in the epilogue, and dW / db are added in fp32 straight into the flat gradient (no bf16 gradient, no cast, no
# AccumulateGrad launch).
def _tokens_nhwc(t: torch.Tensor, C: int) -> torch.Tensor:
    """[..., C] -> contiguous bf16 [1, H, W, C] with H * W = number of tokens (W = 8 when it divides: the backward-weight
    kernel walks 8 x 8 pixel blocks)."""
    t = t.to(torch.bfloat16).contiguous()
    M = t.numel() // C
    return t.view(1, M // 8, 8, C) if M % 8 == 0 else t.view(1, M, 1, C)


# SALUN_LINEAR_GEMM=0: keep the Linear layers on the K11 1x1 convolution kernels (A/B switch)
_USE_K16 = [os.environ.get("SALUN_LINEAR_GEMM", "1") != "0"]


def _al16(t) -> bool:
    return t is None or t.data_ptr() % 16 == 0


class _LinearBF16Fn(FastFunction):
    """y = x W^T + b (+ addend) on bf16 tokens.  Forward and input gradient: K16 (csrc/salun_gemm.hip, direct-to-LDS
    GEMM on the [N, K] / [K, N] weight images) when the feature counts are multiples of 64, else the K11 1x1
    convolution kernels; weight / bias gradients: K11 backward-weight, added in fp32 into the flat gradient."""

    @staticmethod
    def forward(ctx, x, w, bias, mod, addend):
        K, C = w.shape
        x2 = x.to(torch.bfloat16).contiguous().view(-1, C)
        M = x2.shape[0]
        a2 = addend.to(torch.bfloat16).contiguous().view(-1, K) if addend is not None else None
        # K16 reads 16-byte vectors: bias / addend can be views at any 4-byte offset of the flat arena (an odd-sized
        # parameter ahead of them), in which case the K11 kernels, which take any alignment, serve the layer
        k16 = (_USE_K16[0] and ops.gemm_bf16_supported(M, K, C) and _al16(x2) and _al16(bias) and _al16(a2))
        if k16:
            y = ops.gemm_bf16_nt(x2, mod.packed_weight().view(K, C), bias, a2)
        else:
            xn = _tokens_nhwc(x2, C)
            an = _tokens_nhwc(a2, K) if a2 is not None else None
            y = ops.conv2d_bf16_forward(xn, mod.packed_weight(), 1, 1, 0, bias=bias, nbias=None, addend=an)
        ctx.save_for_backward(x2)
        ctx.w_shape = (K, C)
        ctx.mod, ctx.has_bias, ctx.x_shape, ctx.x_dtype = mod, bias is not None, tuple(x.shape), x.dtype
        ctx.addend_dtype = addend.dtype if addend is not None else None
        return y.view(*x.shape[:-1], K)

    @staticmethod
    def backward(ctx, dy):
        x2, = ctx.saved_tensors
        mod = ctx.mod
        K, C = ctx.w_shape
        M = x2.shape[0]
        dyn = _tokens_nhwc(dy, K)
        dx = dw = db = dadd = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = _weight_bias_grad(mod, ctx.has_bias, _tokens_nhwc(x2, C), dyn, (K, C, 1, 1), 1, 0)
            if dw is not None:
                dw = dw.view(K, C)
        if ctx.needs_input_grad[0]:
            dy2 = dyn.view(M, K)
            if _USE_K16[0] and ops.gemm_bf16_supported(M, C, K) and _al16(dy2):
                dx = ops.gemm_bf16_nt(dy2, mod.packed_weight_t()).view(ctx.x_shape)
            else:
                dx = ops.conv2d_bf16_backward_data(dyn, mod.packed_weight(), tuple(_tokens_nhwc(x2, C).shape), 1, 1, 0
                                                   ).view(ctx.x_shape)
            if dx.dtype != ctx.x_dtype:
                dx = dx.to(ctx.x_dtype)
        if ctx.addend_dtype is not None and ctx.needs_input_grad[4]:
            dadd = dy if dy.dtype == ctx.addend_dtype else dy.to(ctx.addend_dtype)
        return dx, dw, db, None, dadd


class SalunLinearBF16(nn.Linear):
    """Same parameters / state_dict as nn.Linear.  Device inputs in the bf16 configuration (a bf16 tensor, or any
    tensor under bf16 autocast) go through the bf16 MFMA kernels; anything else is the plain fp32 F.linear."""

    _img = None
    _img_t = None

    def packed_weight(self) -> torch.Tensor:
        """bf16 image [N, 1, K] (= [N, K]) of the master weights, re-packed once per optimizer step."""
        return weightimg.image(self._img or _slot(self, "_img"), self.weight)

    def packed_weight_t(self) -> torch.Tensor:
        """bf16 image [K, N] (the transposed weights the input-gradient GEMM reads)."""
        return weightimg.image(self._img_t or _slot(self, "_img_t"), self.weight)

    def forward(self, x, addend=None):
        """`addend` (a tensor of the output's shape, e.g. the residual branch) is added in the kernel's epilogue."""
        bf16_mode = x.is_cuda and (x.dtype == torch.bfloat16 or
                                   (torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16))
        if bf16_mode:
            return _LinearBF16Fn.apply(x, self.weight, self.bias, self, addend)
        y = torch.nn.functional.linear(x, self.weight, self.bias)
        return y if addend is None else y + addend


def use_salun_linears_bf16(model: nn.Module) -> int:
    """Re-class the nn.Linear layers of the transformer blocks (feature counts that are multiples of 32) in place;
    returns how many were switched.  The two tiny time-embedding Linears (M = batch rows) stay on the library."""
    from .SD.unet import BasicTransformerBlock
    n = 0
    for blk in model.modules():
        if not isinstance(blk, BasicTransformerBlock):
            continue
        for mod in blk.modules():
            if type(mod) is nn.Linear and mod.in_features % 32 == 0 and mod.out_features % 32 == 0 and \
                    ops.conv2d_bf16_supported(mod.in_features, mod.out_features, 1, 1, 0):
                mod.__class__ = SalunLinearBF16
                _slot(mod, "_img", True)
                _slot(mod, "_img_t", True)
                n += 1
    return n


class _Fp32Island(SalunConv2d):
    """The two 4-channel convolutions of the U-Net (latent head / tail) inside a bf16 model: fp32 MFMA kernels on an
    fp32 NCHW copy of the input; the result keeps fp32 (the head feeds GroupNorm, the tail is the model output)."""

    def forward(self, x):
        with torch.autocast("cuda", enabled=False):  # SalunConv2d refuses autocast regions; this island is fp32 by design
            y = super().forward(x.float().contiguous())
        if self.out_channels % 32 == 0:  # the head: its output feeds the bf16 NHWC network (and the skip concatenations)
            y = y.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        return y


def use_salun_convs_bf16(model: nn.Module) -> int:
    """Re-class eligible nn.Conv2d modules in place; returns how many run on the bf16 kernels."""
    n = 0
    for mod in model.modules():
        if type(mod) is not nn.Conv2d or not _eligible(mod):
            continue
        K, C = mod.out_channels, mod.in_channels
        R, s, p = mod.kernel_size[0], mod.stride[0], mod.padding[0]
        if C % 32 == 0 and K % 32 == 0 and ops.conv2d_bf16_supported(C, K, R, s, p):
            mod.__class__ = SalunConv2dBF16
            _slot(mod, "_img", True)
            n += 1
        else:
            mod.__class__ = _Fp32Island
    return n
