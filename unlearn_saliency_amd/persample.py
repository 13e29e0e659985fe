"""Per-sample gradient inner products from one batched backward ("ghost" dots).

`persample_dots(model, x, y, u0, u1)` returns, for every sample i of the batch, the two inner products

    out[i, 0] = <g_i, u0>,   out[i, 1] = <g_i, u1>,   g_i = d CE(model(x_i), y_i) / d theta   (eval mode)

for two flat tangents u0, u1 laid out like the model's FlatArena (named_parameters() order), in fp64 — without
ever forming a per-sample gradient.  In eval mode no layer couples the samples of a batch, so g_i restricted to a
layer's weights is the outer-product form of that layer's input x_i and output gradient dy_i, and its inner
product with a tangent slice U is a per-sample reduction over the layer's output:

    Conv2d       <dW l_i, U> + <db l_i, u_b> = <dy_i, conv(x_i, U) + u_b>       (same stride / padding)
    BatchNorm2d  sum_c U_gamma[c] sum_pq dy_i x^_i + U_beta[c] sum_pq dy_i       (x^ from the running statistics)
    Linear       sum_m dy_i[m] (U x_i + u_b)[m]

The forward captures each parameterised module's input and (through a tensor hook) its output gradient; one
backward of the summed loss w.r.t. the activations only (parameters are detached for the pass, so no weight
gradient is computed and `.grad` is not touched) yields every dy_i.  The two tangents of a convolution go through
ONE convolution on the package's kernels (`ops.conv2d_forward` with the stacked weight [U_0; U_1]), and the dots are
the K17 reductions of csrc/salun_iu.hip.  Any other module type that holds parameters is refused.

`fisher_diag(model, x, num_classes, F_acc)` reuses the same capture for Fisher forgetting: the
class-weighted squared batch gradients of all classes from one pass over the activations, squared per layer by the K18
kernels of csrc/salun_ff.hip.  `_capture` holds what both share (hooks, detached parameters, `_Fusion`, restoring the
mode and `requires_grad` flags).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, ops_ff, ops_iu
from .flat import arena_of


def _conv_supported(mod: nn.Conv2d) -> bool:
    from .conv import _eligible
    return _eligible(mod)


def _kind(mod: nn.Module) -> str:
    if isinstance(mod, nn.Conv2d):
        if not _conv_supported(mod):
            raise NotImplementedError(f"persample: {mod} is outside the convolution kernels' domain "
                                      "(square 1x1 / 3x3, stride 1 or 2, dilation 1, one group, zero padding, fp32)")
        return "conv"
    if isinstance(mod, nn.Linear):
        return "linear"
    if type(mod) is nn.BatchNorm2d:
        if not (mod.affine and mod.track_running_stats and mod.running_mean is not None):
            raise NotImplementedError(f"persample: {mod} needs affine parameters and running statistics")
        return "bn"
    raise NotImplementedError(f"persample: module type {type(mod).__name__} holds parameters and has no per-sample "
                              "dot (supported: Conv2d, Linear, BatchNorm2d in eval mode)")


class _Fusion:
    """Turns off this package's fused ResNet paths (`fused_block`, `fused_bn`) so that every conv / BN / Linear is a
    module call the hooks see; restores the flags on exit."""

    def __init__(self, model: nn.Module):
        self.saved = [(m, a, getattr(m, a)) for m in model.modules() for a in ("fused_block", "fused_bn")
                      if hasattr(m, a)]

    def __enter__(self):
        for m, a, _ in self.saved:
            setattr(m, a, False)
        return self

    def __exit__(self, *exc):
        for m, a, v in self.saved:
            setattr(m, a, v)


def _param_modules(model: nn.Module) -> list:
    return [(mod, _kind(mod)) for mod in model.modules() if any(True for _ in mod.parameters(recurse=False))]


def _capture(model: nn.Module, x: torch.Tensor, loss_fn, n_backward: int = 1):
    """Runs `model(x)` in eval mode with the package's fused ResNet paths off and the parameters detached, and
    backpropagates `loss_fn(logits, k)` for k < n_backward w.r.t. the activations only (no weight gradient is formed and
    `.grad` is not touched).  Returns (records, logits): one record [module, kind, input, output, [dy of each backward],
    input version] per call of a parameterised module, in call order.  The model's mode, fusion flags and
    `requires_grad` flags are as before afterwards.  The output slot is cleared on return."""
    mods = _param_modules(model)
    records: List[list] = []
    leaves: List[list] = []
    handles = []

    def fwd_hook(mod, inp, output, kind):
        rec = [mod, kind, inp[0].detach(), None, [], inp[0]._version]
        records.append(rec)
        if not output.requires_grad:  # nothing upstream needs a gradient: the activation graph starts here
            output = output.detach().requires_grad_(True)
            leaves.append(rec)
        else:
            # a hook registered before any in-place op on `output` (the ResNet's ReLU(inplace=True)) receives the
            # gradient w.r.t. the value the module produced
            output.register_hook(lambda g, r=rec: r[4].append(g))
        rec[3] = output
        return output

    modes = [(m, m.training) for m in model.modules()]
    grads = [(p, p.requires_grad) for p in model.parameters()]
    try:
        with _Fusion(model):
            model.eval()
            for p, _ in grads:
                p.requires_grad_(False)
            for mod, kind in mods:
                handles.append(mod.register_forward_hook(lambda m, i, o, k=kind: fwd_hook(m, i, o, k)))
            with torch.enable_grad():
                logits = model(x)
                for k in range(n_backward):
                    got = torch.autograd.grad(loss_fn(logits, k), [r[3] for r in leaves], allow_unused=True,
                                              retain_graph=k + 1 < n_backward)
                    for r, g in zip(leaves, got):
                        if g is not None:
                            r[4].append(g)
    finally:
        for h in handles:
            h.remove()
        for p, rg in grads:
            p.requires_grad_(rg)
        for m, t in modes:
            m.training = t
        for r in records:  # record -> output -> tensor hook -> record is a cycle the garbage collector cannot see
            r[3] = None    # through autograd: without this cut every call leaks its activations and graph
    return records, logits.detach()


def _slicer(arena):
    where = {id(p): (o, k) for p, o, k in zip(arena._params, arena.offsets, arena.numels)}

    def sl(u: torch.Tensor, p: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        if p is None:
            return None
        o, k = where[id(p)]
        return u[o:o + k].view(p.shape)
    return sl


def persample_dots(model: nn.Module, x: torch.Tensor, y: torch.Tensor, u0: torch.Tensor, u1: torch.Tensor,
                   out: Optional[torch.Tensor] = None, arena=None) -> torch.Tensor:
    """(B, 2) fp64 device tensor of <g_i, u0>, <g_i, u1> for the per-sample cross-entropy gradients g_i in eval mode.
    `out`, if given, is added into.  The model's mode, fusion flags, running statistics, `num_batches_tracked`,
    `requires_grad` flags and `.grad` are as before afterwards."""
    arena = arena if arena is not None else arena_of(model)
    B = x.shape[0]
    if out is None:
        out = torch.zeros((B, 2), dtype=torch.float64, device=arena.device)
    elif tuple(out.shape) != (B, 2) or out.dtype != torch.float64:
        raise ValueError(f"out must be a ({B}, 2) fp64 tensor")
    if B == 0:
        return out
    for u, nm in ((u0, "u0"), (u1, "u1")):
        if u.numel() != arena.n or u.dtype != torch.float32 or not u.is_contiguous():
            raise ValueError(f"{nm} must be a contiguous fp32 flat vector of {arena.n} elements (the arena layout)")
    sl = _slicer(arena)
    # sum: each sample's own (batch-1) gradient
    records, _ = _capture(model, x, lambda logits, k: F.cross_entropy(logits, y, reduction="sum"))

    stacked: Dict[int, tuple] = {}
    for mod, kind, xin, _, dys, ver in records:
        if not dys:  # the module's output does not reach the loss
            continue
        if xin._version != ver:
            raise RuntimeError(f"persample: the input of {mod} was modified in place after the module ran")
        dy = dys[0].contiguous()
        w, b = mod.weight, getattr(mod, "bias", None)
        if kind == "bn":
            ops_iu.bn_dot(xin.contiguous(), dy, mod.running_mean, mod.running_var, mod.eps, sl(u0, w), sl(u0, b),
                          sl(u1, w), sl(u1, b), out)
            continue
        if kind == "linear":
            if xin.dim() != 2:
                raise NotImplementedError(f"persample: Linear input of shape {tuple(xin.shape)} (only (B, K))")
            ops_iu.linear_dot(xin.contiguous(), dy, sl(u0, w), sl(u0, b), sl(u1, w), sl(u1, b), out)
            continue
        if id(mod) not in stacked:
            w2 = torch.cat([sl(u0, w), sl(u1, w)], 0).contiguous()
            b2 = torch.cat([sl(u0, b), sl(u1, b)], 0).contiguous() if b is not None else None
            stacked[id(mod)] = (w2, b2)
        w2, b2 = stacked[id(mod)]
        P, Q = dy.shape[2], dy.shape[3]
        y2 = ops.conv2d_forward(xin.contiguous(), w2, b2, mod.stride[0], mod.padding[0], P, Q)
        if y2 is None:
            # outside the convolution kernels' domain (an RGB input with a bias: VGG's first layer): the library
            # convolution, counted like every other one (conv.LIBRARY_CONV_CALLS; an error under conv.strict)
            from .conv import _fallback
            _fallback("shape", f"persample tangent convolution {tuple(xin.shape)} * {tuple(w2.shape)}")
            y2 = F.conv2d(xin, w2, b2, mod.stride[0], mod.padding[0]).contiguous()
        ops_iu.conv_dot(y2, dy, out)
    return out


FISHER_FORMS = ("replicate", "loop")


def fisher_diag(model: nn.Module, x: torch.Tensor, num_classes: int, F_acc: torch.Tensor, arena=None,
                form: str = "replicate") -> torch.Tensor:
    """F_acc += sum_y mean_i(prob[i, y]) * grad_y^2 for one batch (the inner loop of the reference's `hessian`,
    Classification/unlearn/fisher.py:50-78), grad_y = d CE_mean(model(x), y) / d theta in eval mode, prob =
    softmax(model(x)); fp32, arena layout.  All `num_classes` class tangents come from one pass over the activations
    (DESIGN.md §9c), and the K18 kernels square each complete class gradient per layer without forming it as a flat
    vector:

      form="replicate"  the batch repeated once per class along the batch axis, loss = sum_y CE_mean(copy y, y), ONE
                        backward (eval mode: every copy has the same activations, so copy 0's input serves all);
      form="loop"       one forward, then one backward per class over the retained graph.

    The model's mode, fusion flags, running statistics, `requires_grad` flags and `.grad` are as before afterwards."""
    arena = arena if arena is not None else arena_of(model)
    if F_acc.numel() != arena.n or F_acc.dtype != torch.float32 or not F_acc.is_contiguous():
        raise ValueError(f"F_acc must be a contiguous fp32 flat vector of {arena.n} elements (the arena layout)")
    if x.shape[0] == 0:
        return F_acc
    records, w = _fisher_capture(model, x, num_classes, form)
    _fisher_square(records, w, x.shape[0], F_acc, _slicer(arena))
    return F_acc


def _fisher_capture(model: nn.Module, x: torch.Tensor, num_classes: int, form: str = "replicate", loss_hook=None):
    """The activation pass of `fisher_diag`: (records whose dy stacks the C class groups, class weights w (C,)).
    `loss_hook`, if given, is called between the forward and the backward (tools/ff_bench.py times the two)."""
    if form not in FISHER_FORMS:
        raise ValueError(f"form must be one of {FISHER_FORMS}")
    B, C = x.shape[0], int(num_classes)

    def hooked(loss_fn):
        def f(lg, k):
            if k == 0 and loss_hook is not None:
                loss_hook()
            return loss_fn(lg, k)
        return f

    if form == "replicate":
        xr = x.unsqueeze(0).expand(C, *x.shape).reshape(C * B, *x.shape[1:])
        yr = torch.arange(C, device=x.device).repeat_interleave(B)
        records, logits = _capture(model, xr, hooked(lambda lg, k: F.cross_entropy(lg, yr, reduction="sum") / B))
        logits = logits[:B]
    else:
        cls = lambda lg, k: F.cross_entropy(lg, torch.full((B,), k, dtype=torch.int64, device=lg.device))
        records, logits = _capture(model, x, hooked(cls), C)
    if logits.shape[1] != C:
        raise ValueError(f"fisher_diag: the model has {logits.shape[1]} outputs, num_classes is {C}")
    w = torch.softmax(logits, dim=-1).mean(0).contiguous()  # mean_i prob[i, y] of each class group
    return records, w


def _fisher_square(records: list, w: torch.Tensor, B: int, F_acc: torch.Tensor, sl) -> None:
    """The K18 part of `fisher_diag`: F_acc += sum_y w_y g_y^2, layer by layer from the captured x and grouped dy."""
    for mod, kind, xin, _, dys, ver in records:
        if not dys:  # the module's output does not reach the loss
            continue
        if xin._version != ver:
            raise RuntimeError(f"fisher_diag: the input of {mod} was modified in place after the module ran")
        dy = (dys[0] if len(dys) == 1 else torch.cat(dys, 0)).contiguous()
        x0 = xin[:B].contiguous()
        wt, b = mod.weight, getattr(mod, "bias", None)
        if kind == "bn":
            ops_ff.vec_sq(dy, w, sl(F_acc, b), B, x0, mod.running_mean, mod.running_var, mod.eps, sl(F_acc, wt))
            continue
        if kind == "linear":
            if xin.dim() != 2:
                raise NotImplementedError(f"fisher_diag: Linear input of shape {tuple(xin.shape)} (only (B, K))")
            ops_ff.linear_sq(x0, dy, w, sl(F_acc, wt))
        else:
            try:
                ops_ff.conv_sq(x0, dy, w, sl(F_acc, wt), mod.stride[0], mod.padding[0])
            except NotImplementedError:
                # outside the backward-weight kernels' domain (2x2 feature maps: VGG's last block): one library
                # backward-weight per class group, counted like every other one (conv.LIBRARY_CONV_CALLS)
                from .conv import _fallback
                _fallback("backward", f"fisher_diag backward-weight {tuple(x0.shape)} * {tuple(wt.shape)}")
                Fw = sl(F_acc, wt)
                for g in range(w.numel()):
                    s = torch.nn.grad.conv2d_weight(x0, wt.shape, dy[g * B:(g + 1) * B], mod.stride, mod.padding)
                    Fw.add_(w[g] * s * s)
        if b is not None:
            ops_ff.vec_sq(dy, w, sl(F_acc, b), B)
