"""Packed weight images for the LDS-DMA ring convolution (csrc/salun_conv_ring.hip, K8r): the lookup by address.

`conv.use_salun_convs(model)` registers the weight of every 3x3 / stride 1 / pad 1 convolution here; `images(w)` then
hands `ops.conv2d_forward` / `ops.conv2d_backward_data` the forward and backward-data images of that weight.  When an
image is stale, and how ALL stale images of the `register()` group are re-packed in ONE launch, is weightimg.py's
business; what is this module's own comes from being asked by ADDRESS (the convolution wrappers see a tensor, not a
module): only registered parameters are served — a cache keyed by address alone would hand a freed-and-reused address a
stale image — and a parameter that a flat arena re-homed after registration is found at its new address.
"""
from __future__ import annotations

import ctypes
import weakref
from typing import Optional

import torch

from . import _lib, weightimg
from .streams import _stream, _stream_handle


def _alloc(p: torch.Tensor):
    K, C = p.shape[0], p.shape[1]
    return tuple(torch.empty(int(_lib.lib().salun_conv3x3_pack_bytes(K, C, dgrad)) // 4, dtype=torch.float32, device=p.device)
                 for dgrad in (0, 1))


def _pack(jobs) -> int:
    arr = (_lib.PackJob * len(jobs))(*jobs)
    _lib.check(_lib.lib().salun_conv3x3_pack_weights(ctypes.cast(arr, ctypes.c_void_p), len(jobs), _stream()),
               "salun_conv3x3_pack_weights")
    return (len(jobs) + 31) // 32


_KIND = weightimg.Kind(_alloc, lambda p, buf: _lib.PackJob(p.data_ptr(), buf[0].data_ptr(), buf[1].data_ptr(),
                                                           p.shape[0], p.shape[1]))
_all: list[weightimg.Image] = []           # every registered weight
_by_ptr: dict[int, weightimg.Image] = {}   # current address -> image (rebuilt when a lookup misses: FlatArena re-homes parameters)
_not_ours: set[int] = set()                # addresses looked up and found unregistered since the last rebuild
ENABLED = [True]       # tools / tests: A/B switch
PACK_LAUNCHES = weightimg.RING_LAUNCHES


def eligible(K: int, C: int, R: int, stride: int, pad: int) -> bool:
    return R == 3 and stride == 1 and pad == 1 and C % 8 == 0 and K % 8 == 0


def register(params) -> Optional[weightimg.Registry]:
    """Register the OIHW [K, C, 3, 3] weights `params` (nn.Parameters that outlive their use) as one pack group: packed
    together whatever device each is on, and — a ring image may be read on another stream than the one that packed it —
    with the stream and an event of the last pack remembered (`images`)."""
    g = weightimg.Registry(lambda jobs: _pack(jobs), PACK_LAUNCHES, per_device=False, ordered=True)
    known = {id(e.param()) for e in _all if e.param() is not None}
    for p in params:
        if not (p.dtype == torch.float32 and p.dim() == 4):   # (the device is looked at when an image is asked for)
            continue
        K, C, R, _ = p.shape
        if not eligible(K, C, R, 1, 1) or p.shape[3] != 3 or id(p) in known:
            continue
        _all.append(weightimg.Image(_KIND, g, weakref.ref(p)))
        known.add(id(p))
    _rebuild()
    return g if g.images else None


def _rebuild() -> None:
    """File every live weight under its current address."""
    _by_ptr.clear()
    _not_ours.clear()
    live = []
    for e in _all:
        p = e.param()
        if p is None:
            continue
        if e.key != weightimg.key(p):   # re-homed (a flat arena was built after registration) or rewritten: its images
            e.key = None                # are stale, and no later key may compare equal to the one they were packed from
        _by_ptr[p.data_ptr()] = e
        live.append(e)
    _all[:] = live


def _lookup(w: torch.Tensor) -> Optional[weightimg.Image]:
    ptr = w.data_ptr()
    e = _by_ptr.get(ptr)
    p = e.param() if e is not None else None
    if p is None or p.data_ptr() != ptr:   # an address not seen before, or one whose parameter died or moved: never
        if e is None and ptr in _not_ours:  # serve the old address again
            return None
        _rebuild()
        e = _by_ptr.get(ptr)
        if e is None:
            _not_ours.add(ptr)
            return None
        p = e.param()
    return e if w.shape == p.shape else None


def images(w: torch.Tensor):
    """(forward image, backward-data image) of a registered weight, current with the parameters; None if `w` is not
    registered (the caller then runs conv_igemm on the OIHW tensor itself)."""
    if not ENABLED[0]:
        return None
    e = _lookup(w)
    if e is None or not w.is_cuda:
        return None
    imgs = weightimg.image(e, e.param())
    g = e.reg
    if g.stream != _stream_handle():
        # packed on another stream (the no-grad target pass of the diffusion steps runs beside the forget pass)
        torch.cuda.current_stream().wait_event(g.event)
    return imgs
