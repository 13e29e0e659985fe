"""Derived images of the fp32 master weights, and the one rule that decides when such an image is stale.

Two kernel families read an image of a weight instead of the weight: the fp32 LDS-DMA ring convolutions (ringpack.py:
forward and backward-data images, looked up by address) and the bf16 convolutions / Linear layers (conv_bf16.py).  A
stale image is silent — forward and backward-data run on last step's weights and the loss still goes down — so what
decides staleness is written here, once: the parameter epoch (`params_written`), the key an image was packed from
(`key`), the registry in which the first stale image asked for re-packs every stale one in one job table (`image`),
and the launch counters.  An image kind supplies only what differs (`Kind`, and its registry's `pack` call); this
module knows no kernel and does not import `ops`.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import torch

from .streams import _stream_handle

# Bumped by every kernel that rewrites parameters through raw pointers (the fused optimizer steps, the proximal step, the
# IU / Fisher-forgetting updates).  `ops.PARAM_EPOCH` is this list; the package itself only calls params_written().
PARAM_EPOCH = [0]


def params_written() -> None:
    """Parameters were (or are about to be) rewritten through raw pointers: every weight image is stale."""
    PARAM_EPOCH[0] += 1


def key(p: torch.Tensor) -> tuple:
    """What an image of `p` is current with.  The epoch: raw-pointer writes.  `p._version`: torch writes on the parameter
    itself.  The address: a re-homed parameter (a flat arena built later, `.to(device)`).  The flat arena's version:
    torch writes on `arena.params`, or any slice of it, do NOT bump the parameter's own counter — `p.data = view` gave
    it a separate one (flat.py).  A parameter marked `_salun_frozen` (SD/ldm_lite.py: frozen_copy) is in no optimizer's
    arena, so no raw-pointer write reaches it: its key leaves the epoch out, and the steps taken on ANOTHER model do not
    re-pack its images.  Parameters without the marker keep the key above exactly."""
    flat = getattr(p, "_salun_flat", None)
    epoch = -1 if getattr(p, "_salun_frozen", False) else PARAM_EPOCH[0]
    return (epoch, p._version, p.data_ptr(), flat._version if flat is not None else -1)


# Launches of the pack kernels so far, per image kind (tests, host profile).  The bf16 one is also the "did anything get
# packed since I looked" signal of SD/train_scripts.forget_and_target (`ops.PACK_CALLS` is the same list).
RING_LAUNCHES = [0]
BF16_LAUNCHES = [0]


class Kind(NamedTuple):
    alloc: Callable                    # alloc(p) -> the image's buffer(s), uninitialised, on p.device
    job: Callable                      # job(p, buf) -> this image's entry of the registry's pack table
    alone: Optional[Callable] = None   # alone(p, buf) -> buf, written by a launch of its own (None: no such form)


class Registry:
    """Images that are re-packed together.  `pack(jobs) -> launches` issues one job table on the current stream.
    `per_device`: a batch takes the stale images on the requesting weight's device (else: on any GPU).  `ordered`: remember
    the stream and an event of the last pack, for consumers on other streams — asked for by the ring kind only: the bf16
    images are ordered by forget_and_target's fall-back to the main stream, and an event record per batch would be a
    device call they do not make today.  `batching[0]` false: every image packs alone, where its kind can."""

    def __init__(self, pack: Callable, launches: list, per_device: bool, ordered: bool = False, batching=(True,)):
        self.pack, self.launches, self.per_device, self.ordered, self.batching = pack, launches, per_device, ordered, batching
        self.images: list = []   # registration order = order of use in a forward pass = order of the jobs in a batch
        self.stream, self.event = 0, None


class Image:
    """One image of one weight.  `param()` -> the weight, or None once its owner is gone (it must not keep it alive);
    `registered` false: known to nobody but its owner, packs alone."""
    __slots__ = ("kind", "reg", "param", "registered", "key", "buf", "device")

    def __init__(self, kind: Kind, reg: Registry, param: Callable, registered: bool = True):
        self.kind, self.reg, self.param, self.registered = kind, reg, param, registered
        self.key = self.buf = self.device = None
        if registered:
            reg.images.append(self)


def image(img: Image, p: torch.Tensor):
    """The buffer(s) of `img`, current with its weight `p`.  A hit — every call but the first after the weights changed,
    several hundred per SD step on a host-bound step — is this frame and key(): no registry walk."""
    if img.key == key(p) and img.device == p.device:
        return img.buf
    return _repack(img, p)


def _repack(img: Image, p: torch.Tensor):
    """`img` is stale: write it — together with every other stale image of its registry, unless it packs alone."""
    reg = img.reg
    batch = (img.registered and reg.batching[0]) or img.kind.alone is None
    if batch:
        todo, live = [], []   # todo: (image, weight, key) of everything this call writes
        for i in reg.images:
            q = i.param()
            if q is None:
                continue
            live.append(i)
            if (q.device != p.device) if reg.per_device else (not q.is_cuda):
                continue
            k = key(q)
            if i.key != k or i.device != q.device:
                todo.append((i, q, k))
        if len(live) != len(reg.images):
            reg.images[:] = live
    else:
        todo = [(img, p, key(p))]
    for i, q, _ in todo:
        if i.device != q.device:   # buffers are reused across re-packs; a new one only on a device change
            i.buf, i.device = i.kind.alloc(q), q.device
    if batch:
        reg.launches[0] += reg.pack([i.kind.job(q, i.buf) for i, q, _ in todo])
    else:
        img.buf = img.kind.alone(p, img.buf)
        reg.launches[0] += 1
    for i, _, k in todo:   # (only now: a failed launch leaves them stale)
        i.key = k
    if reg.ordered:
        reg.stream = _stream_handle()
        if reg.event is None:
            reg.event = torch.cuda.Event()
        reg.event.record()
    return img.buf
