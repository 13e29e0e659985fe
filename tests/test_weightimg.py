"""weightimg.py on the host (no GPU): the one staleness key, and that BOTH image caches — the ring images looked up by
address (ringpack.py) and the bf16 images of the re-classed modules (conv_bf16.py) — go stale on each of the four
events that change a weight: a raw-pointer write (params_written), a torch write on the parameter, a torch write on
the flat arena it is a view of, and re-homing.  The pack launches are replaced by counters, as in test_sd_bf16_host.py."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params_written(mod, arena):
    from unlearn_saliency_amd import weightimg
    weightimg.params_written()


def _write_param(mod, arena):
    with torch.no_grad():
        mod.weight.mul_(2.0)


def _write_flat(mod, arena):
    v = mod.weight._version
    with torch.no_grad():
        arena.params.mul_(0.5)
    assert mod.weight._version == v     # the parameter's own counter does not see it


def _write_flat_slice(mod, arena):
    with torch.no_grad():
        arena.params[3:7].zero_()


def _rehome(mod, arena):
    old = mod.weight.data_ptr()
    mod.weight.data = mod.weight.data.clone()
    assert mod.weight.data_ptr() != old


EVENTS = [_params_written, _write_param, _write_flat, _write_flat_slice, _rehome]


@pytest.mark.parametrize("event", EVENTS, ids=lambda f: f.__name__.strip("_"))
def test_key_changes_on_each_event_and_on_nothing_else(event):
    from unlearn_saliency_amd import ops, weightimg
    from unlearn_saliency_amd.flat import FlatArena
    assert ops.PARAM_EPOCH is weightimg.PARAM_EPOCH and ops.PACK_CALLS is weightimg.BF16_LAUNCHES
    c = nn.Conv2d(16, 32, 3, padding=1)
    arena = FlatArena.from_module(c, device="cpu")
    k = weightimg.key(c.weight)
    assert k == (weightimg.PARAM_EPOCH[0], c.weight._version, c.weight.data_ptr(), arena.params._version)
    c(torch.zeros(1, 16, 4, 4)).sum().backward()            # reading the weight, a backward pass, a write on the bias,
    with torch.no_grad():                                    # a write on the gradients: not events
        c.bias.data.add_(1.0)
        arena.grads.zero_()
    assert weightimg.key(c.weight) == k
    event(c, arena)
    k2 = weightimg.key(c.weight)
    assert k2 != k and weightimg.key(c.weight) == k2
    # without an arena the last component is -1, and the old spelling of the epoch bump is the same event
    d = nn.Conv2d(16, 32, 3, padding=1)
    kd = weightimg.key(d.weight)
    assert kd[3] == -1
    ops.PARAM_EPOCH[0] += 1
    assert weightimg.key(d.weight) != kd


class _OnDevice(nn.Parameter):
    """A host parameter that says it is on the GPU (the ring cache serves device tensors only)."""
    is_cuda = property(lambda self: True)


class _Event:
    def record(self):
        pass


def _ring(monkeypatch, registered):
    from unlearn_saliency_amd import ringpack, weightimg
    packs = []
    monkeypatch.setattr(ringpack, "_pack", lambda jobs: packs.append(len(jobs)) or 1)
    for m in (ringpack, weightimg):
        monkeypatch.setattr(m, "_stream_handle", lambda: 0)
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    mod = nn.Conv2d(16, 32, 3, padding=1)
    mod.weight.__class__ = _OnDevice
    assert ringpack.register([mod.weight]) is not None
    return mod, lambda: ringpack.images(mod.weight), packs


def _bf16(make, fetch):
    def build(monkeypatch, registered):
        from unlearn_saliency_amd import conv_bf16, ops
        packs = []
        monkeypatch.setattr(ops, "conv2d_bf16_pack", lambda w, out=None: packs.append(1) or out)
        monkeypatch.setattr(ops, "pack_bf16", lambda w, transposed=False, out=None: packs.append(1) or out)
        monkeypatch.setattr(ops, "bf16_pack_batch", lambda jobs: packs.append(len(jobs)) or 1)
        mod = make()
        mod.__class__ = conv_bf16.SalunLinearBF16 if isinstance(mod, nn.Linear) else conv_bf16.SalunConv2dBF16
        if registered:
            conv_bf16._slot(mod, "_img", True)
            if isinstance(mod, nn.Linear):
                conv_bf16._slot(mod, "_img_t", True)
        return mod, lambda: fetch(mod), packs
    return build


CACHES = {
    "ring": _ring,
    "bf16_conv": _bf16(lambda: nn.Conv2d(32, 32, 3, padding=1), lambda m: m.packed_weight()),
    "bf16_linear": _bf16(lambda: nn.Linear(64, 32), lambda m: m.packed_weight()),
    "bf16_linear_t": _bf16(lambda: nn.Linear(64, 32), lambda m: m.packed_weight_t()),
}


@pytest.mark.parametrize("event", EVENTS, ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("cache,registered", [(c, r) for c in CACHES for r in (True, False) if r or c != "ring"],
                         ids=lambda v: v if isinstance(v, str) else "batch" if v else "alone")
def test_both_caches_go_stale_on_each_event(monkeypatch, cache, event, registered):
    """One pack at the first use, none while nothing happens, one after the event, none after that — and the image
    keeps its buffer.  (`registered`: the bf16 images of a re-classed model, packed as a batch, or of a module built by
    hand, packed alone; a ring image is always registered.)"""
    from unlearn_saliency_amd.flat import FlatArena
    mod, fetch, packs = CACHES[cache](monkeypatch, registered)
    arena = FlatArena.from_module(mod, device="cpu")      # re-homes the parameter AFTER registration
    first = fetch()
    assert first is not None and len(packs) == 1
    assert fetch() is first and len(packs) == 1
    event(mod, arena)
    again = fetch()
    assert len(packs) == 2, f"{cache}: stale image served after {event.__name__}"
    assert again is first or (isinstance(first, tuple) and all(a is b for a, b in zip(again, first)))
    assert fetch() is again and len(packs) == 2


def test_a_ring_group_repacks_together_and_remembers_who_packed(monkeypatch):
    """All stale images of one register() group are ONE job table; the group remembers the stream of that pack, so that
    a consumer on another stream waits on its event (ringpack.images) — which the bf16 registry does not ask for."""
    from unlearn_saliency_amd import conv_bf16, ringpack, weightimg
    tables, waits, now = [], [], [7]
    monkeypatch.setattr(ringpack, "_pack", lambda jobs: tables.append(len(jobs)) or 1)
    for m in (ringpack, weightimg):
        monkeypatch.setattr(m, "_stream_handle", lambda: now[0])
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: type("S", (), {"wait_event": lambda self, e: waits.append(e)})())
    a, b = nn.Conv2d(16, 32, 3, padding=1), nn.Conv2d(32, 32, 3, padding=1)
    for m in (a, b):
        m.weight.__class__ = _OnDevice
    g = ringpack.register([a.weight, b.weight])
    n0 = ringpack.PACK_LAUNCHES[0]
    ia = ringpack.images(a.weight)
    assert tables == [2] and ringpack.PACK_LAUNCHES[0] == n0 + 1 and g.stream == 7 and not waits
    assert ringpack.images(b.weight) is not None and tables == [2]
    now[0] = 9                                            # the same images asked for from another stream
    assert ringpack.images(a.weight) is ia and waits == [g.event] and tables == [2]
    weightimg.params_written()
    ringpack.images(b.weight)                             # re-packed on stream 9: nothing to wait for there
    assert tables == [2, 2] and g.stream == 9 and len(waits) == 1
    assert ringpack.PACK_LAUNCHES is weightimg.RING_LAUNCHES and conv_bf16.PACK_LAUNCHES is weightimg.BF16_LAUNCHES
    assert not conv_bf16._IMAGES.ordered and conv_bf16._IMAGES.event is None


def test_weightimg_does_not_import_ops():
    code = ("import sys; sys.modules['unlearn_saliency_amd.ops'] = None\n"
            "import unlearn_saliency_amd.weightimg as w\n"
            "w.params_written(); assert w.PARAM_EPOCH[0] == 1\n"
            "assert not [m for m in sys.modules if m.startswith('unlearn_saliency_amd.ops') and sys.modules[m] is not None]\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_only_weightimg_writes_the_epoch_and_the_pack_counters():
    pkg = os.path.join(ROOT, "unlearn_saliency_amd")
    bad = []
    for d, _, files in os.walk(pkg):
        for f in files:
            path = os.path.join(d, f)
            if f.endswith(".py") and path != os.path.join(pkg, "weightimg.py"):
                for i, line in enumerate(open(path, encoding="utf-8"), 1):
                    if re.search(r"(PARAM_EPOCH|PACK_CALLS)\[0\]\s*\+=", line):
                        bad.append(f"{path}:{i}")
    assert not bad, bad
