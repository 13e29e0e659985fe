"""K22 (csrc/salun_prune.hip) on the GPU against torch.nn.utils.prune on CPU tensors and the host restatement
tests/prune_ref_cpu.py.  Two arenas: n_sel = 3315 (the select's full-scan route) and n_sel = 40179 (its single-read
route); segment offsets are neither multiples of 4 elements nor 16-byte aligned, and the elements between the segments
hold the smallest magnitudes of the arena.  Every comparison is exact: masks, counts and bit patterns."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import prune_ref_cpu as PR

pytestmark = pytest.mark.gpu

ARENAS = {"small": PR.SMALL, "large": PR.LARGE}
FULL_SCAN = 1  # SALUN_TOPK_FORCE_FULL_SCAN


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Dev:
    """An arena on the device with its host mirror."""

    def __init__(self, lengths, seed=0, p=None):
        self.n, self.segs, self.p0, self.buf0 = PR.distinct_arena(lengths, seed)
        if p is not None:
            self.p0 = p
        self.n_sel = sum(k for _, k in self.segs)
        self.idx = PR.seg_index(self.segs)
        self.p = torch.from_numpy(self.p0.copy()).cuda()
        self.buf = torch.from_numpy(self.buf0.copy()).cuda()
        self.keep = torch.ones(self.n, dtype=torch.uint8, device="cuda")
        self.table = torch.tensor(self.segs, dtype=torch.int64, device="cuda")
        self.alive = self.n_sel

    def round(self, k, rnd=None, flags=0):
        from unlearn_saliency_amd import ops
        ops.prune_global(self.p, self.buf, self.keep, self.table, self.n_sel, self.alive, k, rnd=rnd, flags=flags)
        self.alive -= k

    def host(self):
        return self.p.cpu().numpy(), self.buf.cpu().numpy(), self.keep.cpu().numpy()


def _check_against(dev, keep_want, p_before, buf_before):
    """keep as wanted; p, buf zero exactly at the pruned positions; every other bit as before."""
    p, buf, keep = dev.host()
    assert np.array_equal(keep, keep_want)
    gone = keep_want == 0
    assert np.all(_bits(p)[gone] == 0) and np.all(_bits(buf)[gone] == 0)
    assert np.array_equal(_bits(p)[~gone], _bits(p_before)[~gone])
    assert np.array_equal(_bits(buf)[~gone], _bits(buf_before)[~gone])


@pytest.mark.parametrize("flags", [0, FULL_SCAN])
@pytest.mark.parametrize("arena", ["small", "large"])
def test_three_rounds_match_torch_prune(arena, flags):
    from unlearn_saliency_amd import ops
    dev = Dev(ARENAS[arena])
    ref = PR.TorchPruned(dev.p0, dev.segs)
    for r in range(3):
        k = ops.prune_amount(0.2, dev.alive)
        dev.round(k, flags=flags)
        route, err = ops.prune_status(dev.p.device, dev.n_sel)
        assert err == 0 and route == (1 if arena == "large" and not flags else 2)
        ref.round(0.2)
        want = np.ones(dev.n, np.uint8)
        want[dev.idx] = ref.mask()
        _check_against(dev, want, dev.p0, dev.buf0)
        assert dev.alive == ref.remaining() == int(want[dev.idx].sum())
    assert dev.alive == dev.n_sel - sum(PR.prune_amount(0.2, a) for a in _alive_chain(dev.n_sel, 0.2, 3))


def _alive_chain(n, amount, rounds):
    out = []
    for _ in range(rounds):
        out.append(n)
        n -= PR.prune_amount(amount, n)
    return out


@pytest.mark.parametrize("arena", ["small", "large"])
def test_amount_zero_and_prune_everything(arena):
    dev = Dev(ARENAS[arena], seed=1)
    dev.round(0)
    p, buf, keep = dev.host()
    assert np.array_equal(_bits(p), _bits(dev.p0)) and np.array_equal(_bits(buf), _bits(dev.buf0)) and keep.all()
    dev.round(PR.prune_amount(0.3, dev.alive))
    dev.round(dev.alive)                       # k_prune == R
    assert dev.alive == 0
    want = np.ones(dev.n, np.uint8)
    want[dev.idx] = 0
    _check_against(dev, want, dev.p0, dev.buf0)


@pytest.mark.parametrize("arena", ["small", "large"])
def test_heavy_ties_at_the_threshold(arena):
    """Quantised magnitudes (about 13 distinct values): exact count, every pruned |p| <= every kept |p|, and among the
    elements AT the threshold magnitude the pruned ones are the highest flat indices."""
    n, segs = PR.layout(ARENAS[arena])
    rng = np.random.default_rng(5)
    p0 = (np.round(rng.standard_normal(n) * 2.0) / 2.0 + 0.25).astype(np.float32)   # never 0
    dev = Dev(ARENAS[arena], seed=5, p=p0)
    hp, hbuf, hkeep = p0.copy(), dev.buf0.copy(), np.ones(n, np.uint8)
    for r in range(2):
        k = PR.prune_amount(0.37, dev.alive)
        before = hkeep.copy()
        dev.round(k)
        PR.prune_round(hp, hbuf, hkeep, segs, k)
        p, buf, keep = dev.host()
        idx = dev.idx
        new = (before[idx] == 1) & (keep[idx] == 0)
        kept = keep[idx] == 1
        assert int(new.sum()) == k and int(kept.sum()) == dev.alive
        mags = np.abs(p0[idx])
        tau = mags[new].max()
        assert tau <= mags[kept].min()
        tie = mags == tau
        if (tie & kept).any():
            assert idx[tie & new].min() > idx[tie & kept].max()
        assert np.array_equal(keep, hkeep) and np.array_equal(_bits(p), _bits(hp)) and np.array_equal(_bits(buf), _bits(hbuf))


@pytest.mark.parametrize("arena", ["small", "large"])
def test_kept_exact_zero_is_not_taken_for_pruned(arena):
    """Some weights already pruned, one KEPT weight exactly 0.0: the next round ranks that zero as the smallest alive
    magnitude (k = 1 takes exactly it), no pruned weight returns and the counts stay exact."""
    dev = Dev(ARENAS[arena], seed=2)
    hp, hbuf, hkeep = dev.p0.copy(), dev.buf0.copy(), np.ones(dev.n, np.uint8)
    k = PR.prune_amount(0.25, dev.alive)
    dev.round(k)
    PR.prune_round(hp, hbuf, hkeep, dev.segs, k)
    z = int(dev.idx[hkeep[dev.idx] == 1][7])            # a kept weight
    dev.p[z] = 0.0
    hp[z] = 0.0
    dev.round(1)
    assert dev.keep[z].item() == 0 and int(dev.keep.sum().item()) == dev.n - k - 1
    PR.prune_round(hp, hbuf, hkeep, dev.segs, 1)
    z2 = int(dev.idx[hkeep[dev.idx] == 1][11])
    dev.p[z2] = -0.0
    hp[z2] = -0.0
    k3 = PR.prune_amount(0.2, dev.alive)
    dev.round(k3)
    PR.prune_round(hp, hbuf, hkeep, dev.segs, k3)
    p, buf, keep = dev.host()
    assert np.array_equal(keep, hkeep) and int(keep[dev.idx].sum()) == dev.alive == dev.n_sel - k - 1 - k3
    assert keep[z2] == 0 and np.array_equal(_bits(p), _bits(hp)) and np.array_equal(_bits(buf), _bits(hbuf))


def test_fused_steps_leave_pruned_weights_at_zero_and_count_matches():
    from unlearn_saliency_amd import ops
    dev = Dev(PR.LARGE, seed=3)
    dev.round(PR.prune_amount(0.4, dev.alive))
    gone = dev.keep == 0
    rng = np.random.default_rng(9)
    for s in range(3):
        g = torch.from_numpy(rng.standard_normal(dev.n).astype(np.float32) + 0.5).cuda()
        ops.masked_sgd_step(dev.p, g, dev.buf, dev.keep, 0.1, 0.9, 5e-4, s == 0)
    p, buf, _ = dev.host()
    gone = gone.cpu().numpy()
    assert np.all(_bits(p)[gone] == 0) and np.all(_bits(buf)[gone] == 0)
    assert not np.array_equal(p[~gone], dev.p0[~gone])
    count = ops.prune_count_zeros(dev.p, dev.table, dev.n_sel)
    assert count.dtype == torch.int64 and int(count.item()) == int((p[dev.idx] == 0).sum()) == int(gone.sum())
    dev.p[dev.idx[5]] = -0.0                        # torch.sum(w == 0) counts a negative zero too
    dev.p[3] = 0.0                                  # outside the segments: not counted
    w = dev.p.cpu()[torch.from_numpy(dev.idx)]
    assert int(ops.prune_count_zeros(dev.p, dev.table, dev.n_sel).item()) == int(torch.sum(w == 0))


def test_a_bad_segment_table_changes_nothing():
    from unlearn_saliency_amd import ops
    dev = Dev(PR.SMALL, seed=4)
    bad = dev.table.clone()
    bad[1, 0] = bad[0, 0] + 3                       # overlaps segment 0: not ascending-disjoint
    with pytest.raises(ops.TopkFailed):
        ops.prune_global(dev.p, dev.buf, dev.keep, bad, dev.n_sel, dev.alive, 100)
    p, buf, keep = dev.host()
    assert np.array_equal(_bits(p), _bits(dev.p0)) and np.array_equal(_bits(buf), _bits(dev.buf0)) and keep.all()
    assert int(ops.prune_count_zeros(dev.p, bad, dev.n_sel).item()) == -1


def _random_round(dev, amount, key):
    from unlearn_saliency_amd import ops
    before = dev.keep.clone()
    k = PR.prune_amount(amount, dev.alive)
    rnd = ops.fill_uniform(dev.n_sel, key)
    dev.round(k, rnd=rnd)
    return before, k, rnd


def test_random_variant():
    """Exact count, only alive segment elements cleared, the same keys give the same set and other keys another; the
    host restatement on the same keys gives the same mask.  On the large arena at amount 0.5 each segment of >= 2000
    elements loses 0.5 +- 0.06 of its weights: for the smallest such segment (2307) sigma = 0.5 / sqrt(2307) = 0.0104,
    so the bound is more than 5 sigma."""
    a = Dev(PR.LARGE, seed=6)
    a.round(PR.prune_amount(0.1, a.alive))          # some weights are already gone
    b = Dev(PR.LARGE, seed=6)
    b.round(PR.prune_amount(0.1, b.alive))
    c = Dev(PR.LARGE, seed=6)
    c.round(PR.prune_amount(0.1, c.alive))
    hp, hbuf, hkeep = a.host()
    before, k, rnd = _random_round(a, 0.5, key=(2 << 40))
    _random_round(b, 0.5, key=(2 << 40))
    _random_round(c, 0.5, key=(2 << 40) + (1 << 34))
    p, buf, keep = a.host()
    before = before.cpu().numpy()
    new = (before == 1) & (keep == 0)
    assert int(new.sum()) == k and not new[np.setdiff1d(np.arange(a.n), a.idx)].any()
    assert np.all(keep <= before)
    assert torch.equal(a.keep, b.keep) and torch.equal(a.p, b.p)
    assert not torch.equal(a.keep, c.keep) and int(c.keep.sum().item()) == int(a.keep.sum().item())
    PR.prune_round(hp, hbuf, hkeep, a.segs, k, keys=rnd.cpu().numpy())
    assert np.array_equal(keep, hkeep) and np.array_equal(_bits(p), _bits(hp)) and np.array_equal(_bits(buf), _bits(hbuf))
    for o, ln in a.segs:
        if ln >= 2000:
            alive_before = int(before[o:o + ln].sum())
            frac = int(new[o:o + ln].sum()) / alive_before
            assert abs(frac - 0.5) <= 0.06, (ln, frac)


class _Ring(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(64, 64, 3, padding=1, bias=False)
        self.bn = nn.BatchNorm2d(64)

    def forward(self, x):
        return self.bn(self.conv(x))


def test_pruning_invalidates_the_packed_weight_images():
    """A 64 -> 64 3x3 layer on an 8x8 map at batch 256 runs on the ring kernels, which read a packed image of the
    weight: after a pruning round the forward must equal the forward of a freshly built model with the same zeroed
    weights, bit for bit, and the model-level API must agree with torch's count of zeros."""
    from unlearn_saliency_amd import ringpack
    from unlearn_saliency_amd.Classification import pruner
    from unlearn_saliency_amd.conv import use_salun_convs
    torch.manual_seed(0)
    net = _Ring().cuda().eval()
    use_salun_convs(net)
    x = torch.randn(256, 64, 8, 8, device="cuda")
    assert pruner.check_sparsity(net) is None      # (builds the arena: the weights are re-homed before the first pack)
    with torch.no_grad():
        y0 = net(x)
    n0 = ringpack.PACK_LAUNCHES[0]
    pruner.pruning_model(net, 0.5)
    with torch.no_grad():
        y1 = net(x)
    assert ringpack.PACK_LAUNCHES[0] == n0 + 1, "the round bumps the parameter epoch: the image is packed again"
    w = net.conv.weight.detach()
    assert int((w == 0).sum()) == 64 * 64 * 9 // 2 and pruner.check_sparsity(net) == 50.0
    sd = net.state_dict()
    assert "conv.weight" not in sd and torch.equal(sd["conv.weight_orig"], w)
    assert torch.equal(sd["conv.weight_mask"], (w != 0).float())
    fresh = _Ring().cuda().eval()
    fresh.load_state_dict({"conv.weight": w.clone(), **{k: v for k, v in sd.items() if k.startswith("bn.")}})
    use_salun_convs(fresh)
    with torch.no_grad():
        y2 = fresh(x)
    assert torch.equal(y1, y2) and not torch.equal(y1, y0)
    # a pruned checkpoint loads into a fresh model the way the reference resumes: masks first, then the state dict
    again = _Ring().cuda().eval()
    use_salun_convs(again)
    pruner.prune_model_custom(again, pruner.extract_mask(sd))
    again.load_state_dict(sd)
    assert pruner.prune_state(again).alive == 64 * 64 * 9 // 2
    with torch.no_grad():
        assert torch.equal(again(x), y1)
    pruner.remove_prune(again)
    assert "conv.weight" in again.state_dict() and pruner.prune_state(again) is None
