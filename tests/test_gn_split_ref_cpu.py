"""The slab arithmetic of K28's mirror (gn_split_ref_cpu.py) against brute force, and against the library's own host-only
queries (salun_gn_split_slabs, salun_gn_split_workspace_bytes touch no device).  No GPU."""
import itertools
from ctypes import c_int64

import pytest

import gn_split_ref_cpu as R

SHAPES = [(C, G, HW) for C, G in ((8, 2), (32, 32), (12, 3), (128, 32), (512, 32), (5, 5), (6, 4))
          for HW in (4, 6, 16, 36, 64, 100, 4096, 16384)]
SLABS = (0, 1, 3, 5, 7, 9, 2048, 4096)


def brute_slabs(nvec, slab):
    """Walk the float4s of a group one by one: a new slab starts every `slab` of them."""
    out, lo = [], 0
    for e in range(nvec):
        if e - lo == slab:
            out.append((lo, e))
            lo = e
    return out + [(lo, nvec)]


def test_slabs_and_boundaries_against_brute_force():
    for (C, G, HW), slab in itertools.product(SHAPES, SLABS):
        if not R.ok(1, C, HW, G, slab):
            assert R.slabs(C, HW, G, slab) == 0 and R.ws_bytes(3, C, HW, G, slab) == 0
            assert C % G or HW % 4, (C, G, HW)
            continue
        nvec = C // G * HW // 4
        want = brute_slabs(nvec, slab or R.AUTO_SLAB)
        assert R.boundaries(C, HW, G, slab) == want
        assert R.slabs(C, HW, G, slab) == len(want)
        # disjoint, in order, covering the group; every slab but the last is full
        assert want[0][0] == 0 and want[-1][1] == nvec and all(a[1] == b[0] for a, b in zip(want, want[1:]))
        assert all(hi - lo == (slab or R.AUTO_SLAB) for lo, hi in want[:-1]) and 0 < want[-1][1] - want[-1][0]
        for N in (1, 3):
            assert R.ws_bytes(N, C, HW, G, slab) == 16 * N * G * len(want)     # one pair of doubles per workgroup


def test_slab_count_depends_on_the_group_size_only():
    for slab in SLABS:
        assert R.slabs(128, 4096, 32, slab) == R.slabs(4, 4096, 1, slab) == R.slabs(8, 2048, 1, slab)


def test_the_automatic_slab_gives_every_cu_a_workgroup_at_the_encoder_shapes():
    for C, side in R.VAE_SHAPES:
        assert 1 * 32 * R.slabs(C, side * side, 32) >= R.CUS, (C, side)
    assert 32 * R.slabs(512, 64 * 64, 32) == R.CUS          # the smallest map: exactly one each


def test_domain():
    assert R.ok(1, 8, 4, 2) and R.ok(2, 12, 36, 3) and R.ok(1, 8, 512 * 512, 2)
    for N, C, HW, G, slab in ((0, 8, 16, 2, 0), (1, 8, 16, 0, 0), (1, 8, 16, 3, 0), (1, 8, 6, 2, 0), (1, 8, 2, 2, 0),
                              (1, 8, 0, 2, 0), (1, 8, 16, 2, -1), (1, 2, 1 << 30, 1, 0), (1 << 21, 64, 64, 64, 1)):
        assert not R.ok(N, C, HW, G, slab), (N, C, HW, G, slab)


def test_the_cases_cover_what_they_say():
    by = {R.case_id(c): c for c in R.CASES}
    assert R.slabs(8, 16, 2, 0) == 1
    b = R.boundaries(8, 16, 2, 3)
    assert len(b) == 6 and b[-1] == (15, 16) and any(lo % 4 for lo, _ in b)        # ragged; inside a channel (hw4 = 4)
    assert R.slabs(32, 64, 32, 5) == 4                                             # cpg = 1: 16 float4s
    assert R.slabs(12, 36, 3, 0) == 1 and R.slabs(12, 36, 3, 7) == 6
    assert R.slabs(8, 512 * 512, 2, 0) == 128
    assert len(by) == len(R.CASES)


@pytest.fixture(scope="module")
def lib():
    from unlearn_saliency_amd import _lib
    _lib.build()
    return _lib.lib()


def test_the_library_queries_agree(lib):
    from unlearn_saliency_amd import _lib
    assert _lib.SALUN_GN_SPLIT_FLUSH == R.FLUSH
    for (C, G, HW), slab in itertools.product(SHAPES, SLABS):
        assert lib.salun_gn_split_slabs(C, c_int64(HW), G, slab) == R.slabs(C, HW, G, slab), (C, G, HW, slab)
        for N in (1, 3):
            assert lib.salun_gn_split_workspace_bytes(N, C, c_int64(HW), G, slab) == R.ws_bytes(N, C, HW, G, slab)
    assert lib.salun_gn_split_slabs(8, c_int64(16), 2, -1) == 0
    assert lib.salun_gn_split_workspace_bytes(0, 8, c_int64(16), 2, 0) == 0
    assert lib.salun_gn_split_slabs(2, c_int64(1 << 30), 1, 0) == 0               # cpg * HW = 2^31
    assert lib.salun_gn_split_workspace_bytes(1 << 21, 64, c_int64(64), 64, 1) == 0   # N G S past 2^31
