"""K26's host side, without a GPU: the coefficient tables libsalun.so computes in C doubles equal the numpy
restatement's integer for integer (the only floating-point part of the kernel), and the LDS query refuses what the
header says it refuses."""
import numpy as np
import pytest

import resample_ref_cpu as R


@pytest.fixture(scope="module")
def built():
    from unlearn_saliency_amd import _lib
    _lib.build()
    return _lib


PAIRS = sorted({(s[i], d[i]) for s, d in R.SIZES for i in (0, 1)} | {(1, 1), (1, 1024), (1024, 1), (1024, 1023),
                                                                   (1023, 1024), (224, 32), (64, 224), (50, 64), (70, 64)})


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_library_tables_equal_the_restatement(built, n_in, n_out):
    from unlearn_saliency_amd import ops_resample
    xmin, cnt, k = ops_resample.axis_table(n_in, n_out)
    rxmin, rcnt, rk = R.axis_table(n_in, n_out)
    assert np.array_equal(xmin, rxmin) and np.array_equal(cnt, rcnt)
    assert k.shape == rk.shape and np.array_equal(k, rk)
    assert (cnt >= 1).all() and (xmin + cnt <= n_in).all()
    assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + cnt) >= 0).all()  # what makes a band's rows contiguous


def test_lds_query_and_refusals(built):
    from unlearn_saliency_amd import ops_resample
    q = ops_resample.lds_bytes
    # 96 -> 64: 16 output rows read 24 source rows + 1 on either side at most
    assert 0 < q(96, 96, 3, 64, 64) <= 27 * 64 * 3
    assert 0 < q(32, 32, 3, 64, 64) <= built.SALUN_RESAMPLE_MAX_LDS
    assert q(1024, 1024, 4, 1024, 1024) > 0                     # same size: two taps per row, always fits
    assert q(1024, 1024, 4, 64, 1024) == 0                      # one output row reads 33 rows of 4096 bytes: refused
    assert q(1024, 64, 4, 1, 64) == 0 and q(1024, 16, 4, 1, 15) > 0
    for bad in ((0, 8, 3, 8, 8), (8, 8, 2, 8, 8), (8, 8, 5, 8, 8), (8, 1025, 3, 8, 8), (8, 8, 3, 1025, 8), (8, 8, 3, 8, 0)):
        assert q(*bad) == 0, bad
