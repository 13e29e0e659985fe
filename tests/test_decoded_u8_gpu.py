"""salun_decoded_to_u8 (csrc/salun_vae.hip) against the numpy fp32 statement of its rule, byte for byte:
    v = x * 0.5 + 0.5 (two roundings);  v = clip(v, 0, 1), NaN -> 0;  u8 = rint(v * 255)  (half to even), NHWC."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rule(x, C):
    """x [B, Cp, HW] float32 -> [B, HW, C] uint8."""
    x = np.asarray(x, np.float32)[:, :C]
    with np.errstate(invalid="ignore"):
        v = x * np.float32(0.5)
        v = v + np.float32(0.5)
        v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(1))).astype(np.float32)
        v = v * np.float32(255)
        return np.rint(v).astype(np.uint8).transpose(0, 2, 1).copy()


def device(x, C):
    from unlearn_saliency_amd import ops_infer
    B, Cp, HW = x.shape
    out = ops_infer.decoded_to_u8(torch.from_numpy(x).cuda().view(B, Cp, 1, HW), C)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, 1, HW, C)
    return out.cpu().numpy().reshape(B, HW, C)


def test_random_data_from_a_padded_tensor():
    x = (np.random.default_rng(0).standard_normal((2, 32, 40)) * 0.8).astype(np.float32)
    got = device(x, 3)
    assert np.array_equal(got, rule(x, 3))
    assert got.min() == 0 and got.max() == 255 and len(np.unique(got)) > 100     # the clamp is hit on both sides


def test_special_values():
    inf, nan = np.float32("inf"), np.float32("nan")
    vals = np.array([-1, 1, inf, -inf, nan, 1.5, -1.5, 3e38, -3e38, 0, -0.0, 1e-45, 0.99999994, -0.99999994],
                    np.float32)
    x = np.stack([vals, vals[::-1], np.roll(vals, 3)])[None]                         # [1, 3, 14]
    got = device(x, 3)
    assert np.array_equal(got, rule(x, 3))
    assert list(got[0, :5, 0]) == [0, 255, 255, 0, 0]


def test_the_255_rounding_ties():
    k = np.arange(255, dtype=np.float64)
    ties = (2 * (k + 0.5) / 255 - 1).astype(np.float32)
    x = np.stack([ties, np.nextafter(ties, np.float32(2)), np.nextafter(ties, np.float32(-2))])[None]   # [1, 3, 255]
    got, want = device(x, 3), rule(x, 3)
    assert np.array_equal(got, want)
    # where the fp32 tie is an exact .5 the even neighbour is taken: both parities occur among the results
    exact = (want[0, :, 0].astype(np.int64) - k.astype(np.int64))
    assert set(exact.tolist()) <= {0, 1} and 0 < exact.sum() < 255


def test_padded_and_bare_tensors_give_the_same_bytes():
    x3 = np.random.default_rng(1).standard_normal((3, 3, 77)).astype(np.float32)
    x32 = np.full((3, 32, 77), np.nan, np.float32)
    x32[:, :3] = x3
    a, b = device(x3, 3), device(x32, 3)
    assert np.array_equal(a, b) and np.array_equal(a, rule(x3, 3))


def test_refusals():
    from unlearn_saliency_amd import ops_infer
    from unlearn_saliency_amd._lib import SalunError
    x = torch.zeros((1, 3, 2, 2), device="cuda")
    for C in (0, 4, 5):
        with pytest.raises(SalunError):
            ops_infer.decoded_to_u8(x, C)
    with pytest.raises(SalunError):
        ops_infer.decoded_to_u8(torch.zeros((1, 8, 2, 2), device="cuda"), 5)
