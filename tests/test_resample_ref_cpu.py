"""The numpy restatement of K26's arithmetic (tests/resample_ref_cpu.py) equals Pillow's antialiased bilinear resize
byte for byte, and resize-then-mirror equals mirror-then-resize — the order the STL-10 data path relies on
(DDPM/datasets/stl10.py resizes once on the uint8 originals; the flip comes later, where the CIFAR-10 path has it)."""
import numpy as np
import pytest
from PIL import Image

import resample_ref_cpu as R

MODES = {1: "L", 3: "RGB", 4: "CMYK"}  # CMYK: four independent 8-bit channels (RGBA would premultiply alpha first)


def pillow_resize(x, size):
    oh, ow = size
    out = []
    for img in x:
        c = img.shape[-1]
        im = Image.fromarray(img[..., 0] if c == 1 else img, MODES[c])
        out.append(np.asarray(im.resize((ow, oh), Image.BILINEAR)).reshape(oh, ow, c))
    return np.stack(out)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("src,dst", R.SIZES)
def test_restatement_equals_pillow_byte_for_byte(src, dst, c):
    for kind in R.KINDS:
        x = R.make_input(kind, 2, src[0], src[1], c)
        want = pillow_resize(x, dst)
        got = R.resize_u8(x, dst)
        assert got.shape == want.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), (kind, int((got != want).sum()))


def test_same_size_is_the_identity():
    x = R.make_input("random", 1, 6, 6, 3)
    assert np.array_equal(R.resize_u8(x, (6, 6)), x)


@pytest.mark.parametrize("n_in,n_out", [(96, 64), (32, 64), (7, 4), (33, 64), (97, 64), (6, 6)])
def test_tables_are_mirror_symmetric(n_in, n_out):
    """Output sample n_out - 1 - i reads the mirrored taps of output sample i with the same weights: why a horizontal
    flip commutes with the resize."""
    xmin, cnt, k = R.axis_table(n_in, n_out)
    dense = np.zeros((n_out, n_in), np.int64)  # (a tap window may carry a zero weight at one end: compare densely)
    for i in range(n_out):
        dense[i, xmin[i]:xmin[i] + cnt[i]] = k[i, :cnt[i]]
    assert np.array_equal(dense[::-1, ::-1], dense)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("src,dst", R.SIZES[:2])
def test_resize_then_mirror_equals_mirror_then_resize(src, dst, c):
    for kind in ("random", "cols"):
        x = R.make_input(kind, 2, src[0], src[1], c)
        a = R.resize_u8(x, dst)[:, :, ::-1]
        b = R.resize_u8(np.ascontiguousarray(x[:, :, ::-1]), dst)
        assert np.array_equal(a, b), kind
        assert np.array_equal(pillow_resize(x, dst)[:, :, ::-1], pillow_resize(np.ascontiguousarray(x[:, :, ::-1]), dst))
