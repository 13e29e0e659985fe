"""K26 (`salun_resample_u8`, csrc/salun_resample.hip) on the device equals the numpy restatement of Pillow's 8-bit
bilinear resample (tests/resample_ref_cpu.py, pinned to Pillow in test_resample_ref_cpu.py) byte for byte.

Every call runs inside a guarded byte buffer after the pattern of tests/guarded_arena.py: guard bytes before and after
the source and the destination, the destination pre-filled with a sentinel, the source ONE byte off any alignment; after
the call everything but the destination must hold the bytes it was given."""
import functools
from ctypes import c_int64, c_void_p

import numpy as np
import pytest
import torch

import resample_ref_cpu as R

pytestmark = pytest.mark.gpu

GUARD = 4096
GUARD_BYTE, SENTINEL = 0xA5, 0x5A
EINVAL = -22

# the issue's sizes, then: a tail band (37 = 2 x 16 + 5 rows) that mixes down- and upscaling; a downscale strong enough
# that a 16-row band would not fit LDS (the launch takes 8-row bands); one output row out of 1024 (a one-row band)
EXTRA_SIZES = [((40, 50), (37, 70)), ((1024, 8), (32, 64)), ((1024, 16), (1, 15))]


class ByteArena:
    """guard | 1 byte | src | guard | dst (sentinel) | guard in one flat uint8 allocation."""

    def __init__(self, src: np.ndarray, dst_bytes: int):
        self.s0 = GUARD + 1
        self.d0 = (self.s0 + src.size + GUARD + 15) // 16 * 16
        self.dn = dst_bytes
        host = np.full(self.d0 + dst_bytes + GUARD, GUARD_BYTE, np.uint8)
        host[self.s0:self.s0 + src.size] = src.reshape(-1)
        host[self.d0:self.d0 + dst_bytes] = SENTINEL
        self.host = torch.from_numpy(host)
        self.dev = self.host.cuda()

    @property
    def src(self):
        return c_void_p(self.dev.data_ptr() + self.s0)

    @property
    def dst(self):
        return c_void_p(self.dev.data_ptr() + self.d0)

    def result(self, written=True):
        """The destination bytes, after checking that nothing else changed (written=False: nothing at all)."""
        torch.cuda.synchronize()
        after = self.dev.cpu()
        assert torch.equal(after[:self.d0], self.host[:self.d0]), "a guard or the source was written"
        assert torch.equal(after[self.d0 + self.dn:], self.host[self.d0 + self.dn:]), "the guard after dst was written"
        if not written:
            assert torch.equal(after, self.host), "a refused call wrote to dst"
        return after[self.d0:self.d0 + self.dn]


@functools.lru_cache(maxsize=None)
def case(kind, b, src, dst, c):
    x = R.make_input(kind, b, src[0], src[1], c)
    return x, torch.from_numpy(R.resize_u8(x, dst))


def call(arena, b, src, dst, c, src_ptr="arena", dst_ptr="arena"):
    from unlearn_saliency_amd import _lib
    from unlearn_saliency_amd.ops import _stream
    src_ptr = arena.src if src_ptr == "arena" else src_ptr
    dst_ptr = arena.dst if dst_ptr == "arena" else dst_ptr
    return _lib.lib().salun_resample_u8(src_ptr, dst_ptr, c_int64(b), src[0], src[1], c, dst[0], dst[1], _stream())


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("src,dst", R.SIZES + EXTRA_SIZES)
def test_kernel_equals_the_restatement(src, dst, b, c):
    for kind in R.KINDS:
        x, want = case(kind, b, src, dst, c)
        arena = ByteArena(x, want.numel())
        assert call(arena, b, src, dst, c) == 0
        got = arena.result().view(want.shape)
        assert torch.equal(got, want), (kind, int((got != want).sum()))


def test_python_entry_on_an_unaligned_slice():
    from unlearn_saliency_amd import ops_resample
    x, want = case("random", 3, (96, 96), (64, 64), 3)
    flat = torch.zeros(x.size + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = torch.from_numpy(x).reshape(-1).cuda()
    xd = flat[1:].view(x.shape)
    assert xd.data_ptr() % 2 == 1
    got = ops_resample.resize_u8(xd, (64, 64))
    assert got.dtype == torch.uint8 and got.is_cuda and torch.equal(got.cpu(), want)
    with pytest.raises(ValueError):
        ops_resample.resize_u8(xd, (64, 1025))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops_resample.resize_u8(torch.from_numpy(x), (64, 64))


def test_image_offsets_beyond_2_to_the_31():
    """B x H x W x C > 2^31 bytes: the last image starts past what a 32-bit offset reaches."""
    b, src, dst, c = 513, (1024, 1024), (8, 8), 4
    per = src[0] * src[1] * c
    assert (b - 1) * per >= 2 ** 31
    x = torch.empty((b, src[0], src[1], c), dtype=torch.uint8, device="cuda")
    x.zero_()
    for i in (0, b - 1):
        x[i] = torch.from_numpy(R.make_input("random", 1, src[0], src[1], c, seed=2700 + i)[0]).cuda()
    from unlearn_saliency_amd import ops_resample
    got = ops_resample.resize_u8(x, dst).cpu()
    for i in (0, 1, b - 1):
        want = torch.from_numpy(R.resize_u8(x[i:i + 1].cpu().numpy(), dst))
        assert torch.equal(got[i:i + 1], want), i
    assert int(got[b - 1].max()) > 0


@pytest.mark.parametrize("b,src,dst,c", [
    (1, (8, 8), (8, 8), 2), (1, (8, 8), (8, 8), 5), (1, (1025, 8), (8, 8), 3), (1, (8, 1025), (8, 8), 3),
    (1, (8, 8), (1025, 8), 3), (1, (8, 8), (8, 1025), 3), (1, (0, 8), (8, 8), 3), (1, (8, 8), (8, 0), 3),
    (0, (8, 8), (8, 8), 3), (-1, (8, 8), (8, 8), 3),
    (1, (1024, 1024), (64, 1024), 4),   # inside the limits, but one output row needs 33 x 4096 bytes of LDS: refused
])
def test_outside_the_limits_is_einval_and_writes_nothing(b, src, dst, c):
    # buffers of the size the arguments name (of 8 x 8 x 3 where they name none)
    ok = lambda v: 1 <= v <= 1024
    full = b >= 1 and c in (1, 3, 4) and all(ok(v) for v in src + dst)
    x = np.zeros((1,) + src + (c,), np.uint8) if full else R.make_input("random", 1, 8, 8, 3)
    arena = ByteArena(x, dst[0] * dst[1] * c if full else 8 * 8 * 3)
    assert call(arena, b, src, dst, c) == EINVAL
    arena.result(written=False)


def test_bad_pointers_are_einval_and_write_nothing():
    x = R.make_input("random", 1, 8, 8, 3)
    arena = ByteArena(x, 8 * 8 * 3)
    assert call(arena, 1, (8, 8), (8, 8), 3, src_ptr=c_void_p(None)) == EINVAL
    assert call(arena, 1, (8, 8), (8, 8), 3, dst_ptr=c_void_p(None)) == EINVAL
    assert call(arena, 1, (8, 8), (8, 8), 3, dst_ptr=arena.src) == EINVAL
    arena.result(written=False)
