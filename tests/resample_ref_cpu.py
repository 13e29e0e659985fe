"""numpy restatement of K26's arithmetic (include/salun.h): Pillow's 8-bit antialiased bilinear resample, horizontal
pass first and then vertical.  Test infrastructure only: tests/test_resample_ref_cpu.py pins it to
`PIL.Image.resize((OW, OH), Image.BILINEAR)` byte for byte, tests/test_resample_gpu.py pins the kernel to it.

Everything that is floating point is a Python float (a C double) and is evaluated one operation at a time, in the
order the header gives; the pixel work is int64 and exact."""
import numpy as np

PRECISION_BITS = 22


def axis_table(n_in: int, n_out: int):
    """-> (xmin [n_out] int, count [n_out] int, k [n_out, ksize] int64) of one axis."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    ksize = int(np.ceil(support)) * 2 + 1
    xmins, counts, ks = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64), np.zeros((n_out, ksize), np.int64)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        n = xmax - xmin
        w = []
        for x in range(n):
            v = (x + xmin - center + 0.5) * ss
            w.append(max(0.0, 1.0 - abs(v)))
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            ks[xx, x] = int(v * float(1 << PRECISION_BITS) + 0.5)
        xmins[xx], counts[xx] = xmin, n
    return xmins, counts, ks


def _pass(img: np.ndarray, axis: int, n_out: int) -> np.ndarray:
    """One pass along `axis` of a [..., H, W, C] uint8 array."""
    xmins, counts, ks = axis_table(img.shape[axis], n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for xx in range(n_out):
        n = int(counts[xx])
        taps = src[xmins[xx]:xmins[xx] + n]
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(ks[xx, :n], taps, axes=(0, 0))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_u8(x: np.ndarray, size) -> np.ndarray:
    """x uint8 [B, H, W, C] (or [H, W, C]) -> uint8 [B, OH, OW, C]: horizontal pass, rounded to uint8, then vertical."""
    oh, ow = size
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.ndim in (3, 4)
    h = _pass(x, x.ndim - 2, ow)
    return np.ascontiguousarray(_pass(h, x.ndim - 3, oh))


# ------------------------------------------------------------------------------------------------ shared test inputs
SIZES = [((96, 96), (64, 64)), ((32, 32), (64, 64)), ((5, 7), (3, 4)), ((97, 33), (64, 64)), ((6, 6), (6, 6))]
KINDS = ("random", "zeros", "ones", "rows", "cols")


def make_input(kind: str, b: int, h: int, w: int, c: int, seed: int = 2600) -> np.ndarray:
    """uint8 [b, h, w, c]: counter-based random, all 0, all 255, alternating 0 / 255 rows or columns."""
    from unlearn_saliency_amd import rng
    if kind == "random":
        return rng.u8(b * h * w * c, seed + 7 * h + w + c).reshape(b, h, w, c)
    x = np.zeros((b, h, w, c), np.uint8)
    if kind == "ones":
        x[:] = 255
    elif kind == "rows":
        x[:, 1::2] = 255
    elif kind == "cols":
        x[:, :, 1::2] = 255
    elif kind != "zeros":
        raise ValueError(kind)
    return x
