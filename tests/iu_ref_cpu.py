"""CPU restatement of the IU / WoodFisher baseline (reference Classification/unlearn/Wfisher.py:47-198) in plain
PyTorch autograd, fp64 when given an fp64 model — written from the algorithm, not copied — in two forms:

  literal_woodfisher   the reference's walk with two flat vectors o and k, one batch-1 gradient per retain sample;
  scalar_woodfisher    the same walk on the scalars a_i = <g_0, g_i>, b_i = <v, g_i>:  k = v - beta g_0, o = s g_0.

Also the fixture data of tests/golden/make_golden_iu.py (forget / retain sets from the counter-based generator)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from unlearn_saliency_amd import rng

N_WF = 1000          # the reference's N
ALPHA = 0.2
BATCH = 64
N_FORGET = 40
MODEL_SEED = 31
MASK_SEED = 950
CASES = (1100, 300)  # retain sizes: early return after 1,002 samples / the walk runs out of samples


def iu_datasets(n_retain: int, n_forget: int = N_FORGET):
    """(forget, retain) 8x8 uint8 ArrayDatasets with the test transform (no augmentation draws).  The forget images are
    brighter than the retain images so that v = mean forget gradient - mean retain gradient is not a small
    difference of large terms."""
    from unlearn_saliency_amd.Classification.dataset import ArrayDataset
    fx = (128 + rng.u8(n_forget * 8 * 8 * 3, 1500) // 2).astype(np.uint8).reshape(n_forget, 8, 8, 3)
    fy = (rng.u8(n_forget, 1501) % 10).astype(np.int64)
    rx = rng.u8(n_retain * 8 * 8 * 3, 1502).reshape(n_retain, 8, 8, 3)
    ry = (rng.u8(n_retain, 1503) % 10).astype(np.int64)
    return ArrayDataset(fx, fy, transform="test"), ArrayDataset(rx, ry, transform="test")


def mask_flat(n: int) -> np.ndarray:
    return (rng.u8(n, MASK_SEED) & 1).astype(np.int64)


def images(ds, lo: int, hi: int, dtype=torch.float64):
    xs, ys = zip(*[ds[i] for i in range(lo, hi)])
    return torch.stack(xs).to(dtype), torch.tensor(ys, dtype=torch.int64)


def flat_grad(model, x, y) -> torch.Tensor:
    """gradient of the mean cross-entropy of the batch, flat in named_parameters() order."""
    g = torch.autograd.grad(F.cross_entropy(model(x), y), list(model.parameters()))
    return torch.cat([t.reshape(-1) for t in g])


def grad_sum(model, ds, bs: int = BATCH, dtype=torch.float64):
    """sum over unshuffled batches of n_b * grad(mean CE), and the sample count."""
    acc = None
    for lo in range(0, len(ds), bs):
        x, y = images(ds, lo, min(lo + bs, len(ds)), dtype)
        g = flat_grad(model, x, y) * x.shape[0]
        acc = g if acc is None else acc + g
    return acc, len(ds)


def iu_v(model, forget, retain, bs: int = BATCH, dtype=torch.float64):
    Fg, T = grad_sum(model, forget, bs, dtype)
    Rg, T2 = grad_sum(model, retain, bs, dtype)
    return Fg / (T + T2) - Rg * (T / ((T + T2) * T2))


def walk_len(n_retain: int) -> int:
    return min(n_retain, N_WF + 2)


def sample_grads(model, retain, dtype=torch.float64):
    """the batch-1 gradients of the walk's samples, stacked (n, P)."""
    return torch.stack([flat_grad(model, *images(retain, i, i + 1, dtype)) for i in range(walk_len(len(retain)))])


def literal_woodfisher(G: torch.Tensor, v: torch.Tensor, N: float = N_WF) -> torch.Tensor:
    """The reference loop on the per-sample gradients G (rows in walk order) -> k."""
    k = v.clone()
    o = None
    for g in G:
        if o is None:
            o = g.clone()
            continue
        t = torch.dot(o, g)
        k = k - (torch.dot(k, g) / (N + t)) * o
        o = o - (t / (N + t)) * o
    return k


def scalar_woodfisher(a, b, N: float = N_WF):
    """beta, s of k = v - beta g_0, o = s g_0 from a_i = <g_0, g_i>, b_i = <v, g_i> (i = 1 .. n-1), in Python floats."""
    s, beta = 1.0, 0.0
    for ai, bi in zip(a, b):
        t = s * ai
        beta += (bi - beta * ai) * s / (N + t)
        s *= N / (N + t)
    return beta, s


def scalar_form(G: torch.Tensor, v: torch.Tensor, N: float = N_WF) -> torch.Tensor:
    g0 = G[0]
    a = (G[1:] @ g0).tolist()
    b = (G[1:] @ v).tolist()
    beta, _ = scalar_woodfisher(a, b, N)
    return v - beta * g0
