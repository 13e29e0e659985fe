"""CPU restatement of Fisher forgetting (reference Classification/unlearn/fisher.py:50-114, `fisher_new`) in plain
PyTorch, fp64 when given an fp64 model — written from the algorithm, not copied — in two forms of the `hessian` pass:

  literal_grad2   the reference's loop: per batch of 32 and class y, the gradient of CE_mean(output, y), then
                  F += mean_i(prob[i, y]) * grad^2;
  grouped_grad2   the form the K18 kernels compute: per-sample logit Jacobians J_i from one pass, the
                  class-y batch gradient g_y = sum_i J_i^T (p_i - e_y) / B, then F += sum_y w_y g_y^2.

Both divide by the number of batches.  `mean_var` restates `get_mean_var`; also the fixture data of
tests/golden/make_golden_ff.py."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from unlearn_saliency_amd import rng

MODEL_SEED = 31
N_RETAIN = 300   # 9 full batches of 32 and a ragged batch of 12
BATCH = 32
ALPHA = 0.2
NUM_CLASSES = 10
NOISE_SEED = 7
# (name, num_indexes_to_replace, dataset, class_to_replace)
CASES = (("last_row", 4500, "cifar10", -1),    # the headline configuration: the LAST class row is overridden
         ("class3", 4500, "cifar10", 3),       # an explicit class
         ("no_override", 100, "cifar10", 3))   # the override does not apply


def case_args(name: str) -> SimpleNamespace:
    for n, k, ds, c in CASES:
        if n == name:
            return SimpleNamespace(num_indexes_to_replace=k, dataset=ds, class_to_replace=c, num_classes=NUM_CLASSES,
                                   alpha=ALPHA, gpu=0, seed=NOISE_SEED)
    raise KeyError(name)


def retain_dataset(n: int = N_RETAIN):
    """8x8 uint8 ArrayDataset with the test transform (no augmentation draws)."""
    from unlearn_saliency_amd.Classification.dataset import ArrayDataset
    x = rng.u8(n * 8 * 8 * 3, 1800).reshape(n, 8, 8, 3)
    y = (rng.u8(n, 1801) % 10).astype(np.int64)
    return ArrayDataset(x, y, transform="test")


def batches(ds, bs: int = BATCH, dtype=torch.float64):
    for lo in range(0, len(ds), bs):
        xs = [ds[i][0] for i in range(lo, min(lo + bs, len(ds)))]
        yield torch.stack(xs).to(dtype)


def literal_grad2(model, ds, bs: int = BATCH, dtype=torch.float64):
    """The reference's hessian() loop -> list of grad2 tensors in parameters() order."""
    model.eval()
    params = list(model.parameters())
    acc = [torch.zeros_like(p) for p in params]
    nb = 0
    for x in batches(ds, bs, dtype):
        out = model(x)
        prob = torch.softmax(out, dim=-1).detach()
        for y in range(out.shape[1]):
            loss = F.cross_entropy(out, torch.full((x.shape[0],), y, dtype=torch.int64))
            g = torch.autograd.grad(loss, params, retain_graph=True)
            for a, t in zip(acc, g):
                a += prob[:, y].mean() * t.pow(2)
        nb += 1
    return [a / nb for a in acc]


def grouped_grad2(model, ds, bs: int = BATCH, dtype=torch.float64):
    """The grouped form: one Jacobian pass per batch, the class gradients as combinations of per-sample logit
    gradients."""
    from torch.func import functional_call, jacrev, vmap
    model.eval()
    names = [n for n, _ in model.named_parameters()]
    theta = {n: p.detach() for n, p in model.named_parameters()}
    buffers = {n: b for n, b in model.named_buffers()}

    def logits1(th, xi):
        return functional_call(model, (th, buffers), (xi.unsqueeze(0),))[0]

    acc = {n: torch.zeros_like(theta[n]) for n in names}
    nb = 0
    for x in batches(ds, bs, dtype):
        B = x.shape[0]
        with torch.no_grad():
            prob = torch.softmax(model(x), dim=-1)
        J = vmap(jacrev(logits1), in_dims=(None, 0))(theta, x)  # name -> (B, C, *shape)
        C = prob.shape[1]
        D = (prob.unsqueeze(0) - torch.eye(C, dtype=dtype).unsqueeze(1)) / B  # D[y, i, c] = (p_ic - [c == y]) / B
        w = prob.mean(0)
        for n in names:
            g = torch.einsum("yic,ic...->y...", D, J[n])
            acc[n] += torch.einsum("y,y...->...", w, g.pow(2))
        nb += 1
    return [acc[n] / nb for n in names]


def override_row(args):
    if (args.num_indexes_to_replace == 4500 and args.dataset == "cifar10") or \
       (args.num_indexes_to_replace == 450 and args.dataset == "cifar100"):
        return args.class_to_replace
    return None


def mean_var(p: torch.Tensor, grad2: torch.Tensor, args):
    """get_mean_var(p, args): (mu, var)."""
    var = 1.0 / (grad2 + 1e-8)
    var = var.clamp(max=1e3)
    if p.shape[0] == args.num_classes:
        var = var.clamp(max=1e2)
    var = args.alpha * var
    if p.ndim > 1:
        var = var.mean(dim=1, keepdim=True).expand_as(p).clone()
    mu = p.detach().clone()
    row = override_row(args)
    if p.shape[0] == args.num_classes and row is not None:
        mu[row] = 0
        var[row] = 0.0001
    if p.shape[0] == args.num_classes or p.ndim == 1:
        var = var * 10
    return mu, var
