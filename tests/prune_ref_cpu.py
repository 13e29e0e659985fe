"""Host restatement of K22 (global unstructured pruning on a flat arena) and the torch.nn.utils.prune reference the
GPU tests compare against.  Pure numpy / CPU torch; nothing here touches the package's kernels.

A round, given k_prune: among the elements of the segments with keep == 1, the k_prune with the smallest key (|p|, or
the given keys) get keep = 0, p = 0, buf = 0; ties at the threshold go highest flat index first; everything else is
left alone."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.utils.prune as tprune

GAPS = (16, 7, 5)            # non-conv elements in front of segment 0, 1, 2: offsets are not multiples of 4
SMALL = (432, 2307, 576)     # n_sel = 3315 < 8192: the select's full-scan route
LARGE = SMALL + (36864,)     # n_sel = 40179 >= 8192: its single-read route


def layout(lengths, tail=3):
    """-> (n, [(off, len)]) with the gaps in front of the first three segments, 9 elements in front of any further one
    and `tail` elements after the last."""
    segs, off = [], 0
    for j, ln in enumerate(lengths):
        off += GAPS[j] if j < len(GAPS) else 9
        segs.append((off, ln))
        off += ln
    return off + tail, segs


def seg_index(segs):
    return np.concatenate([np.arange(o, o + k, dtype=np.int64) for o, k in segs])


def distinct_arena(lengths, seed):
    """Continuous random segment values whose |p| are pairwise distinct (verified), and gap elements that hold the
    smallest magnitudes of the whole arena (a select that leaks outside the segments would take them first)."""
    n, segs = layout(lengths)
    rng = np.random.default_rng(seed)
    idx = seg_index(segs)
    vals = rng.standard_normal(idx.size).astype(np.float32)
    for _ in range(64):  # float32 normals collide in magnitude at these sizes: re-draw the collisions (and anything tiny)
        mags = np.abs(vals)
        first = np.zeros(vals.size, bool)
        first[np.unique(mags, return_index=True)[1]] = True
        again = ~first | (mags <= 1e-6)
        if not again.any():
            break
        vals[again] = rng.standard_normal(int(again.sum())).astype(np.float32)
    p = np.zeros(n, np.float32)
    p[idx] = vals
    mags = np.abs(vals)
    assert np.unique(mags).size == mags.size and mags.min() > 1e-6, "|p| must be pairwise distinct"
    gap = np.setdiff1d(np.arange(n), idx)
    p[gap] = (rng.uniform(1e-9, 1e-7, gap.size) * rng.choice([-1.0, 1.0], gap.size)).astype(np.float32)
    assert np.abs(p[gap]).max() < np.abs(p[idx]).min() and np.all(p[gap] != 0)
    buf = rng.standard_normal(n).astype(np.float32)
    return n, segs, p, buf


def prune_amount(amount, alive):
    return int(round(float(amount) * int(alive)))


def prune_round(p, buf, keep, segs, k_prune, keys=None):
    """In place on numpy arrays.  `keys`: one value per segment element (compact order) to rank by instead of |p|.
    Returns the flat indices that were cleared."""
    idx = seg_index(segs)
    key = np.abs(p[idx]) if keys is None else np.asarray(keys, np.float32)
    live = keep[idx] == 1
    cand, ckey = idx[live], key[live]
    assert 0 <= k_prune <= cand.size
    order = np.lexsort((-cand, ckey))     # key ascending; equal keys: flat index descending
    victims = cand[order[:k_prune]]
    keep[victims] = 0
    p[victims] = 0.0
    if buf is not None:
        buf[victims] = 0.0
    return victims


class _Holder(nn.Module):
    def __init__(self, w):
        super().__init__()
        self.weight = nn.Parameter(torch.from_numpy(np.ascontiguousarray(w)).clone())


class TorchPruned:
    """torch.nn.utils.prune.global_unstructured on CPU modules that hold the segments of a flat vector."""

    def __init__(self, p, segs):
        self.segs = segs
        self.mods = [_Holder(p[o:o + k]) for o, k in segs]

    def round(self, amount, random=False):
        method = tprune.RandomUnstructured if random else tprune.L1Unstructured
        tprune.global_unstructured([(m, "weight") for m in self.mods], pruning_method=method, amount=amount)

    def mask(self):
        """u8 per segment element, compact order (1 where torch has not pruned)."""
        out = []
        for m in self.mods:
            w = getattr(m, "weight_mask", None)
            out.append(np.ones(m.weight.numel(), np.uint8) if w is None else w.detach().numpy().astype(np.uint8))
        return np.concatenate(out)

    def remaining(self):
        return int(self.mask().sum())


# ------------------------------------------------------------------------------------------------------------------
# The three pruning baselines restated on CPU torch (plain SGD on the effective weights), for tests/golden/prune_*.npz
class PruneCNN(nn.Module):
    """792 convolution weights: few enough that the magnitudes around a pruning threshold lie far apart."""

    def __init__(self, num_classes=10):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 8, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(8)
        self.conv2 = nn.Conv2d(8, 8, 3, 2, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(8)
        self.fc = nn.Linear(8, num_classes)

    def forward(self, x):
        x = torch.relu(self.bn1(self.conv1(x)))
        x = torch.relu(self.bn2(self.conv2(x)))
        return self.fc(x.mean(dim=(2, 3)))


CONVS = ("conv1.weight", "conv2.weight")


def prune_cnn_state(seed):
    """Convolution weights N(0, 1) (wide, so that thresholds fall into gaps), fc N(0, 0.2), BN at its defaults."""
    g = np.random.default_rng(seed)
    sd = PruneCNN().state_dict()
    for k, v in sd.items():
        if k in CONVS:
            v.copy_(torch.from_numpy(g.standard_normal(tuple(v.shape)).astype(np.float32)))
        elif k.startswith("fc."):
            v.copy_(torch.from_numpy((0.2 * g.standard_normal(tuple(v.shape))).astype(np.float32)))
    return sd


def loaders_from(batches):
    return [(torch.from_numpy(np.asarray(x, np.float32)), torch.from_numpy(np.asarray(y, np.int64))) for x, y in batches]


class HostPruned:
    """A plain torch model whose convolution weights are the effective weights; masks kept beside it."""

    def __init__(self, model, opt):
        self.model, self.opt = model, opt
        self.w = [dict(model.named_parameters())[n] for n in CONVS]
        self.masks = [torch.ones_like(w) for w in self.w]
        self.rounds = []

    def prune(self, amount):
        sizes = [w.numel() for w in self.w]
        segs, off = [], 0
        for s in sizes:
            segs.append((off, s))
            off += s
        p = torch.cat([w.detach().reshape(-1) for w in self.w]).numpy().copy()
        keep = torch.cat([m.reshape(-1) for m in self.masks]).numpy().astype(np.uint8)
        k = prune_amount(amount, int(keep.sum()))
        if k:
            prune_round(p, None, keep, segs, k)
        with torch.no_grad():
            for w, m, (o, s) in zip(self.w, self.masks, segs):
                m.copy_(torch.from_numpy(keep[o:o + s].astype(np.float32)).view_as(m))
                w.mul_(m)
                buf = self.opt.state.get(w, {}).get("momentum_buffer")
                if buf is not None:
                    buf.mul_(m)
        self.rounds.append(keep.copy())

    def mask_grads(self):
        for w, m in zip(self.w, self.masks):
            if w.grad is not None:
                w.grad.mul_(m)


def _pass(hp, batches, crit, sign):
    hp.model.train()
    hits = seen = 0
    for x, y in batches:
        out = hp.model(x)
        loss = sign * crit(out, y)
        hp.opt.zero_grad()
        loss.backward()
        hp.mask_grads()
        hp.opt.step()
        hits += int((out.argmax(1) == y).sum())
        seen += x.shape[0]
    return hits * 100.0 / seen


def host_validate(model, batches):
    model.eval()
    hits = seen = 0
    with torch.no_grad():
        for x, y in batches:
            hits += int((model(x).argmax(1) == y).sum())
            seen += x.shape[0]
    return hits * 100.0 / seen


def _sgd(model, lr, a):
    opt = torch.optim.SGD(model.parameters(), lr, momentum=a["momentum"], weight_decay=a["weight_decay"])
    return opt, torch.optim.lr_scheduler.MultiStepLR(opt, milestones=a["milestones"], gamma=0.1)


def _result(hp, accs):
    return {"masks": hp.rounds, "accs": np.asarray(accs, np.float64),
            "sd": {k: v.detach().numpy().copy() for k, v in hp.model.state_dict().items()}}


def host_ga_prune_bi(model, L, a):
    crit = nn.CrossEntropyLoss()
    opt, sched = _sgd(model, a["lr"], a)
    hp, accs = HostPruned(model, opt), []
    for epoch in range(a["epochs"]):
        acc = _pass(hp, L["forget"], crit, -1.0)
        accs.append((acc, host_validate(model, L["val"]), host_validate(model, L["test"])))
        sched.step()
        hp.prune(a["rate"])
    return _result(hp, accs)


def host_ga_prune(model, L, a):
    crit = nn.CrossEntropyLoss()
    opt, sched = _sgd(model, a["lr"], a)
    hp, accs, init, rounds = HostPruned(model, opt), [], None, []
    for state in range(a["pruning_times"]):
        for epoch in range(a["epochs"]):
            if state == 0 and epoch == a["rewind_epoch"]:
                init = {k: v.clone() for k, v in model.state_dict().items()}
            acc = _pass(hp, L["forget"], crit, -1.0)
            accs.append((acc, host_validate(model, L["val"]), host_validate(model, L["test"])))
            sched.step()
        hp.prune(a["rate"])
        rounds = hp.rounds
        if state < a["pruning_times"] - 1:
            masks = [m.clone() for m in hp.masks]
            model.load_state_dict(init)
            opt, sched = _sgd(model, a["lr"], a)
            hp = HostPruned(model, opt)
            hp.rounds = rounds
            with torch.no_grad():
                for w, m, m0 in zip(hp.w, hp.masks, masks):
                    m.copy_(m0)
                    w.mul_(m)
            for _ in range(a["rewind_epoch"]):
                sched.step()
    return _result(hp, accs)


def host_ft_prune_bi(model, L, a):
    crit = nn.CrossEntropyLoss()
    opt, sched = _sgd(model, a["unlearn_lr"], a)
    hp, accs = HostPruned(model, opt), []
    E = a["unlearn_epochs"]
    rate = 1 - (1 - a["rate"]) ** (1 / ((E - 1) // 2 + 1))
    for epoch in range(E):
        if (E - epoch) % 2 == 0:
            hp.prune(rate)
        accs.append((_pass(hp, L["retain"], crit, 1.0),))
        sched.step()
    return _result(hp, accs)


HOST_METHODS = {"ga_prune_bi": host_ga_prune_bi, "ga_prune": host_ga_prune, "ft_prune_bi": host_ft_prune_bi}


def golden_setup(z):
    """(fresh model at the golden's initial state, loaders as CPU tensors, the run's settings) from a loaded npz."""
    from fixtures import tiny_batches
    model = PruneCNN()
    model.load_state_dict({k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init_")})
    L = {name: loaders_from(tiny_batches(int(nb), 16, int(seed)))
         for name, nb, seed in zip(z["loader_names"], z["loader_nb"], z["loader_seed"])}
    a = {k[4:]: z[k].item() for k in z.files if k.startswith("arg_")}
    a["milestones"] = [int(v) for v in str(a["decreasing_lr"]).split(",")]
    return model, L, a


def golden_masks(z):
    return [z[f"mask_r{i}"] for i in range(int(z["rounds"]))]
