"""The pruning baselines through the registry on the tiny BN network: counts follow torch.nn.utils.prune's
round(amount * remaining) chain exactly, pruned weights are exactly 0 after training on them, the saved checkpoints have
the hooked-model layout and the reference's keys, and a pruned checkpoint resumes."""
import os
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import prune_ref_cpu as PR
from fixtures import TinyCNN, tiny_batches, tiny_state

pytestmark = pytest.mark.gpu
N_CONV = 3 * 8 * 9 + 8 * 16 * 9


class _L(list):
    dataset = None


def _loader(nb, seed):
    return _L([(torch.from_numpy(x).float().cuda(), torch.from_numpy(y).cuda()) for x, y in tiny_batches(nb, 16, seed)])


def _setup(d, **kw):
    model = TinyCNN().cuda()
    model.load_state_dict(tiny_state(7))
    loaders = {"forget": _loader(2, 100), "retain": _loader(3, 200), "val": _loader(2, 300), "test": _loader(2, 400)}
    args = SimpleNamespace(lr=0.01, unlearn_lr=0.01, momentum=0.9, weight_decay=5e-4, decreasing_lr="91,136",
                           rewind_epoch=0, epochs=2, unlearn_epochs=3, rate=0.3, random_prune=False, pruning_times=2,
                           prune_type="rewind_lt", warmup=0, print_freq=50, save_dir=d, seed=2, unlearn="x",
                           dataset="cifar10", num_classes=10, alpha=0.0, no_l1_epochs=0)
    for k, v in kw.items():
        setattr(args, k, v)
    return model, loaders, args


def _conv_zeros(model):
    return sum(int((m.weight == 0).sum()) for m in model.modules() if isinstance(m, nn.Conv2d))


def _chain(amount, rounds, n=N_CONV):
    for _ in range(rounds):
        n -= PR.prune_amount(amount, n)
    return n


@pytest.mark.parametrize("random_prune", [False, True])
def test_ga_prune_bi(random_prune):
    from unlearn_saliency_amd.Classification import pruner, unlearn
    with tempfile.TemporaryDirectory() as d:
        model, loaders, args = _setup(d, unlearn="GA_prune_bi", random_prune=random_prune)
        before = {k: v.clone() for k, v in model.state_dict().items()}
        unlearn.get_unlearn_method("GA_prune_bi")(loaders, model, nn.CrossEntropyLoss(), args)
        st = pruner.prune_state(model)
        assert st is not None and st.alive == _chain(0.3, 2) == N_CONV - _conv_zeros(model)
        sd = model.state_dict()
        assert "conv1.weight" not in sd and sd["conv1.weight_mask"].dtype == torch.float32
        assert torch.equal(sd["conv1.weight_orig"] != 0, sd["conv1.weight_mask"] == 1)
        assert not torch.equal(sd["fc.weight"], before["fc.weight"])
        ck = torch.load(os.path.join(d, "0checkpoint.pth.tar"), weights_only=False)
        assert sorted(ck) == sorted(["state", "result", "epoch", "state_dict", "best_sa", "optimizer", "scheduler",
                                     "init_weight"])
        assert ck["epoch"] == 2 and ck["init_weight"] is None and len(ck["result"]["train_ta"]) == 2
        # the checkpoint of epoch 2 was written after ONE round, and trained one epoch under its mask
        m1 = torch.cat([ck["state_dict"][k].reshape(-1) for k in ("conv1.weight_mask", "conv2.weight_mask")])
        w1 = torch.cat([ck["state_dict"][k].reshape(-1) for k in ("conv1.weight_orig", "conv2.weight_orig")])
        assert int(m1.sum()) == _chain(0.3, 1) and torch.all(w1[m1 == 0] == 0) and torch.all(w1[m1 == 1] != 0)
        # save / --resume round trip
        unlearn.save_unlearn_checkpoint(model, {"accuracy": {}}, args)
        fresh = TinyCNN().cuda()
        got = unlearn.load_unlearn_checkpoint(fresh, torch.device("cuda"), args)
        assert got is not None and got[1] == {"accuracy": {}}
        assert pruner.prune_state(fresh).alive == st.alive
        for k, v in sd.items():
            assert torch.equal(fresh.state_dict()[k], v), k


def test_ft_prune_bi_with_and_without_a_saliency_mask():
    from unlearn_saliency_amd.Classification import pruner, unlearn
    from unlearn_saliency_amd.Classification.unlearn.FT_prune_bi import prune_schedule
    with tempfile.TemporaryDirectory() as d:
        for with_mask in (False, True):
            model, loaders, args = _setup(d, unlearn="FT_prune_bi", unlearn_epochs=4)
            rate, fire = prune_schedule(4, 0.3)
            assert fire == [0, 2]
            before = {k: v.clone() for k, v in model.named_parameters()}
            mask = None
            if with_mask:
                mask = {k: (torch.arange(v.numel(), device="cuda").view_as(v) % 2) for k, v in model.named_parameters()}
            unlearn.get_unlearn_method("FT_prune_bi")(loaders, model, nn.CrossEntropyLoss(), args, mask)
            st = pruner.prune_state(model)
            assert st.alive == _chain(rate, 2) == N_CONV - _conv_zeros(model)
            if with_mask:  # outside the saliency mask a weight is either untouched or pruned
                for k, v in model.named_parameters():
                    off = mask[k] == 0
                    assert torch.all((v[off] == before[k][off]) | (v[off] == 0)), k
                    assert (v[~off] != before[k][~off]).float().mean() > 0.5, k


def test_ga_prune_rewinds_under_the_mask():
    from unlearn_saliency_amd.Classification import pruner, unlearn
    with tempfile.TemporaryDirectory() as d:
        model, loaders, args = _setup(d, unlearn="GA_prune")
        init = {k: v.clone() for k, v in model.state_dict().items()}
        unlearn.get_unlearn_method("GA_prune")(loaders, model, nn.CrossEntropyLoss(), args)
        assert pruner.prune_state(model) is None and "conv1.weight" in model.state_dict()
        assert _conv_zeros(model) == N_CONV - _chain(0.3, 2)
        rewind = torch.load(os.path.join(d, "epoch_1_rewind_weight.pt"), weights_only=False)
        for k, v in init.items():
            assert torch.equal(rewind[k], v), k
        ck = torch.load(os.path.join(d, "1checkpoint.pth.tar"), weights_only=False)
        assert ck["state"] == 1 and torch.equal(ck["init_weight"]["conv1.weight"], init["conv1.weight"])
        m = ck["state_dict"]["conv2.weight_mask"]
        assert int(m.sum()) + int(ck["state_dict"]["conv1.weight_mask"].sum()) == _chain(0.3, 1)
        assert torch.all(ck["state_dict"]["conv2.weight_orig"][m == 0] == 0)
        # lt: the reference reads `initalization` before any assignment
        model2, loaders2, args2 = _setup(d, unlearn="GA_prune", prune_type="lt")
        with pytest.raises(NameError, match="initalization"):
            unlearn.get_unlearn_method("GA_prune")(loaders2, model2, nn.CrossEntropyLoss(), args2)


def test_ft_prune_bi_on_a_model_that_arrives_pruned_keeps_the_callers_saliency_mask():
    """unlearn_epochs = 2 fires at epoch 0 on a model that already carries a prune state with ANOTHER saliency mask
    (a previous call): this call's mask must hold — weights outside it stay bit-identical or get pruned, weights the
    previous mask alone allowed do not move."""
    from unlearn_saliency_amd.Classification import pruner, unlearn
    with tempfile.TemporaryDirectory() as d:
        model, loaders, args = _setup(d, unlearn="FT_prune_bi", unlearn_epochs=2)
        crit = nn.CrossEntropyLoss()
        odd = {k: (torch.arange(v.numel(), device="cuda").view_as(v) % 2) for k, v in model.named_parameters()}
        even = {k: 1 - v for k, v in odd.items()}
        unlearn.get_unlearn_method("FT_prune_bi")(loaders, model, crit, args, odd)
        st = pruner.prune_state(model)
        alive1 = st.alive
        before = {k: v.detach().clone() for k, v in model.named_parameters()}
        unlearn.get_unlearn_method("FT_prune_bi")(loaders, model, crit, args, even)
        assert st.alive == alive1 - PR.prune_amount(prune_rate_of(2, 0.3), alive1)
        for k, v in model.named_parameters():
            off = even[k] == 0
            assert torch.all((v[off] == before[k][off]) | (v[off] == 0)), k
            alive_on = (even[k] == 1) & (v != 0)
            assert (v[alive_on] != before[k][alive_on]).float().mean() > 0.5, k
        # and without a mask on the same pruned model: everything alive moves, pruned weights stay 0
        before = {k: v.detach().clone() for k, v in model.named_parameters()}
        unlearn.get_unlearn_method("FT_prune_bi")(loaders, model, crit, args)
        assert pruner.prune_state(model).saliency is None
        for k, v in model.named_parameters():
            alive = v != 0
            assert (v[alive] != before[k][alive]).float().mean() > 0.9, k
        assert N_CONV - _conv_zeros(model) == pruner.prune_state(model).alive


def prune_rate_of(epochs, rate):
    from unlearn_saliency_amd.Classification.unlearn.FT_prune_bi import prune_schedule
    return prune_schedule(epochs, rate)[0]


# ------------------------------------------------------------------------------------------------ the goldens
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ATOL = 1e-4   # the GA / FT plugin goldens' GPU tolerance; the fixtures' gaps are >= 20 x this


def _golden_run(tag, monkeypatch):
    """Run this build's method on the golden's model / loaders / settings; -> (z, model, masks per round, args, dir)."""
    from unlearn_saliency_amd.Classification import pruner
    z = np.load(os.path.join(GOLDEN, f"prune_{tag}.npz"))
    model, L, a = PR.golden_setup(z)
    model = model.cuda()
    loaders = {k: _L([(x.cuda(), y.cuda()) for x, y in v]) for k, v in L.items()}
    rounds = []
    real = pruner.pruning_model

    def recording(m, px, optimizer=None):
        real(m, px, optimizer=optimizer)
        st = pruner.prune_state(m)
        rounds.append(torch.cat([st.mask_of(j).reshape(-1) for j in range(len(st.names))]).cpu().numpy())

    monkeypatch.setattr(pruner, "pruning_model", recording)
    return z, model, loaders, a, rounds


def _compare(z, model, rounds, accs):
    want = PR.golden_masks(z)
    assert len(rounds) == len(want)
    for g, w in zip(rounds, want):
        assert np.array_equal(g, w)
    print("accs", accs, z["accs"])
    assert np.allclose(np.asarray(accs, np.float64), z["accs"], rtol=0, atol=ATOL)
    sd = model.state_dict()
    for k in z.files:
        if not k.startswith("sd_") or "num_batches" in k:
            continue
        name = k[3:]
        if name in sd:
            got = sd[name]
        else:  # a model that still carries its prune state: effective weights = orig * mask
            got = sd[name + "_orig"] * sd[name + "_mask"]
        err = float((got.cpu().double() - torch.from_numpy(z[k]).double()).abs().max())
        print(name, "max abs err", err)
        assert err <= ATOL, (name, err)


def _ns(a, d, **kw):
    return SimpleNamespace(lr=a["lr"], unlearn_lr=a["unlearn_lr"], momentum=a["momentum"], weight_decay=a["weight_decay"],
                           decreasing_lr=a["decreasing_lr"], rewind_epoch=a["rewind_epoch"], epochs=a["epochs"],
                           unlearn_epochs=a["unlearn_epochs"], rate=a["rate"], pruning_times=a["pruning_times"],
                           random_prune=False, prune_type="rewind_lt", warmup=0, print_freq=50, save_dir=d, seed=2,
                           dataset="cifar10", num_classes=10, alpha=0.0, no_l1_epochs=0, **kw)


@pytest.mark.parametrize("tag", ["ga_prune_bi", "ga_prune"])
def test_ga_methods_match_the_reference_goldens(tag, monkeypatch):
    from unlearn_saliency_amd.Classification import unlearn
    z, model, loaders, a, rounds = _golden_run(tag, monkeypatch)
    name = {"ga_prune_bi": "GA_prune_bi", "ga_prune": "GA_prune"}[tag]
    with tempfile.TemporaryDirectory() as d:
        unlearn.get_unlearn_method(name)(loaders, model, nn.CrossEntropyLoss(), _ns(a, d, unlearn=name))
        last = torch.load(os.path.join(d, ("1" if tag == "ga_prune" else "0") + "checkpoint.pth.tar"), weights_only=False)
    r = last["result"]
    _compare(z, model, rounds, list(zip(r["train_ta"], r["val_ta"], r["test_ta"])))
    if tag == "ga_prune":
        assert "AverageMeter" in str(z["reference_error"])   # what the reference's GA_prune does as shipped


@pytest.mark.parametrize("epochs", [3, 4])
def test_ft_prune_bi_matches_the_reference_goldens(epochs, monkeypatch):
    """The loop the reference's wrapper would run (its registry route raises TypeError, recorded in the golden): this
    build's epoch plugin under this build's optimizer and schedule."""
    from unlearn_saliency_amd.Classification import unlearn
    from unlearn_saliency_amd.flat import arena_of
    from unlearn_saliency_amd.optim import FusedMaskedSGD
    z, model, loaders, a, rounds = _golden_run(f"ft_prune_bi_e{epochs}", monkeypatch)
    assert a["unlearn_epochs"] == epochs and "positional argument" in str(z["reference_registry_error"])
    with tempfile.TemporaryDirectory() as d:
        args = _ns(a, d, unlearn="FT_prune_bi")
        opt = FusedMaskedSGD(arena_of(model), args.unlearn_lr, momentum=args.momentum, weight_decay=args.weight_decay)
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[91, 136], gamma=0.1)
        inner = unlearn.get_unlearn_method("FT_prune_bi").__wrapped_iter__
        accs = []
        for epoch in range(epochs):
            accs.append((float(inner(loaders, model, nn.CrossEntropyLoss(), opt, epoch, args, None)),))
            sched.step()
        opt.close()
    _compare(z, model, rounds, accs)
    first = list(rounds)   # (the second recorder below wraps the first, which goes on appending)
    # and through the registry, where this build runs: the same masks
    z2, model2, loaders2, a2, rounds2 = _golden_run(f"ft_prune_bi_e{epochs}", monkeypatch)
    with tempfile.TemporaryDirectory() as d:
        unlearn.get_unlearn_method("FT_prune_bi")(loaders2, model2, nn.CrossEntropyLoss(), _ns(a2, d, unlearn="FT_prune_bi"))
    assert len(rounds2) == len(first) and all(np.array_equal(x, y) for x, y in zip(rounds2, first))
