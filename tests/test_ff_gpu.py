"""Fisher forgetting (`--unlearn fisher_new`) on the GPU: the K18 kernels (csrc/salun_ff.hip) against fp64 host
restatements, the Fisher pass (persample.fisher_diag) against the reference's fp64 run (tests/golden/ff_*.npz) and the
literal per-class loop, the plugin against the golden mu / var, and the command line on full-size ResNet-18.

Tolerances are relative to the fp64 truth.  The reference's own fp32 run is 2.1e-7 off it in grad2 (recorded in the
goldens as fp32_rel_err_grad2); the bounds below are 1e-5, i.e. about 50x that, which covers the fp32 MFMA sums of the
backward-weight kernels (measured on the MI355X: <= 2e-6 on the kernel shapes, ~4e-7 on TinyCNN)."""
import os
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import ff_ref_cpu as FF
from fixtures import TinyCNN, tiny_state

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rand(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _weights(G, seed):
    w = np.abs(_rand(G, seed)) + 0.1
    return (w / w.sum()).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. kernels
CONV_SHAPES = [  # (C, K, H, R, stride, pad)
    (3, 64, 32, 3, 1, 1),      # RGB stem
    (64, 64, 32, 3, 1, 1),
    (64, 128, 32, 3, 2, 1),
    (64, 128, 32, 1, 2, 0),
    (512, 512, 4, 3, 1, 1),
]
GB = [(1, 1), (1, 12), (10, 12), (10, 32)]


@pytest.mark.parametrize("C,K,H,R,stride,pad", CONV_SHAPES)
@pytest.mark.parametrize("G,B", GB)
def test_conv_sq_vs_fp64_host(C, K, H, R, stride, pad, G, B):
    from unlearn_saliency_amd import ops_ff
    P = (H + 2 * pad - R) // stride + 1
    x, dy = _rand((B, C, H, H), 1), _rand((G * B, K, P, P), 2)
    w = _weights(G, 3)
    xd = torch.from_numpy(x).double()
    want = torch.zeros((K, C, R, R), dtype=torch.float64)
    for g in range(G):
        s = torch.nn.grad.conv2d_weight(xd, (K, C, R, R), torch.from_numpy(dy[g * B:(g + 1) * B]).double(),
                                        stride=stride, padding=pad)
        want += float(w[g]) * s * s
    want = want.numpy() + 0.5
    outs = []
    for _ in range(2):
        F = torch.full((K, C, R, R), 0.5, device="cuda")  # added into
        ops_ff.conv_sq(_t(x), _t(dy), _t(w), F, stride, pad)
        outs.append(F.cpu().numpy())
    assert _rel(outs[0] - 0.5, want - 0.5) <= 1e-5
    assert np.max(np.abs(outs[0] - want)) <= 1e-4 * np.max(np.abs(want - 0.5)) + 1e-6
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


@pytest.mark.parametrize("G,B", [(1, 1), (1, 32), (10, 12), (10, 32)])
def test_linear_sq_vs_fp64_host(G, B):
    from unlearn_saliency_amd import ops_ff
    M, K = 10, 512
    x, dy, w = _rand((B, K), 4), _rand((G * B, M), 5), _weights(G, 6)
    want = np.full((M, K), 0.25)
    for g in range(G):
        s = dy[g * B:(g + 1) * B].astype(np.float64).T @ x.astype(np.float64)
        want += w[g] * s * s
    outs = []
    for _ in range(2):
        F = torch.full((M, K), 0.25, device="cuda")
        ops_ff.linear_sq(_t(x), _t(dy), _t(w), F)
        outs.append(F.cpu().numpy())
    assert _rel(outs[0] - 0.25, want - 0.25) <= 1e-6
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


@pytest.mark.parametrize("C,H,G,B", [(64, 32, 10, 32), (512, 4, 10, 12), (8, 8, 1, 1), (10, 1, 10, 32)])
def test_vec_sq_vs_fp64_host(C, H, G, B):
    from unlearn_saliency_amd import ops_ff
    x, dy, w = _rand((B, C, H, H), 7), _rand((G * B, C, H, H), 8), _weights(G, 9)
    rm = _rand(C, 10) * 0.1
    rv = (np.abs(_rand(C, 11)) + 0.5).astype(np.float32)
    eps = 1e-5
    xh = (x.astype(np.float64) - rm[None, :, None, None]) / np.sqrt(rv.astype(np.float64)[None, :, None, None] + eps)
    want_b, want_g = np.ones(C), np.ones(C)
    for g in range(G):
        d = dy[g * B:(g + 1) * B].astype(np.float64)
        want_b += w[g] * d.sum((0, 2, 3)) ** 2
        want_g += w[g] * (d * xh).sum((0, 2, 3)) ** 2
    outs = []
    for _ in range(2):
        Fb, Fg, Fbias = (torch.ones(C, device="cuda") for _ in range(3))
        ops_ff.vec_sq(_t(dy), _t(w), Fb, B, _t(x), _t(rm), _t(rv), eps, Fg)
        ops_ff.vec_sq(_t(dy), _t(w), Fbias, B)  # a bias: the beta sums alone
        outs.append([t.cpu().numpy() for t in (Fb, Fg, Fbias)])
    assert _rel(outs[0][0] - 1, want_b - 1) <= 1e-6
    assert _rel(outs[0][1] - 1, want_g - 1) <= 1e-6
    assert np.array_equal(outs[0][2], outs[0][0])
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _golden(name):
    return np.load(os.path.join(GOLDEN, f"ff_{name}.npz"))


def _tiny():
    m = TinyCNN()
    m.load_state_dict(tiny_state(FF.MODEL_SEED))
    return m.cuda()


@pytest.mark.parametrize("name", ["last_row", "class3", "no_override"])
def test_apply_vs_host_get_mean_var(name):
    """salun_ff_apply against the host restatement of get_mean_var on the golden grad2, with z regenerated by
    ops.fill_normal (the override at index -1, at an explicit index, and not at all)."""
    from unlearn_saliency_amd import ops, ops_ff
    from unlearn_saliency_amd.flat import arena_of
    g, args = _golden(name), FF.case_args(name)
    model = _tiny()
    arena = arena_of(model)
    names = [n for n, _ in model.named_parameters()]
    nb = 10
    F = torch.cat([torch.from_numpy(g[f"g2_32_{n}"]).reshape(-1) * nb for n in names]).float().cuda()
    mu_want, var_want = [], []
    for n, p in zip(names, arena._params):
        mu, var = FF.mean_var(p.detach().cpu().double(), F[arena.offsets[names.index(n)]:][:p.numel()]
                              .cpu().double().view(p.shape) / nb, args)
        mu_want.append(mu.reshape(-1))
        var_want.append(var.reshape(-1))
    mu_want, var_want = torch.cat(mu_want).numpy(), torch.cat(var_want).numpy()
    z = ops.fill_normal(arena.n, args.seed).cpu().numpy().astype(np.float64)
    want = mu_want + np.sqrt(var_want) * z
    ops_ff.apply(arena.params, F, [p.shape for p in arena._params], args.num_classes, FF.override_row(args), nb,
                 args.alpha, args.seed)
    got = arena.params.cpu().numpy()
    scale = np.abs(np.sqrt(var_want) * z) + np.abs(mu_want)
    assert np.all(np.abs(got - want) <= 1e-5 * scale + 1e-7), np.max(np.abs(got - want) / (scale + 1e-7))
    fcw = model.fc.weight.detach().cpu().numpy()
    row = FF.override_row(args)
    if row is not None:  # mu = 0, var = 1e-4 x 10: the row is exactly sqrt(1e-3) z
        off = arena.offsets[names.index("fc.weight")]
        zr = z[off:off + fcw.size].reshape(fcw.shape)[row]
        assert np.allclose(fcw[row], np.float32(np.sqrt(np.float32(1e-3))) * zr, rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------- 2. Fisher pass
@pytest.mark.parametrize("form", ["replicate", "loop"])
def test_fisher_diag_tinycnn_vs_fp64_golden(form):
    from unlearn_saliency_amd.flat import arena_of
    from unlearn_saliency_amd.persample import fisher_diag
    g = _golden("last_row")
    model = _tiny()
    arena = arena_of(model)
    names = [n for n, _ in model.named_parameters()]
    F = arena.new_like()
    nb = 0
    for x in FF.batches(FF.retain_dataset(), FF.BATCH, torch.float32):
        fisher_diag(model, x.cuda(), FF.NUM_CLASSES, F, arena=arena, form=form)
        nb += 1
    assert nb == 10
    assert model.training and all(p.requires_grad for p in model.parameters())
    got = (F / nb).cpu().numpy()
    for n, o, k in zip(names, arena.offsets, arena.numels):
        assert _rel(got[o:o + k], g[f"g2_64_{n}"].reshape(-1)) <= 1e-5, (n, _rel(got[o:o + k], g[f"g2_64_{n}"]))
    F2 = arena.new_like()
    for x in FF.batches(FF.retain_dataset(), FF.BATCH, torch.float32):
        fisher_diag(model, x.cuda(), FF.NUM_CLASSES, F2, arena=arena, form=form)
    assert torch.equal(F.view(torch.int32), F2.view(torch.int32))  # deterministic


def test_fisher_diag_resnet18_vs_literal_loop():
    """Full-size ResNet-18 (CIFAR stem), two batches (4 and a ragged 3) against the reference's per-class loop in
    fp64 on the host."""
    from unlearn_saliency_amd import conv as sconv
    from unlearn_saliency_amd.Classification.models import model_dict
    from unlearn_saliency_amd.flat import arena_of
    from unlearn_saliency_amd.persample import fisher_diag
    torch.manual_seed(0)
    ref = model_dict["resnet18"](num_classes=10)
    for m in ref.modules():  # non-trivial running statistics
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.uniform_(-0.1, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    fast = model_dict["resnet18"](num_classes=10).cuda()
    fast.load_state_dict(ref.state_dict())
    sconv.use_salun_convs(fast)
    arena = arena_of(fast)
    xs = [torch.rand(4, 3, 32, 32), torch.rand(3, 3, 32, 32)]
    F = arena.new_like()
    sconv.reset_library_conv_calls()
    for x in xs:
        fisher_diag(fast, x.cuda(), 10, F, arena=arena)
    torch.cuda.synchronize()
    assert sconv.library_conv_calls() == 0, sconv.LIBRARY_CONV_CALLS
    got = (F / len(xs)).cpu().numpy()

    class _DS:
        def __init__(self, xs):
            self.items = [(t, 0) for x in xs for t in x]

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            return self.items[i]

    ref = ref.double().eval()
    torch.set_num_threads(16)
    want = torch.cat([t.reshape(-1) for t in FF.literal_grad2(ref, _DS(xs), bs=4)]).numpy()
    assert _rel(got, want) <= 1e-5, _rel(got, want)
    for n, o, k in zip([n for n, _ in fast.named_parameters()], arena.offsets, arena.numels):
        assert _rel(got[o:o + k], want[o:o + k]) <= 1e-4, n


def test_fisher_diag_refuses_unsupported_modules():
    from unlearn_saliency_amd.flat import arena_of
    from unlearn_saliency_amd.persample import fisher_diag
    m = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.GroupNorm(2, 8), nn.Flatten(), nn.Linear(8 * 4 * 4, 10)).cuda()
    a = arena_of(m)
    with pytest.raises(NotImplementedError, match="GroupNorm"):
        fisher_diag(m, torch.rand(2, 3, 4, 4, device="cuda"), 10, a.new_like())


# --------------------------------------------------------------------------------------------- 3. plugin
def _plugin_inputs(name):
    from unlearn_saliency_amd.Classification.dataset import BatchLoader
    return {"retain": BatchLoader(FF.retain_dataset(), 64, True)}, FF.case_args(name)


@pytest.mark.parametrize("name", ["last_row", "class3", "no_override"])
def test_fisher_new_plugin_vs_golden(name):
    from unlearn_saliency_amd import ops
    from unlearn_saliency_amd.Classification import unlearn
    g = _golden(name)
    loaders, args = _plugin_inputs(name)
    model = _tiny()
    names = [n for n, _ in model.named_parameters()]
    model.train()
    out = unlearn.get_unlearn_method("fisher_new")(loaders, model, nn.CrossEntropyLoss(), args)
    assert out is model and not model.training  # left in eval mode, as the reference leaves it
    now = np.concatenate([p.detach().reshape(-1).cpu().numpy() for p in model.parameters()]).astype(np.float64)
    mu = np.concatenate([g[f"mu_64_{n}"].reshape(-1) for n in names])
    sd = np.sqrt(np.concatenate([g[f"var_64_{n}"].reshape(-1) for n in names]))
    z = ops.fill_normal(now.size, args.seed).cpu().numpy().astype(np.float64)
    want = mu + sd * z
    assert np.all(np.abs(now - want) <= 1e-5 * (np.abs(sd * z) + np.abs(mu)) + 1e-7)
    for n, b in model.named_buffers():  # running statistics untouched
        assert np.array_equal(b.cpu().numpy(), g["sd_" + n].astype(b.cpu().numpy().dtype)), n


def test_fisher_new_refuses_a_mask_and_data_parallel(monkeypatch):
    from unlearn_saliency_amd import dist as sdist
    from unlearn_saliency_amd.Classification import unlearn
    loaders, args = _plugin_inputs("last_row")
    model = _tiny()
    before = [p.detach().clone() for p in model.parameters()]
    mask = {n: torch.ones_like(p) for n, p in model.named_parameters()}
    with pytest.raises(NotImplementedError, match="mask"):
        unlearn.get_unlearn_method("fisher_new")(loaders, model, nn.CrossEntropyLoss(), args, mask)
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
    monkeypatch.setattr(sdist, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size 1"):
        unlearn.get_unlearn_method("fisher_new")(loaders, model, nn.CrossEntropyLoss(), args)


# ------------------------------------------------------------------------------------------ 4. command line
def test_main_forget_fisher_new_resnet18(capsys):
    from unlearn_saliency_amd import conv as sconv
    from unlearn_saliency_amd.Classification import main_forget
    with tempfile.TemporaryDirectory() as d:
        sconv.reset_library_conv_calls()
        result = main_forget.main(["--synthetic", "--device_loader", "--unlearn", "fisher_new", "--alpha", "1e-6",
                                   "--num_indexes_to_replace", "4500", "--save_dir", d, "--batch_size", "256"])
        text = capsys.readouterr().out
        assert "number of forget dataset 4500" in text and "number of retain dataset 40500" in text
        assert sconv.library_conv_calls() == 0, sconv.LIBRARY_CONV_CALLS
        assert os.path.exists(os.path.join(d, "fisher_newcheckpoint.pth.tar"))
        acc = result["accuracy"]
        assert list(acc.keys()) == ["retain", "forget", "val", "test"]
        assert all(0.0 <= float(v) <= 100.0 for v in acc.values())
        sd = torch.load(os.path.join(d, "fisher_newcheckpoint.pth.tar"), weights_only=False)["state_dict"]
        assert all(torch.isfinite(v).all() for v in sd.values() if v.dtype.is_floating_point)
        w = sd["fc.weight"] if "fc.weight" in sd else sd["module.fc.weight"]
        # the (4500, cifar10, class -1) quirk: the last class row is pure noise of variance 1e-3
        assert float(w[-1].pow(2).mean().sqrt()) == pytest.approx(float(np.sqrt(1e-3)), rel=0.2)
