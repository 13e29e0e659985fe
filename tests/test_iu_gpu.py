"""IU / WoodFisher (`--unlearn wfisher`) on the GPU: the K17 kernels (csrc/salun_iu.hip) against fp64 host
restatements, the per-sample pass (persample.py) against per-sample autograd gradients, the plugin against the
reference's fp64 run (tests/golden/iu_*.npz), and the command line on full-size ResNet-18."""
import copy
import os
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import iu_ref_cpu as IU
from fixtures import TinyCNN, tiny_state

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _t(a, offset=0):
    """`a` on the device; offset 1 puts it one element into its allocation (not 16-byte aligned: the scalar route)."""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return torch.cat([t.new_zeros(offset), t])[offset:] if offset else t


def _rand(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("B,K,P,Q", [(1, 3, 7, 7), (5, 16, 8, 8), (3, 64, 3, 11), (2, 8, 32, 32), (1, 512, 4, 4)])
def test_conv_dot_vs_fp64_host(B, K, P, Q):
    from unlearn_saliency_amd import ops_iu
    y2, dy = _rand((B, 2 * K, P, Q), 1), _rand((B, K, P, Q), 2)
    want = np.stack([(y2[:, :K].astype(np.float64) * dy).reshape(B, -1).sum(1),
                     (y2[:, K:].astype(np.float64) * dy).reshape(B, -1).sum(1)], 1) + 0.5
    outs = []
    for _ in range(2):
        out = torch.full((B, 2), 0.5, dtype=torch.float64, device="cuda")  # accumulated into
        ops_iu.conv_dot(_t(y2), _t(dy), out)
        outs.append(out.cpu().numpy())
    scale = np.abs(y2).reshape(B, 2, -1).max() * np.abs(dy).reshape(B, -1).sum(1)[:, None]
    assert np.all(np.abs(outs[0] - want) <= 1e-12 * scale + 1e-12)
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))


@pytest.mark.parametrize("B,C,H,W", [(1, 3, 7, 7), (4, 16, 5, 5), (2, 64, 4, 4), (3, 8, 32, 32), (1, 5, 1, 1)])
def test_bn_dot_vs_fp64_host(B, C, H, W):
    from unlearn_saliency_amd import ops_iu
    x, dy = _rand((B, C, H, W), 3), _rand((B, C, H, W), 4)
    rm = _rand(C, 5) * 0.1
    rv = (np.abs(_rand(C, 6)) + 0.5).astype(np.float32)
    u = [_rand(C, 10 + j) for j in range(4)]
    eps = 1e-5
    xh = (x.astype(np.float64) - rm[None, :, None, None]) / np.sqrt(rv.astype(np.float64)[None, :, None, None] + eps)
    want = np.stack([(dy * (u[2 * j][None, :, None, None] * xh + u[2 * j + 1][None, :, None, None])).reshape(B, -1)
                     .sum(1) for j in range(2)], 1)
    outs = []
    for _ in range(2):
        out = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
        ops_iu.bn_dot(_t(x), _t(dy), _t(rm), _t(rv), eps, _t(u[0]), _t(u[1]), _t(u[2]), _t(u[3]), out)
        outs.append(out.cpu().numpy())
    scale = (np.abs(dy) * (np.abs(xh) + 1) * 3).reshape(B, -1).sum(1)[:, None]
    assert np.all(np.abs(outs[0] - want) <= 1e-12 * scale)
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))


@pytest.mark.parametrize("B,M,K,bias", [(1, 10, 16, True), (7, 10, 512, True), (3, 5, 33, False), (300, 10, 512, True)])
def test_linear_dot_vs_fp64_host(B, M, K, bias):
    from unlearn_saliency_amd import ops_iu
    x, dy = _rand((B, K), 7), _rand((B, M), 8)
    w0, w1 = _rand((M, K), 9), _rand((M, K), 10)
    b0, b1 = (_rand(M, 11), _rand(M, 12)) if bias else (None, None)
    want = []
    for w, b in ((w0, b0), (w1, b1)):
        z = x.astype(np.float64) @ w.astype(np.float64).T + (0.0 if b is None else b.astype(np.float64))
        want.append((dy * z).sum(1))
    want = np.stack(want, 1)
    opt = lambda a: None if a is None else _t(a)
    outs = []
    for _ in range(2):
        out = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
        ops_iu.linear_dot(_t(x), _t(dy), _t(w0), opt(b0), _t(w1), opt(b1), out)
        outs.append(out.cpu().numpy())
    assert np.allclose(outs[0], want, rtol=1e-12, atol=1e-10)
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))


@pytest.mark.parametrize("n", [1002, 300])
def test_recurrence_vs_fp64_host_loop(n):
    from unlearn_saliency_amd import ops_iu
    rng = np.random.default_rng(n)
    a = np.abs(rng.standard_normal(n - 1)) * 50.0  # <g_0, g_i> of nearby samples: mostly positive, O(N / 20)
    b = rng.standard_normal(n - 1) * 5.0
    beta, s = IU.scalar_woodfisher(a.tolist(), b.tolist())
    got = ops_iu.recurrence(_t(np.stack([a, b], 1))).cpu().numpy()
    assert abs(got[0] - beta) <= 1e-13 * max(1.0, abs(beta))
    assert abs(got[1] - s) <= 1e-13 * s
    # the literal two-vector loop on explicit vectors agrees with the scalar form the kernel runs
    G = torch.from_numpy(rng.standard_normal((min(n, 60), 40)))
    v = torch.from_numpy(rng.standard_normal(40))
    ab = np.stack([(G[1:] @ G[0]).numpy(), (G[1:] @ v).numpy()], 1)
    bt = float(ops_iu.recurrence(_t(ab), 30.0)[0])
    k = IU.literal_woodfisher(G, v, 30.0)
    assert torch.allclose(v - bt * G[0], k, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [1_000_003, 1, 4097])
def test_apply_bit_exact_vs_host(masked, n, offset=0):
    from unlearn_saliency_amd import ops_iu
    p, v, g = _rand(n, 20), _rand(n, 21), _rand(n, 22)
    m = (np.random.default_rng(23).integers(0, 2, n)).astype(np.uint8) if masked else None
    beta, alpha = 0.3712, 0.2
    want = (p.astype(np.float64) + alpha * (v.astype(np.float64) - beta * g.astype(np.float64))).astype(np.float32)
    if masked:
        want = np.where(m != 0, want, p)
    d_p = _t(p.copy(), offset)
    ops_iu.apply(d_p, _t(v, offset), _t(g, offset), torch.tensor([beta, 1.0], dtype=torch.float64, device="cuda"),
                 None if m is None else _t(m, offset), alpha)
    assert np.array_equal(d_p.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("offset", [0, 1])
def test_apply_bit_exact_vs_host_wrap(offset):
    """The same check once past the streaming kernels' grid-stride wrap (2048 workgroups x 4096-element tiles, then a
    second pass whose first tile has two full sub-vectors, a third with 100 live lanes and a fourth with none, then a
    3-element tail), on the float4 route and on the scalar route."""
    test_apply_bit_exact_vs_host(True, 2048 * 4096 + 4 * (2 * 256 + 100) + 3, offset)


def test_apply_unaligned_tail():
    from unlearn_saliency_amd import ops_iu
    n = 1031
    base = _rand(n + 1, 30)
    v, g = _rand(n + 1, 31), _rand(n + 1, 32)
    m = (np.arange(n + 1) % 3 != 0).astype(np.uint8)
    d_p = _t(base.copy())
    beta = torch.tensor([-1.25, 1.0], dtype=torch.float64, device="cuda")
    ops_iu.apply(d_p[1:], _t(v)[1:], _t(g)[1:], beta, _t(m)[1:], 0.5)  # 4-byte-offset views: the scalar path
    want = base.copy()
    upd = (base[1:].astype(np.float64) + 0.5 * (v[1:].astype(np.float64) + 1.25 * g[1:].astype(np.float64)))
    want[1:] = np.where(m[1:] != 0, upd.astype(np.float32), base[1:])
    assert np.array_equal(d_p.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------- 2. per-sample pass
def _product_resnet18():
    from unlearn_saliency_amd.Classification.models import model_dict
    from unlearn_saliency_amd.conv import use_salun_convs
    from unlearn_saliency_amd.norm import use_fused_bn
    torch.manual_seed(0)
    m = model_dict["resnet18"](num_classes=10).cuda()
    with torch.no_grad():  # running statistics away from (0, 1) so that the eval-mode BN term is exercised
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 2.0)
                mod.bias.uniform_(-0.1, 0.1)
    use_salun_convs(m)
    use_fused_bn(m)
    return m


def _tiny():
    m = TinyCNN()
    m.load_state_dict(tiny_state(IU.MODEL_SEED))
    return m.cuda()


def _per_sample_grads(model, x, y):
    """batch-1 autograd gradients (eval) on an independent copy of the model with its own flat arena."""
    from unlearn_saliency_amd.flat import arena_of
    ref = copy.deepcopy(model)
    ref.eval()
    a = arena_of(ref)
    out = []
    for i in range(x.shape[0]):
        a.zero_grad()
        nn.functional.cross_entropy(ref(x[i:i + 1]), y[i:i + 1]).backward()
        out.append(a.grads.double().clone())
    a.zero_grad()
    nn.functional.cross_entropy(ref(x), y, reduction="sum").backward()
    return torch.stack(out), a.grads.double().clone()


@pytest.mark.parametrize("which", ["tiny", "resnet18"])
def test_persample_dots_vs_per_sample_autograd(which):
    from unlearn_saliency_amd import conv as sconv
    from unlearn_saliency_amd.flat import arena_of
    from unlearn_saliency_amd.persample import persample_dots
    model = _tiny() if which == "tiny" else _product_resnet18()
    shape = (16, 3, 8, 8) if which == "tiny" else (16, 3, 32, 32)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(shape, device="cuda", generator=g)
    y = torch.randint(0, 10, (shape[0],), device="cuda", generator=g)
    arena = arena_of(model)
    u0 = torch.randn(arena.n, device="cuda", generator=g)
    u1 = torch.randn(arena.n, device="cuda", generator=g) * 1e-2
    G, Gsum = _per_sample_grads(model, x, y)

    model.train()  # persample runs in eval and puts the mode back
    arena.grads.copy_(torch.randn(arena.n, device="cuda", generator=g))
    grads_before = arena.grads.clone()
    bufs_before = {k: b.clone() for k, b in model.named_buffers()}
    flags_before = [(m, getattr(m, "fused_bn", None), getattr(m, "fused_block", None)) for m in model.modules()]
    sconv.reset_library_conv_calls()
    got = persample_dots(model, x, y, u0, u1)
    got2 = persample_dots(model, x, y, u0, u1)
    torch.cuda.synchronize()
    if which == "resnet18":
        assert sconv.library_conv_calls() == 0, sconv.LIBRARY_CONV_CALLS
    assert torch.equal(got.view(torch.int64), got2.view(torch.int64))  # deterministic
    assert model.training and all(p.requires_grad for p in model.parameters())
    assert torch.equal(arena.grads, grads_before)
    assert all(p.grad.data_ptr() == arena.grads.data_ptr() + 4 * o for p, o in zip(arena._params, arena.offsets))
    for k, b in model.named_buffers():
        assert torch.equal(b, bufs_before[k]), k
    assert [(m, getattr(m, "fused_bn", None), getattr(m, "fused_block", None)) for m in model.modules()] == flags_before

    for j, u in enumerate((u0.double(), u1.double())):
        want = G @ u
        tol = 1e-5 * G.norm(dim=1) * u.norm()
        assert torch.all((got[:, j] - want).abs() <= tol), (which, j, (got[:, j] - want).abs().max().item())
        # batch identity: sum_i <g_i, u> = <grad sum_i l_i, u>
        assert abs(float(got[:, j].sum()) - float(Gsum @ u)) <= 1e-5 * float(Gsum.norm() * u.norm()) + float(tol.sum())


def test_persample_refuses_unsupported_modules():
    from unlearn_saliency_amd.flat import arena_of
    from unlearn_saliency_amd.persample import persample_dots
    m = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.GroupNorm(2, 8), nn.Flatten(), nn.Linear(8 * 4 * 4, 10)).cuda()
    a = arena_of(m)
    u = torch.zeros(a.n, device="cuda")
    with pytest.raises(NotImplementedError, match="GroupNorm"):
        persample_dots(m, torch.rand(2, 3, 4, 4, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"), u, u)


# --------------------------------------------------------------------------------------------- 4. plugin
def _golden(n_retain, masked):
    return np.load(os.path.join(GOLDEN, f"iu_{n_retain}_{'masked' if masked else 'unmasked'}.npz"))


def _plugin_inputs(n_retain):
    from unlearn_saliency_amd.Classification.dataset import BatchLoader
    forget, retain = IU.iu_datasets(n_retain)
    loaders = {"forget": BatchLoader(forget, IU.BATCH, True), "retain": BatchLoader(retain, IU.BATCH, True)}
    args = SimpleNamespace(batch_size=IU.BATCH, alpha=IU.ALPHA, gpu=0)
    return loaders, args


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("n_retain", IU.CASES)
def test_wfisher_plugin_vs_fp64_golden(n_retain):
    from unlearn_saliency_amd.Classification import unlearn
    from unlearn_saliency_amd.Classification.unlearn.Wfisher import iu_perturbation
    loaders, args = _plugin_inputs(n_retain)
    for masked in (False, True):
        gd = _golden(n_retain, masked)
        model = _tiny()
        names = [n for n, _ in model.named_parameters()]
        p0 = np.concatenate([p.detach().reshape(-1).cpu().numpy() for p in model.parameters()])
        iu = iu_perturbation(loaders, model, nn.CrossEntropyLoss(), args)
        assert iu.n == IU.walk_len(n_retain) and iu.ab.shape == (iu.n - 1, 2)
        k = (iu.v.double() - iu.beta[0] * iu.g0.double()).cpu().numpy()
        assert _rel(iu.v.cpu().numpy(), gd["v64"]) <= 1e-5
        assert _rel(k, gd["k64"]) <= 1e-5, _rel(k, gd["k64"])

        model = _tiny()
        mask = None
        if masked:
            mflat = gd["mask"].astype(np.int64)
            off = np.cumsum([0] + [p.numel() for p in model.parameters()])
            mask = {n: torch.from_numpy(mflat[off[i]:off[i + 1]]).view_as(p).cuda()
                    for i, (n, p) in enumerate(model.named_parameters())}
        method = unlearn.get_unlearn_method("wfisher")
        method(loaders, model, nn.CrossEntropyLoss(), args, mask) if masked else \
            method(loaders, model, nn.CrossEntropyLoss(), args)
        now = np.concatenate([model.state_dict()[n].reshape(-1).cpu().numpy() for n in names])
        want = np.concatenate([gd["sd64_" + n].reshape(-1) for n in names])
        m = gd["mask"] != 0 if masked else np.ones_like(now, bool)
        delta, want_delta = now.astype(np.float64) - p0, want - p0
        assert _rel(delta, want_delta) <= 1e-5 + 4 * np.finfo(np.float32).eps * np.linalg.norm(p0) / np.linalg.norm(
            want_delta)
        if masked:
            assert np.array_equal(now[~m].view(np.uint32), p0[~m].view(np.uint32))  # bit-unchanged
            assert (now[m] != p0[m]).mean() > 0.5
        for n, b in model.named_buffers():
            assert np.array_equal(b.cpu().numpy(), gd["sd64_" + n].astype(b.cpu().numpy().dtype)), n


def test_wfisher_walk_is_deterministic():
    """Given v and g_0, the walk (per-sample dots of every batch, then the recurrence) is bit-identical between runs.
    (F, R and g_0 themselves come from the model's own backward, whose library kernels need not be.)"""
    from unlearn_saliency_amd.Classification.dataset import BatchLoader
    from unlearn_saliency_amd.Classification.unlearn.Wfisher import _head, iu_perturbation
    from unlearn_saliency_amd import ops_iu
    from unlearn_saliency_amd.persample import persample_dots
    loaders, args = _plugin_inputs(1100)
    model = _tiny()
    iu = iu_perturbation(loaders, model, nn.CrossEntropyLoss(), args)
    ab = torch.zeros_like(iu.ab)
    off = 0
    for i, (x, y) in enumerate(BatchLoader(_head(loaders["retain"].dataset, iu.n), IU.BATCH, False)):
        x, y = x.cuda(), y.cuda()
        if i == 0:
            x, y = x[1:], y[1:]
        persample_dots(model, x, y, iu.g0, iu.v, out=ab[off:off + x.shape[0]])
        off += x.shape[0]
    assert off == iu.n - 1 == 1001
    assert torch.equal(ab.view(torch.int64), iu.ab.view(torch.int64))
    beta = ops_iu.recurrence(ab, 1000.0)
    assert torch.equal(beta.view(torch.int64), iu.beta.view(torch.int64))


def test_wfisher_refuses_data_parallel(monkeypatch):
    from unlearn_saliency_amd import dist as sdist
    from unlearn_saliency_amd.Classification import unlearn
    loaders, args = _plugin_inputs(300)
    monkeypatch.setattr(sdist, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        unlearn.get_unlearn_method("wfisher")(loaders, _tiny(), nn.CrossEntropyLoss(), args)


# ------------------------------------------------------------------------------------------ 5. command line
def test_main_forget_wfisher_resnet18(capsys):
    from unlearn_saliency_amd import conv as sconv
    from unlearn_saliency_amd.Classification import main_forget
    with tempfile.TemporaryDirectory() as d:
        sconv.reset_library_conv_calls()
        result = main_forget.main(["--synthetic", "--device_loader", "--unlearn", "wfisher", "--alpha", "0.2",
                                   "--num_indexes_to_replace", "4500", "--save_dir", d, "--batch_size", "256"])
        text = capsys.readouterr().out
        assert "number of forget dataset 4500" in text and "number of retain dataset 40500" in text
        assert sconv.library_conv_calls() == 0, sconv.LIBRARY_CONV_CALLS
        assert os.path.exists(os.path.join(d, "wfishercheckpoint.pth.tar"))
        assert os.path.exists(os.path.join(d, "wfishereval_result.pth.tar"))
        acc = result["accuracy"]
        assert list(acc.keys()) == ["retain", "forget", "val", "test"]
        assert all(0.0 <= float(v) <= 100.0 for v in acc.values())
        sd = torch.load(os.path.join(d, "wfishercheckpoint.pth.tar"), weights_only=False)["state_dict"]
        assert all(torch.isfinite(v).all() for v in sd.values() if v.dtype.is_floating_point)
