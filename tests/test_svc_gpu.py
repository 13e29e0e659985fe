"""K25 (csrc/salun_svc.hip) on the device: RBF C-SVC gram / fit / decision against sklearn's recorded answers
(tests/golden/svc_rbf.npz, made by tests/golden/make_golden_svc.py) and the float64 model (tests/svc_ref_cpu.py).

The bounds are the fixture's and the issue's, the same ones tests/test_svc_ref_cpu.py holds the model to:
  feasibility   0 <= alpha <= C exactly, |sum y alpha| <= 1e-9
  certificate   m(alpha) - M(alpha) <= eps + 2 n C 2^-24, on the host in float64 from the unrounded kernel
  decisions     max|dec_dev - dec_ref| <= b = 4 max(gap, 1e-3); the measured maxima are printed and, when
                SALUN_MEASURED_DIR is set, appended to svc_bounds_measured.txt there (profiles/ has the last ones)
  predictions   sklearn's on every query with |dec_ref| > b; attack accuracy within the fixture's within-b fraction
"""
import os
import sys
from ctypes import c_double, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

import svc_ref_cpu as R

pytestmark = pytest.mark.gpu

C, EPS = 3.0, 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svc_rbf.npz")
_g = np.load(GOLDEN)
CASES = [str(c) for c in _g["cases"]]
_fits: dict = {}


def case(name):
    return {k: _g[f"{name}/{k}"] for k in ("X", "y", "Q", "dual_coef", "support", "intercept", "dec_ref", "gap", "b",
                                            "frac", "pred_ref")}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_fit(name):
    """One device fit per case, shared by the tests below and left unchanged."""
    from unlearn_saliency_amd import ops_svc
    if name not in _fits:
        c = case(name)
        model = ops_svc.fit(dev(c["X"]), dev(c["y"]), C=C, eps=EPS)
        dec, pred = ops_svc.decision(model, dev(c["Q"]))
        _fits[name] = dict(alpha=model.alpha.cpu().numpy(), rho=float(model.rho.cpu()), it=int(model.status[0]),
                           dec=dec.cpu().numpy(), pred=pred.cpu().numpy(), gamma=model.gamma)
    return _fits[name]


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")
    if d and os.path.isdir(d):
        with open(os.path.join(d, "svc_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("name", CASES)
def test_fit_is_feasible_and_optimal(name):
    c, f = case(name), device_fit(name)
    a, n = f["alpha"], len(c["y"])
    assert f["it"] < 1e5
    assert (a >= 0).all() and (a <= C).all()
    clipped = a > C - 1e-12
    assert (a[clipped] == C).all()                                     # a clipped value IS C, bit for bit
    assert abs(np.sum(np.where(c["y"] > 0, a, -a))) <= 1e-9
    cert = R.certificate(c["X"], c["y"], a, C, f["gamma"])
    print(f"{name}: iterations {f['it']} certificate {cert:.3e}")
    assert cert <= EPS + 2 * n * C * 2.0 ** -24


@pytest.mark.parametrize("name", CASES)
def test_decisions_and_predictions_match_sklearn(name):
    c, f = case(name), device_fit(name)
    b = float(c["b"])
    err = float(np.abs(f["dec"] - c["dec_ref"]).max())
    log(f"{name}: n {len(c['y'])} iterations {f['it']} max|dec_dev - dec_ref| {err:.3e} bound b {b:.3e}")
    assert err <= b
    assert np.array_equal(f["pred"].astype(bool), f["dec"] > 0)
    clear = np.abs(c["dec_ref"]) > b
    assert np.array_equal(f["pred"][clear], c["pred_ref"][clear])
    acc = lambda p: 0.5 * (p[:300].mean() + 1 - p[300:].mean())
    assert abs(acc(f["pred"].astype(bool)) - acc(c["pred_ref"].astype(bool))) <= float(c["frac"]) + 1e-12


def test_closed_form_two_points():
    from unlearn_saliency_amd import ops_svc
    X = np.array([[0.25], [0.75]], np.float32)
    K12 = float(R.rbf_gram(X, 1.0)[0, 1])
    model = ops_svc.fit(dev(X), dev(np.array([1, 0], np.uint8)), C=C, eps=EPS)
    a, rho = model.alpha.cpu().numpy(), float(model.rho.cpu())
    want = min(C, 1.0 / (1.0 - K12))
    assert abs(a[0] - want) <= 2.0 ** -23 * want and abs(a[1] - want) <= 2.0 ** -23 * want
    assert abs(rho) <= 2.0 ** -23
    far = np.array([[0.0], [40.0]], np.float32)                         # K12 = 0: 1 / (1 - K12) = 1 < C
    model = ops_svc.fit(dev(far), dev(np.array([0, 1], np.uint8)), C=C, eps=EPS)
    assert np.abs(model.alpha.cpu().numpy() - 1.0).max() <= 2.0 ** -23 and abs(float(model.rho.cpu())) <= 2.0 ** -23


@pytest.mark.parametrize("d", [1, 10, 16])
def test_gram_entries(d):
    from unlearn_saliency_amd import ops_svc
    for n in (2, 255, 256, 257, 1025):
        X = np.random.default_rng(100 * d + n).random((n, d)).astype(np.float32)
        gamma = 1.0 / d
        ws = ops_svc.rbf_gram(dev(X), gamma)
        got = ws[:4 * n * n].view(torch.float32).view(n, n).cpu().numpy()
        want = R.rbf_gram(X, gamma)
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (n, d, int(ulps.max()))
        assert (ulps != 0).mean() <= 0.01, (n, d, float((ulps != 0).mean()))
        assert (np.diag(got) == 1.0).all()


@pytest.mark.parametrize("name", ["conf1d_1024_1024", "prob10d_1024_1024"])
def test_decision_kernel_alone(name):
    """sklearn's own dual_coef_ / support_ / intercept_ through the decision kernel."""
    from unlearn_saliency_amd import ops_svc
    c = case(name)
    gamma = 1.0 / c["X"].shape[1]
    rho = dev(np.array([-float(c["intercept"])]))
    for nsv in (1, 64, 1025):
        Xs, coef = c["X"][c["support"][:nsv]], c["dual_coef"][:nsv]
        for m in (1, 255, 257):
            dec, pred = ops_svc.decision_values(dev(Xs), dev(coef), rho, gamma, dev(c["Q"][:m]))
            want = R.decision(Xs, coef, -float(c["intercept"]), c["Q"][:m], gamma)
            assert np.abs(dec.cpu().numpy() - want).max() <= 2.0 ** -40 * np.abs(coef).sum(), (nsv, m)
            assert np.array_equal(pred.cpu().numpy().astype(bool), dec.cpu().numpy() > 0)
    # the whole support set reproduces sklearn's decision_function
    dec, _ = ops_svc.decision_values(dev(c["X"][c["support"]]), dev(c["dual_coef"]), rho, gamma, dev(c["Q"]))
    assert np.abs(dec.cpu().numpy() - c["dec_ref"]).max() <= 2.0 ** -40 * np.abs(c["dual_coef"]).sum()


def test_fit_is_deterministic():
    from unlearn_saliency_amd import ops_svc
    c = case("prob10d_1024_1024")
    X, y = dev(c["X"]), dev(c["y"])
    a = ops_svc.fit(X, y, C=C, eps=EPS)
    b = ops_svc.fit(X, y, C=C, eps=EPS)
    assert torch.equal(a.alpha.view(torch.int64), b.alpha.view(torch.int64))
    assert torch.equal(a.rho.view(torch.int64), b.rho.view(torch.int64)) and torch.equal(a.status, b.status)
    first = device_fit("prob10d_1024_1024")
    assert np.array_equal(a.alpha.cpu().numpy().view(np.int64), first["alpha"].view(np.int64))


def test_iteration_bound_is_reported():
    from unlearn_saliency_amd import ops_svc
    c = case("conf1d_64_64")
    X, y = dev(c["X"]), dev(c["y"])
    model = ops_svc.fit(X, y, C=C, eps=EPS, max_iter=1, wait=False)
    assert model.status.cpu().tolist() == [1, 0]
    a = model.alpha.cpu().numpy()
    assert (a >= 0).all() and (a <= C).all() and np.count_nonzero(a) == 2
    assert np.sum(np.where(c["y"] > 0, a, -a)) == 0
    assert np.isfinite(float(model.rho.cpu()))
    with pytest.raises(ops_svc.SvcNotConverged) as e:
        ops_svc.fit(X, y, C=C, eps=EPS, max_iter=1)
    assert e.value.iterations == 1
    assert ops_svc.default_max_iter(20_000) == 10_000_000 and ops_svc.default_max_iter(4) == 10_000_000


def test_error_codes():
    from unlearn_saliency_amd import _lib, ops_svc
    L = _lib.lib()
    q = lambda n: L.salun_svc_rbf_workspace_bytes(c_int64(n))
    assert q(1) == 0 and q(0) == 0 and q(65_537) == 0 and q(2) > 0
    assert q(65_536) >= 4 * 65_536 ** 2 and q(20_000) >= 4 * 20_000 ** 2
    n, d = 64, 3
    X = torch.rand(n, d, device="cuda")
    y = (torch.arange(n, device="cuda") % 2).to(torch.uint8)
    ws = torch.zeros(q(n), dtype=torch.uint8, device="cuda")
    alpha = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    rho = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    status = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    p = lambda t: c_void_p(t.data_ptr())
    null = c_void_p(None)

    def gram(X_=p(X), n_=n, d_=d, ws_=p(ws), bytes_=ws.numel(), gamma=0.5):
        return L.salun_svc_rbf_gram(X_, c_int64(n_), d_, c_double(gamma), ws_, c_size_t(bytes_), null)

    def fit(y_=p(y), n_=n, alpha_=p(alpha), rho_=p(rho), status_=p(status), ws_=p(ws), bytes_=ws.numel(), C_=C,
            eps=EPS, max_iter=10):
        return L.salun_svc_rbf_fit(y_, c_int64(n_), c_double(C_), c_double(eps), c_int64(max_iter), alpha_, rho_,
                                   status_, ws_, c_size_t(bytes_), null)

    def decide(X_=p(X), coef_=p(alpha), rho_=p(rho), n_=n, d_=d, Z_=p(X), m_=n, dec_=p(alpha), pred_=p(y)):
        return L.salun_svc_rbf_decision(X_, coef_, rho_, c_int64(n_), d_, c_double(0.5), Z_, c_int64(m_), dec_, pred_,
                                        null)

    E, S = _lib.SALUN_EINVAL, _lib.SALUN_ENOSPC
    assert gram(n_=1) == E and gram(n_=0) == E and gram(n_=65_537) == E
    assert gram(d_=0) == E and gram(d_=17) == E and gram(X_=null) == E and gram(ws_=null) == E
    assert gram(gamma=0.0) == E and gram(gamma=float("nan")) == E and gram(gamma=float("inf")) == E
    assert gram(bytes_=ws.numel() - 1) == S and gram(bytes_=0) == S
    assert fit(n_=1) == E and fit(n_=65_537) == E and fit(y_=null) == E and fit(alpha_=null) == E
    assert fit(rho_=null) == E and fit(status_=null) == E and fit(ws_=null) == E
    assert fit(C_=0.0) == E and fit(eps=0.0) == E and fit(max_iter=-1) == E
    assert fit(bytes_=ws.numel() - 1) == S
    assert decide(n_=0) == E and decide(d_=0) == E and decide(d_=17) == E and decide(m_=0) == E
    assert decide(X_=null) == E and decide(coef_=null) == E and decide(rho_=null) == E and decide(Z_=null) == E
    assert decide(dec_=null, pred_=null) == E
    torch.cuda.synchronize()
    assert bool((alpha == 7.0).all()) and float(rho) == 7.0 and status.tolist() == [7, 7]   # nothing was launched
    assert not bool(ws.any())
    # the wrapper: sklearn's ValueErrors
    bad = X.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        ops_svc.fit(bad, y)
    with pytest.raises(ValueError, match="both classes"):
        ops_svc.fit(X, torch.ones_like(y))
    with pytest.raises(ValueError, match="both classes"):
        ops_svc.fit(X, torch.zeros_like(y))
    with pytest.raises(ValueError):
        ops_svc.fit(torch.rand(8, 17, device="cuda"), y[:8])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops_svc.fit(X.cpu(), y.cpu())


# ------------------------------------------------------------------------------------------------- end to end
KEYS = ("correctness", "confidence", "entropy", "m_entropy", "prob")


def _eval_fixture():
    from fixtures import TinyCNN, eval_loaders, tiny_state
    model = TinyCNN()
    model.load_state_dict(tiny_state(21))
    return model.cuda(), eval_loaders()


def _check_against_reference(m):
    assert set(m) == set(KEYS)
    for k in KEYS:
        assert abs(m[k] - float(_g["e2e_ref_" + k])) <= float(_g["e2e_frac_" + k]) + 1e-9, (k, m[k])


def test_svc_mia_device_backend_matches_the_reference():
    from unlearn_saliency_amd.Classification.evaluation import SVC_MIA
    model, ld = _eval_fixture()
    m = SVC_MIA(shadow_train=ld["shadow_train"], shadow_test=ld["shadow_test"], target_train=None,
                target_test=ld["target_test"], model=model, backend="device")
    _check_against_reference(m)
    with pytest.raises(ValueError, match="backend"):
        SVC_MIA(shadow_train=ld["shadow_train"], shadow_test=ld["shadow_test"], target_train=None,
                target_test=ld["target_test"], model=model, backend="host")


def test_svc_mia_device_backend_does_not_import_sklearn(monkeypatch):
    from unlearn_saliency_amd.Classification.evaluation import SVC_MIA
    for name in [k for k in sys.modules if k == "sklearn" or k.startswith("sklearn.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "sklearn", None)                 # `import sklearn` now raises ImportError
    model, ld = _eval_fixture()
    m = SVC_MIA(shadow_train=ld["shadow_train"], shadow_test=ld["shadow_test"], target_train=None,
                target_test=ld["target_test"], model=model, backend="device")
    _check_against_reference(m)
    with pytest.raises(ImportError):
        SVC_MIA(shadow_train=ld["shadow_train"], shadow_test=ld["shadow_test"], target_train=None,
                target_test=ld["target_test"], model=model)           # the default backend needs it


def test_main_random_with_mia_device(tmp_path, monkeypatch, capsys):
    """main_random.py --synthetic --device_loader --mia device: the checkpoint holds five finite attack accuracies,
    fitted on the full-size shadow set (10,000 + 10,000 points) from device-resident loaders, without sklearn."""
    from unlearn_saliency_amd.Classification import arg_parser, main_random
    from unlearn_saliency_amd.Classification.models import model_dict
    assert arg_parser.mia_backend(arg_parser.parse_args([])) == "sklearn"
    assert arg_parser.mia_backend(arg_parser.parse_args(["--mia", "device"])) == "device"
    with pytest.raises(SystemExit):
        arg_parser.parse_args(["--mia", "host"])
    capsys.readouterr()
    monkeypatch.setitem(sys.modules, "sklearn", None)
    mask = {k: torch.ones_like(v, dtype=torch.int64) for k, v in model_dict["resnet18"](num_classes=10).named_parameters()}
    torch.save(mask, tmp_path / "ones.pt")
    result = main_random.main(["--synthetic", "--device_loader", "--mia", "device", "--save_dir", str(tmp_path / "out"),
                               "--mask_path", str(tmp_path / "ones.pt"), "--unlearn", "RL", "--unlearn_epochs", "1",
                               "--unlearn_lr", "0.013", "--num_indexes_to_replace", "200", "--class_to_replace", "0",
                               "--seed", "2", "--batch_size", "256"])
    assert "SVC_MIA skipped" not in capsys.readouterr().out
    ckpt = torch.load(tmp_path / "out" / "RLcheckpoint.pth.tar", weights_only=False)
    for res in (result, ckpt["evaluation_result"]):
        mia = res["SVC_MIA_forget_efficacy"]
        assert set(mia) == set(KEYS)
        assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in mia.values()), mia
