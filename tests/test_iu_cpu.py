"""IU / WoodFisher on the CPU: the literal loop and the scalar recurrence (tests/iu_ref_cpu.py) agree in fp64, and both
match the reference's own run (tests/golden/iu_*.npz, tests/golden/make_golden_iu.py): the fp64 run to 1e-10, its fp32
run to within the fp32 error the golden records."""
import os

import numpy as np
import pytest
import torch

import iu_ref_cpu as IU
from fixtures import TinyCNN, tiny_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(n_retain, masked):
    return np.load(os.path.join(GOLDEN, f"iu_{n_retain}_{'masked' if masked else 'unmasked'}.npz"))


def _model64():
    m = TinyCNN()
    m.load_state_dict(tiny_state(IU.MODEL_SEED))
    return m.double().eval()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.fixture(scope="module", params=IU.CASES)
def case(request):
    n_retain = request.param
    model = _model64()
    forget, retain = IU.iu_datasets(n_retain)
    v = IU.iu_v(model, forget, retain)
    G = IU.sample_grads(model, retain)
    return n_retain, model, v, G


def test_walk_length_follows_the_reference():
    assert IU.walk_len(1100) == 1002 and IU.walk_len(300) == 300


def test_literal_and_scalar_forms_agree_in_fp64(case):
    _, _, v, G = case
    k_lit = IU.literal_woodfisher(G, v)
    k_sc = IU.scalar_form(G, v)
    assert _rel(k_sc, k_lit) <= 1e-12
    assert _rel(k_lit, v) > 1e-3  # the walk does move k


def test_scalar_recurrence_tracks_o():
    """o_i = s_i g_0: the scale s of the scalar form is the literal loop's o over g_0."""
    g = torch.randn(30, 50, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    a = (g[1:] @ g[0]).tolist()
    _, s = IU.scalar_woodfisher(a, [0.0] * len(a), N=5.0)
    o = g[0].clone()
    for gi in g[1:]:
        t = torch.dot(o, gi)
        o = o - (t / (5.0 + t)) * o
    assert _rel(s * g[0], o) <= 1e-12


def test_both_forms_match_the_fp64_golden(case):
    n_retain, _, v, G = case
    gd = _golden(n_retain, False)
    assert _rel(v, gd["v64"]) <= 1e-10
    assert _rel(IU.literal_woodfisher(G, v), gd["k64"]) <= 1e-10
    assert _rel(IU.scalar_form(G, v), gd["k64"]) <= 1e-10


@pytest.mark.parametrize("masked", [False, True])
def test_final_parameters_match_the_fp64_golden(case, masked):
    n_retain, model, v, G = case
    gd = _golden(n_retain, masked)
    k = IU.scalar_form(G, v).numpy()
    m = gd["mask"].astype(np.float64) if masked else np.ones_like(k)
    p0 = np.concatenate([p.detach().reshape(-1).numpy() for p in model.parameters()])
    want = np.concatenate([gd["sd64_" + n].reshape(-1) for n, _ in model.named_parameters()])
    assert _rel(p0 + IU.ALPHA * k * m, want) <= 1e-10
    if masked:
        assert np.array_equal(want[m == 0], p0[m == 0])
        assert 0.3 < m.mean() < 0.7
    # the running statistics are untouched by IU
    for n, b in model.named_buffers():
        assert np.array_equal(gd["sd64_" + n], b.numpy()), n


@pytest.mark.parametrize("masked", [False, True])
def test_fp32_golden_within_its_recorded_error(case, masked):
    n_retain, _, v, G = case
    gd = _golden(n_retain, masked)
    k = IU.scalar_form(G, v).numpy()
    err = float(gd["fp32_rel_err_k"])
    assert err < 1e-5
    assert _rel(gd["k32"], k) <= 2 * err + 1e-12
    assert _rel(gd["v32"], v.numpy()) <= 2 * float(gd["fp32_rel_err_v"]) + 1e-12
