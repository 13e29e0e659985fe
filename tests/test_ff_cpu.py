"""Fisher forgetting on the CPU: the literal per-class loop and the grouped form (tests/ff_ref_cpu.py) agree in fp64,
and both match the reference's own run (tests/golden/ff_*.npz, tests/golden/make_golden_ff.py); the host restatement
of get_mean_var reproduces the golden mu / var, including the class-row override."""
import os

import numpy as np
import pytest
import torch

import ff_ref_cpu as FF
from fixtures import TinyCNN, tiny_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASE_NAMES = [c[0] for c in FF.CASES]


def _golden(name):
    return np.load(os.path.join(GOLDEN, f"ff_{name}.npz"))


def _model(dtype=torch.float64):
    m = TinyCNN()
    m.load_state_dict(tiny_state(FF.MODEL_SEED))
    return m.to(dtype).eval()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.fixture(scope="module")
def grad2_forms():
    model = _model()
    ds = FF.retain_dataset()
    return model, FF.literal_grad2(model, ds), FF.grouped_grad2(model, ds)


def test_retain_set_has_a_ragged_last_batch():
    assert FF.N_RETAIN == 9 * FF.BATCH + 12


def test_literal_and_grouped_forms_agree_in_fp64(grad2_forms):
    _, lit, grp = grad2_forms
    for a, b in zip(lit, grp):
        assert _rel(b.numpy(), a.numpy()) <= 1e-12


def test_both_forms_match_the_reference_fp64_golden(grad2_forms):
    model, lit, grp = grad2_forms
    g = _golden("last_row")
    for (n, _), a, b in zip(model.named_parameters(), lit, grp):
        want = g[f"g2_64_{n}"]
        assert _rel(a.numpy(), want) <= 1e-12, n
        assert _rel(b.numpy(), want) <= 1e-12, n


def test_fp32_reference_is_close_to_fp64():
    g = _golden("last_row")
    assert float(g["fp32_rel_err_grad2"]) < 1e-5


@pytest.mark.parametrize("name", CASE_NAMES)
def test_mean_var_matches_golden(name):
    g = _golden(name)
    args = FF.case_args(name)
    model = _model()
    for n, p in model.named_parameters():
        mu, var = FF.mean_var(p, torch.from_numpy(g[f"g2_64_{n}"]), args)
        assert np.array_equal(mu.numpy(), g[f"mu_64_{n}"]), n
        assert _rel(var.numpy(), g[f"var_64_{n}"]) <= 1e-14, n


def test_override_cases_pin_the_rows():
    """(4500, cifar10, -1) zeroes the LAST class row of fc.weight / fc.bias with variance 1e-3; an explicit class
    overrides that row; the third case overrides nothing."""
    last, c3, none = _golden("last_row"), _golden("class3"), _golden("no_override")
    for key in ("fc.weight", "fc.bias"):
        assert np.all(last[f"mu_64_{key}"][-1] == 0) and np.allclose(last[f"var_64_{key}"][-1], 1e-3, rtol=1e-12)
        assert np.all(c3[f"mu_64_{key}"][3] == 0) and np.allclose(c3[f"var_64_{key}"][3], 1e-3, rtol=1e-12)
        assert not np.any(np.all(none[f"mu_64_{key}"].reshape(10, -1) == 0, axis=1))
        assert np.all(none[f"var_64_{key}"] > 1e-3)


def test_capture_frees_its_activations_without_the_garbage_collector():
    """The Fisher pass runs once per batch of 32 over the whole retain set: whatever `_capture` returns must be freed by
    reference counting alone (a record -> output -> hook -> record cycle kept every batch's activations alive until a
    garbage-collector pass, and filled the device on a 40,500-sample retain set)."""
    import gc
    import weakref
    from unlearn_saliency_amd import persample
    m = TinyCNN().eval()
    enabled = gc.isenabled()
    gc.disable()
    try:
        recs, _ = persample._capture(m, torch.rand(20, 3, 8, 8), lambda lg, k: lg.sum())
        refs = [weakref.ref(r[4][0]) for r in recs if r[4]]
        assert len(refs) >= 4
        del recs
        assert all(r() is None for r in refs)
    finally:
        if enabled:
            gc.enable()
