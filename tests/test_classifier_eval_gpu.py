"""The ResNet-34 of the classifier evaluation on the device (DDPM/models/resnet34.InferencePlan: K26, the normalise
kernel, K27, the 3 x 3 pool, the evaluation head) against a float64 copy of the same module tree on the CPU, and
DDPM/classifier_evaluation.py end to end.  Weights, inputs, references and the way the tolerance is measured (not
chosen) are in classifier_eval_fixture.py; its premises are asserted on the CPU by test_classifier_eval_host.py."""
import os

import numpy as np
import pytest
import torch

import classifier_eval_fixture as X

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_plan = {}


def plan():
    if "p" not in _plan:
        from unlearn_saliency_amd.DDPM.models.resnet34 import InferencePlan
        _plan["p"] = InferencePlan(X.models()[0], "cuda")
    return _plan["p"]


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")
    if d and os.path.isdir(d):
        with open(os.path.join(d, "classifier_eval_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("n,side", [(4, 56), (2, 224)], ids=["4x56", "2x224"])
def test_logits_against_the_float64_network(n, side):
    from unlearn_saliency_amd import conv_infer
    conv_infer.reset_library_infer_calls()
    want, figure, bound = X.network_reference(n, side)
    logits, p = plan().forward(X.network_inputs(n, side).cuda(), X.LABEL)
    got = logits.cpu().double()
    err = float((got - want).abs().max())
    top = float(want.abs().max())
    log(f"resnet34 {n} x {side} x {side}: fp32 CPU library {figure:.3e}, device {err / top:.3e} of max |logit| "
        f"(allowed {X.DEVICE_FACTOR} x the library's)")
    assert err <= bound, (err / top, figure)
    assert all(v == 0 for v in conv_infer.LIBRARY_INFER_CALLS.values()), conv_infer.LIBRARY_INFER_CALLS
    assert torch.allclose(p.cpu().double(), torch.softmax(want, -1), rtol=0, atol=10 * bound)
    again, _ = plan().forward(X.network_inputs(n, side).cuda(), X.LABEL)
    assert torch.equal(again, logits)                               # the same bits on a second run


def write_samples(root):
    from unlearn_saliency_amd.DDPM import pngio
    folder = os.path.join(root, "tmp", "a", "b", "class_samples", "0")
    os.makedirs(folder)
    for i, im in enumerate(X.images()):
        pngio.write_png(os.path.join(folder, f"{i}.png"), im)
    return folder


def test_end_to_end_script(tmp_path, monkeypatch, capsys):
    from unlearn_saliency_amd import conv_infer
    from unlearn_saliency_amd.DDPM import classifier_evaluation as ce
    ref = X.pipeline_reference()
    monkeypatch.chdir(tmp_path)
    write_samples(str(tmp_path))
    torch.save(X.state_dict(), "cifar10_resnet34.pth")
    csv_path = os.path.join("results", "cifar10", "forget", "result.csv")
    os.makedirs(os.path.dirname(csv_path))
    name0, vals0 = X.GOLDEN_ROWS[0]
    ce.update_csv(csv_path, name0, dict(zip(ce.COLUMNS, vals0)))     # a foreign row that must survive
    conv_infer.reset_library_infer_calls()
    argv = ["--sample_path", "tmp/a/b/class_samples/0", "--dataset", "cifar10", "--label_of_forgotten_class", str(X.LABEL),
            "-b", str(X.BATCH)]
    assert ce.main(argv) == 0
    out = capsys.readouterr().out.strip().splitlines()
    assert [ln.split(":")[0] for ln in out[-3:]] == ["Average entropy", "Average prob of forgotten class",
                                                     "Average accuracy of forgotten class"]
    entropy, prob, acc = (float(ln.split(":")[1]) for ln in out[-3:])
    tol = X.FIGURE_FACTOR * ref["bound"]
    log(f"classifier_evaluation 12 x 32 x 32, -b {X.BATCH}: |entropy - f64| = {abs(entropy - ref['entropy']):.3e}, "
        f"|prob - f64| = {abs(prob - ref['prob']):.3e} (allowed {tol:.3e}); fp32 CPU library figure {ref['figure']:.3e}")
    assert acc == ref["accuracy"]
    assert abs(entropy - ref["entropy"]) <= tol and abs(prob - ref["prob"]) <= tol
    assert all(v == 0 for v in conv_infer.LIBRARY_INFER_CALLS.values()), conv_infer.LIBRARY_INFER_CALLS
    # twice gives one row, named a/b; the foreign row survives; pandas reads the values back
    assert ce.main(argv) == 0
    rows = open(csv_path).read().splitlines()
    assert rows[0] == "," + ",".join(ce.COLUMNS) and [r.split(",")[0] for r in rows[1:]] == [name0, "a/b"]
    assert rows[1] == "other/run,1.25,0.1,0.0"
    assert [float(v) for v in rows[2].split(",")[1:]] == [entropy, prob, acc]
    pd = pytest.importorskip("pandas")
    df = pd.read_csv(csv_path, index_col=0)
    assert list(df.index) == [name0, "a/b"] and df.at["a/b", "accuracy of forgotten class"] == acc
    assert abs(df.at["a/b", "entropy"] - entropy) <= 1e-15 * abs(entropy)
    # the writer's format, byte for byte against the file pandas recorded from fixed numbers
    fixed = os.path.join("fixed", "result.csv")
    for name, vals in X.GOLDEN_ROWS:
        ce.update_csv(fixed, name, dict(zip(ce.COLUMNS, vals)))
    assert open(fixed, "rb").read() == open(os.path.join(GOLDEN, "classifier_eval_result.csv"), "rb").read()


def test_validate_u8_ragged_batches_equal_one_batch_in_hits_and_count():
    from unlearn_saliency_amd.DDPM import classifier_evaluation as ce
    u8 = torch.from_numpy(X.images()).cuda()
    a = ce.validate_u8(u8, X.LABEL, plan(), batch_size=5)
    b = ce.validate_u8(u8, X.LABEL, plan(), batch_size=12)
    ref = X.pipeline_reference()
    assert a["n"] == b["n"] == 12 and a["accuracy"] == b["accuracy"] == ref["accuracy"]
    assert abs(a["entropy"] - b["entropy"]) <= 1e-12 and abs(a["prob"] - b["prob"]) <= 1e-12   # same per-sample bits
