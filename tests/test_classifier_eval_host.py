"""The host side of DDPM/classifier_evaluation.py and DDPM/models/resnet34.py (no GPU needed): the parser, the refusal
without a device, the module tree's names, the folded BatchNorm, the folder reader, the CSV writer, and the premise of
the end-to-end GPU test (every sample's float64 top-two gap is far above the rounding allowance)."""
import json
import os

import numpy as np
import pytest
import torch

import classifier_eval_fixture as X
import conv_infer_ref_cpu as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def ce():
    from unlearn_saliency_amd.DDPM import classifier_evaluation
    return classifier_evaluation


def test_parser_flags_and_defaults_are_the_references():
    p = ce().build_parser()
    a = p.parse_args([])
    assert (a.sample_path, a.dataset, a.label_of_forgotten_class, a.batch_size) == (None, None, 0, 64)
    a = p.parse_args(["--sample_path", "x/y", "--dataset", "stl10", "--label_of_forgotten_class", "3", "-b", "7"])
    assert (a.sample_path, a.dataset, a.label_of_forgotten_class, a.batch_size) == ("x/y", "stl10", 3, 7)
    assert p.parse_args(["--batch-size", "9"]).batch_size == 9
    with pytest.raises(SystemExit):
        p.parse_args(["--dataset", "imagenet"])
    # the additive flags
    a = p.parse_args([])
    assert a.classifier_path is None and a.synthetic is False and a.entropy_zero_safe is False
    assert a.result_csv == "results/cifar10/forget/result.csv"
    assert ce().IMAGE_EXTENSIONS == {"bmp", "jpg", "jpeg", "pgm", "png", "ppm", "tif", "tiff", "webp"}


def test_entry_point_refuses_without_a_gpu(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce().main(["--sample_path", str(tmp_path), "--dataset", "cifar10", "--synthetic"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ce().validate_u8(torch.zeros((1, 32, 32, 3), dtype=torch.uint8), 0)


def test_state_dict_has_torchvisions_keys_and_shapes():
    from unlearn_saliency_amd.DDPM.models.resnet34 import resnet34
    want = json.load(open(os.path.join(GOLDEN, "resnet34_state_dict_keys.json")))
    sd = resnet34(10).state_dict()
    assert list(sd.keys()) == list(want.keys())
    assert {k: list(v.shape) for k, v in sd.items()} == want
    assert sum(k.endswith("num_batches_tracked") for k in sd) == 36 and sum(v.dim() == 4 for v in sd.values()) == 36
    assert resnet34(10)(torch.zeros(1, 3, 33, 47)).shape == (1, 10)          # a plain module that runs anywhere


def test_standin_weights_follow_their_recipe():
    sd = X.state_dict()
    for k, v in sd.items():
        if k.endswith("running_var") or (k.endswith("weight") and v.dim() == 1):
            assert 0.5 <= float(v.min()) and float(v.max()) <= 1.5, k
        elif k.endswith("running_mean") or (k.endswith("bias") and not k.startswith("fc")):
            assert float(v.abs().max()) < 0.6 and float(v.std()) < 0.15, k
    w = sd["layer2.0.conv1.weight"]
    assert abs(float(w.std()) - (2.0 / (128 * 9)) ** 0.5) < 0.05 * (2.0 / (128 * 9)) ** 0.5       # Kaiming, fan_out


def test_plan_scale_and_shift_are_the_float64_formula_rounded_once():
    from unlearn_saliency_amd.DDPM.models.resnet34 import fold_bn
    m32, _ = X.models()
    for bn in (m32.bn1, m32.layer3[0].downsample[1], m32.layer4[2].bn2):
        scale, shift = fold_bn(bn)
        s64, h64 = R.fold_bn(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)
        assert scale.dtype == torch.float32 and torch.equal(scale, s64.float()) and torch.equal(shift, h64.float())


def test_folder_reader_order_and_extensions(tmp_path):
    from unlearn_saliency_amd.DDPM import pngio
    names = ["10.png", "2.png", "a.PNG", "b.jpg", "c.txt", "d.npy", "0.webp", "z.jpeg"]
    for n in names:
        (tmp_path / n).write_bytes(b"")
    (tmp_path / "sub").mkdir()
    (tmp_path / "sub" / "deep.png").write_bytes(b"")
    got = [f.name for f in ce().list_images(str(tmp_path))]
    assert got == sorted(["10.png", "2.png", "b.jpg", "0.webp", "z.jpeg"])           # sorted as paths: "10" before "2"
    img = X.images()[0]
    pngio.write_png(str(tmp_path / "one.png"), img)
    grey = img[:, :, 0]
    pngio.write_png(str(tmp_path / "grey.png"), grey)
    back = ce().read_images([tmp_path / "one.png", tmp_path / "grey.png"])
    assert np.array_equal(back[0], img) and back[1].shape == (32, 32, 3) and np.array_equal(back[1][:, :, 2], grey)


def test_csv_writer_equals_the_pandas_golden(tmp_path):
    path = tmp_path / "results" / "deep" / "result.csv"
    for name, vals in X.GOLDEN_ROWS:
        ce().update_csv(str(path), name, dict(zip(ce().COLUMNS, vals)))
    golden = open(os.path.join(GOLDEN, "classifier_eval_result.csv"), "rb").read()
    assert path.read_bytes() == golden
    pd = pytest.importorskip("pandas")
    df = pd.read_csv(path, index_col=0)
    assert list(df.index) == ["other/run", "a/b", "nan/row"] and list(df.columns) == list(ce().COLUMNS)
    assert df.at["a/b", "entropy"] == 0.6875 and np.isnan(df.at["nan/row", "entropy"])
    assert ce().row_name("tmp/a/b/class_samples/0") == "a/b"


def test_every_end_to_end_sample_has_a_decided_argmax():
    """The premise of test_classifier_eval_gpu.py's accuracy check: no sample may be excused."""
    p = X.pipeline_reference()
    assert p["gap"] > X.GAP_FACTOR * p["bound"], (p["gap"], p["bound"])
    assert 1e-8 < p["figure"] < 1e-5                      # an fp32 network's error, not zero and not broken
    assert p["accuracy"] == 1.0 and 0.1 < p["entropy"] < 2.3 and 0.05 < p["prob"] < 0.95
