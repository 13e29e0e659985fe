"""VGG-16-BN (`--arch vgg16_bn_lth`) on the host: the registry builds it, its state_dict is the reference's (names,
shapes, order: tests/golden/vgg16_bn_lth.json), and its plain module path in float64 reproduces the reference model's
float64 logits and gradients (tests/golden/vgg16_bn_lth.npz; the same library arithmetic, so 1e-12 relative)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import vgg_fixture as VF


@pytest.fixture(scope="module")
def golden(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "vgg16_bn_lth.json")))
    return meta, np.load(os.path.join(golden_dir, "vgg16_bn_lth.npz"))


def _build():
    from unlearn_saliency_amd.Classification.models import model_dict
    return model_dict["vgg16_bn_lth"](num_classes=10)


def test_registry_builds_the_reference_tree(golden):
    meta, _ = golden
    model = _build()
    sd = model.state_dict()
    assert list(sd) == meta["names"]
    assert [list(v.shape) for v in sd.values()] == meta["shapes"]
    assert [n for n, _ in model.named_parameters()] == meta["param_names"]
    assert [type(m).__name__ for m in model.features] == meta["modules"]
    assert isinstance(model.features, nn.Sequential) and isinstance(model.classifier, nn.Linear)
    assert sum(p.numel() for p in model.parameters()) == 14_728_266
    assert all(m.bias is not None for m in model.features if isinstance(m, nn.Conv2d))
    assert VF.LAST_CONV in sd and meta["sample_stride"] == VF.SAMPLE_STRIDE


def test_initialisation_is_the_references():
    torch.manual_seed(3)
    model = _build()
    convs = [m for m in model.features if isinstance(m, nn.Conv2d)]
    assert len(convs) == 13
    for m in convs:
        fan_out = m.out_channels * 9
        assert not bool(m.bias.detach().any())
        assert abs(float(m.weight.detach().std()) / np.sqrt(2.0 / fan_out) - 1.0) < 0.1
    for m in model.features:
        if isinstance(m, nn.BatchNorm2d):
            assert bool((m.weight == 1).all()) and bool((m.bias == 0).all())
    assert abs(float(model.classifier.weight.detach().std()) / 0.01 - 1.0) < 0.1
    assert not bool(model.classifier.bias.detach().any())


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_plain_path_in_float64_reproduces_the_golden(golden, mode):
    _, g = golden
    model = _build().double()
    assert not model.fused_bn
    logits, grads = VF.run(model, train=mode == "train", want_grads=True)
    want = g["logits_" + mode]
    assert np.abs(logits.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    scale = max(float(np.linalg.norm(g[f"grad_{mode}_{n}"])) for n in VF.GRAD_NAMES)
    for n in VF.GRAD_NAMES:
        w = g[f"grad_{mode}_{n}"]
        err = float(np.linalg.norm(grads[n].numpy() - w))
        # relative to the tensor's own norm; the one tensor that is zero in exact arithmetic (a convolution bias ahead
        # of a train-mode BatchNorm: the golden holds rounding noise) is held against the largest gradient norm
        den = scale if (mode, n) == ("train", "features.0.bias") else float(np.linalg.norm(w))
        assert err <= 1e-12 * den, (n, err, den)


def test_narrow_configuration_and_imagenet_refusal():
    from unlearn_saliency_amd.Classification.models.vgg_lth import VGG, vgg16_bn_lth
    net = VGG([32, "M", 32, "M", 64, "M", 64, "M", 64], num_classes=10)
    assert net.classifier.in_features == 64
    assert net(torch.rand(2, 3, 32, 32)).shape == (2, 10)
    with pytest.raises(TypeError):
        vgg16_bn_lth(num_classes=10, imagenet=True)
    with pytest.raises(TypeError):
        VGG(imagenet=True)
    assert isinstance(vgg16_bn_lth(num_classes=10, imagenet=False), VGG)


def test_arg_parser_accepts_the_arch_with_no_new_flag(golden_dir):
    from unlearn_saliency_amd.Classification import arg_parser
    args = arg_parser.parse_args(["--arch", "vgg16_bn_lth"])
    assert args.arch == "vgg16_bn_lth"
    assert set(vars(args)) == set(vars(arg_parser.parse_args([])))      # (tests/test_cli.py pins that set)
    assert "arch" in json.load(open(os.path.join(golden_dir, "cli.json")))["classification_defaults"]


def test_fused_switches_cover_the_model():
    """`use_fused_bn` reports the 13 BatchNorm layers and `use_fused_head` accepts the features / classifier pair; a
    model with neither pair is still refused."""
    from unlearn_saliency_amd.cls_head import head_parts, use_fused_head
    from unlearn_saliency_amd.norm import use_fused_bn
    model = _build()
    assert use_fused_bn(model) == 13 and model.fused_bn
    use_fused_head(model)
    maps, linear = head_parts(model)
    assert linear is model.classifier and maps == model.feature_maps
    with pytest.raises(TypeError, match="features"):
        use_fused_head(nn.Sequential(nn.Linear(3, 3)))

    class Seq(nn.Module):  # a `features` Sequential + `classifier` without a feature_maps method of its own
        def __init__(self):
            super().__init__()
            self.features = nn.Sequential(nn.Conv2d(3, 4, 3))
            self.classifier = nn.Linear(4, 2)

    maps, linear = head_parts(Seq())
    assert maps(torch.rand(1, 3, 5, 5)).shape == (1, 4, 3, 3)
