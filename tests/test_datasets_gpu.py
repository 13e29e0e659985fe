"""CIFAR-100 / SVHN / Tiny-ImageNet on the GPU: batch assembly at 64 x 64, the two architectures at the new shapes on
this package's kernels, the classifier head at 100 / 101 / 200 classes, RL's merged branch against the reference, and
one end-to-end run per dataset."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import datasets_fixture as dfx

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _deterministic():
    torch.backends.cudnn.deterministic = True
    yield


# ------------------------------------------------------------------ batch assembly
def test_image_batch_at_64_is_bit_equal_to_the_restatement():
    """B = 5 at 64 x 64, pad 4: the four corner offsets and the centre, flip on and off."""
    from unlearn_saliency_amd import ops
    from unlearn_saliency_amd.Classification.dataset import synthetic_images
    (x, _), _ = synthetic_images("TinyImagenet", 9, 1)
    data = torch.from_numpy(x).cuda()
    offsets = [(0, 0), (8, 8), (0, 8), (8, 0), (4, 4)]
    idx = torch.tensor([7, 0, 3, 8, 3], dtype=torch.int64, device="cuda")
    crop = torch.tensor(offsets, dtype=torch.int32, device="cuda")
    for flips in ([0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [1, 0, 1, 0, 1]):
        flip = torch.tensor(flips, dtype=torch.uint8, device="cuda")
        got = ops.image_batch(data, idx, crop, flip, pad=4).cpu().numpy()
        assert got.shape == (5, 3, 64, 64)
        for b in range(5):
            want = dfx.crop_flip(x[int(idx[b])], offsets[b][0], offsets[b][1], bool(flips[b]))
            assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), (flips, b)
    plain = ops.image_batch(data, idx, None, None, pad=4).cpu().numpy()
    assert np.array_equal(plain[1], dfx.crop_flip(x[0], 4, 4, False))


@pytest.mark.parametrize("name", ["cifar100", "TinyImagenet"])
def test_device_loader_matches_host_loader_at_32_and_64(name):
    from unlearn_saliency_amd.Classification.dataset import ArrayDataset, BatchLoader, synthetic_images
    (x, y), _ = synthetic_images(name, 300, 1)
    ds = ArrayDataset(x, y, transform="test")
    host = BatchLoader(ds, 128, shuffle=False)
    dev = BatchLoader(ds, 128, shuffle=False, device_resident=True, device=torch.device("cuda"))
    n = 0
    for (xh, yh), (xd, yd) in zip(host, dev):
        assert xd.shape[2] == xd.shape[3] == x.shape[1]
        assert torch.equal(xh, xd.cpu()) and torch.equal(yh, yd.cpu())
        n += 1
    assert n == len(host) == len(dev) == 3
    # new labels reach the device without a second upload of the images
    ds.targets = (y + 1) % 7
    assert torch.equal(next(iter(dev))[1].cpu(), torch.from_numpy(ds.targets[:128]))
    assert dev.image_uploads == 1


# ------------------------------------------------------------------ the two architectures at 64 x 64
FWD, DGRAD, WGRAD = 0, 1, 2   # SALUN_ROUTE_*
WGRAD_SHARED = 1
AMPLE = 1 << 40


def _route(L, direction, N, C, H, K, R, s, p, flags=0, ws=0):
    P = (H + 2 * p - R) // s + 1
    buf, ns = ctypes.create_string_buffer(256), ctypes.c_int(-1)
    rc = L.salun_conv2d_route(direction, N, C, H, H, K, R, s, p, P, P, flags, ws, buf, len(buf), ctypes.byref(ns))
    assert rc in (0, -22)
    return buf.value.decode() if rc == 0 else None


def predicted_library_calls(model, N, H):
    """What `conv.LIBRARY_CONV_CALLS` must read after one forward + backward of `model` (a VGG: a chain of 3x3 / 1
    convolutions and 2x2 pools) on [N, 3, H, H], from the host route query alone: a refused forward sends the layer's
    backward to the library as well; an accepted one leaves backward-weight / backward-data there only where their own
    routes are refused."""
    from unlearn_saliency_amd import _lib
    L = _lib.lib()
    want = {"shape": 0, "dtype_or_autocast": 0, "backward": 0}
    first = True
    for m in model.features:
        if isinstance(m, nn.MaxPool2d):
            H //= 2
        if not isinstance(m, nn.Conv2d):
            continue
        C, K, R, s, p = m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0]
        fwd = _route(L, FWD, N, C, H, K, R, s, p, 0, L.salun_conv2d_data_workspace_bytes(N, K, H, H, R, s))
        if fwd is None:
            want["shape"] += 1
            want["backward"] += 1 + (not first)
        else:
            wg = [_route(L, WGRAD, N, C, H, K, R, s, p, f, AMPLE) for f in (WGRAD_SHARED, 0)]
            want["backward"] += all(r is None for r in wg)
            dg = _route(L, DGRAD, N, C, H, K, R, s, p, 0, L.salun_conv2d_data_workspace_bytes(N, C, H, H, R, 1))
            want["backward"] += (not first) and dg is None
        first = False
    return want


def _step_pair(make, head, x, y):
    """(loss, head-weight gradient) of one training step on library modules and on this package's kernels (strict: a
    convolution the kernels refuse raises), from the same weights; -> (losses, gradients, library-call counts)."""
    from unlearn_saliency_amd import conv as sconv
    from unlearn_saliency_amd.norm import use_fused_bn
    ref, fast = make().cuda(), make().cuda()
    fast.load_state_dict(ref.state_dict())
    n_conv = sum(isinstance(m, nn.Conv2d) for m in fast.modules())
    assert sconv.use_salun_convs(fast) == n_conv and use_fused_bn(fast) > 0
    losses, grads = [], []
    sconv.reset_library_conv_calls()
    for net in (ref, fast):
        net.train()
        sconv.strict(net is fast)
        try:
            loss = nn.functional.cross_entropy(net(x), y)
            loss.backward()
        finally:
            sconv.strict(False)
        losses.append(float(loss))
        grads.append(head(net).weight.grad)
    torch.cuda.synchronize()
    calls = dict(sconv.LIBRARY_CONV_CALLS)
    sconv.reset_library_conv_calls()
    return losses, grads, calls


def _assert_step_matches(losses, grads):
    # the tolerances of smoke(): 1e-4 relative on the loss; rtol 1e-3, atol 1e-4 * max on the head's weight gradient
    print("loss library / own:", losses, " max |grad| difference:", float((grads[0] - grads[1]).abs().max()),
          "of", float(grads[0].abs().max()))
    assert abs(losses[0] - losses[1]) <= 1e-4 * abs(losses[0]), losses
    assert torch.allclose(grads[0], grads[1], rtol=1e-3, atol=1e-4 * float(grads[0].abs().max()))


def test_resnet18_200_classes_at_64_runs_on_own_kernels():
    from unlearn_saliency_amd.Classification.models import model_dict
    torch.manual_seed(0)
    x, y = torch.rand(8, 3, 64, 64, device="cuda"), torch.randint(0, 200, (8,), device="cuda")
    losses, grads, calls = _step_pair(lambda: model_dict["resnet18"](num_classes=200), lambda m: m.fc, x, y)
    assert sum(calls.values()) == 0, calls
    assert grads[1].shape == (200, 512)
    _assert_step_matches(losses, grads)


def test_vgg16_bn_200_classes_at_64_library_calls_as_predicted():
    """At 64 x 64 the last three convolutions see 4 x 4 maps, which backward-weight has a route for (at 32 x 32 they
    see 2 x 2 and go to the library): the route query predicts no library call, strict mode or not."""
    import vgg_fixture as VF
    from unlearn_saliency_amd.Classification.models import model_dict
    make = lambda: VF.fill_state(model_dict["vgg16_bn_lth"](num_classes=200))
    want = predicted_library_calls(make(), 4, 64)
    assert want == {"shape": 0, "dtype_or_autocast": 0, "backward": 0}, want
    assert predicted_library_calls(make(), 8, 32)["backward"] == 3  # the predictor reproduces the 32 x 32 finding
    torch.manual_seed(0)
    x, y = torch.rand(4, 3, 64, 64, device="cuda"), torch.randint(0, 200, (4,), device="cuda")
    losses, grads, calls = _step_pair(make, lambda m: m.classifier, x, y)
    assert calls == want, (calls, want)
    _assert_step_matches(losses, grads)


# ------------------------------------------------------------------ K23 at the new class counts
@pytest.mark.parametrize("K", [100, 101, 200])
@pytest.mark.parametrize("HW", [16, 64])
def test_cls_head_at_the_new_class_counts(K, HW):
    """B = 3, C = 512 (layer4's width), HW = 16 (32 x 32 input) and 64 (64 x 64), K = 100, 200 and boundary_expanding's
    101: against cls_head_ref_cpu.py's float64 model, inside that file's per-element bounds."""
    from test_cls_head_gpu import _gaussian_case
    _gaussian_case((3, 512, HW, K), 1.0, 1.0)


# ------------------------------------------------------------------ merged RL against the reference
@pytest.fixture(scope="module")
def rl_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "rl_merged.npz"))


@pytest.mark.parametrize("resident", [False, True], ids=["host_loader", "device_loader"])
@pytest.mark.parametrize("tag,use_mask", [("masked", True), ("unmasked", False)])
def test_merged_rl_matches_the_reference(rl_golden, tag, use_mask, resident):
    """`RL` with dataset="cifar100" on the fixture of tests/golden/make_golden_datasets.py: the same numpy and torch
    seeds give the labels the reference drew and the order its DataLoader walked, on either loader path; the trained
    weights agree to rtol 1e-5 / atol 1e-6 and masked-out weights keep their bits."""
    from unlearn_saliency_amd.Classification import unlearn
    from unlearn_saliency_amd.Classification.dataset import BatchLoader
    g = rl_golden
    model = dfx.rl_model()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    for k, v in init.items():
        assert np.array_equal(v.numpy(), g["init_" + k]), k
    model.cuda()
    names = [n for n, _ in model.named_parameters()]
    sizes = [p.numel() for p in model.parameters()]
    mflat = dfx.rl_mask_flat(sum(sizes))
    off = np.cumsum([0] + sizes)
    mask = {n: torch.from_numpy(mflat[off[i]:off[i + 1]]).view_as(p)
            for i, (n, p) in enumerate(model.named_parameters())} if use_mask else None
    fds, rds = dfx.rl_merged_datasets()
    mk = lambda ds: BatchLoader(ds, dfx.RL_BATCH, True, device_resident=resident, device=torch.device("cuda"))
    seen = []
    ce = nn.CrossEntropyLoss()

    def criterion(out, tgt):
        seen.append(tgt.detach().cpu().numpy().copy())
        return ce(out, tgt)

    np.random.seed(dfx.RL_NUMPY_SEED)
    torch.manual_seed(dfx.RL_TORCH_SEED)
    unlearn.get_unlearn_method("RL")({"forget": mk(fds), "retain": mk(rds)}, model, criterion, dfx.rl_args(), mask)
    assert [len(s) for s in seen] == g[tag + "_step_sizes"].tolist() == [32, 32, 32, 32, 3] * dfx.RL_EPOCHS
    assert np.array_equal(np.concatenate(seen), g[tag + "_step_targets"])
    sd = model.state_dict()
    for k, v in sd.items():
        assert np.allclose(v.cpu().numpy(), g[f"{tag}_sd_{k}"], rtol=1e-5, atol=1e-6), k
    moved = np.concatenate([sd[n].reshape(-1).cpu().numpy() for n in names])
    was = np.concatenate([init[n].reshape(-1).numpy() for n in names])
    if use_mask:
        frozen = mflat == 0
        assert np.array_equal(moved[frozen].view(np.uint32), was[frozen].view(np.uint32))
        assert (moved[~frozen] != was[~frozen]).mean() > 0.5
    else:
        assert (moved != was).mean() > 0.9


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("name,arch", [("cifar100", "vgg16_bn_lth"), ("svhn", "resnet18"),
                                       ("TinyImagenet", "resnet18")])
def test_end_to_end_per_dataset(tmp_path, name, arch):
    """generate_mask -> main_random (RL with with_0.5.pt) -> accuracies -> SVC_MIA on the device, on a synthetic set
    shrunk to 2,000 training images."""
    from unlearn_saliency_amd.Classification import generate_mask, main_random
    from unlearn_saliency_amd.Classification.dataset import DATASETS
    from unlearn_saliency_amd.Classification.models import model_dict
    spec = DATASETS[name]
    common = ["--dataset", name, "--arch", arch, "--synthetic", "--device_loader", "--num_classes", str(spec.classes),
              "--batch_size", "256", "--num_indexes_to_replace", "200", "--seed", "2", "--save_dir", str(tmp_path)]
    sizes = (2000, 400)
    generate_mask.main(common + ["--thresholds", "0.5"], synthetic_sizes=sizes)
    assert os.listdir(tmp_path) == ["with_0.5.pt"]
    mask = torch.load(tmp_path / "with_0.5.pt", map_location="cpu", weights_only=False)
    want = {n: tuple(p.shape) for n, p in model_dict[arch](num_classes=spec.classes).named_parameters()}
    assert {n: tuple(v.shape) for n, v in mask.items()} == want and list(mask) == list(want)
    total = sum(v.numel() for v in mask.values())
    assert sum(int(v.sum()) for v in mask.values()) == int(total * 0.5)
    result = main_random.main(common + ["--unlearn", "RL", "--unlearn_epochs", "1", "--unlearn_lr", "0.01",
                                        "--mask_path", str(tmp_path / "with_0.5.pt"), "--mia", "device"],
                              synthetic_sizes=sizes)
    assert set(result["accuracy"]) == {"retain", "forget", "val", "test"}
    assert all(0.0 <= float(v) <= 100.0 for v in result["accuracy"].values())
    mia = result["SVC_MIA_forget_efficacy"]
    assert mia and all(np.isfinite(float(v)) for v in mia.values())
    assert os.path.exists(tmp_path / "RLcheckpoint.pth.tar")
