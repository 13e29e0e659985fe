"""The device side of SD/eval-scripts/imageclassify.py: the crop-and-normalise kernel, the row top-k, K26 at this
feature's sizes, SD/resnet50.InferencePlan50 against a float64 copy of the same module tree on the CPU, and the command
line end to end.  Weights, inputs, references and the way the tolerance is measured (not chosen) are in
imageclassify_fixture.py; its premises are asserted on the CPU by test_imageclassify_host.py."""
import csv
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import conv_infer_ref_cpu as R
import imageclassify_fixture as X
from guarded_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
_plan = {}


def plan(pointwise="auto"):
    if pointwise not in _plan:
        from unlearn_saliency_amd.SD.resnet50 import InferencePlan50
        _plan[pointwise] = InferencePlan50(X.models()[0], "cuda", pointwise=pointwise)
    return _plan[pointwise]


def cli():
    path = os.path.join(ROOT, "unlearn_saliency_amd", "SD", "eval-scripts", "imageclassify.py")
    spec = importlib.util.spec_from_file_location("sd_cli_imageclassify", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")
    if d and os.path.isdir(d):
        with open(os.path.join(d, "imageclassify_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


def stream():
    from unlearn_saliency_amd.streams import _stream
    return _stream()


# ------------------------------------------------------------------------------------------ crop and normalise
def test_crop_and_normalise_equals_the_model_on_every_corner_and_the_centre():
    from unlearn_saliency_amd import conv_infer, ops_infer
    from unlearn_saliency_amd._lib import SalunError
    from unlearn_saliency_amd.SD.resnet50 import NORM_MEAN, NORM_STD
    g = torch.Generator().manual_seed(2)
    src = torch.randint(0, 256, (2, 9, 11, 3), generator=g, dtype=torch.uint8)
    table = ops_infer.u8_norm_table(NORM_MEAN, NORM_STD).cuda()
    dev = src.cuda()
    OH, OW = 4, 5
    for top, left in ((0, 0), (0, 6), (5, 0), (5, 6), (2, 3)):
        got = conv_infer.u8_crop_to_chw_norm(dev, table, top, left, OH, OW)
        want = R.normalize_u8(src[:, top:top + OH, left:left + OW], NORM_MEAN, NORM_STD)
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), (top, left)
    whole = conv_infer.u8_crop_to_chw_norm(dev, table, 0, 0, 9, 11)
    assert torch.equal(whole, conv_infer.u8_to_chw_norm(dev, table))                 # the old entry point, unchanged
    out = torch.full((2, 3, OH, OW), 7.0, device="cuda")
    for top, left, oh, ow in ((6, 0, OH, OW), (0, 7, OH, OW), (-1, 0, OH, OW), (0, 0, 10, 5), (0, 0, 0, 5)):
        with pytest.raises((SalunError, ValueError)):
            ops_infer.u8_crop_to_chw_norm(dev, table, top, left, oh, ow, out=out if oh == OH and ow == OW else None)
    assert bool((out == 7.0).all())                                                  # a refused window writes nothing
    assert conv_infer.library_infer_calls() == 0


# ------------------------------------------------------------------------------------------ row top-k
def topk_in_arena(rows, k):
    B, K = rows.shape
    a = Arena().put("p", torch.from_numpy(rows)).put("values", shape=(B, k), out=True)
    a.put("indices", shape=(B, 2 * k), out=True).upload()                            # int64 as two words each
    from unlearn_saliency_amd import _lib
    rc = _lib.lib().salun_row_topk(a.ptr("p"), a.ptr("values"), a.ptr("indices"), ctypes.c_int64(B), K, k, stream())
    after = a.download()
    return rc, a.part(after, "values").numpy(), a.part(after, "indices").view(torch.int64).numpy()


@pytest.mark.parametrize("K", [1, 5, 1000, 1024])
def test_row_topk_is_torch_topk_without_ties_and_the_stated_rule_with_them(K):
    for k in sorted({1, min(5, K), K}):
        free = X.topk_rows(K, "free")
        rc, v, i = topk_in_arena(free, k)
        tv, ti = torch.from_numpy(free).topk(k, -1)
        assert rc == 0 and np.array_equal(i, ti.numpy()) and np.array_equal(v, tv.numpy()), (K, k)
        ties = X.topk_rows(K, "ties")
        rc, v, i = topk_in_arena(ties, k)
        mv, mi = X.topk_model(ties, k)
        assert rc == 0 and np.array_equal(i, mi), (K, k)
        assert np.array_equal(v.view(np.uint32) & 0x7FC00000 == 0x7FC00000, np.isnan(mv))
        keep = ~np.isnan(mv)
        assert np.array_equal(v.view(np.uint32)[keep], mv.view(np.uint32)[keep]), (K, k)     # the entries' own bits


def test_row_topk_refusals_write_nothing():
    rows = X.topk_rows(5, "free")
    from unlearn_saliency_amd import _lib
    for K, k in ((5, 0), (5, 6), (1025, 5), (0, 1)):
        a = Arena().put("p", torch.from_numpy(rows)).put("values", shape=(4, 8), out=True)
        a.put("indices", shape=(4, 16), out=True).upload()
        rc = _lib.lib().salun_row_topk(a.ptr("p"), a.ptr("values"), a.ptr("indices"), ctypes.c_int64(4), K, k, stream())
        after = a.download()
        assert rc == EINVAL and bool((a.part(after, "values").view(torch.int32) == SENTINEL).all()), (K, k)


# ------------------------------------------------------------------------------------------ K26 at this feature's sizes
def test_k26_equals_pillow_at_the_sizes_of_the_preset():
    from PIL import Image
    from unlearn_saliency_amd import ops_resample
    from unlearn_saliency_amd.SD.resnet50 import resized_size
    r = np.random.default_rng(11)
    for shape in ((2, 512, 512, 3), (1, 300, 500, 3)):
        u8 = r.integers(0, 256, shape, dtype=np.uint8)
        OH, OW = resized_size(shape[1], shape[2])
        assert min(OH, OW) == 232 and ops_resample.lds_bytes(shape[1], shape[2], 3, OH, OW) > 0
        got = ops_resample.resize_u8(torch.from_numpy(u8).cuda(), (OH, OW)).cpu().numpy()
        want = np.stack([np.asarray(Image.fromarray(im).resize((OW, OH), Image.BILINEAR)) for im in u8])
        assert got.shape == want.shape and np.array_equal(got, want), shape


# ------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize("n,side", X.NETWORK_CASES, ids=["3x64", "2x224"])
def test_logits_and_top5_against_the_float64_network(n, side):
    """Measured on an MI355X (profiles/imageclassify_bounds_measured.txt): see the lines this test logs."""
    from unlearn_saliency_amd import conv_infer, ops_infer
    conv_infer.reset_library_infer_calls()
    ref = X.network_reference(n, side)
    x = X.network_inputs(n, side).cuda()
    logits, p = plan().forward(x)
    assert plan().kernel_calls == {"k30": 33 - len(_on_k27(side)), "k27": 20 + len(_on_k27(side))}
    err = float((logits.cpu().double() - ref["l64"]).abs().max())
    peak = float(ref["l64"].abs().max())
    ratio = (err / peak) / ref["figure"]
    log(f"resnet50 {n} x {side} x {side}: fp32 CPU library {ref['figure']:.3e}, device {err / peak:.3e} of max |logit| = "
        f"{ratio:.2f} x the library's (allowed {X.DEVICE_FACTOR} x); undecided (row, rank) pairs "
        f"{int((~ref['decided']).sum())} of {ref['decided'].numel()}")
    assert err <= ref["bound"], (err / peak, ref["figure"])
    assert conv_infer.library_infer_calls() == 0, conv_infer.LIBRARY_INFER_CALLS
    decided = ref["decided"]
    assert float((~decided).float().mean()) <= X.MAX_LEFT_OUT
    values, indices = ops_infer.row_topk(p, X.TOPK)
    assert torch.equal(indices.cpu()[decided], ref["top"][decided])
    assert torch.equal(values, p.gather(1, indices))
    again, _ = plan().forward(x)
    assert torch.equal(again, logits)                                # the same bits on a second run
    # every 1 x 1 / stride-1 layer forced to K27: identical, because K30 runs K27's chain
    forced, _ = plan("k27").forward(x)
    assert plan("k27").kernel_calls == {"k30": 0, "k27": 53}
    assert torch.equal(forced.view(torch.int32), logits.view(torch.int32))
    assert conv_infer.library_infer_calls() == 0


def _on_k27(side):
    """The 1 x 1 / stride-1 layers of the network at this input side that the plan's table keeps on K27."""
    from unlearn_saliency_amd.SD.resnet50 import POINTWISE_ON_K27
    m = X.models()[0]
    out, s = [], (side + 1) // 2
    s = (s + 1) // 2
    for i in range(4):
        for j, blk in enumerate(getattr(m, f"layer{i + 1}")):
            s_in = s
            if blk.stride == 2:
                s = (s - 1) // 2 + 1
            for conv, hw in ((blk.conv1, s_in * s_in), (blk.conv3, s * s)) + \
                    (((blk.downsample[0], s_in * s_in),) if blk.downsample is not None and blk.stride == 1 else ()):
                if (conv.in_channels, hw, conv.out_channels) in POINTWISE_ON_K27:
                    out.append((i, j))
    return out


def test_preprocess_is_resize_crop_normalise_of_pillow_and_buffers_are_allocated_once():
    from PIL import Image
    from unlearn_saliency_amd import conv_infer
    from unlearn_saliency_amd.SD import resnet50 as R50
    conv_infer.reset_library_infer_calls()
    r = np.random.default_rng(3)
    u8 = r.integers(0, 256, (2, 300, 500, 3), dtype=np.uint8)
    got = plan().preprocess_u8(torch.from_numpy(u8).cuda())
    OH, OW = R50.resized_size(300, 500)
    top, left = R50.crop_origin(OH, OW)
    big = np.stack([np.asarray(Image.fromarray(im).resize((OW, OH), Image.BILINEAR)) for im in u8])
    want = R.normalize_u8(torch.from_numpy(big[:, top:top + 224, left:left + 224]), R50.NORM_MEAN, R50.NORM_STD)
    assert torch.equal(got.cpu(), want)
    ptrs = [b.data_ptr() for b in plan()._buffers(2, 224, 224)]
    plan().classify_u8(torch.from_numpy(u8).cuda())
    assert [b.data_ptr() for b in plan()._buffers(2, 224, 224)] == ptrs
    assert conv_infer.library_infer_calls() == 0


# ------------------------------------------------------------------------------------------ the command line
def test_end_to_end_script(tmp_path, capsys):
    from unlearn_saliency_amd import conv_infer
    from unlearn_saliency_amd.DDPM import pngio
    m = cli()
    folder = tmp_path / "eval" / "run-a"
    folder.mkdir(parents=True)
    for name, im in zip(X.CLI_NAMES, X.cli_images()):
        pngio.write_png(str(folder / name), im)
    (folder / "readme.txt").write_text("not an image")
    prompts = tmp_path / "prompts.csv"
    prompts.write_text(X.CLI_PROMPTS)
    conv_infer.reset_library_infer_calls()
    argv = ["--folder_path", str(folder), "--prompts_path", str(prompts), "--synthetic", "--seed", str(X.WEIGHT_SEED),
            "--batch_size", "3", "--topk", "3"]
    assert m.main(argv) == 0
    assert conv_infer.library_infer_calls() == 0
    save = folder / "run-a_classification.csv"
    first = save.read_bytes()
    table = list(csv.reader(first.decode().splitlines()))
    head = ["", "case_number", "prompt", "evaluation_seed"]
    for k in (1, 2, 3):
        head += [f"category_top{k}", f"index_top{k}", f"scores_top{k}"]
    assert table[0] == head
    assert [r[:4] for r in table[1:]] == [["0", "0", "first prompt", "1"], ["1", "0", "first prompt", "1"],
                                          ["2", "2", "second, with a comma", "2"], ["3", "2", "second, with a comma", "2"],
                                          ["4", "5", "third prompt", "4"], ["5", "5", "third prompt", "4"]]
    # the scores and indices are InferencePlan50's on the same bytes (each image alone: an image's result does not
    # depend on its batch), formatted as a float32 column
    for row, im in zip(table[1:], X.cli_images()):
        v, i = plan().classify_u8(torch.from_numpy(im[None]).cuda(), 3)
        assert [row[5 + 3 * k] for k in range(3)] == [str(int(j)) for j in i[0].cpu()]
        assert [row[4 + 3 * k] for k in range(3)] == [f"class_{int(j):04d}" for j in i[0].cpu()]
        assert [row[6 + 3 * k] for k in range(3)] == m.format_scores(v[0].cpu().numpy())
    assert m.main(argv) == 0
    assert save.read_bytes() == first                                 # a second run writes the same file
