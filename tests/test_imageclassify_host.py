"""The host side of SD/eval-scripts/imageclassify.py and SD/resnet50.py (no GPU): torchvision's preprocessing formulas, the
row top-k rule, the ResNet-50 module tree, the CSV writer against pandas, the checkpoint search and the parser."""
import csv
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

import imageclassify_fixture as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "imageclassify_merge.csv")


def cli():
    path = os.path.join(ROOT, "unlearn_saliency_amd", "SD", "eval-scripts", "imageclassify.py")
    spec = importlib.util.spec_from_file_location("sd_cli_imageclassify", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------ preprocessing formulas
@pytest.mark.parametrize("h,w,resized,origin", [
    (512, 512, (232, 232), (4, 4)),          # square
    (300, 500, (232, 386), (4, 81)),         # landscape: int(232 * 500 / 300) = 386
    (500, 300, (386, 232), (81, 4)),         # portrait
    (333, 517, (232, 360), (4, 68)),         # odd sizes: int(232 * 517 / 333) = 360
    (232, 233, (232, 233), (4, 4)),          # (233 - 224) / 2 = 4.5 rounds to even: 4
    (240, 227, (245, 232), (10, 4)),         # (245 - 224) / 2 = 10.5 rounds to even: 10
    (224, 224, (232, 232), (4, 4)),
])
def test_resize_and_crop_formulas_are_torchvisions(h, w, resized, origin):
    from unlearn_saliency_amd.SD import resnet50 as R50
    assert R50.resized_size(h, w) == resized
    short, long = min(h, w), max(h, w)
    assert min(resized) == 232 and max(resized) == int(232 * long / short)
    assert (resized[0] >= resized[1]) == (h >= w) or resized[0] == resized[1]
    assert R50.crop_origin(*resized) == origin
    top, left = origin
    assert 0 <= top and top + 224 <= resized[0] and 0 <= left and left + 224 <= resized[1]
    assert (R50.NORM_MEAN, R50.NORM_STD) == ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


# ------------------------------------------------------------------------------------------ the top-k rule
@pytest.mark.parametrize("K", [1, 5, 1000, 1024])
def test_topk_model_is_torch_topk_on_tie_free_rows(K):
    rows = X.topk_rows(K, "free")
    for k in sorted({1, min(5, K), K}):
        v, i = X.topk_model(rows, k)
        tv, ti = torch.from_numpy(rows).topk(k, -1)
        assert np.array_equal(i, ti.numpy()) and np.array_equal(v, tv.numpy())


def test_topk_model_follows_the_stated_rule_on_ties_and_nans():
    nan, inf = float("nan"), float("inf")
    row = np.array([[1.0, nan, 3.0, -0.0, 3.0, nan, 0.0, inf, -inf, 1.0]], np.float32)
    v, i = X.topk_model(row, 10)
    assert i.tolist() == [[1, 5, 7, 2, 4, 0, 9, 3, 6, 8]]
    assert np.array_equal(v.view(np.uint32), row[0, i[0]][None].view(np.uint32))       # the entries' own bits (-0 stays -0)
    rows = X.topk_rows(1000, "ties")
    assert np.isnan(rows).any() and (rows == 0).any()
    v, i = X.topk_model(rows, 1000)
    for b in range(rows.shape[0]):
        assert sorted(i[b].tolist()) == list(range(1000))
        for a, c in zip(i[b][:-1], i[b][1:]):
            x, y = rows[b, a], rows[b, c]
            assert np.isnan(x) or (not np.isnan(y) and x >= y)
            if (np.isnan(x) and np.isnan(y)) or x == y:
                assert a < c


# ------------------------------------------------------------------------------------------ the module tree
def test_resnet50_has_torchvisions_keys_shapes_and_parameter_count():
    from unlearn_saliency_amd.SD import resnet50 as R50
    m = R50.resnet50()
    assert sum(p.numel() for p in m.parameters()) == 25_557_032 == R50.NUM_PARAMETERS
    sd = m.state_dict()
    assert tuple(sd["conv1.weight"].shape) == (64, 3, 7, 7) and tuple(sd["fc.weight"].shape) == (1000, 2048)
    assert tuple(sd["layer1.0.downsample.0.weight"].shape) == (256, 64, 1, 1)
    assert tuple(sd["layer1.0.conv1.weight"].shape) == (64, 64, 1, 1)
    assert tuple(sd["layer4.2.conv3.weight"].shape) == (2048, 512, 1, 1)
    assert tuple(sd["layer3.5.bn2.running_var"].shape) == (256,) and "layer3.5.bn3.num_batches_tracked" in sd
    assert m.layer2[0].conv2.stride == (2, 2) and m.layer2[0].conv1.stride == (1, 1)      # v1.5: the stride is on conv2
    assert m.layer2[0].downsample[0].stride == (2, 2) and m.layer1[0].downsample[0].stride == (1, 1)
    assert [len(getattr(m, f"layer{i}")) for i in (1, 2, 3, 4)] == [3, 4, 6, 3]
    assert "layer1.1.downsample.0.weight" not in sd and "layer2.0.downsample.1.running_mean" in sd
    convs = [c for c in m.modules() if isinstance(c, torch.nn.Conv2d)]
    pw1 = [c for c in convs if c.kernel_size == (1, 1) and c.stride == (1, 1)]
    assert len(convs) == 53 and len([c for c in convs if c.kernel_size == (1, 1)]) == 36 and len(pw1) == 33
    # conv keys: 53 weights, 53 BatchNorms of five entries each, fc
    assert len(sd) == 53 + 53 * 5 + 2
    assert set(R50.standin_state_dict(3)) == set(sd)
    from unlearn_saliency_amd.DDPM.models import resnet34 as R34
    assert R50._Conv is R34._Conv and R50.fold_bn is R34.fold_bn                            # shared, not copied


@pytest.mark.parametrize("n,side", X.NETWORK_CASES, ids=["3x64", "2x224"])
def test_the_fp32_library_alone_decides_enough_of_the_top5(n, side):
    """The premise of the GPU comparison: with the device's bound (8 x the fp32 CPU library's own distance from float64)
    at most 10 % of the (row, rank) pairs are too close to call, and the fp32 library agrees on every other one."""
    ref = X.network_reference(n, side)
    assert float(ref["l64"].abs().max()) < 20                  # the stand-in head keeps the logits within a few units
    decided = ref["decided"]
    assert float((~decided).float().mean()) <= X.MAX_LEFT_OUT, (~decided).sum()
    top32 = torch.softmax(ref["l32"], -1).topk(X.TOPK, -1).indices
    assert torch.equal(top32[decided], ref["top"][decided])


# ------------------------------------------------------------------------------------------ the CSV writer
def own_merge():
    m = cli()
    table = list(csv.reader(io.StringIO(X.PROMPTS_CSV)))
    cases, categories, indices, scores = X.merge_results()
    header, rows = m.merged_rows(table[0], table[1:], cases, categories, indices, scores, X.MERGE_TOPK)
    return m, header, rows


def test_csv_writer_equals_the_recorded_pandas_bytes(tmp_path):
    m, header, rows = own_merge()
    path = str(tmp_path / "out.csv")
    m.write_csv(path, header, rows)
    got = open(path, "rb").read()
    assert got == open(GOLDEN, "rb").read()
    lines = got.decode().splitlines()
    assert lines[0] == (",case_number,prompt,evaluation_seed,class,note,category_top1,index_top1,scores_top1,"
                        "category_top2,index_top2,scores_top2")
    # inner join: left rows in file order, a row's images in name order; case 7 (no image) and image 9 (no row) drop out;
    # both rows of case 3 get all three images
    assert [ln.split(",")[1] for ln in lines[1:]] == ["3", "3", "3", "1", "3", "3", "3", "0", "0"]
    assert [ln.split(",")[0] for ln in lines[1:]] == [str(i) for i in range(9)]
    assert lines[1].startswith('0,3,"a photo of a tench, in a lake",2915,tench,1.50,name 0,0,0.99999994,')
    assert lines[8].endswith(',0,1.0,"cassette player, ""deck""",482,0.0')
    assert "0.12345679,name 1,1,1e-45" in lines[9] and "3.0000001e-05" in got.decode() and "1.1754944e-38" in got.decode()


def test_csv_writer_equals_pandas_byte_for_byte(tmp_path):
    pytest.importorskip("pandas")
    m, header, rows = own_merge()
    path = str(tmp_path / "out.csv")
    m.write_csv(path, header, rows)
    assert open(path, "rb").read() == X.merge_with_pandas()


# ------------------------------------------------------------------------------------------ files and flags
def test_checkpoint_search_order_and_error_messages(tmp_path):
    m = cli()
    cwd, th, home = str(tmp_path / "cwd"), str(tmp_path / "th"), str(tmp_path / "home")
    name = m.DEFAULT_CLASSIFIER
    assert name == "resnet50-11ad3fa6.pth"
    want = [os.path.join(cwd, name), os.path.join(th, "hub", "checkpoints", name),
            os.path.join(home, ".cache", "torch", "hub", "checkpoints", name)]
    assert m.checkpoint_candidates(name, cwd, {"TORCH_HOME": th}, home) == want
    assert m.checkpoint_candidates(name, cwd, {}, home) == [want[0], want[2]]
    assert m.checkpoint_candidates("some/dir/file.pth", cwd, {"TORCH_HOME": th}, home) == ["some/dir/file.pth"]
    with pytest.raises(SystemExit) as e:
        m.find_checkpoint(name, cwd, {"TORCH_HOME": th}, home)
    assert all(p in str(e.value) for p in want) and "Nothing is downloaded" in str(e.value)
    for p in reversed(want):                                  # the later places first: an earlier one then wins
        os.makedirs(os.path.dirname(p))
        open(p, "wb").close()
        assert m.find_checkpoint(name, cwd, {"TORCH_HOME": th}, home) == p
    # no --categories: the error names the flag, and comes before the folder is looked at
    with pytest.raises(SystemExit) as e:
        m.main(["--folder_path", str(tmp_path / "no such folder"), "--prompts_path", "none.csv"])
    assert "--categories" in str(e.value) and "--synthetic" in str(e.value)
    cats = tmp_path / "cats.txt"
    cats.write_text("\n".join(f"n{i}" for i in range(999)) + "\n")
    with pytest.raises(SystemExit, match="999 lines"):
        m.read_categories(str(cats))
    cats.write_text("\n".join(f"n{i}" for i in range(1000)) + "\n")
    assert m.read_categories(str(cats))[999] == "n999"
    assert m.synthetic_categories()[0] == "class_0000" and m.synthetic_categories()[999] == "class_0999"


def test_parser_defaults_are_the_references():
    m = cli()
    a = m.build_parser().parse_args(["--folder_path", "eval/ua/run-x", "--prompts_path", "prompts/imagenette.csv"])
    assert (a.save_path, a.device, a.topk, a.batch_size) == (None, "cuda:0", 5, 250)
    assert (a.classifier_path, a.categories, a.synthetic) == ("resnet50-11ad3fa6.pth", None, False)
    assert m.default_save_path("eval/ua/run-x") == "eval/ua/run-x/run-x_classification.csv"
    with pytest.raises(SystemExit):
        m.build_parser().parse_args(["--prompts_path", "p.csv"])
    # the file rule: `.png` or `.jpg` anywhere in the name; the case number is what stands before the first `_`
    assert m.case_number("12_3.png") == 12 and m.case_number("7.png") == 7 and m.case_number("5_0.jpg") == 5


def test_image_names_are_sorted_and_filtered(tmp_path):
    m = cli()
    for name in ("3_1.png", "10_0.png", "1_0.jpg", "notes.txt", "2_0.png.bak", "x.jpeg"):
        (tmp_path / name).write_bytes(b"")
    assert m.image_names(str(tmp_path)) == ["10_0.png", "1_0.jpg", "2_0.png.bak", "3_1.png"]
