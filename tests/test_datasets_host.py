"""Host-side tests of the CIFAR-100 / SVHN / Tiny-ImageNet data layer, `setup_model_dataset` per dataset and the
bookkeeping of RL's merged branch.  No GPU: the loaders run their host path, RL's pass is a recording stand-in."""
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import datasets_fixture as dfx
from unlearn_saliency_amd.Classification import arg_parser, dataset as D, utils


@pytest.fixture(scope="module")
def splits(golden_dir):
    return np.load(os.path.join(golden_dir, "datasets_splits.npz"))


# ------------------------------------------------------------------ splits against the reference
@pytest.mark.parametrize("name", ["cifar100", "svhn"])
@pytest.mark.parametrize("seed", dfx.SPLIT_SEEDS)
def test_split_and_marking_match_the_reference(splits, name, seed):
    """Every array tests/golden/make_golden_datasets.py recorded from the reference's loader, reproduced exactly:
    validation indices, training indices (and their order), marked label vectors, filtered test sets."""
    loaders = getattr(D, name + "_dataloaders")
    source = dfx.split_source(name)
    key = f"{name}_s{seed}_"
    train, val, test = loaders(batch_size=16, seed=seed, source=source)
    assert np.array_equal(dfx.image_index(val.dataset.data), splits[key + "valid_idx"])
    assert np.array_equal(dfx.image_index(train.dataset.data), splits[key + "train_idx"])
    assert len(test.dataset) == int(splits[key + "test_len"]) == len(source[1][1])
    assert np.array_equal(train.dataset.targets, source[0][1][splits[key + "train_idx"]])
    for tag, kw in dfx.split_cases(name):
        train, val, test = loaders(batch_size=16, seed=seed, only_mark=True, source=source, **kw)
        assert np.array_equal(train.dataset.targets, splits[key + tag + "_train_targets"]), tag
        assert len(test.dataset) == int(splits[key + tag + "_test_len"]), tag
        assert np.array_equal(test.dataset.targets, splits[key + tag + "_test_targets"]), tag
        assert (train.dataset.targets < 0).sum() > 0
    # the rules the recorded lengths spell out
    n_test = len(source[1][1])
    assert int(splits[key + "random_test_len"]) == n_test
    assert int(splits[key + "class_none_test_len"]) == n_test - int((source[1][1] == dfx.CLASS_NONE[name]).sum())
    if name == "svhn":
        assert int(splits[key + "class_4454_test_len"]) == n_test - int((source[1][1] == dfx.SVHN_BIG_CLASS).sum())
    else:
        assert int(splits[key + "class_count_test_len"]) == n_test


def test_transforms_per_dataset():
    """cifar100 augments unless no_aug; svhn never augments; Tiny-ImageNet always does (reference dataset.py:85-95,
    193-206, 386-393)."""
    src = dfx.split_source("cifar100")
    assert D.cifar100_dataloaders(source=src)[0].dataset.transform == D.TRAIN_TRANSFORM
    assert D.cifar100_dataloaders(source=src)[1].dataset.transform == D.TRAIN_TRANSFORM
    assert D.cifar100_dataloaders(source=src, no_aug=True)[0].dataset.transform == D.TEST_TRANSFORM
    src = dfx.split_source("svhn")
    assert D.svhn_dataloaders(source=src)[0].dataset.transform == D.TEST_TRANSFORM
    assert D.svhn_dataloaders(source=src, no_aug=False)[1].dataset.transform == D.TEST_TRANSFORM
    src = D.synthetic_images("TinyImagenet", 400, 200)
    assert D.tiny_imagenet_dataloaders(source=src, no_aug=True)[0].dataset.transform == D.TRAIN_TRANSFORM
    assert D.tiny_imagenet_dataloaders(source=src)[2].dataset.transform == D.TEST_TRANSFORM


def test_tiny_imagenet_rules(monkeypatch):
    """The reference's Tiny-ImageNet loader needs image files and torchvision's ImageFolder, so its rules are checked
    against a written-out restatement of dataset.py:445-526 instead of a recording: the validation split takes 0 % (the
    training set stays whole, in order), `rng.choice(class_idx, 0)` is still drawn once per class, the returned
    validation loader IS the test set, and the test set loses the class when the count is None or 500."""
    (xtr, ytr), (xte, yte) = D.synthetic_images("TinyImagenet", 1000, 400)
    assert xtr.shape == (1000, 64, 64, 3) and int(ytr.max()) == 199
    draws = []
    real = np.random.RandomState

    class Recording(real):
        def choice(self, a, size=None, replace=True, p=None):
            draws.append((len(a), size))
            return super().choice(a, size, replace, p)

    monkeypatch.setattr(np.random, "RandomState", Recording)
    train, val, test = D.tiny_imagenet_dataloaders(batch_size=64, source=((xtr, ytr), (xte, yte)), seed=3)
    assert draws == [(5, 0)] * 200
    monkeypatch.setattr(np.random, "RandomState", real)
    assert len(train.dataset) == 1000 and np.array_equal(train.dataset.targets, ytr)
    assert np.array_equal(train.dataset.data, xtr)
    assert val.dataset is test.dataset and len(val.dataset) == 400 and not val.shuffle and train.shuffle
    for count, filtered in ((None, True), (500, True), (2, False)):
        ytr5 = np.concatenate([ytr, np.full(500, 5)]) if count == 500 else ytr
        xtr5 = np.concatenate([xtr, xtr[:500]]) if count == 500 else xtr
        train, val, test = D.tiny_imagenet_dataloaders(source=((xtr5, ytr5), (xte, yte)), class_to_replace=5,
                                                       num_indexes_to_replace=count, only_mark=True, seed=3)
        want = yte[yte != 5] if filtered else yte
        assert np.array_equal(test.dataset.targets, want), count
        assert val.dataset is test.dataset
        marked = np.flatnonzero(train.dataset.targets < 0)
        pool = np.flatnonzero(ytr5 == 5)
        if count is None:
            assert np.array_equal(marked, pool)
        else:  # replace_class: RandomState(seed - 1).choice over the class's indices
            assert np.array_equal(np.sort(marked), np.sort(real(2).choice(pool, size=count, replace=False)))
        assert np.array_equal(-train.dataset.targets[marked] - 1, ytr5[marked])


def test_empty_dataset_iterates_zero_batches():
    empty = D.ArrayDataset(np.zeros((0, 64, 64, 3), np.uint8), np.zeros(0, np.int64), D.TRAIN_TRANSFORM)
    loader = D.BatchLoader(empty, 32, shuffle=True)
    assert len(loader) == 0 and list(loader) == []
    # a rank whose shard of a ragged tail is empty gets a batch of the data's shape
    ds = D.ArrayDataset(np.zeros((1, 64, 48, 3), np.uint8), np.zeros(1, np.int64))
    (x, y), = list(D.BatchLoader(ds, 4, shuffle=False, rank=0, world_size=2))
    assert tuple(x.shape) == (0, 3, 64, 48) and y.numel() == 0


# ------------------------------------------------------------------ host path at 64 x 64
def test_host_batches_at_64_crop_flip_restated():
    """RandomCrop(64, 4) + flip of the host path against crop_flip() fed the same draws: under a fixed torch seed the
    loader takes one 64-bit draw for its iterator, then randint, randint, rand per sample in batch order."""
    (x, y), _ = D.synthetic_images("TinyImagenet", 11, 1)
    ds = D.ArrayDataset(x, y, D.TRAIN_TRANSFORM)
    torch.manual_seed(77)
    batches = list(D.BatchLoader(ds, 4, shuffle=False))
    assert [tuple(b[0].shape) for b in batches] == [(4, 3, 64, 64), (4, 3, 64, 64), (3, 3, 64, 64)]
    assert batches[0][0].dtype == torch.float32 and batches[0][1].dtype == torch.int64
    torch.manual_seed(77)
    torch.empty((), dtype=torch.int64).random_()
    seen_offsets, flips = set(), set()
    for i in range(11):
        dy = int(torch.randint(0, 9, size=(1,)).item())
        dx = int(torch.randint(0, 9, size=(1,)).item())
        flip = bool(torch.rand(1) < 0.5)
        seen_offsets.add((dy, dx))
        flips.add(flip)
        got = batches[i // 4][0][i % 4].numpy()
        assert np.array_equal(got, dfx.crop_flip(x[i], dy, dx, flip)), i
        assert int(batches[i // 4][1][i % 4]) == int(y[i])
    assert len(seen_offsets) > 5 and flips == {True, False}
    # and at 32: the CIFAR-10 path is what it was
    (x, y), _ = D.synthetic_cifar10(5, 1)
    torch.manual_seed(78)
    (xb, _), = list(D.BatchLoader(D.ArrayDataset(x, y, D.TRAIN_TRANSFORM), 8, shuffle=False))
    torch.manual_seed(78)
    torch.empty((), dtype=torch.int64).random_()
    for i in range(5):
        dy, dx = int(torch.randint(0, 9, size=(1,)).item()), int(torch.randint(0, 9, size=(1,)).item())
        assert np.array_equal(xb[i].numpy(), dfx.crop_flip(x[i], dy, dx, bool(torch.rand(1) < 0.5)))


def test_synthetic_sets():
    for name, spec in D.DATASETS.items():
        (xtr, ytr), (xte, yte) = D.synthetic_images(name, 2 * spec.classes + 1, spec.classes)
        assert xtr.shape == (2 * spec.classes + 1, spec.image, spec.image, 3) and xtr.dtype == np.uint8
        assert np.array_equal(ytr, np.arange(len(ytr)) % spec.classes) and len(yte) == spec.classes
    # the generic generator makes CIFAR-10's set exactly as synthetic_cifar10 does
    a, b = D.synthetic_images("cifar10", 20, 10), D.synthetic_cifar10(20, 10)
    assert all(np.array_equal(p, q) for s, t in zip(a, b) for p, q in zip(s, t))
    # pieces of the index-addressed generator are the whole
    from unlearn_saliency_amd import rng
    assert np.array_equal(D._u8_chunked(1003, 9, chunk_words=16), rng.u8(1003, 9))
    assert [D.DATASETS[n][4:] for n in ("cifar100", "svhn", "TinyImagenet")] == [(50_000, 10_000), (73_257, 26_032),
                                                                               (100_000, 10_000)]


# ------------------------------------------------------------------ setup_model_dataset
def _args(name, *extra):
    return arg_parser.parse_args(["--dataset", name, "--synthetic", "--batch_size", "64", "--seed", "2",
                                  "--num_indexes_to_replace", "100", *extra])


@pytest.mark.parametrize("name,arch,extra", [
    ("svhn", "resnet18", ()), ("cifar100", "vgg16_bn_lth", ("--num_classes", "100")),
    ("TinyImagenet", "resnet18", ("--num_classes", "200"))])
def test_setup_model_dataset_per_dataset(name, arch, extra, capsys):
    spec = D.DATASETS[name]
    args = _args(name, "--arch", arch, *extra)
    torch.manual_seed(1234)
    n_train, n_test = max(10 * spec.classes, 1000), 2 * spec.classes
    model, full, val, test, marked = utils.setup_model_dataset(args, synthetic_sizes=(n_train, n_test))
    out = capsys.readouterr().out
    head = model.fc if arch == "resnet18" else model.classifier
    assert head.out_features == spec.classes
    assert torch.allclose(model.normalize.mean, torch.tensor(spec.mean))
    assert torch.allclose(model.normalize.std, torch.tensor(spec.std))
    # only the cifar10 branch re-seeds around the model construction (reference utils.py:134-143)
    assert torch.initial_seed() == 1234 and "setup random seed" not in out
    assert "warning: --num_classes" not in out
    if name == "TinyImagenet":
        assert len(full.dataset) == n_train and val.dataset is test.dataset and len(test.dataset) == n_test
        assert full.dataset.data.shape[1:] == (64, 64, 3)
    else:
        assert len(full.dataset) == n_train - n_train // 10 and len(val.dataset) == n_train // 10
        assert len(test.dataset) == n_test
    assert len(full) == -(-len(full.dataset) // 64) and len(marked.dataset) == len(full.dataset)
    assert int((marked.dataset.targets < 0).sum()) == 100
    if name == "TinyImagenet":  # no split to differ by seed (the full loader is cut with seed 1, the marked one with 2)
        restored = np.where(marked.dataset.targets < 0, -marked.dataset.targets - 1, marked.dataset.targets)
        assert np.array_equal(restored, full.dataset.targets)
    want_tf = D.TEST_TRANSFORM if name == "svhn" else D.TRAIN_TRANSFORM
    assert full.dataset.transform == marked.dataset.transform == want_tf


def test_setup_model_dataset_cifar10_reseeds_and_warns(capsys):
    args = _args("cifar10", "--num_classes", "100", "--train_seed", "5")
    torch.manual_seed(1234)
    model, full, val, test, marked = utils.setup_model_dataset(args)
    out = capsys.readouterr().out
    assert torch.initial_seed() == 5 and out.count("setup random seed = 5") == 2
    assert model.fc.out_features == 10 and len(full.dataset) == 45000
    assert "warning: --num_classes 100 differs from cifar10's 10 classes" in out
    assert torch.allclose(model.normalize.mean, torch.tensor((0.4914, 0.4822, 0.4465)))


def test_no_aug_reaches_cifar100_only():
    kw = dict(synthetic_sizes=(400, 200))
    assert utils.setup_model_dataset(_args("cifar100", "--no-aug"), **kw)[4].dataset.transform == D.TEST_TRANSFORM
    assert utils.setup_model_dataset(_args("cifar100", "--no-aug"), **kw)[1].dataset.transform == D.TRAIN_TRANSFORM
    assert utils.setup_model_dataset(_args("TinyImagenet", "--no-aug"), **kw)[4].dataset.transform == D.TRAIN_TRANSFORM


def test_scope_errors():
    for name in ("imagenet", "cifar10_no_val", "cifar100_no_val"):
        with pytest.raises(NotImplementedError, match="out of scope"):
            utils.setup_model_dataset(_args(name))
    with pytest.raises(ValueError, match="Dataset not supprot yet !"):
        utils.setup_model_dataset(_args("mnist"))


# ------------------------------------------------------------------ file readers
def test_cifar100_pickle_reader(tmp_path):
    base = tmp_path / "cifar-100-python"
    base.mkdir()
    rows = np.arange(2 * 3072, dtype=np.int64).reshape(2, 3072) % 251
    for nm, labs in (("train", [17, 99]), ("test", [3, 0])):
        with open(base / nm, "wb") as f:
            pickle.dump({"data": rows.astype(np.uint8), "fine_labels": labs, "coarse_labels": [1, 2]}, f)
    assert D.have_cifar100(str(tmp_path)) and not D.have_cifar100(str(base))
    (xtr, ytr), (xte, yte) = D._load_cifar100_files(str(tmp_path))
    assert xtr.shape == (2, 32, 32, 3) and xtr.dtype == np.uint8 and ytr.tolist() == [17, 99] and yte.tolist() == [3, 0]
    # row layout: 1024 red, 1024 green, 1024 blue, each row-major
    assert xtr[1, 2, 5, 0] == rows[1, 2 * 32 + 5] and xtr[1, 2, 5, 2] == rows[1, 2048 + 2 * 32 + 5]


def test_svhn_mat_reader(tmp_path):
    sio = pytest.importorskip("scipy.io")
    x = (np.arange(32 * 32 * 3 * 3) % 253).astype(np.uint8).reshape(32, 32, 3, 3)
    sio.savemat(str(tmp_path / "train_32x32.mat"), {"X": x, "y": np.array([[10], [1], [9]], np.uint8)})
    sio.savemat(str(tmp_path / "test_32x32.mat"), {"X": x[..., :2], "y": np.array([[2], [10]], np.uint8)})
    assert D.have_svhn(str(tmp_path))
    (xtr, ytr), (xte, yte) = D._load_svhn_files(str(tmp_path))
    assert xtr.shape == (3, 32, 32, 3) and ytr.tolist() == [0, 1, 9] and yte.tolist() == [2, 0]
    assert np.array_equal(xtr[2], x[..., 2]) and np.array_equal(xte[1], x[..., 1])
    train, val, test = D.svhn_dataloaders(data_dir=str(tmp_path), batch_size=2)
    assert hasattr(train.dataset, "targets") and len(train.dataset) == 3 and len(val.dataset) == 0


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize("layout", ["pristine", "reference"])
def test_tiny_imagenet_folder(tmp_path, layout):
    Image = pytest.importorskip("PIL.Image")
    wnids = ["n02", "n01", "n03"]
    pixel = lambda k: np.full((64, 64, 3), k, np.uint8)
    k = 0
    for w in wnids:
        (tmp_path / "train" / w / "images").mkdir(parents=True)
        (tmp_path / "train" / w / f"{w}_boxes.txt").write_text("ignored\n")
        for j in (1, 0):
            k += 1
            Image.fromarray(pixel(k)).save(tmp_path / "train" / w / "images" / f"{w}_{j}.png")
    per_class = 27
    if layout == "pristine":
        (tmp_path / "val" / "images").mkdir(parents=True)
        (tmp_path / "test" / "images").mkdir(parents=True)  # the unlabelled test images of the download: never read
        lines = []
        for i in range(per_class * 3):
            w = wnids[i % 3]
            Image.fromarray(pixel(100 + i)).save(tmp_path / "val" / "images" / f"val_{i:03d}.png")
            lines.append(f"val_{i:03d}.png\t{w}\t0\t0\t63\t63\n")
        (tmp_path / "val" / "val_annotations.txt").write_text("".join(lines))
    else:
        for ci, w in enumerate(sorted(wnids)):
            (tmp_path / "test" / w / "images").mkdir(parents=True)
            for j in range(2):
                Image.fromarray(pixel(200 + 10 * ci + j)).save(tmp_path / "test" / w / "images" / f"t_{j}.png")
    before = _tree(tmp_path)
    assert D.have_tiny_imagenet(str(tmp_path))
    classes, train, test = D.tiny_imagenet_file_lists(str(tmp_path))
    assert classes == ["n01", "n02", "n03"]
    assert [os.path.basename(p) for p, _ in train] == ["n01_0.png", "n01_1.png", "n02_0.png", "n02_1.png", "n03_0.png",
                                                      "n03_1.png"]
    assert [lab for _, lab in train] == [0, 0, 1, 1, 2, 2]
    (xtr, ytr), (xte, yte) = D._load_tiny_imagenet_files(str(tmp_path))
    assert xtr.shape == (6, 64, 64, 3) and xtr[:, 0, 0, 0].tolist() == [4, 3, 2, 1, 6, 5]
    if layout == "pristine":
        # per class, sorted by file name: the first 25 are validation, the remaining 2 test
        assert yte.tolist() == [0, 0, 1, 1, 2, 2]
        want = [100 + i for c in ("n01", "n02", "n03")
                for i in sorted(i for i in range(per_class * 3) if wnids[i % 3] == c)[25:]]
        assert xte[:, 0, 0, 0].tolist() == want
    else:
        assert yte.tolist() == [0, 0, 1, 1, 2, 2] and xte[:, 0, 0, 0].tolist() == [200, 201, 210, 211, 220, 221]
    assert _tree(tmp_path) == before  # the user's files are where they were
    train_l, val_l, test_l = D.tiny_imagenet_dataloaders(data_dir=str(tmp_path), batch_size=4)
    assert len(train_l.dataset) == 6 and val_l.dataset is test_l.dataset and len(test_l.dataset) == 6


def test_tiny_imagenet_without_pil_names_synthetic(tmp_path, monkeypatch):
    import builtins
    (tmp_path / "train" / "n01").mkdir(parents=True)
    (tmp_path / "test" / "n01").mkdir(parents=True)
    real_import = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real_import(name, *a, **k)

    monkeypatch.setattr(builtins, "__import__", no_pil)
    with pytest.raises(ImportError, match="--synthetic"):
        D.tiny_imagenet_dataloaders(data_dir=str(tmp_path))


# ------------------------------------------------------------------ merged RL bookkeeping
def test_merged_rl_bookkeeping(monkeypatch):
    """The RL plugin's merged branch with the optimisation pass replaced by a recorder (the loaders run their host
    path): ceil((n_f + n_r) / batch) steps in one pass, every forget sample once with the label drawn for it this epoch,
    retain labels untouched, new labels in the second epoch, the images concatenated once per call."""
    import sys
    import unlearn_saliency_amd.Classification.unlearn  # noqa: F401  (the package attribute `RL` is the plugin)
    RL_mod = sys.modules["unlearn_saliency_amd.Classification.unlearn.RL"]
    n_f, n_r, K, bs = 41, 90, 100, 32
    fds = D.ArrayDataset(dfx.index_images(n_f, 4), np.arange(n_f) % K, D.TRAIN_TRANSFORM)
    rx = dfx.index_images(n_f + n_r, 4)[n_f:]
    rds = D.ArrayDataset(rx, (np.arange(n_r) * 7) % K, D.TRAIN_TRANSFORM)
    rds.transform = fds.transform = D.TEST_TRANSFORM  # index-coded pixels must survive the batch
    loaders = {"forget": D.BatchLoader(fds, bs, True), "retain": D.BatchLoader(rds, bs, True)}
    calls = []

    def recorder(loader, model, criterion, optimizer, epoch, args, **kw):
        batches = [(np.round(x[:, :, 0, 0].numpy() * 255).astype(np.int64), y.numpy().copy()) for x, y in loader]
        calls.append((loader, kw, batches))
        if kw.get("top1") is not None:
            kw["top1"].update(12.5, 1)

    monkeypatch.setattr(RL_mod, "run_pass", recorder)
    drawn = []
    real_randint = np.random.randint
    monkeypatch.setattr(np.random, "randint", lambda *a, **k: (drawn.append(real_randint(*a, **k)), drawn[-1])[1])
    args = SimpleNamespace(dataset="TinyImagenet", num_classes=K, warmup=0, batch_size=bs, unlearn_epochs=2,
                           print_freq=50)
    model = SimpleNamespace(train=lambda: None)
    plugin = RL_mod.RL.__wrapped_iter__
    np.random.seed(3)
    torch.manual_seed(3)
    assert plugin(loaders, model, None, None, 0, args) == 12.5
    assert plugin(loaders, model, None, None, 1, args) == 12.5
    assert len(calls) == 2 and len(drawn) == 2 and drawn[0].shape == (n_f,) and not np.array_equal(*drawn)
    assert 0 <= drawn[0].min() and drawn[0].max() < K
    np.random.seed(3)
    assert np.array_equal(drawn[0], real_randint(0, K, (n_f,)))  # numpy's global generator, as seeded
    for (loader, kw, batches), labels in zip(calls, drawn):
        assert len(batches) == len(loader) == -(-(n_f + n_r) // bs) == 5
        assert [len(y) for _, y in batches] == [32, 32, 32, 32, 3]
        assert kw["loader_len"] == 2 + 3 and kw["print_offset"] == 2 and kw["track"] and "label_fn" not in kw
        px = np.concatenate([p for p, _ in batches])
        idx = px[:, 0] | (px[:, 1] << 8) | (px[:, 2] << 16)
        ys = np.concatenate([y for _, y in batches])
        assert sorted(idx.tolist()) == list(range(n_f + n_r)) and not np.array_equal(idx, np.arange(n_f + n_r))
        f = idx < n_f
        assert np.array_equal(ys[f], labels[idx[f]])
        assert np.array_equal(ys[~f], rds.targets[idx[~f] - n_f])
    assert calls[0][0] is calls[1][0] and calls[0][0].dataset.data is calls[1][0].dataset.data  # one concatenation
    assert np.array_equal(fds.targets, np.arange(n_f) % K)  # the caller's forget set keeps its labels
    assert RL_mod._merged is None  # nothing of the call is held after its last epoch

    # svhn keeps the two-pass branch; the merged branch refuses a warm-up and more than one rank
    calls.clear()
    args.dataset = "svhn"
    plugin(loaders, model, None, None, 0, args)
    assert [c[0] for c in calls] == [loaders["forget"], loaders["retain"]] and "label_fn" in calls[0][1]
    args.dataset, args.warmup = "cifar100", 1
    with pytest.raises(NameError):
        plugin(loaders, model, None, None, 0, args)
    args.warmup = 0
    monkeypatch.setattr(RL_mod.sdist, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="one GPU"):
        plugin(loaders, model, None, None, 0, args)


def test_label_swap_keeps_the_resident_images(monkeypatch):
    """`BatchLoader._resident` caches images and labels apart: new labels upload the label vector alone (`.to` is
    replaced by a counting identity, so this runs on the host)."""
    ds = D.ArrayDataset(dfx.index_images(10, 4), np.arange(10))
    loader = D.BatchLoader(ds, 4, False, device_resident=True, device=torch.device("cpu"))
    data0, t0 = loader._resident()
    ds.targets = np.arange(10)[::-1].copy()
    data1, t1 = loader._resident()
    assert data1 is data0 and loader.image_uploads == 1 and t1.tolist() == list(range(9, -1, -1)) and t0[0] == 0
    assert loader._resident()[1] is t1
    ds.data = ds.data.copy()
    assert loader._resident()[0] is not data0 and loader.image_uploads == 2
