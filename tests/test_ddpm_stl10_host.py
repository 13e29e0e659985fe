"""Host-side tests of the STL-10 diffusion data layer and configs.  No GPU: the reader runs on files written into
tmp_path, the one device call of the data path (K26, ops_resample.resize_u8) is replaced by its numpy restatement, and
the models are built on the meta device."""
import glob
import os

import numpy as np
import pytest
import torch

import resample_ref_cpu as RS
from unlearn_saliency_amd.DDPM import datasets as DS
from unlearn_saliency_amd.DDPM.datasets import stl10
from unlearn_saliency_amd.DDPM.functions import load_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "unlearn_saliency_amd", "DDPM", "configs")
N_TRAIN, N_TEST = 12, 8


def _images(n, base):
    """n images [96, 96, 3] of a flat grey `base + i` with four distinct corners and one marked pixel at row 5, col 90."""
    x = np.empty((n, 96, 96, 3), np.uint8)
    for i in range(n):
        x[i] = base + i
        x[i, 0, 0], x[i, 0, 95], x[i, 95, 0], x[i, 95, 95] = (1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12)
        x[i, 5, 90] = (200, 100 + i, 50)
    return x


@pytest.fixture()
def stl10_dir(tmp_path):
    base = tmp_path / "stl10_binary"
    os.makedirs(base)
    xtr, xte = _images(N_TRAIN, 20), _images(N_TEST, 120)
    ytr = (np.arange(N_TRAIN) % 10 + 1).astype(np.uint8)           # stored 1..10
    yte = ((np.arange(N_TEST) * 3) % 10 + 1).astype(np.uint8)
    for split, x, y in (("train", xtr, ytr), ("test", xte, yte)):
        x.transpose(0, 3, 2, 1).tofile(str(base / f"{split}_X.bin"))  # the file's order: image, plane, COLUMN, row
        y.tofile(str(base / f"{split}_y.bin"))
    return str(tmp_path), np.concatenate([xtr, xte]), np.concatenate([ytr, yte]).astype(np.int64) - 1


@pytest.fixture()
def host_resize(monkeypatch):
    """K26 replaced by its restatement on host tensors; records the calls."""
    from unlearn_saliency_amd import ops_resample
    calls = []

    def resize_u8(x, size):
        calls.append((tuple(x.shape), tuple(size)))
        return torch.from_numpy(RS.resize_u8(x.numpy(), size))

    monkeypatch.setattr(ops_resample, "resize_u8", resize_u8)
    return calls


def _config(path, batch=4, flip=False):
    cfg = load_config(os.path.join(CONFIGS, "stl10_saliency_unlearn.yml"))
    cfg.data.path, cfg.data.random_flip, cfg.training.batch_size = path, flip, batch
    return cfg


def test_reader_axis_order_labels_and_split_order(stl10_dir):
    path, x_want, y_want = stl10_dir
    assert stl10.have_stl10(path) and not stl10.have_stl10(os.path.join(path, "nowhere"))
    x, y = stl10.load_stl10_files(path)
    assert x.shape == (N_TRAIN + N_TEST, 96, 96, 3) and x.dtype == np.uint8 and y.dtype == np.int64
    assert tuple(x[3, 0, 95]) == (4, 5, 6) and tuple(x[3, 95, 0]) == (7, 8, 9)      # (row, column), not transposed
    assert tuple(x[3, 5, 90]) == (200, 103, 50) and tuple(x[3, 90, 5]) == (23, 23, 23)
    assert np.array_equal(x, x_want)
    assert np.array_equal(y, y_want) and y.min() == 0 and y.max() == 9              # stored 1..10, minus one
    assert x[N_TRAIN - 1, 40, 40, 0] == 20 + N_TRAIN - 1 and x[N_TRAIN, 40, 40, 0] == 120   # train, then test


def test_get_dataset_resizes_once_and_keeps_the_order(stl10_dir, host_resize):
    path, x_want, y_want = stl10_dir
    loader = DS.get_dataset(None, _config(path), device=torch.device("cpu"))
    assert host_resize == [((N_TRAIN + N_TEST, 96, 96, 3), (64, 64))]            # the whole set, one call, uint8 originals
    want = torch.from_numpy(RS.resize_u8(x_want, (64, 64))).permute(0, 3, 1, 2).float().div(255)
    assert torch.equal(loader.x, want) and torch.equal(loader.c, torch.from_numpy(y_want))
    assert loader.flip is False and loader.batch_size == 4
    assert DS.get_dataset(None, _config(path, flip=True), device=torch.device("cpu")).flip is True  # drawn per pass


def test_get_forget_dataset_counts_and_frozen_flip(stl10_dir, host_resize, capsys):
    path, x_want, y_want = stl10_dir
    label = 0
    n_forget = int((y_want == label).sum())
    assert n_forget == 3  # train images 0 and 10, test image 0
    remain, forget = DS.get_forget_dataset(None, _config(path), label, device=torch.device("cpu"))
    assert capsys.readouterr().out.split() == [str(N_TRAIN + N_TEST - n_forget), str(n_forget)]
    assert len(remain.x) == N_TRAIN + N_TEST - n_forget and len(forget.x) == n_forget
    assert bool((forget.c == label).all()) and not bool((remain.c == label).any())
    want = torch.from_numpy(RS.resize_u8(x_want, (64, 64))).permute(0, 3, 1, 2).float().div(255)
    assert torch.equal(forget.x, want[torch.from_numpy(y_want == label)])
    # with the flip: drawn once from numpy's generator, applied AFTER the resize, frozen in both loaders
    np.random.seed(11)
    flip = torch.from_numpy(np.random.rand(N_TRAIN + N_TEST) < 0.5)
    np.random.seed(11)
    remain, forget = DS.get_forget_dataset(None, _config(path, flip=True), label, device=torch.device("cpu"))
    mirrored = torch.where(flip[:, None, None, None], want.flip(3), want)
    assert torch.equal(forget.x, mirrored[torch.from_numpy(y_want == label)])
    assert torch.equal(remain.x, mirrored[torch.from_numpy(y_want != label)])
    assert remain.flip is False and forget.flip is False
    # ... which is what resizing the mirrored originals gives (the reference's order, mirrored first here)
    again = torch.from_numpy(RS.resize_u8(np.ascontiguousarray(x_want[:, :, ::-1]), (64, 64))).permute(0, 3, 1, 2)
    assert torch.equal(again.float().div(255), want.flip(3))


def test_synthetic_stand_in_and_dispatch(host_resize, tmp_path):
    x, y = stl10.synthetic_stl10(30, 20)
    assert x.shape == (50, 96, 96, 3) and x.dtype == np.uint8
    assert np.array_equal(y, np.concatenate([np.arange(30) % 10, np.arange(20) % 10]))
    assert (stl10.N_TRAIN, stl10.N_TEST) == (5_000, 8_000)
    assert stl10.resize_target(96, 96, 64) == (64, 64) and stl10.resize_target(96, 192, 64) == (64, 128)
    cfg = _config(str(tmp_path))
    cfg.data.dataset = "LSUN"
    with pytest.raises(ValueError, match="CIFAR10 or STL10"):
        DS.get_dataset(None, cfg, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="CIFAR10 or STL10"):
        DS.get_forget_dataset(None, cfg, 0, device=torch.device("cpu"))


def test_cifar10_path_does_not_touch_the_resize(host_resize):
    cfg = load_config(os.path.join(CONFIGS, "cifar10_saliency_unlearn.yml"))
    cfg.data.random_flip = False
    from unlearn_saliency_amd.Classification.dataset import synthetic_cifar10
    loader = DS.get_dataset(None, cfg, device=torch.device("cpu"), synthetic=True)
    (x, y), _ = synthetic_cifar10(64, 8)  # index-addressed generator: the first 64 images of the full set
    assert host_resize == [] and loader.x.shape == (50_000, 3, 32, 32)
    assert torch.equal(loader.x[:64], torch.from_numpy(x[:64]).permute(0, 3, 1, 2).float().div(255))


@pytest.mark.parametrize("name", sorted(os.path.basename(p) for p in glob.glob(os.path.join(CONFIGS, "stl10_*.yml"))))
def test_shipped_configs_build_the_reference_model(name, golden_dir):
    from unlearn_saliency_amd.DDPM.models.diffusion import Conditional_Model
    g = np.load(os.path.join(golden_dir, "ddpm_stl10.npz"))
    cfg = load_config(os.path.join(CONFIGS, name))
    assert cfg.data.image_size == 64 and cfg.model.ch_mult == [1, 2, 2, 2, 4] and cfg.model.attn_resolutions == [16]
    with torch.device("meta"):
        sd = Conditional_Model(cfg).state_dict()
    assert list(sd) == list(g["state_names"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(g["state_shapes"])


def test_all_five_configs_are_shipped_with_the_reference_values():
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CONFIGS, "stl10_*.yml")))
    assert names == ["stl10_fim.yml", "stl10_forget.yml", "stl10_saliency_unlearn.yml", "stl10_sample.yml",
                     "stl10_train.yml"]
    unlearn = load_config(os.path.join(CONFIGS, "stl10_saliency_unlearn.yml"))
    cifar = load_config(os.path.join(CONFIGS, "cifar10_saliency_unlearn.yml"))
    train = load_config(os.path.join(CONFIGS, "stl10_train.yml"))
    assert vars(unlearn.training) == vars(cifar.training) and vars(unlearn.optim) == vars(cifar.optim)
    assert vars(unlearn.data) == vars(train.data)
    assert {k: v for k, v in vars(unlearn.model).items() if k != "ema"} == \
           {k: v for k, v in vars(train.model).items() if k != "ema"}
    assert (train.training.batch_size, train.training.n_iters, train.optim.lr) == (128, 250000, 0.0002)
    forget = load_config(os.path.join(CONFIGS, "stl10_forget.yml"))
    assert (forget.training.batch_size, forget.training.n_iters, forget.training.lmbda) == (64, 20000, 10)
