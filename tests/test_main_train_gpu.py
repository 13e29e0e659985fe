"""Classification/main_train.py end to end on the GPU, on a cut-down synthetic set: the files it writes and their keys,
resume == uninterrupted bit for bit, memorisation of a 64-image set, and the checkpoint as `--model_path` of the
unlearning driver."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

N_TRAIN, N_TEST = 400, 100           # 360 train / 40 validation images after the 10 % split


@pytest.fixture()
def small_set(monkeypatch):
    from unlearn_saliency_amd.Classification import dataset
    monkeypatch.setattr(dataset, "synthetic_cifar10",
                        functools.partial(dataset.synthetic_cifar10, n_train=N_TRAIN, n_test=N_TEST))


def _argv(save_dir, epochs, *more):
    return ["--synthetic", "--device_loader", "--save_dir", str(save_dir), "--epochs", str(epochs), "--decreasing_lr",
            "1,2", "--lr", "0.05", "--batch_size", "128", "--seed", "3", "--print_freq", "2", *more]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One uninterrupted 3-epoch run, and a 2-epoch run resumed for the third epoch (shared by the tests below)."""
    from unlearn_saliency_amd.Classification import dataset, main_train
    real = dataset.synthetic_cifar10
    dataset.synthetic_cifar10 = functools.partial(real, n_train=N_TRAIN, n_test=N_TEST)
    try:
        full, part = tmp_path_factory.mktemp("full"), tmp_path_factory.mktemp("part")
        result = main_train.main(_argv(full, 3))
        main_train.main(_argv(part, 2))
        after2 = torch.load(part / "0checkpoint.pth.tar", map_location="cpu", weights_only=False)
        main_train.main(_argv(part, 3, "--resume", "--checkpoint", str(part / "0checkpoint.pth.tar")))
    finally:
        dataset.synthetic_cifar10 = real
    return full, part, result, after2


def test_files_and_keys(runs, golden_dir):
    from unlearn_saliency_amd.Classification import main_train
    from unlearn_saliency_amd.Classification.models.resnet_cifar import resnet18
    full, _, result, after2 = runs
    g = np.load(os.path.join(golden_dir, "train_epoch.npz"))
    for name in ("0checkpoint.pth.tar", "0model_SA_best.pth.tar"):
        assert (full / name).exists(), name
    ck = torch.load(full / "0checkpoint.pth.tar", map_location="cpu", weights_only=False)
    assert list(ck) == [str(k) for k in g["checkpoint_keys"]] == list(main_train.CHECKPOINT_KEYS)
    assert ck["epoch"] == 3 and after2["epoch"] == 2
    assert len(ck["result"]["train_ta"]) == len(ck["result"]["val_ta"]) == 3 and ck["result"] == result
    assert ck["best_sa"] == max(ck["result"]["val_ta"])
    model = resnet18(num_classes=10)
    want = model.state_dict()
    assert list(ck["state_dict"]) == list(want) and all(ck["state_dict"][k].shape == v.shape for k, v in want.items())
    opt = ck["optimizer"]
    assert sorted(opt) == [str(k) for k in g["sgd_top_keys"]]
    assert sorted(opt["param_groups"][0]) == [str(k) for k in g["sgd_group_keys"]]
    names = [n for n, _ in model.named_parameters()]
    assert opt["param_groups"][0]["params"] == list(range(len(names))) and sorted(opt["state"]) == list(range(len(names)))
    for i, (n, p) in enumerate(model.named_parameters()):
        assert sorted(opt["state"][i]) == [str(k) for k in g["sgd_state_keys"]]
        assert opt["state"][i]["momentum_buffer"].shape == p.shape, n
    # lr 0.05 through milestones 1 and 2
    assert abs(opt["param_groups"][0]["lr"] - 0.05 * 0.1 * 0.1) < 1e-12 and opt["param_groups"][0]["initial_lr"] == 0.05
    # the reference's own optimizer takes the entry as it is
    sgd = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-4)
    sgd.load_state_dict(opt)
    assert torch.equal(sgd.state[next(model.parameters())]["momentum_buffer"], opt["state"][0]["momentum_buffer"])


def test_resumed_run_equals_the_uninterrupted_run_bit_for_bit(runs):
    full, part, _, _ = runs
    a = torch.load(full / "0checkpoint.pth.tar", map_location="cpu", weights_only=False)
    b = torch.load(part / "0checkpoint.pth.tar", map_location="cpu", weights_only=False)
    assert a["epoch"] == b["epoch"] == 3 and a["result"] == b["result"]
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]) and (v.dtype != torch.float32 or torch.equal(
            v.view(torch.int32), b["state_dict"][k].view(torch.int32))), k
    for i, ent in a["optimizer"]["state"].items():
        assert torch.equal(ent["momentum_buffer"].view(torch.int32),
                           b["optimizer"]["state"][i]["momentum_buffer"].view(torch.int32)), i


def test_checkpoint_loads_through_model_path_of_the_unlearning_driver(runs, small_set, tmp_path, monkeypatch):
    """`_driver.run --model_path` reads ckpt["state_dict"]: with the `raw` method (no unlearning) the saved model is the
    trained one, key for key and bit for bit."""
    from unlearn_saliency_amd.Classification import _driver
    full, _, _, _ = runs
    monkeypatch.setattr(_driver, "validate", lambda *a, **k: 0.0)     # the accuracies are not what this test is about
    monkeypatch.setitem(__import__("sys").modules, "unlearn_saliency_amd.Classification.evaluation", None)
    _driver.run(["--synthetic", "--device_loader", "--unlearn", "raw", "--save_dir", str(tmp_path), "--model_path",
                 str(full / "0model_SA_best.pth.tar"), "--num_indexes_to_replace", "20", "--class_to_replace", "0",
                 "--batch_size", "128", "--seed", "3"], use_mask=False)
    want = torch.load(full / "0model_SA_best.pth.tar", map_location="cpu", weights_only=False)["state_dict"]
    got = torch.load(tmp_path / "rawcheckpoint.pth.tar", map_location="cpu", weights_only=False)["state_dict"]
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)


def test_training_memorises_a_64_image_set():
    """trainer.train on 64 fixed images (no augmentation, one batch per epoch): the training accuracy of the last epoch
    is above the first epoch's.  ResNet-18 on the HIP path with the fused head, as main_train.py configures it."""
    from types import SimpleNamespace
    from unlearn_saliency_amd.Classification.dataset import ArrayDataset, BatchLoader, synthetic_cifar10
    from unlearn_saliency_amd.Classification.models.resnet_cifar import resnet18
    from unlearn_saliency_amd.Classification.trainer import get_optimizer_and_scheduler, train
    from unlearn_saliency_amd.cls_head import use_fused_head
    from unlearn_saliency_amd.conv import use_salun_convs
    from unlearn_saliency_amd.norm import use_fused_bn
    (xtr, ytr), _ = synthetic_cifar10(n_train=64, n_test=10)
    loader = BatchLoader(ArrayDataset(xtr, ytr, transform="test"), 64, shuffle=False, device_resident=True,
                         device=torch.device("cuda"))
    torch.manual_seed(1)
    model = resnet18(num_classes=10).cuda()
    use_salun_convs(model), use_fused_bn(model), use_fused_head(model)
    args = SimpleNamespace(lr=0.05, momentum=0.9, weight_decay=5e-4, decreasing_lr="91,136", warmup=0, print_freq=50,
                           imagenet_arch=False, alpha=0.0, epochs=12)
    optimizer, scheduler = get_optimizer_and_scheduler(model, args)
    accs = []
    for epoch in range(args.epochs):
        accs.append(train(loader, model, nn.CrossEntropyLoss(), optimizer, epoch, args))
        scheduler.step()
    optimizer.close()
    assert accs[-1] > accs[0], accs
