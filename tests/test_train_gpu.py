"""`Classification.trainer.train` on the GPU: the reference's two epochs on the tiny BN network
(tests/golden/train_epoch.npz, written by make_golden_train.py from the reference's own trainer/train.py) with the fused
head K23, a masked epoch, and the fused head against the library head on one ResNet-18 step."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import cls_head_ref_cpu as R
from fixtures import TinyCNN, tiny_batches, tiny_state

pytestmark = pytest.mark.gpu


class TinyHead(TinyCNN):
    """The fixture network with the features() / fc split that use_fused_head needs (same parameters, same forward)."""

    def features(self, x):
        x = torch.relu(self.bn1(self.conv1(x)))
        return torch.relu(self.bn2(self.conv2(x)))


class ListLoader(list):
    def __init__(self, batches):
        super().__init__(batches)
        self.dataset = SimpleNamespace(targets=np.zeros(0))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "train_epoch.npz"))


def _setup(g, fused=True):
    from unlearn_saliency_amd.cls_head import use_fused_head
    model = TinyHead()
    init = tiny_state(int(g["state_seed"]))
    for k, v in init.items():                                       # the fixture's own copy of the initial state
        assert np.array_equal(v.numpy(), g["init_" + k]), k
    model.load_state_dict(init)
    model.cuda()
    if fused:
        use_fused_head(model)
    batches = tiny_batches(int(g["nb"]), int(g["bs"]), int(g["batch_seed"]))
    for i, (x, y) in enumerate(batches):
        assert np.array_equal(x, g[f"x{i}"]) and np.array_equal(y, g[f"y{i}"])
    loader = ListLoader([(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()) for x, y in batches])
    args = SimpleNamespace(**json.loads(str(g["args"])))
    return model, init, loader, args


def _run(model, loader, args, epochs, mask=None):
    from unlearn_saliency_amd.Classification.trainer import get_optimizer_and_scheduler, train
    optimizer, scheduler = get_optimizer_and_scheduler(model, args)
    lrs, accs = [], []
    optimizer.register_step_pre_hook(lambda opt, a, k: lrs.append(opt.param_groups[0]["lr"]))
    for epoch in range(epochs):
        accs.append(train(loader, model, nn.CrossEntropyLoss(), optimizer, epoch, args, mask=mask))
        scheduler.step()
    return optimizer, lrs, accs


@pytest.mark.parametrize("fused", [True, False])
def test_train_reproduces_the_reference_epochs(golden, fused):
    """Final parameters, BN buffers and momentum buffers by the rule test_classification_gpu.py compares RL epochs with
    (rtol 1e-5, atol 1e-6); the learning rate of every step and the returned accuracies as recorded."""
    from unlearn_saliency_amd.Classification.trainer.train import sgd_state_dict
    g = golden
    model, _, loader, args = _setup(g, fused)
    optimizer, lrs, accs = _run(model, loader, args, int(g["epochs"]))
    assert np.allclose(lrs, g["lr_steps"], rtol=1e-15, atol=0)
    assert abs(optimizer.param_groups[0]["lr"] - float(g["lr_after"])) <= 1e-15 * float(g["lr_after"])
    assert np.allclose(accs, g["acc"], rtol=1e-12, atol=0)
    for k, v in model.state_dict().items():
        assert np.allclose(v.cpu().numpy(), g["sd_" + k], rtol=1e-5, atol=1e-6), k
    state = sgd_state_dict(optimizer)["state"]
    for i, n in enumerate(g["names"]):
        assert np.allclose(state[i]["momentum_buffer"].cpu().numpy(), g["mom_" + str(n)], rtol=1e-5, atol=1e-6), n
    optimizer.close()


def test_masked_epoch_leaves_masked_out_parameters_bit_identical(golden):
    model, init, loader, args = _setup(golden)
    rng = np.random.default_rng(0)
    mask = {n: torch.from_numpy((rng.random(tuple(p.shape)) < 0.5).astype(np.int64)) for n, p in model.named_parameters()}
    optimizer, _, _ = _run(model, loader, args, 1, mask=mask)
    sd = model.state_dict()
    for n, m in mask.items():
        now, was = sd[n].cpu().numpy(), init[n].numpy()
        frozen = m.numpy() == 0
        assert np.array_equal(now[frozen].view(np.uint32), was[frozen].view(np.uint32)), n
        assert (now[~frozen] != was[~frozen]).mean() > 0.5, n
    optimizer.close()


def test_fused_and_library_head_agree_on_a_resnet18_step():
    """Both heads compute the same function of layer4's output f.  K23 lies within its bound E of the float64 model of
    that function (cls_head_ref_cpu.bounds), the library head within the any-order bound E' of the same derivation
    (its summation orders are not known), so the two differ by at most E + E' — for fc.weight.grad, fc.bias.grad and
    the gradient entering layer4."""
    from unlearn_saliency_amd.Classification.models.resnet_cifar import resnet18
    from unlearn_saliency_amd.cls_head import fused_cls_head
    torch.manual_seed(5)
    net = resnet18(num_classes=10).cuda().train()
    x = torch.rand(64, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (64,), device="cuda")
    with torch.no_grad():
        f = net.features(x)
    fa, fb = f.clone().requires_grad_(), f.clone().requires_grad_()
    loss_a, logits_a = fused_cls_head(fa, net.fc, y)
    loss_a.backward()
    ga = [fa.grad.clone(), net.fc.weight.grad.clone(), net.fc.bias.grad.clone()]
    net.fc.weight.grad = net.fc.bias.grad = None
    logits_b = net.fc(torch.flatten(net.avgpool(fb), 1))
    loss_b = F.cross_entropy(logits_b, y)
    loss_b.backward()
    gb = [fb.grad, net.fc.weight.grad, net.fc.bias.grad]
    B, C, H, W = f.shape
    xs = f.cpu().numpy().reshape(B, C, H * W)
    w, bias = net.fc.weight.detach().cpu().numpy(), net.fc.bias.detach().cpu().numpy()
    ex = R.model(xs, w, bias, y.cpu().numpy())
    e1, e2 = R.bounds(ex, xs, w, bias), R.bounds(ex, xs, w, bias, any_order=True)
    for a, b, n in zip(ga, gb, ("dx", "dw", "db")):
        want, tol = getattr(ex, n), getattr(e1, n) + getattr(e2, n)
        a, b = a.cpu().numpy().astype(np.float64).reshape(want.shape), b.cpu().numpy().astype(np.float64).reshape(want.shape)
        assert (np.abs(a - want) <= getattr(e1, n)).all(), n
        assert (np.abs(a - b) <= tol).all(), (n, float((np.abs(a - b) / tol).max()))
    assert abs(float(loss_a.detach()) - float(loss_b.detach())) <= e1.loss_mean + e2.loss_mean
    assert (np.abs(logits_a.cpu().numpy() - logits_b.detach().cpu().numpy()) <= e1.logits + e2.logits).all()


def test_l1_step_adds_the_penalty_gradient(golden):
    """One step from the same state with and without `l1`: the first SGD step is p - lr (g + wd p), and the penalty adds
    alpha * sign(p) to g, so the two results differ by lr * alpha * sign(p0) (compared by the rule of the epochs above:
    rtol 1e-5, atol 1e-6).  One batch per epoch: `warmup_lr` gives the full lr at its only step."""
    import copy
    results = []
    for l1 in (False, True):
        model, init, loader, args = _setup(golden)
        args = copy.copy(args)
        args.alpha = 0.01
        from unlearn_saliency_amd.Classification.trainer import get_optimizer_and_scheduler, train
        optimizer, _ = get_optimizer_and_scheduler(model, args)
        train(ListLoader(loader[:1]), model, nn.CrossEntropyLoss(), optimizer, 0, args, l1=l1)
        optimizer.close()
        results.append({n: p.detach().cpu().numpy().astype(np.float64) for n, p in model.named_parameters()})
    plain, pen = results
    for n, v in plain.items():
        want = args.lr * args.alpha * np.sign(init[n].numpy().astype(np.float64))
        assert np.allclose(v - pen[n], want, rtol=1e-5, atol=1e-6), n


def test_imagenet_arch_schedule_is_warmup_then_cosine(golden):
    """`--imagenet_arch`: LambdaLR with (e + 1) / warmup inside the warmup and 0.5 (1 + cos(pi (e - warmup) / (epochs -
    warmup))) after it, stepped once per epoch."""
    import copy
    import math
    from unlearn_saliency_amd.Classification.trainer import get_optimizer_and_scheduler
    model, _, _, args = _setup(golden, fused=False)
    args = copy.copy(args)
    args.imagenet_arch, args.warmup, args.epochs, args.lr = True, 2, 6, 0.1
    optimizer, scheduler = get_optimizer_and_scheduler(model, args)
    seen = []
    for _ in range(args.epochs):
        seen.append(optimizer.param_groups[0]["lr"])
        optimizer.step()
        scheduler.step()
    optimizer.close()
    want = [0.1 * ((e + 1) / 2 if e < 2 else 0.5 * (1.0 + math.cos(math.pi * (e - 2) / 4))) for e in range(6)]
    assert np.allclose(seen, want, rtol=1e-14, atol=0)
