"""kappa = (mu^2 + sigma^2) / (sigma^2 + eps) of the inputs of every normalisation layer, on the CPU in float64: the
quantity the error of the fused statistics grows with (tests/norm_ref_cpu.py).  Measured on the
networks of the test fixtures with their seeded parameters: ResNet-18 at its random initialisation on a uniform batch,
and the reduced CFG-DDPM U-Net of tests/fixtures.py.  These are untrained networks; trained activations can sit further
from zero, which is why the bound tier goes to mu / sigma = 2^8.      python tools/norm_kappa.py"""
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def kappa(mu, var, eps):
    return float(((mu * mu + var) / (var + eps)).max())


def report(name, values):
    values = sorted(values)
    print(f"{name}: {len(values)} layers, kappa max {values[-1]:.3g}, median {values[len(values) // 2]:.3g}")


def main():
    from fixtures import ddpm_batch, ddpm_small_config, fill_params
    from unlearn_saliency_amd.Classification.models import model_dict
    from unlearn_saliency_amd.DDPM.models.diffusion import Conditional_Model
    torch.manual_seed(0)
    bn, gn = [], []

    def bn_hook(mod, inp):
        x = inp[0].detach().double()
        bn.append(kappa(x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False), mod.eps))

    def gn_hook(mod, inp):
        x = inp[0].detach().double()
        xg = x.reshape(x.shape[0], mod.num_groups, -1)
        gn.append(kappa(xg.mean(2), xg.var(2, unbiased=False), mod.eps))

    net = model_dict["resnet18"](num_classes=10).train()
    for mod in net.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.register_forward_pre_hook(bn_hook)
    net(torch.rand(64, 3, 32, 32))
    report("ResNet-18, BatchNorm inputs", bn)
    unet = fill_params(Conditional_Model(ddpm_small_config()), 7000).train()
    for mod in unet.modules():
        if isinstance(mod, nn.GroupNorm):
            mod.register_forward_pre_hook(gn_hook)
    xb, cb = ddpm_batch(4, 77)
    unet(torch.from_numpy(xb).float() * 2 - 1, torch.tensor([5.0, 300.0, 640.0, 999.0]), torch.from_numpy(cb), "train",
         cond_drop_prob=0.0)
    report("reduced CFG-DDPM U-Net, GroupNorm inputs", gn)


if __name__ == "__main__":
    main()
