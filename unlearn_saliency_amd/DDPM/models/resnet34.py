"""The classifier that scores generated images (DDPM/classifier_evaluation.py): torchvision's ResNet-34 with a 10-way
head, written out because torchvision is not a dependency of this package.

`ResNet34` is a plain `nn.Module` that runs anywhere.  Its module tree carries torchvision's names — `conv1`, `bn1`,
`layer{1..4}.{i}.conv{1,2}`, `layer{1..4}.{i}.bn{1,2}`, `layer{2..4}.0.downsample.{0,1}`, `fc` — so its `state_dict()` has
torchvision's keys and shapes (`num_batches_tracked` included) and a checkpoint written by
`torchvision.models.resnet34` with `fc = nn.Linear(512, 10)` loads as it is.

`InferencePlan(model)` is the device form of `model.eval()`: built once after `load_state_dict`, it folds every
BatchNorm into the per-channel `scale` / `shift` of the convolution in front of it and runs the network on K26
(resize), the normalise kernel, K27 (all 36 convolutions, the residual add and the ReLU in their epilogues), the
3 x 3 / stride-2 pool and the evaluation head — 40 launches per batch, no library convolution.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

LAYERS = (3, 4, 6, 3)
WIDTHS = (64, 128, 256, 512)
NORM_MEAN = (0.5, 0.5, 0.5)     # classifier_evaluation.py:91-92
NORM_STD = (0.5, 0.5, 0.5)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or inplanes != planes:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
        self.stride = stride

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + identity)


class ResNet34(nn.Module):
    def __init__(self, num_classes: int = 10):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inplanes = 64
        for i, (planes, blocks) in enumerate(zip(WIDTHS, LAYERS)):
            stride = 1 if i == 0 else 2
            layer = [BasicBlock(inplanes, planes, stride)] + [BasicBlock(planes, planes) for _ in range(blocks - 1)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*layer))
            inplanes = planes
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, num_classes)
        for m in self.modules():                       # torchvision's initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def resnet34(num_classes: int = 10) -> ResNet34:
    return ResNet34(num_classes)


def standin_state_dict(seed: int = 0, num_classes: int = 10) -> dict:
    """Seeded stand-in weights for runs without a trained checkpoint (`--synthetic`, the tests): Kaiming convolutions,
    gamma and running_var uniform in [0.5, 1.5], beta and running_mean from N(0, 0.1)."""
    g = torch.Generator().manual_seed(seed)
    model = ResNet34(num_classes)
    sd = model.state_dict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        if v.dim() == 4:
            fan_out = v.shape[0] * v.shape[2] * v.shape[3]
            v.copy_(torch.randn(v.shape, generator=g) * (2.0 / fan_out) ** 0.5)
        elif k.endswith("running_var") or (k.endswith(".weight") and v.dim() == 1):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif k.endswith("running_mean") or (k.endswith(".bias") and not k.startswith("fc.")):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif k == "fc.weight":      # untrained BatchNorms let the features grow to a few hundred: a head this small keeps
            v.copy_(torch.randn(v.shape, generator=g) * 4e-4)        # the logits of a 224 x 224 image within a few units
        elif k == "fc.bias":
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
    return sd


def fold_bn(bn: nn.BatchNorm2d):
    """scale = gamma / sqrt(var + eps), shift = beta - mean * scale, in float64, each rounded ONCE to fp32."""
    var, mean = bn.running_var.detach().double().cpu(), bn.running_mean.detach().double().cpu()
    gamma, beta = bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu()
    scale = gamma / torch.sqrt(var + bn.eps)
    shift = beta - mean * scale
    return scale.float(), shift.float()


class _Conv:
    """One convolution of the plan: its weight, folded BatchNorm, stride and padding, on the device."""
    __slots__ = ("w", "scale", "shift", "stride", "pad", "K", "R")

    def __init__(self, conv: nn.Conv2d, bn: nn.BatchNorm2d, device):
        self.w = conv.weight.detach().to(device=device, dtype=torch.float32).contiguous()
        scale, shift = fold_bn(bn)
        self.scale, self.shift = scale.to(device), shift.to(device)
        self.stride, self.pad = conv.stride[0], conv.padding[0]
        self.K, self.R = conv.out_channels, conv.kernel_size[0]

    def out_size(self, n: int) -> int:
        return (n + 2 * self.pad - self.R) // self.stride + 1


class InferencePlan:
    """`model.eval()` of a ResNet34 on the device kernels.  Build it once after `load_state_dict`; `forward_u8` and
    `forward` run a batch.  Activations ping-pong in three buffers allocated once per batch size."""

    def __init__(self, model: ResNet34, device="cuda", size: int = 224, mean=NORM_MEAN, std=NORM_STD):
        from ... import ops_infer
        self.device = torch.device(device)
        self.size = int(size)
        self.stem = _Conv(model.conv1, model.bn1, self.device)
        self.blocks = []
        for i in range(4):
            for blk in getattr(model, f"layer{i + 1}"):
                down = None if blk.downsample is None else _Conv(blk.downsample[0], blk.downsample[1], self.device)
                self.blocks.append((_Conv(blk.conv1, blk.bn1, self.device), _Conv(blk.conv2, blk.bn2, self.device), down))
        self.fc_w = model.fc.weight.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.fc_b = model.fc.bias.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.table = ops_infer.u8_norm_table(mean, std).to(self.device)
        self._bufs: dict = {}

    # the largest activation of a batch is the stem's output: 64 channels at half the input side
    def _buffers(self, B: int, H: int, W: int):
        key = (B, H, W)
        if key not in self._bufs:
            n = B * 64 * self.stem.out_size(H) * self.stem.out_size(W)
            self._bufs[key] = [torch.empty(max(n, B * 3 * H * W), dtype=torch.float32, device=self.device)
                               for _ in range(4)]
        return self._bufs[key]

    def features(self, x_norm: torch.Tensor) -> torch.Tensor:
        """Normalised fp32 images [B, 3, H, W] -> the last feature map [B, 512, h, w] (a view of a plan buffer)."""
        from ... import conv_infer as ci
        B, _, H, W = (int(v) for v in x_norm.shape)
        bufs = self._buffers(B, H, W)
        free = [b for b in bufs if b.data_ptr() != x_norm.data_ptr()][:3]

        def run(cv: _Conv, x, out, addend=None, relu=True):
            return ci.conv_bn_act(x, cv.w, cv.scale, cv.shift, addend, relu, cv.stride, cv.pad, out=out)

        y = run(self.stem, x_norm, free[0])
        x = ci.maxpool3x3s2(y, out=free[1][:B * 64 * ((y.shape[2] + 1) // 2) * ((y.shape[3] + 1) // 2)])
        cur = 1                                    # index of the buffer that holds the block's input
        for c1, c2, down in self.blocks:
            a, b = [i for i in range(3) if i != cur]
            P, Q = c1.out_size(x.shape[2]), c1.out_size(x.shape[3])
            n_out = B * c1.K * P * Q
            h = run(c1, x, free[a][:n_out])
            if down is None:
                x = run(c2, h, free[b][:n_out], addend=x)
                cur = b
            else:
                idn = run(down, x, free[b][:n_out], relu=False)
                x = run(c2, h, free[cur][:n_out], addend=idn)      # the block's input is dead once conv1 and down ran
        return x

    def forward(self, x_norm: torch.Tensor, label: int = 0, meters=None, zero_safe: bool = False):
        """-> (logits [B, 10], p [B, 10]); adds to `meters` (ops_infer.EvalMeters) when given."""
        from ... import ops_infer
        return ops_infer.cls_head_eval(self.features(x_norm), self.fc_w, self.fc_b, label, meters, zero_safe)

    def forward_u8(self, images_u8_nhwc: torch.Tensor, label: int = 0, meters=None, zero_safe: bool = False):
        """uint8 [B, h, w, 3] device images -> resize to size x size (K26) -> normalise -> network -> evaluation head."""
        from ... import conv_infer as ci
        from ... import ops_resample
        B, h, w, _ = (int(v) for v in images_u8_nhwc.shape)
        u8 = images_u8_nhwc if (h, w) == (self.size, self.size) else \
            ops_resample.resize_u8(images_u8_nhwc.contiguous(), (self.size, self.size))
        bufs = self._buffers(B, self.size, self.size)
        x = ci.u8_to_chw_norm(u8, self.table, out=bufs[3][:B * 3 * self.size * self.size])
        return self.forward(x, label, meters, zero_safe)


def library_forward(model: ResNet34, x: torch.Tensor) -> torch.Tensor:
    """The same network on the library modules (`model.eval()` under no_grad): the comparison of the benchmark."""
    with torch.no_grad():
        return model(x)
