"""The classifier that scores generated images (SD/eval-scripts/imageclassify.py): torchvision's ResNet-50 (v1.5), written
out because torchvision is not a dependency of this package.

`ResNet50` is a plain `nn.Module` that runs anywhere.  Its module tree carries torchvision's names - `conv1`, `bn1`,
`layer{1..4}.{j}.conv{1,2,3}`, `layer{1..4}.{j}.bn{1,2,3}`, `layer{1..4}.0.downsample.{0,1}`, `fc` - blocks (3, 4, 6, 3),
expansion 4, the stride on `conv2` - so `resnet50-11ad3fa6.pth` (ResNet50_Weights.DEFAULT) loads as it is: 25,557,032
parameters.

`InferencePlan50(model)` is the device form of `model.eval()`: every BatchNorm folded into the `scale` / `shift` of the
convolution in front of it (`fold_bn` and `_Conv` are DDPM/models/resnet34.py's), and per batch
    K26 resize -> crop + normalise -> stem (K27) -> 3 x 3 / 2 pool -> 16 bottlenecks -> evaluation head -> row top-k.
Of the 53 convolutions the 33 that are 1 x 1 / stride 1 run on K30 (csrc/salun_conv1x1_infer.hip) and the stem, the
3 x 3 and the three 1 x 1 / stride-2 projections on K27; K30 and K27 return the same bits for a 1 x 1 layer, so
`pointwise="k27"` moves those 33 to K27 without changing a result (POINTWISE_ON_K27 does it per shape).  The last
1 x 1 of a block carries the residual add and the ReLU in its epilogue; a projection runs ahead of it with relu = False.

Preprocessing is torchvision's `ImageClassification(crop_size=224, resize_size=232)` on a PIL image:
    resize   the SHORTER side to 232 with Pillow's antialiased bilinear (K26 is bit-identical to Pillow); the longer side
             becomes int(232 * long / short)                                               `resized_size`
    crop     224 x 224 at top = int(round((H - 224) / 2.0)), left likewise                   `crop_origin`
    scale    ((u / 255) - mean) / std, mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225)
A size pair K26 refuses (salun_resample_u8_lds_bytes == 0) is resized by Pillow on the host for those images, counted in
conv_infer.LIBRARY_INFER_CALLS["resize_host"].
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..DDPM.models.resnet34 import _Conv, fold_bn  # noqa: F401  (one definition of the folded convolution)

LAYERS = (3, 4, 6, 3)
WIDTHS = (64, 128, 256, 512)
EXPANSION = 4
NUM_PARAMETERS = 25_557_032
RESIZE_SIZE, CROP_SIZE = 232, 224
NORM_MEAN = (0.485, 0.456, 0.406)
NORM_STD = (0.229, 0.224, 0.225)
# (C, HW, K) of the 1 x 1 / stride-1 layers (at 224 x 224) that stay on K27 because K30 did not beat it there by more
# than the overlap of the two measured ranges
# (tools/imageclassify_bench.py; README "Stable Diffusion: classification of generated images").  Identical bits make
# this a table entry.
POINTWISE_ON_K27: frozenset = frozenset({(64, 3136, 256), (256, 196, 1024), (512, 49, 2048)})


def resized_size(h: int, w: int, size: int = RESIZE_SIZE):
    """(OH, OW) of transforms.Resize(size) on an h x w image: the shorter side becomes `size`."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def crop_origin(h: int, w: int, crop: int = CROP_SIZE):
    """(top, left) of transforms.CenterCrop(crop) on an h x w image with h, w >= crop."""
    return int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))


class Bottleneck(nn.Module):
    expansion = EXPANSION

    def __init__(self, inplanes: int, planes: int, stride: int = 1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * EXPANSION, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * EXPANSION)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if stride != 1 or inplanes != planes * EXPANSION:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * EXPANSION, 1, stride, bias=False),
                                            nn.BatchNorm2d(planes * EXPANSION))
        self.stride = stride

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + identity)


class ResNet50(nn.Module):
    def __init__(self, num_classes: int = 1000):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inplanes = 64
        for i, (planes, blocks) in enumerate(zip(WIDTHS, LAYERS)):
            stride = 1 if i == 0 else 2
            layer = [Bottleneck(inplanes, planes, stride)]
            inplanes = planes * EXPANSION
            layer += [Bottleneck(inplanes, planes) for _ in range(blocks - 1)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*layer))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * EXPANSION, num_classes)
        for m in self.modules():                       # torchvision's initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def resnet50(num_classes: int = 1000) -> ResNet50:
    return ResNet50(num_classes)


FC_STD = 1e-4   # the 2048 pooled features of the untrained stand-in average ~300 at 224 x 224: logits within ~6 units


def standin_state_dict(seed: int = 0, num_classes: int = 1000) -> dict:
    """Seeded stand-in weights for runs without torchvision's checkpoint (`--synthetic`, the tests), after the ResNet-34
    stand-in: Kaiming convolutions, gamma and running_var uniform in [0.5, 1.5], beta and running_mean from N(0, 0.1),
    and an `fc` small enough (std FC_STD) that the logits of a 224 x 224 image stay within a few units."""
    g = torch.Generator().manual_seed(seed)
    sd = ResNet50(num_classes).state_dict()
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
        elif k == "fc.weight":
            v.copy_(torch.randn(v.shape, generator=g) * FC_STD)
        elif k == "fc.bias":
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
    return sd


class InferencePlan50:
    """`model.eval()` of a ResNet50 on the device kernels.  Build it once after `load_state_dict`.  Activations live in
    four buffers allocated once per (batch, height, width)."""

    def __init__(self, model: ResNet50, device="cuda", pointwise: str = "auto"):
        from .. import ops_infer
        if pointwise not in ("auto", "k30", "k27"):
            raise ValueError("pointwise: auto, k30 or k27")
        self.device = torch.device(device)
        self.pointwise = pointwise
        self.stem = _Conv(model.conv1, model.bn1, self.device)
        self.blocks = []
        for i in range(4):
            for blk in getattr(model, f"layer{i + 1}"):
                down = None if blk.downsample is None else _Conv(blk.downsample[0], blk.downsample[1], self.device)
                self.blocks.append((_Conv(blk.conv1, blk.bn1, self.device), _Conv(blk.conv2, blk.bn2, self.device),
                                    _Conv(blk.conv3, blk.bn3, self.device), down))
        self.fc_w = model.fc.weight.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.fc_b = model.fc.bias.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.table = ops_infer.u8_norm_table(NORM_MEAN, NORM_STD).to(self.device)
        self._bufs: dict = {}
        self.kernel_calls = {"k30": 0, "k27": 0}     # convolutions of the last `features` call, by kernel

    # The largest activation is the stem's output (64 channels at half the side) or a layer1 output (256 channels at a
    # quarter of it): the same number of elements where the side is a multiple of 4, the former otherwise.
    def _buffers(self, B: int, H: int, W: int):
        key = (B, H, W)
        if key not in self._bufs:
            P, Q = self.stem.out_size(H), self.stem.out_size(W)
            n = B * max(64 * P * Q, 256 * ((P + 1) // 2) * ((Q + 1) // 2), 3 * H * W)
            self._bufs[key] = [torch.empty(n, dtype=torch.float32, device=self.device) for _ in range(4)]
        return self._bufs[key]

    def _run(self, cv: _Conv, x, out, addend=None, relu=True):
        from .. import conv_infer as ci
        pw = cv.R == 1 and cv.stride == 1 and self.pointwise != "k27" and not (
            self.pointwise == "auto" and (int(x.shape[1]), int(x.shape[2] * x.shape[3]), cv.K) in POINTWISE_ON_K27)
        self.kernel_calls["k30" if pw else "k27"] += 1
        if pw:
            return ci.conv1x1_bn_act(x, cv.w, cv.scale, cv.shift, addend, relu, out=out)
        return ci.conv_bn_act(x, cv.w, cv.scale, cv.shift, addend, relu, cv.stride, cv.pad, out=out)

    def features(self, x_norm: torch.Tensor) -> torch.Tensor:
        """Normalised fp32 images [B, 3, H, W] -> the last feature map [B, 2048, h, w] (a view of a plan buffer)."""
        from .. import conv_infer as ci
        B, _, H, W = (int(v) for v in x_norm.shape)
        bufs = self._buffers(B, H, W)
        free = [b for b in bufs if b.data_ptr() != x_norm.data_ptr()][:3]
        self.kernel_calls = {"k30": 0, "k27": 0}
        y = self._run(self.stem, x_norm, free[0])
        ph, pq = (y.shape[2] + 1) // 2, (y.shape[3] + 1) // 2
        x = ci.maxpool3x3s2(y, out=free[1][:B * 64 * ph * pq])
        # Four roles per block - input, conv1's output, conv2's output, the projection - in three buffers: conv1's
        # output is dead once conv2 ran, and the block's input once conv1 and the projection ran.
        cur = 1
        for c1, c2, c3, down in self.blocks:
            a, b = [i for i in range(3) if i != cur]
            h, w = int(x.shape[2]), int(x.shape[3])
            P, Q = c2.out_size(h), c2.out_size(w)
            h1 = self._run(c1, x, free[a][:B * c1.K * h * w])
            h2 = self._run(c2, h1, free[b][:B * c2.K * P * Q])
            n_out = B * c3.K * P * Q
            if down is None:
                x = self._run(c3, h2, free[a][:n_out], addend=x)
                cur = a
            else:
                idn = self._run(down, x, free[a][:n_out], relu=False)
                x = self._run(c3, h2, free[cur][:n_out], addend=idn)
        return x

    def forward(self, x_norm: torch.Tensor):
        """-> (logits [B, 1000], p [B, 1000])."""
        from .. import ops_infer
        return ops_infer.cls_head_eval(self.features(x_norm), self.fc_w, self.fc_b, 0, None)

    def preprocess_u8(self, images_u8_nhwc: torch.Tensor) -> torch.Tensor:
        """uint8 [B, h, w, 3] device images of ONE size -> normalised fp32 [B, 3, 224, 224] (a view of a plan buffer)."""
        from .. import conv_infer as ci
        from .. import ops_resample
        B, h, w, C = (int(v) for v in images_u8_nhwc.shape)
        OH, OW = resized_size(h, w)
        if (OH, OW) == (h, w):
            u8 = images_u8_nhwc.contiguous()
        elif ops_resample.lds_bytes(h, w, C, OH, OW) != 0:
            u8 = ops_resample.resize_u8(images_u8_nhwc.contiguous(), (OH, OW))
        else:
            import numpy as np
            from PIL import Image
            ci.LIBRARY_INFER_CALLS["resize_host"] += B
            host = images_u8_nhwc.cpu().numpy()
            u8 = torch.from_numpy(np.stack([np.asarray(Image.fromarray(im).resize((OW, OH), Image.BILINEAR))
                                            for im in host])).to(self.device)
        top, left = crop_origin(OH, OW)
        bufs = self._buffers(B, CROP_SIZE, CROP_SIZE)
        return ci.u8_crop_to_chw_norm(u8, self.table, top, left, CROP_SIZE, CROP_SIZE,
                                      out=bufs[3][:B * 3 * CROP_SIZE * CROP_SIZE])

    def classify_u8(self, images_u8_nhwc: torch.Tensor, topk: int = 5):
        """uint8 [B, h, w, 3] device images of one size -> (scores [B, topk] fp32, indices [B, topk] int64): the
        reference's `model(batch).softmax(1)` and `torch.topk`."""
        from .. import ops_infer
        _, p = self.forward(self.preprocess_u8(images_u8_nhwc))
        return ops_infer.row_topk(p, topk)


def library_forward(model: ResNet50, x: torch.Tensor) -> torch.Tensor:
    """The same network on the library modules (`model.eval()` under no_grad): the comparison of the benchmark."""
    with torch.no_grad():
        return model(x)
