"""What test_classifier_eval_host.py (CPU) and test_classifier_eval_gpu.py share: the seeded stand-in ResNet-34, its
float64 copy on the CPU, the inputs of the network comparison, the 12 end-to-end images and their float64 pipeline
(PIL resize -> ToTensor / Normalize -> float64 network -> the reference's formulas).  Everything is computed once per
process and left unchanged.

The tolerance of the network comparison is not a fixed number.  `library_figure(x)` is the largest
|logit - float64| / max |float64 logit| of the SAME module tree in fp32 on the CPU library; the device is allowed
DEVICE_FACTOR = 8 times that, because its kernels sum in another order through 36 layers.  LOGIT_BOUND(x) is that
allowance as an absolute number.  The end-to-end seed is chosen so that every sample's float64 top-two gap is above
GAP_FACTOR = 100 times the bound (asserted on the CPU): no sample's argmax can depend on the rounding."""
import functools

import numpy as np
import torch

import conv_infer_ref_cpu as R

WEIGHT_SEED = 0
IMAGE_SEED = 1
LABEL = 4          # the class every stand-in sample falls into: the head is untrained, its argmax barely moves
DEVICE_FACTOR, GAP_FACTOR, FIGURE_FACTOR = 8, 100, 10
N_IMAGES, SIDE, BATCH = 12, 32, 5
GOLDEN_ROWS = [("other/run", (1.25, 0.1, 0.0)), ("a/b", (2.0, 0.3, 1.0)), ("a/b", (0.6875, 1e-05, 0.0625)),
               ("nan/row", (float("nan"), 0.5, 0.25))]


@functools.lru_cache(None)
def state_dict():
    from unlearn_saliency_amd.DDPM.models.resnet34 import standin_state_dict
    return standin_state_dict(WEIGHT_SEED)


@functools.lru_cache(None)
def models():
    """(fp32 module, float64 module) with the same state_dict, both in eval mode on the CPU."""
    from unlearn_saliency_amd.DDPM.models.resnet34 import resnet34
    m32, m64 = resnet34(10), resnet34(10).double()
    m32.load_state_dict(state_dict())
    m64.load_state_dict(state_dict())
    return m32.eval(), m64.eval()


@functools.lru_cache(None)
def network_inputs(n, side):
    g = torch.Generator().manual_seed(100 + side)
    return torch.randn((n, 3, side, side), generator=g, dtype=torch.float32)


def _logits(x32):
    m32, m64 = models()
    with torch.no_grad():
        return m32(x32).double(), m64(x32.double())


@functools.lru_cache(None)
def network_reference(n, side):
    """-> (float64 logits, the library's fp32 figure, the absolute logit bound of the device)."""
    l32, l64 = _logits(network_inputs(n, side))
    top = float(l64.abs().max())
    figure = float((l32 - l64).abs().max()) / top
    return l64, figure, DEVICE_FACTOR * figure * top


@functools.lru_cache(None)
def images():
    """12 uint8 images of 32 x 32 x 3: smooth random fields, so that neighbouring samples differ visibly."""
    r = np.random.default_rng(IMAGE_SEED)
    coarse = r.integers(0, 256, (N_IMAGES, 4, 4, 3)).astype(np.float64)
    img = np.kron(coarse, np.ones((1, 8, 8, 1))) + r.normal(0, 12, (N_IMAGES, SIDE, SIDE, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


@functools.lru_cache(None)
def pipeline_reference():
    """The float64 pipeline of the 12 images -> dict(logits, figure, bound, entropy, prob, accuracy, gap)."""
    from PIL import Image
    big = np.stack([np.asarray(Image.fromarray(im).resize((224, 224), Image.BILINEAR)) for im in images()])
    x = R.normalize_u8(torch.from_numpy(big), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    l32, l64 = _logits(x)
    top = float(l64.abs().max())
    figure = float((l32 - l64).abs().max()) / top
    f = R.eval_figures(l64, LABEL)
    return dict(logits=l64, figure=figure, bound=DEVICE_FACTOR * figure * top, entropy=f.entropy_sum / N_IMAGES,
                prob=f.prob_sum / N_IMAGES, accuracy=f.hits / N_IMAGES, gap=float(R.top_two_gap(l64).min()))
