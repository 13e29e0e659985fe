"""The VGG-16-BN fixture shared by tests/golden/make_golden_vgg.py (which feeds it to the reference's model in
float64) and by test_vgg_host.py / test_vgg_gpu.py: one fill rule for every state_dict entry, one batch.  Everything
comes from the counter-based generator, one seed per tensor, so it regenerates identically anywhere."""
import numpy as np
import torch

from unlearn_saliency_amd import rng

SEED = 4100
BATCH = 8
LAST_CONV = "features.40.weight"
GRAD_NAMES = ("classifier.weight", "features.0.weight", "features.0.bias", "features.1.weight", LAST_CONV)
# the last convolution's weight gradient has 2.36 M elements (19 MB in float64): the fixture keeps every 97th
SAMPLE_STRIDE = {LAST_CONV: 97}


def fill_state(model, seed=SEED):
    """Every floating-point state_dict entry from its own seed: convolution weights N(0, 2 / fan_in) (activations keep
    their scale through the thirteen layers), the classifier N(0, 0.05^2), biases N(0, 0.05^2), BatchNorm weights
    U[0.8, 1.2), running means N(0, 0.1^2), running variances U[0.5, 1.5)."""
    with torch.no_grad():
        for i, (k, v) in enumerate(model.state_dict().items()):
            if not v.dtype.is_floating_point:
                continue
            s, n = seed + 1000 * i, v.numel()
            if v.dim() == 4:
                a = rng.normal(n, s, 0.0, float(np.sqrt(2.0 / (v.shape[1] * v.shape[2] * v.shape[3]))))
            elif v.dim() == 2:
                a = rng.normal(n, s, 0.0, 0.05)
            elif k.endswith("running_var"):
                a = rng.uniform(n, s, 0.5, 1.5)
            elif k.endswith("running_mean"):
                a = rng.normal(n, s, 0.0, 0.1)
            elif k.endswith("weight"):                       # BatchNorm
                a = rng.uniform(n, s, 0.8, 1.2)
            elif k.endswith("bias"):
                a = rng.normal(n, s, 0.0, 0.05)
            else:                                            # normalize.mean / normalize.std stay as built
                continue
            v.copy_(torch.from_numpy(a).view_as(v))
    return model


# The batch is the first of the seeds SEED + 500_000 + 1000 k for which the float64 reference decides every ReLU and
# every pool window with a margin of at least 2^-20 in both modes (no BatchNorm output closer to zero, no positive
# window maximum closer to its runner-up): make_golden_vgg.py asserts that.  An fp32 path whose activations are off by
# less than that takes the same decisions; without the margin one flipped ReLU among the 524,288 outputs of the first
# layers moves their weight gradients by about 1e-3 relative, whatever the code under test does.
BATCH_SEED = SEED + 503_000
DECISION_MARGIN = 2.0 ** -20


def batch(seed=BATCH_SEED):
    x = rng.uniform(BATCH * 3 * 32 * 32, seed, 0.0, 1.0).reshape(BATCH, 3, 32, 32)
    y = (rng.u8(BATCH, seed + 1) % 10).astype(np.int64)
    return torch.from_numpy(x), torch.from_numpy(y)


def sample(name, t):
    """The part of gradient `name` that the fixture keeps (flat)."""
    return t.reshape(-1)[::SAMPLE_STRIDE.get(name, 1)]


def run(model, train, want_grads):
    """Logits of the fixture batch in the model's own dtype / device and, if asked, the gradients of the mean
    cross-entropy for GRAD_NAMES (sampled).  The model is filled first, so running statistics start from the rule."""
    import torch.nn.functional as F
    fill_state(model)
    p = next(model.parameters())
    x, y = batch()
    x, y = x.to(device=p.device, dtype=p.dtype), y.to(p.device)
    model.train(train)
    model.zero_grad(set_to_none=True)
    logits = model(x)
    grads = {}
    if want_grads:
        F.cross_entropy(logits, y).backward()
        params = dict(model.named_parameters())
        grads = {n: sample(n, params[n].grad.detach()) for n in GRAD_NAMES}
    return logits.detach(), grads
