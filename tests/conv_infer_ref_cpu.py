"""float64 models of K27 and the kernels around it (csrc/salun_conv_infer.hip, salun_pool.hip, salun_imgnorm.hip, the
evaluation head of salun_cls_head.hip), the inputs the exact-answer tests feed them and the shapes they run.  Importable
without a GPU; validated against torch's float64 conv2d, max_pool2d and batch_norm by test_conv_infer_ref_cpu.py; used by
test_conv_infer_gpu.py, test_classifier_kernels_gpu.py and test_classifier_eval_gpu.py.

The convolution itself is conv_ref_cpu.forward (the definition written out tap by tap; it takes any square filter).
K27's epilogue is
    y = act(((conv * scale[k]) + shift[k]) + addend),   act(o) = o < 0 ? 0 : o,
each term optional.  `absolute=True` computes the same expression over absolute values with no activation: the
quantity a rounding-error bound is a multiple of.

Exact tier: as in conv_ref_cpu.py, x and w are small integers times powers of two that sit on the axes the reduction
does not run over (image n: 2^(-7 (n mod 3)), output channel k: 2^(5 (k mod 3))).  scale[k] is a non-zero integer of
[-2, 2] with no power of two of its own, so conv * scale stays on the element's grid; shift[k] carries the channel's
scale (a whole multiple of every image's grid), addend the element's.  test_conv_infer_ref_cpu.py asserts that abs_sum
stays below 2^24 grid steps for every case: then every partial sum in every order, the multiplication and both
additions are exact in fp32, and y must EQUAL the model.
"""
from types import SimpleNamespace

import torch

import conv_ref_cpu as B
from conv_ref_cpu import U, Case, bound_gamma, gaussian, impulses, integers, scales  # noqa: F401  (re-exported)

# (N, C, H, W, K, R, stride, pad): the smallest shapes at which K27's index arithmetic can go wrong
CASES = [Case(*s) for s in [
    (3, 8, 7, 7, 32, 3, 1, 1),          # 147 pixels: tail tile, odd width
    (2, 8, 14, 14, 32, 3, 2, 1),        # 14 -> 7
    (2, 8, 14, 14, 32, 1, 2, 0),
    (1, 16, 5, 9, 64, 3, 1, 1),         # rectangular
    (1, 8, 28, 28, 64, 3, 1, 1),
    (1, 8, 56, 56, 64, 3, 1, 1),
    (2, 3, 20, 20, 64, 7, 2, 3),        # stem shape
    (1, 3, 224, 224, 64, 7, 2, 3),      # the stem itself
    (1, 64, 9, 9, 128, 3, 1, 1),        # 128-channel tile
    (1, 512, 7, 7, 512, 3, 1, 1),       # longest reduction
]]
TILES = (1, 2, 3)                        # SALUN_INFER_TILE_64X64, _128X64, _128X128
EPILOGUES = [(), ("scale",), ("shift",), ("addend",), ("scale", "shift"), ("scale", "addend"), ("shift", "addend"),
             ("scale", "shift", "addend")]
REFUSED = {"K = 48": dict(K=48), "R = 5": dict(R=5, pad=2), "stride 3": dict(stride=3)}


def route(c, tile=0):
    """The label K27's plan gives (the mirror of plan_infer in csrc/salun_conv_infer.hip), or None where it refuses."""
    N, C, H, W, K, R, s, pad = c
    P, Q = c.P, c.Q
    if N < 1 or not 1 <= C <= 65536 or K < 32 or K % 32 or K > 65536 or R not in (1, 3, 7) or (R != 7 and C % 8):
        return None
    if s not in (1, 2) or not 0 <= pad < R or not all(1 <= v <= 1024 for v in (H, W, P, Q)):
        return None
    if (P - 1) * s - pad >= H or (Q - 1) * s - pad >= W or N * P * Q > 1 << 40:
        return None
    pb, kb = (0, 64, 128, 128), (0, 64, 64, 128)
    blocks = lambda t: -(-N * P * Q // pb[t]) * -(-K // kb[t])
    t = tile
    if t == 0:
        t = 3 if (K % 128 == 0 and blocks(3) >= 256) else 2 if blocks(2) >= 256 else 1
    return f"infer<{R},{s}>/{pb[t]}x{kb[t]}/{'generic' if C % 16 else 'fast'}/B{blocks(t)}"


def epilogue(conv, scale=None, shift=None, addend=None, relu=False, absolute=False):
    if absolute:
        scale, shift, addend = (None if t is None else t.abs() for t in (scale, shift, addend))
    y = conv
    if scale is not None:
        y = y * scale[None, :, None, None]
    if shift is not None:
        y = y + shift[None, :, None, None]
    if addend is not None:
        y = y + addend
    return torch.where(y < 0, torch.zeros_like(y), y) if (relu and not absolute) else y


def forward(x, w, c, scale=None, shift=None, addend=None, relu=False, absolute=False):
    conv = B.forward(x, w, c.stride, c.pad, c.P, c.Q, absolute=absolute)
    return epilogue(conv, scale, shift, addend, relu, absolute)


def inputs(c, kind):
    """x, w, scale, shift, addend of one case (float64 tensors that fp32 holds exactly) and `unit`, each element's grid."""
    N, C, H, W, K, R = c.N, c.C, c.H, c.W, c.K, c.R
    sn, sk = scales(N, B.IMG_EXP), scales(K, B.CH_EXP)
    if kind == "int":
        x = integers((N, C, H, W), -3, 3, 1, B.IMG_EXP)
        w = integers((K, C, R, R), -2, 2, 2, B.CH_EXP)
        scale = integers((K,), 1, 2, 9) * (1 - 2 * (torch.arange(K) % 2)).double()       # +-1, +-2: never 0
        shift = integers((K,), -2, 2, 3, B.CH_EXP)
        addend = integers((N, K, c.P, c.Q), -2, 2, 5, B.IMG_EXP, B.CH_EXP)
    else:
        x, w = gaussian((N, C, H, W), 1, B.IMG_EXP), gaussian((K, C, R, R), 2, B.CH_EXP)
        scale, shift = gaussian((K,), 9), gaussian((K,), 3, B.CH_EXP)
        addend = gaussian((N, K, c.P, c.Q), 5, B.IMG_EXP, B.CH_EXP)
    return SimpleNamespace(x=x, w=w, scale=scale, shift=shift, addend=addend,
                           unit=sn.view(N, 1, 1, 1) * sk.view(1, K, 1, 1))


def terms_of(t, names):
    return {n: getattr(t, n) for n in names}


# ------------------------------------------------------------------------------------------ pool, normalise, BatchNorm
def maxpool3x3s2(x):
    """MaxPool2d(3, 2, 1) of [..., H, W] with F.max_pool2d's selection: scan the window row by row from -inf, take a
    value when it is greater than the running maximum or is NaN; padding is skipped."""
    H, W = x.shape[-2:]
    OH, OW = (H + 1) // 2, (W + 1) // 2
    xp = x.new_full(x.shape[:-2] + (2 * OH + 1, 2 * OW + 1), float("-inf"))
    xp[..., 1:1 + H, 1:1 + W] = x
    m = x.new_full(x.shape[:-2] + (OH, OW), float("-inf"))
    for r in range(3):
        for s in range(3):
            v = xp[..., r:r + 2 * OH:2, s:s + 2 * OW:2]
            m = torch.where((v > m) | torch.isnan(v), v, m)
    return m


def pool_data(shape, seed=0):
    """fp32 data with NaN, +-0, -inf and equal maxima sprinkled in."""
    g = torch.Generator().manual_seed(seed + 17)
    x = torch.randint(-3, 4, shape, generator=g).float()          # few distinct values: equal maxima in most windows
    special = torch.tensor([float("nan"), 0.0, -0.0, float("-inf"), 3.0])
    pick = torch.randint(0, 12, shape, generator=g)
    for i, v in enumerate(special):
        x = torch.where(pick == i, v, x)
    return x


def normalize_u8(u8_nhwc, mean, std):
    """ToTensor + Normalize as torch computes them, in fp32 on the CPU: [B, H, W, C] uint8 -> [B, C, H, W] fp32."""
    t = u8_nhwc.permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32).view(1, -1, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(1, -1, 1, 1)
    return t.sub_(m).div_(s)


def fold_bn(gamma, beta, mean, var, eps):
    """scale, shift in float64 with conv * scale + shift == batch_norm(conv) in eval mode."""
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return scale, beta.double() - mean.double() * scale


# ------------------------------------------------------------------------------------------ the evaluation figures
def eval_figures(logits64, label, drop_zero_below=None):
    """The reference's formulas (classifier_evaluation.py:25-36) in float64, as SUMS over the batch: entropy, p[label],
    hits.  drop_zero_below: classes whose probability is below it contribute nothing to the entropy (the 0 * log 0 = 0
    convention, for rows where fp32 underflows)."""
    p = torch.softmax(logits64, -1)
    terms = p * torch.log(p)
    if drop_zero_below is not None:
        terms = torch.where(p < drop_zero_below, torch.zeros_like(terms), terms)
    ent = -terms.sum(1)
    return SimpleNamespace(p=p, entropy=ent, entropy_sum=float(ent.sum()), prob_sum=float(p[:, label].sum()),
                           hits=int((logits64.argmax(-1) == label).sum()), count=logits64.shape[0])


def top_two_gap(logits64):
    top = logits64.topk(2, -1).values
    return top[:, 0] - top[:, 1]
