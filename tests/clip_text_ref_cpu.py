"""torch-float64 restatement of K29 (csrc/salun_clip_text.hip) and of the whole CLIP text forward on the CPU (test
infrastructure only, like attn_ref_cpu.py): the exact answers, the first-order per-element error bounds of the rounding
points the kernel header declares, the attention inputs with known answers, and the reader of the recorded fixture
tests/golden/clip_text.npz (tools/make_clip_text_golden.py writes it).

Rounding points (salun_clip_text.hip header), all fp32, U = 2^-24:
  embed       one add.
  LayerNorm   sum in at most ADDS(W) additions per path, mean = sum / W, d = x - mean, q = sum d * d (same order),
              var = q / W, r = 1 / sqrt(var + eps) (IEEE sqrt and division), y = ((d * r) * gamma) + beta.
  attention   s = (fma chain over d = 0..63) * scale, e = expf(s - m) or exactly 0 above the diagonal, l = sum e in
              <= 4 (qi + 1) + 1 additions, acc = fma chain over the 16 (qi + 1) keys of the visited tiles, o = acc / l.
  quick-GELU  t = 1.702f * x, e = expf(-t), s = 1 / (1 + e), y = x * s.
expf is OCML's: 1 ulp = 2 U (norm_ref_cpu.EXP_ULP["expf"], from the HIP math API reference).
"""
import json
import math
import os

import numpy as np
import torch

from norm_ref_cpu import EXP_ULP

U = 2.0 ** -24
F64 = torch.float64
EXP_U = EXP_ULP["expf"]          # relative error of expf in units of U
SLACK = 1.001                    # second-order terms
D = 64                           # head width of the attention kernel
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_text.npz")


# ------------------------------------------------------------------------------------------------------ exact answers
def embed(ids, tok, pos):
    return tok.to(F64)[ids] + pos.to(F64)[:ids.shape[1]]


def layer_norm(x, gamma, beta, eps):
    x = x.to(F64)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.to(F64) + beta.to(F64)


def quick_gelu(x):
    x = x.to(F64)
    return x / (1.0 + torch.exp(-1.702 * x))


def split_heads(qkv, B, T, H):
    """[B T, 3 H D] -> q, k, v as [B, H, T, D]"""
    q, k, v = qkv.to(F64).view(B, T, 3, H, D).permute(2, 0, 3, 1, 4)
    return q, k, v


def attn_causal(qkv, B, T, H, scale):
    """-> o [B T, H D] and the weights P [B, H, T, T]"""
    q, k, v = split_heads(qkv, B, T, H)
    s = q @ k.transpose(-1, -2) * scale
    s = s.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), 1), -math.inf)
    P = torch.softmax(s, -1)
    return (P @ v).transpose(1, 2).reshape(B * T, H * D), P


def forward(w, cfg, ids):
    """The whole text model in float64 from a {name: tensor} state dict under transformers' names."""
    w = {k: v.to(F64) for k, v in w.items()}
    B, T = ids.shape
    W, H = cfg["width"], cfg["heads"]
    assert W // H == D
    p = "text_model."
    x = embed(ids, w[p + "embeddings.token_embedding.weight"], w[p + "embeddings.position_embedding.weight"]).view(B * T, W)
    for i in range(cfg["layers"]):
        L = f"{p}encoder.layers.{i}."
        lin = lambda t, n: t @ w[L + n + ".weight"].T + w[L + n + ".bias"]
        h = layer_norm(x, w[L + "layer_norm1.weight"], w[L + "layer_norm1.bias"], cfg["eps"])
        qkv = torch.cat([lin(h, "self_attn.q_proj"), lin(h, "self_attn.k_proj"), lin(h, "self_attn.v_proj")], 1)
        x = x + lin(attn_causal(qkv, B, T, H, D ** -0.5)[0], "self_attn.out_proj")
        h = layer_norm(x, w[L + "layer_norm2.weight"], w[L + "layer_norm2.bias"], cfg["eps"])
        x = x + lin(quick_gelu(lin(h, "mlp.fc1")), "mlp.fc2")
    return layer_norm(x, w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"], cfg["eps"]).view(B, T, W)


# ------------------------------------------------------------------------------------------------------ bounds
def ln_adds(W):
    """Additions on any element's path into a row sum: a lane's ceil(W / 256) float4 = 4 ceil(W / 256) elements
    (one addition less than elements, but the first adds to 0: counted), then the 6-step butterfly."""
    return 4 * ((W + 255) // 256) + 6


def ln_bound(x, gamma, beta, eps):
    """|kernel - exact| <= this, per element, for fp32-valued x, gamma, beta."""
    x, g, b = x.to(F64), gamma.to(F64).abs(), beta.to(F64)
    W = x.shape[-1]
    n = ln_adds(W)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    v = var + eps
    r = 1.0 / torch.sqrt(v)
    e_mean = (n + 1) * U * x.abs().mean(-1, keepdim=True)               # the sum's additions + the division
    e_d = e_mean + U * d.abs()                                           # + the subtraction
    dd = d.abs() + e_d
    e_q = (2 * d.abs() * e_d + e_d * e_d).sum(-1, keepdim=True) + (n + 1) * U * (dd * dd).sum(-1, keepdim=True)
    e_var = e_q / W + U * (var + e_q / W)                                # + the division
    e_v = e_var + U * (v + e_var) + U * eps                              # + the addition; eps rounded to fp32
    rel_r = e_v / (2 * v) + 2 * U                                        # sqrt and division
    y = d * r * gamma.to(F64) + b
    e_t = g * r * (e_d + d.abs() * (rel_r + 2 * U))                      # d * r, then * gamma
    return SLACK * (e_t + U * (y.abs() + e_t))                           # + beta


def gelu_bound(x):
    x = x.to(F64)
    t = 1.702 * x
    e = torch.exp(-t)
    frac = torch.where(torch.isinf(e), torch.ones_like(e), e / (1.0 + e))
    rel_s = frac * (EXP_U * U + 2 * U * t.abs()) + 2 * U                # (constant + product) in t, expf; 1 + e; 1 / .
    return SLACK * quick_gelu(x).abs() * (rel_s + U)


def attn_bound(qkv, B, T, H, scale):
    """First-order bound of |o_kernel - o_exact| [B T, H D] (the construction of attn_ref_cpu.bounds, for fp32)."""
    q, k, v = split_heads(qkv, B, T, H)
    o, P = attn_causal(qkv, B, T, H, scale)
    s = q @ k.transpose(-1, -2) * scale
    allowed = ~torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
    m = s.masked_fill(~allowed, -math.inf).max(-1, keepdim=True).values
    # relative error of e_j: the chain (64 roundings on sum |q k|), scale's rounding and product, the subtraction, expf
    rho = scale * 64 * U * (q.abs() @ k.abs().transpose(-1, -2)) + 2 * U * s.abs() + U * (s - m).abs() + EXP_U * U
    rho = torch.where(allowed, rho, torch.zeros_like(rho))
    qi = (torch.arange(T) // 16 + 1).to(F64).view(1, 1, T, 1)
    n_pv, n_l = 16 * qi, 4 * qi + 1
    A = P @ v.abs()                                                      # sum_j p_j |v_jd|
    rbar = (P * rho).sum(-1, keepdim=True)
    b = (P * rho) @ v.abs() + A * (n_pv * U + rbar + n_l * U + U)
    return SLACK * b.transpose(1, 2).reshape(B * T, H * D)


# ------------------------------------------------------------------------------------------------------ known answers
ONEHOT_Q = 1024.0                # query amplitude: one step of a key's amplitude is 1024 / 8 = 128 in the scaled score


def onehot_case(B, H, T, seed=0):
    """qkv [B T, 3 H D] with scaled one-hot q and k and an integer v, and the key each query selects [B, H, T].
    Key j lives in channel class j mod 4 with amplitude j div 4 + 1 in classes 0, 1 (growing: the best key of the class
    is its LAST one, so for a query in the middle the global best lies in the future) and 32 - j div 4 in classes 2, 3
    (shrinking: the best key is the first).  Query t carries 1024 in one class that has a key <= t: a shrinking class
    where t = 2 mod 3 and one exists, else a growing one.  The class-to-channel map differs per (b, h).  Scaled by 1 / 8 the
    selected key leads every other allowed key by >= 128, so expf gives exactly 0 for them and 1 for it."""
    g = torch.Generator().manual_seed(1000 * T + 10 * B * H + seed)
    q = torch.zeros(B, H, T, D, dtype=F64)
    k = torch.zeros(B, H, T, D, dtype=F64)
    v = torch.randint(-4, 5, (B, H, T, D), generator=g).to(F64)
    sel = torch.zeros(B, H, T, dtype=torch.int64)
    for b in range(B):
        for h in range(H):
            chan = [(11 * c + 5 * (b * H + h) + 3) % D for c in range(4)]
            for j in range(T):
                c = j % 4
                k[b, h, j, chan[c]] = (j // 4 + 1) if c < 2 else (32 - j // 4)
            for t in range(T):
                grow, shrink = [c for c in (0, 1) if c <= t], [c for c in (2, 3) if c <= t]
                pool = shrink if (t % 3 == 2 and shrink) else grow
                c = pool[(t // 3) % len(pool)]
                q[b, h, t, chan[c]] = ONEHOT_Q
                same = [j for j in range(t + 1) if j % 4 == c]
                sel[b, h, t] = same[-1] if c < 2 else same[0]
    qkv = torch.stack([q, k, v]).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * H * D)     # [B, T, 3, H, D]
    return qkv, sel


def gaussian_case(B, H, T, seed=0):
    g = torch.Generator().manual_seed(77 * T + B * H + seed)
    return torch.randn(B * T, 3 * H * D, generator=g, dtype=torch.float32).to(F64)


# ------------------------------------------------------------------------------------------------------ the fixture
def load_golden():
    z = np.load(GOLDEN)
    out = {"vocab": json.loads(str(z["vocab_json"])), "merges": str(z["merges_txt"]),
           "prompts": json.loads(str(z["prompts_json"])), "ids": torch.from_numpy(z["ids"]),
           "config": json.loads(str(z["config_json"])), "model_prompts": z["model_prompts"].tolist(),
           "hidden": torch.from_numpy(z["hidden"]), "yardstick": float(z["yardstick"]),
           "weights": {k[3:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith("w::")}}
    return out


def write_vocab(golden, folder):
    """The fixture's vocabulary as the two files the tokenizer reads."""
    with open(os.path.join(folder, "vocab.json"), "w", encoding="utf-8") as f:
        json.dump(golden["vocab"], f, ensure_ascii=False)
    with open(os.path.join(folder, "merges.txt"), "w", encoding="utf-8") as f:
        f.write(golden["merges"])
    return folder
