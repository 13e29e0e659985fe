"""K29 (csrc/salun_clip_text.hip) and the text encoder built on it (SD/clip_text.py: TextPlan) on the device, against
the float64 model of clip_text_ref_cpu.py and the recorded fixture tests/golden/clip_text.npz.

  * embed: bit-equal to tok[ids] + pos.
  * causal attention, exact answers: scaled one-hot q / k and an integer v (clip_text_ref_cpu.onehot_case) — the weights
    are exactly one-hot, so o[t] is one row of v bit for bit; for more than half of the queries the best key overall lies
    in the future.  Every operand sits in a guarded arena: all around the [B T, 3 W] operand is NaN, the output is
    surrounded by sentinels.  (A padding column j >= T that took part with a zero key would score 0, 128 below the
    selected key, and vanish: what these inputs catch of the padding is a read past row T — it meets NaN.)
  * causal attention, LayerNorm, quick-GELU on Gaussian inputs: every element within the first-order bound of the
    rounding points the kernel header declares; the largest error / bound ratio per case is logged (with
    SALUN_MEASURED_DIR set, appended to clip_text_bounds_measured.txt there; profiles/ has the last recording).
  * the network: TextPlan within DEVICE_FACTOR x the fp32-CPU yardstick of the float64 hidden states, on the fixture's
    tiny model and on a seeded model with the v1 layer shape; causality end to end; the command lines.
"""
import csv
import ctypes
import importlib.util
import json
import os
import sys

import pytest
import torch

import clip_text_ref_cpu as R
import fixtures
from guarded_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
DEVICE_FACTOR = 8
F64 = torch.float64
c_int64, c_double = ctypes.c_int64, ctypes.c_double


def L():
    from unlearn_saliency_amd import _lib
    return _lib.lib()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")
    if d and os.path.isdir(d):
        with open(os.path.join(d, "clip_text_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


def check_bound(name, got, want, bound):
    err = (got.to(F64) - want).abs()
    assert bool(torch.isfinite(got).all()), name
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                              torch.zeros_like(err)))
    log(f"{name}: err/bound {float(ratio.max()):.4f} max err {float(err.max()):.3e}")
    assert bool((err <= bound).all()), (name, float(ratio.max()))


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.fixture(scope="module")
def vocab_dir(golden, tmp_path_factory):
    return R.write_vocab(golden, str(tmp_path_factory.mktemp("clip_vocab")))


# ------------------------------------------------------------------------------------------------------ embed
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("W", [128, 768])
def test_embed_is_bit_equal(B, W):
    V, T = 1000, 77
    g = torch.Generator().manual_seed(B * 1000 + W)
    tok, pos = torch.randn(V, W, generator=g), torch.randn(T, W, generator=g)
    ids = torch.randint(0, V, (B, T), generator=g)
    ids[0, 0], ids[-1, -1], ids[0, 1] = 0, V - 1, V - 1
    a = Arena().put("tok", tok).put("pos", pos).put("x", shape=(B, T, W), out=True).upload()
    d_ids = ids.cuda()
    rc = L().salun_clip_embed(ctypes.c_void_p(d_ids.data_ptr()), a.ptr("tok"), a.ptr("pos"), a.ptr("x"), c_int64(B), T, W,
                              c_int64(V), stream())
    assert rc == 0
    got = a.result("x")
    want = tok[ids] + pos
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_embed_wrapper_refuses_a_bad_id_before_the_launch():
    from unlearn_saliency_amd import ops_clip
    tok, pos = torch.zeros(10, 8, device="cuda"), torch.zeros(4, 8, device="cuda")
    with pytest.raises(ValueError, match="10"):
        ops_clip.clip_embed(torch.tensor([[1, 10, 2, 3]]), tok, pos)


# ------------------------------------------------------------------------------------------------------ attention
def run_attn(a, B, H, T, D=64, scale=0.125, t_arg=None):
    W = H * 64
    return L().salun_attn_causal_f32(a.ptr("qkv"), a.ptr("o"), B, H, T if t_arg is None else t_arg, D, c_int64(3 * W), 0, W,
                                     2 * W, c_int64(W), c_double(scale), stream())


@pytest.mark.parametrize("BH", [(1, 1), (2, 3)])
@pytest.mark.parametrize("T", [1, 2, 15, 16, 17, 33, 64, 77])
def test_attention_exact_answers_and_no_leak_from_the_padding(T, BH):
    B, H = BH
    qkv, sel = R.onehot_case(B, H, T)
    _, _, v = R.split_heads(qkv, B, T, H)
    want = torch.gather(v, 2, sel[..., None].expand(-1, -1, -1, R.D)).transpose(1, 2).reshape(B * T, H * R.D).float()
    a = Arena().put("qkv", qkv.float()).put("o", shape=(B * T, H * R.D), out=True).upload()     # NaN all around qkv
    assert run_attn(a, B, H, T) == 0
    got = a.result("o")
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), float((got - want).abs().max())


@pytest.mark.parametrize("B,H,T", [(2, 3, 77), (1, 2, 33), (2, 1, 5)])
def test_attention_within_the_bound_and_deterministic(B, H, T):
    qkv = R.gaussian_case(B, H, T)
    want, _ = R.attn_causal(qkv, B, T, H, 0.125)
    bound = R.attn_bound(qkv, B, T, H, 0.125)
    a = Arena().put("qkv", qkv.float()).put("o", shape=(B * T, H * R.D), out=True).upload()
    assert run_attn(a, B, H, T) == 0
    got = a.result("o").clone()
    check_bound(f"attn_causal B{B} H{H} T{T}", got, want, bound)
    a.restore(o=None)
    assert run_attn(a, B, H, T) == 0
    assert torch.equal(a.result("o").view(torch.int32), got.view(torch.int32))


def test_attention_refuses_what_lies_outside_its_domain():
    from unlearn_saliency_amd import _lib
    B, H, T = 1, 2, 8
    a = Arena().put("qkv", R.gaussian_case(B, H, T).float()).put("o", shape=(B * T, H * R.D), out=True).upload()
    assert run_attn(a, B, H, T, t_arg=_lib.SALUN_CLIP_ATTN_MAX_T + 1) == EINVAL
    assert run_attn(a, B, H, T, D=32) == EINVAL and run_attn(a, B, H, T, D=128) == EINVAL
    assert run_attn(a, B, H, T, t_arg=0) == EINVAL
    assert bool((a.result("o").view(torch.int32) == SENTINEL).all())
    assert _lib.SALUN_CLIP_ATTN_MAX_T >= 77


# ------------------------------------------------------------------------------------------------------ LayerNorm
def ln_rows(rows, W, kind, g):
    x = torch.randn(rows, W, generator=g) * 2.0 + 0.5
    if kind == "equal" or (kind == "mixed" and rows > 2):
        x[0] = 3.25 if kind == "equal" else -117.3
    if kind == "large" or (kind == "mixed" and rows > 2):
        x[rows // 2, W // 3] = 1.0e4
    return x


@pytest.mark.parametrize("W", [128, 768])
@pytest.mark.parametrize("rows,kind", [(1, "gauss"), (1, "equal"), (1, "large"), (77, "mixed"), (154, "mixed")])
def test_layer_norm_within_the_bound(rows, kind, W):
    g = torch.Generator().manual_seed(rows * 7 + W)
    x = ln_rows(rows, W, kind, g)
    gamma, beta, eps = 1.0 + 0.2 * torch.randn(W, generator=g), 0.3 * torch.randn(W, generator=g), 1e-5
    a = Arena().put("x", x).put("gamma", gamma).put("beta", beta).put("y", shape=(rows, W), out=True).upload()
    rc = L().salun_ln_f32_forward(a.ptr("x"), a.ptr("gamma"), a.ptr("beta"), a.ptr("y"), c_int64(rows), W, c_double(eps),
                                  stream())
    assert rc == 0
    check_bound(f"ln_f32 {rows}x{W} {kind}", a.result("y"), R.layer_norm(x, gamma, beta, eps), R.ln_bound(x, gamma, beta, eps))


def test_layer_norm_refuses_a_width_outside_its_domain():
    a = Arena().put("x", torch.zeros(2, 6)).put("gamma", torch.ones(6)).put("beta", torch.zeros(6)) \
        .put("y", shape=(2, 6), out=True).upload()
    for W in (6, 0, 2052):
        assert L().salun_ln_f32_forward(a.ptr("x"), a.ptr("gamma"), a.ptr("beta"), a.ptr("y"), c_int64(2), W,
                                        c_double(1e-5), stream()) == EINVAL
    assert bool((a.result("y").view(torch.int32) == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------ quick-GELU
@pytest.mark.parametrize("n,skew", [(128, 0), (77 * 768, 0), (154 * 768, 0), (1003, 0), (4099, 1)])
def test_quick_gelu_within_the_bound(n, skew):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 3.0
    m = min(n, 81)
    x[:m] = torch.linspace(-40.0, 40.0, m)
    x[m - 1], x[m // 2] = 0.0, -0.0
    a = Arena().put("x", x, out=True, skew=skew).upload()
    assert L().salun_quick_gelu(a.ptr("x"), c_int64(n), stream()) == 0
    got = a.result("x")
    check_bound(f"quick_gelu n={n} skew={skew}", got, R.quick_gelu(x), R.gelu_bound(x))
    zero = x == 0
    assert torch.equal(got[zero].view(torch.int32), x[zero].view(torch.int32))      # +0 -> +0, -0 -> -0


# ------------------------------------------------------------------------------------------------------ the network
def device_model(config, weights):
    from unlearn_saliency_amd.SD.clip_text import ClipTextLite
    m = ClipTextLite(config)
    m.load_state_dict(weights)
    return m.cuda().eval()


def test_plan_on_the_fixtures_model(golden):
    from unlearn_saliency_amd.SD import clip_text
    plan = clip_text.TextPlan(device_model(golden["config"], golden["weights"]))
    ids = golden["ids"][golden["model_prompts"]]
    got = plan.forward(ids).cpu().double()
    err = float((got - golden["hidden"]).abs().max())
    log(f"text_plan fixture: err {err:.3e} yardstick {golden['yardstick']:.3e} ratio {err / golden['yardstick']:.3f}")
    assert err <= DEVICE_FACTOR * golden["yardstick"]
    assert plan.launches == 2 + 8 * golden["config"]["layers"]
    assert all(v == 0 for v in clip_text.LIBRARY_TEXT_CALLS.values()), clip_text.LIBRARY_TEXT_CALLS


def test_plan_on_the_v1_layer_shape(golden, vocab_dir):
    """Width 768, 12 heads, MLP 3072, two layers, vocabulary 1000, seeded; B = 2 with the empty prompt as one row.  The
    float64 answer and the fp32 yardstick are computed on the CPU here."""
    from unlearn_saliency_amd.SD import clip_text
    cfg = dict(vocab_size=1000, width=768, layers=2, heads=12, mlp=3072, positions=77, eps=1e-5)
    torch.manual_seed(29)
    cpu = clip_text.ClipTextLite(cfg).eval()
    with torch.no_grad():
        for n, p in cpu.named_parameters():                  # the default initialisation leaves the scores flat
            if "embedding" in n:
                p.copy_(torch.randn_like(p) * (1.0 if "token" in n else 0.5))
            elif p.dim() == 2:
                p.copy_(torch.randn_like(p) * (1.5 if "q_proj" in n or "k_proj" in n else 1.0) / p.shape[1] ** 0.5)
            elif "layer_norm" not in n:
                p.copy_(torch.randn_like(p) * 0.1)
    tok = clip_text.ClipTokenizerLite(vocab_dir)
    ids = tok.encode(["", "the image of a chain and 10 things!!!"])
    assert ids.shape == (2, 77) and int(ids.max()) < 1000
    weights = {k: v.clone() for k, v in cpu.state_dict().items()}
    with torch.no_grad():
        want = R.forward(weights, cfg, ids)
        yard = float((cpu(ids).double() - want).abs().max())
    plan = clip_text.TextPlan(device_model(cfg, weights))
    got = plan.encode(["", "the image of a chain and 10 things!!!"], tok).cpu().double()
    err = float((got - want).abs().max())
    log(f"text_plan v1-shape: err {err:.3e} yardstick {yard:.3e} ratio {err / yard:.3f}")
    assert err <= DEVICE_FACTOR * yard
    assert all(v == 0 for v in clip_text.LIBRARY_TEXT_CALLS.values())


def test_causality_end_to_end(golden):
    from unlearn_saliency_amd.SD import clip_text
    plan = clip_text.TextPlan(device_model(golden["config"], golden["weights"]))
    ids = golden["ids"][golden["model_prompts"]][:2].clone()
    base = plan.forward(ids).cpu()
    for p in (1, 16, 40, 76):
        other = ids.clone()
        other[:, p:] = (other[:, p:] + 7) % golden["config"]["vocab_size"]
        got = plan.forward(other).cpu()
        assert torch.equal(got[:, :p].view(torch.int32), base[:, :p].view(torch.int32)), p
        assert not torch.equal(got[:, p:], base[:, p:])


def test_cond_stage_feeds_latent_diffusion_lite(golden, vocab_dir):
    from unlearn_saliency_amd.SD import clip_text
    from unlearn_saliency_amd.SD.ldm_lite import LatentDiffusionLite
    cfg = dict(golden["config"], width=64, heads=1, mlp=128)
    torch.manual_seed(3)
    plan = clip_text.TextPlan(clip_text.ClipTextLite(cfg).cuda().eval())
    tok = clip_text.ClipTokenizerLite(vocab_dir)
    ucfg = dict(fixtures.sd_tiny_config(), context_dim=64)
    model = LatentDiffusionLite(ucfg, first_stage=lambda x: x[:, :1].repeat(1, 4, 1, 1), cond_stage=plan.cond_stage(tok)).cuda()
    z, c = model.get_input({"jpg": torch.zeros(2, 8, 8, 3, device="cuda"), "txt": ["a chain", ""]})
    assert tuple(c.shape) == (2, 77, 64) and c.is_cuda and bool(torch.isfinite(c).all())
    assert torch.equal(c, plan.encode(["a chain", ""], tok))


# ------------------------------------------------------------------------------------------------------ command lines
def _script(name, sub):
    folder = os.path.join(ROOT, "unlearn_saliency_amd", "SD", sub)
    if folder not in sys.path:
        sys.path.insert(0, folder)
    spec = importlib.util.spec_from_file_location("sd_cli_" + name.replace("-", "_").replace(".py", ""),
                                                  os.path.join(folder, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ROWS = [(3, "Image of tench", 11), (7, "Image of chain saw", 12)]
# test_generate_images_gpu.py's decoder: the first stage's factor of 8, 4 x 4 latents -> 32 x 32 images
DDCONFIG = dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 1, 2, 2),
                num_res_blocks=1, attn_resolutions=(), dropout=0.0)


def prompts_csv(tmp_path):
    path = tmp_path / "prompts.csv"
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["", "case_number", "prompt", "evaluation_seed", "class"])
        for i, (case, prompt, seed) in enumerate(ROWS):
            w.writerow([i, case, prompt, seed, "x"])
    return str(path)


def test_encode_prompts_synthetic_writes_the_contexts_file(tmp_path, vocab_dir):
    from unlearn_saliency_amd.SD import clip_text
    mod = _script("encode_prompts.py", "train-scripts")
    out = tmp_path / "ctx.pt"
    mod.main(["--prompts_path", prompts_csv(tmp_path), "--prompt", "Van Gogh, the chain", "--tokenizer", vocab_dir,
              "--out", str(out), "--synthetic", "--width", "128", "--batch_size", "4"])
    ctx = torch.load(out, weights_only=False)
    assert list(ctx) == ["", "Image of tench", "Image of chain saw", "Van Gogh, the chain", "Van Gogh", "the chain"]
    for p, c in ctx.items():
        assert tuple(c.shape) == (1, 77, 128) and c.dtype == torch.float32 and bool(torch.isfinite(c).all()), p
    assert not torch.equal(ctx[""], ctx["Van Gogh"])
    assert torch.equal(ctx[""][0, 0], ctx["Van Gogh"][0, 0])          # BOS sees only itself
    assert all(v == 0 for v in clip_text.LIBRARY_TEXT_CALLS.values())


def test_generate_images_synthetic_with_a_tokenizer(tmp_path, vocab_dir):
    """The configuration of test_generate_images_gpu.py with the context width raised from 24 to 64, the narrowest the
    text encoder's 64-wide heads allow."""
    from unlearn_saliency_amd.SD import clip_text
    g = _script("generate-images.py", "eval-scripts")
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in dict(fixtures.sd_tiny_config(), context_dim=64).items()}
    dd = {k: (list(v) if isinstance(v, tuple) else v) for k, v in DDCONFIG.items()}
    argv = ["--model_name", "tiny", "--prompts_path", prompts_csv(tmp_path), "--save_path", str(tmp_path / "a"),
            "--synthetic", "--unet_config", json.dumps(cfg), "--ddconfig", json.dumps(dd), "--num_samples", "2",
            "--rounds", "1", "--ddim_steps", "3", "--image_size", "32", "--tokenizer", vocab_dir]
    written = g.main(argv)
    want = sorted(f"{case}_{num}.png" for case, _, _ in ROWS for num in range(2))
    assert sorted(os.listdir(tmp_path / "a" / "tiny")) == want and len(written) == len(want)
    assert all(v == 0 for v in clip_text.LIBRARY_TEXT_CALLS.values())
