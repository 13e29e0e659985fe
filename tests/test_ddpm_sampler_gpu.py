"""DDPM sampling on the DEVICE (K19, csrc/salun_sampler.hip; DDPM/sample.py): the fused reverse step against the tensor-op
loop it replaces and against the reference's recorded trajectories (`ddpm_f4.npz`), its index-keyed noise, the uint8
image kernel against the torch expression sequence of `inverse_data_transform` + `save_image(normalize=True)`, and the
sampling modes end to end on the reduced U-Net."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fixtures import ddpm_small_config, fill_params
from test_f4_vs_golden import StubEps, _ReplayRandn
from unlearn_saliency_amd import ops, ops_sampler, rng
from unlearn_saliency_amd.DDPM.functions import denoising as DN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
EPS32 = 2.0 ** -24


def _normal(shape, seed):
    return torch.from_numpy(rng.normal(int(np.prod(shape)), seed).reshape(shape)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------- one step vs `_loop`
# (i, j) of the step under test: the first step of the golden's sequence, a middle one, and the last (i == 0, j == -1)
STEPS = {"first": (875, 750), "middle": (375, 250), "last": (0, -1)}


@pytest.mark.parametrize("shape", [(3, 3, 16, 16), (2, 3, 5, 5)], ids=["vec3blocks", "odd75"])
@pytest.mark.parametrize("where", list(STEPS))
@pytest.mark.parametrize("cond_scale", [0.0, 2.0])
@pytest.mark.parametrize("variant,eta", [("ddpm_noisy", 0.0), ("generalized", 0.0), ("generalized", 1.0)])
def test_step_with_explicit_noise_matches_the_tensor_op_loop(variant, eta, cond_scale, where, shape):
    """`salun_sampler_step` with an explicit noise tensor against `denoising._loop` on the same inputs.  (2,3,5,5) has
    75 floats per image — no multiple of the 4-float vector — and takes the scalar path; (3,3,16,16) is 576 vectors,
    three workgroups.  The kernel does `_loop`'s operations in `_loop`'s order in fp32 without contraction, and sqrt
    and division are correctly rounded on both sides, so only exp / log of the ancestral sigma can differ, by an ulp
    or two.  Bound: 8 roundings of 2^-24 relative to the largest intermediate M = (max|x| + max|e|) / sqrt(abar_t) +
    max|z| + max|e| (x0's terms before they cancel; every later coefficient is <= 1)."""
    i, j = STEPS[where]
    betas = torch.linspace(1e-4, 0.02, 1000).to(DEV)
    x, ec, en, z = (_normal(shape, 100 + k) for k in range(4))
    guided = cond_scale != 0
    e = ((1 + cond_scale) * ec - cond_scale * en) if guided else ec
    seq = [i] if j < 0 else [j, i]
    with _ReplayRandn([z.cpu().numpy()] * len(seq)):
        xs, x0s = DN._loop(x, seq, lambda xt, t: e, betas, variant == "ddpm_noisy", eta, "all")
    want, want0 = xs[1].to(DEV), x0s[0].to(DEV)
    abar = DN.alpha_bar_table(betas)
    got0 = torch.empty_like(x)
    got = ops_sampler.sampler_step(x, ec, en if guided else None, cond_scale, abar, i + 1, j + 1,
                                   ops_sampler.VARIANTS[variant], eta, noise=z, x0=got0)
    M = float((x.abs().max() + e.abs().max()) / abar[i + 1].sqrt() + z.abs().max() + e.abs().max())
    d, d0 = float((got - want).abs().max()), float((got0 - want0).abs().max())
    print(f"{variant} eta={eta} s={cond_scale} {where} {shape}: x_next {d:.2e}, x0 {d0:.2e}, bound {8 * EPS32 * M:.2e}")
    assert torch.isfinite(got).all() and d <= 8 * EPS32 * M and d0 <= 8 * EPS32 * M, (d, d0, M)
    # in place: x_next written over x_t gives the same bits
    xi = x.clone()
    ops_sampler.sampler_step(xi, ec, en if guided else None, cond_scale, abar, i + 1, j + 1,
                             ops_sampler.VARIANTS[variant], eta, noise=z, out=xi)
    assert torch.equal(_bits(xi), _bits(got))


def test_step_rejects_bad_arguments():
    from unlearn_saliency_amd._lib import SalunError
    x = _normal((2, 3, 4, 4), 1)
    abar = DN.alpha_bar_table(torch.linspace(1e-4, 0.02, 10).to(DEV))
    with pytest.raises(SalunError):  # table index out of range
        ops_sampler.sampler_step(x, x, None, 0.0, abar, 11, 3, ops_sampler.ANCESTRAL, noise=x)
    with pytest.raises(SalunError):  # a noisy step with neither a noise tensor nor image ids
        ops_sampler.sampler_step(x, x, None, 0.0, abar, 5, 4, ops_sampler.ANCESTRAL)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops_sampler.sampler_step(x.cpu(), x, None, 0.0, abar, 5, 4, ops_sampler.ANCESTRAL, noise=x)


# ----------------------------------------------------------------------- a whole trajectory vs the reference's record
class StubPair(StubEps):
    """The golden generator's eps model split into the pair whose guidance combine gives its output back:
    stub(x, t, c, s) = base + 0.01 c s = (1 + s) (base + 0.01 c s / (1 + s)) - s base."""

    def __init__(self, cond_scale):
        super().__init__()
        self.k = cond_scale / (1.0 + cond_scale)

    def eps_pair(self, x, t, c, null=True):
        base = self.forward(x, t)
        if c is None:
            return base, None
        return base + 0.01 * c.view(-1, 1, 1, 1).float() * self.k, (base if null else None)


@pytest.mark.parametrize("name,variant,eta,cond_scale", [("ddim_cond", "generalized", 0.3, 2.0),
                                                         ("ddpm_cond", "ddpm_noisy", 0.0, 2.0),
                                                         ("ddim_eta", "generalized", 0.7, 0.0),
                                                         ("ddpm", "ddpm_noisy", 0.0, 0.0)])
def test_fused_trajectory_matches_the_reference_record(golden_dir, name, variant, eta, cond_scale):
    """`fused_steps_conditional` over the golden's 8-step sequence with the golden's recorded noise, against the states
    and x0 estimates the reference's samplers produced.  Tolerance: the one `test_f4_gpu.py` applies to this golden
    (1e-5 of the trajectory's scale), unchanged."""
    g = np.load(os.path.join(golden_dir, "ddpm_f4.npz"))
    x = torch.from_numpy(g["x"]).to(DEV)
    seq = [int(v) for v in g["seq"]]
    betas = torch.linspace(1e-4, 0.02, 1000).to(DEV)
    c = torch.tensor([1, 5, 9], device=DEV) if cond_scale else None
    noise = [torch.from_numpy(z).to(DEV) for z in g[name + "_randn"]]
    x_before = x.clone()
    xs, x0s = DN.fused_steps_conditional(x, c, None, seq, StubPair(cond_scale).to(DEV), betas, cond_scale, variant, eta,
                                         seed=0, noise=noise, keep="all")
    assert len(xs) == len(seq) + 1 and len(x0s) == len(seq) and torch.equal(x, x_before)
    scale = max(float(np.abs(b).max()) for b in g[name + "_xs"])
    e1 = max(float(np.abs(a.cpu().numpy() - b).max()) for a, b in zip(xs, g[name + "_xs"])) / scale
    s0 = max(float(np.abs(b).max()) for b in g[name + "_x0"])
    e0 = max(float(np.abs(a.cpu().numpy() - b).max()) for a, b in zip(x0s, g[name + "_x0"])) / s0
    print(f"{name}: fused trajectory vs the reference's: x_t {e1:.2e}, x_0 prediction {e0:.2e} of scale")
    assert e1 <= 1e-5 and e0 <= 1e-5, (e1, e0)
    last, last0 = DN.fused_steps_conditional(x, c, None, seq, StubPair(cond_scale).to(DEV), betas, cond_scale, variant,
                                             eta, seed=0, noise=noise)  # keep="last": in place after the first step
    assert torch.equal(_bits(last[0]), _bits(xs[-1])) and torch.equal(_bits(last0[0]), _bits(x0s[-1]))
    assert torch.equal(x, x_before)


# ------------------------------------------------------------------------------------------------ index-keyed noise
@pytest.mark.parametrize("shape", [(3, 8, 8), (3, 5, 5)])
def test_keyed_noise_is_fill_normal_on_the_same_key(shape):
    ids = torch.tensor([7, 0, 123456789012, 7], dtype=torch.int64, device=DEV)
    chw = int(np.prod(shape))
    for step in (0, 3):
        z = ops_sampler.sampler_noise(ids, shape, seed=1234, step=step)
        for b, i in enumerate(ids.tolist()):
            want = ops.fill_normal(chw, ops_sampler.sampler_key(1234, step, i))
            assert torch.equal(_bits(z[b].reshape(-1)), _bits(want)), (step, i)
    assert not torch.equal(ops_sampler.sampler_noise(ids, shape, 1234, 0), ops_sampler.sampler_noise(ids, shape, 1234, 1))
    assert not torch.equal(ops_sampler.sampler_noise(ids, shape, 1234, 0), ops_sampler.sampler_noise(ids, shape, 1235, 0))


@pytest.mark.parametrize("shape", [(5, 3, 8, 8), (5, 3, 5, 5)])
@pytest.mark.parametrize("variant,eta", [("ddpm_noisy", 0.0), ("generalized", 1.0)])
def test_counter_mode_draws_by_image_id(variant, eta, shape):
    """The step's own draw equals the regenerated keyed noise bit for bit, two launches agree bit for bit, and permuting
    the rows together with `image_ids` permutes the output rows."""
    betas = torch.linspace(1e-4, 0.02, 1000).to(DEV)
    abar = DN.alpha_bar_table(betas)
    x, ec, en = (_normal(shape, 200 + k) for k in range(3))
    ids = torch.tensor([11, 3, 40, 41, 2 ** 40 + 5], dtype=torch.int64, device=DEV)
    kind = ops_sampler.VARIANTS[variant]
    run = lambda x_, ec_, en_, ids_, **kw: ops_sampler.sampler_step(x_, ec_, en_, 2.0, abar, 501, 376, kind, eta,
                                                                    seed=99, image_ids=ids_, step=4, **kw)
    a = run(x, ec, en, ids)
    z = ops_sampler.sampler_noise(ids, shape[1:], seed=99, step=4)
    assert torch.equal(_bits(a), _bits(run(x, ec, en, None, noise=z)))  # drawn in the kernel == read from memory
    assert torch.equal(_bits(a), _bits(run(x, ec, en, ids)))
    assert not torch.equal(a, run(x, ec, en, ids + 1))
    perm = torch.tensor([3, 0, 4, 2, 1], device=DEV)
    b = run(x[perm].contiguous(), ec[perm].contiguous(), en[perm].contiguous(), ids[perm].contiguous())
    assert torch.equal(_bits(b), _bits(a[perm]))


# --------------------------------------------------------------------------------------------------- float -> uint8
def _u8_inputs(shape, seed, lo, hi):
    """Images whose normalised values (v - lo) / (hi - lo) * 255 + 0.5 lie at least 0.1 from an integer: v = lo +
    (k + u) / 255 * (hi - lo), k an integer level, |u| <= 0.4, with the levels 0 and 255 present in every image."""
    n = int(np.prod(shape))
    k = np.floor(rng.uniform(n, seed, 0.0, 256.0)).clip(0, 255).astype(np.float64).reshape(shape[0], -1)
    u = rng.uniform(n, seed + 1, -0.4, 0.4).astype(np.float64).reshape(shape[0], -1)
    k[:, 0], u[:, 0], k[:, -1], u[:, -1] = 0.0, 0.0, 255.0, 0.0
    u = np.where(k == 0, np.abs(u), np.where(k == 255, -np.abs(u), u))
    v = lo + (k + u) / 255.0 * (hi - lo)
    return torch.from_numpy((2.0 * v - 1.0).astype(np.float32).reshape(shape))


def _u8_reference(x, lohi=None, off_boundary=True):
    """The torch expression sequence on the host: datasets.inverse_data_transform (rescaled), then torchvision's
    norm_ip / save_image arithmetic, per image or with one range."""
    v = torch.clamp((x + 1.0) / 2.0, 0.0, 1.0)
    out = []
    for img in v:
        lo, hi = (float(img.min()), float(img.max())) if lohi is None else lohi
        t = img.clone().clamp_(min=lo, max=hi).sub_(lo).div_(max(hi - lo, 1e-5))
        q = t.mul(255).add_(0.5).clamp_(0, 255)
        frac = (q.double() - q.double().floor())
        inside = q < 255  # (the maximum itself lands on 255.5 and is clamped)
        assert not off_boundary or ((frac[inside] >= 1e-3) & (frac[inside] <= 1 - 1e-3)).all(), \
            "an input sits on a rounding boundary"
        out.append(q.permute(1, 2, 0).to(torch.uint8))
    return torch.stack(out)


@pytest.mark.parametrize("shape", [(3, 3, 8, 8), (2, 3, 5, 5), (4, 1, 7, 9), (2, 3, 32, 32)])
def test_images_to_u8_per_image_matches_the_torch_sequence(shape):
    x = _u8_inputs(shape, 300, 0.125, 0.875)
    x[0] = _u8_inputs((1,) + shape[1:], 310, 0.0, 1.0)[0]
    x[0].view(-1)[1:3] = torch.tensor([-1.75, 2.5])  # outside the model's range: the first clamp
    got = ops_sampler.images_to_u8(x.to(DEV)).cpu()
    want = _u8_reference(x)
    assert got.shape == want.shape == (shape[0], shape[2], shape[3], shape[1]) and got.dtype == torch.uint8
    assert int(want.min()) == 0 and int(want.max()) == 255
    assert torch.equal(got, want), int((got.int() - want.int()).abs().max())


def test_images_to_u8_constant_images_use_the_floor():
    """hi - lo below 1e-5: the denominator is the floor 1e-5, not the image's own range."""
    x = torch.zeros(3, 3, 4, 4)
    x[0] += 0.25                     # constant: every byte 0
    x[1].view(-1)[5] = 2.0 ** -17    # v = 0.5 + 2^-18: (2^-18 / 1e-5) * 255 + 0.5 = 97.77 -> 97
    x[2] -= 3.0                      # constant after the clamp to [0, 1]
    got = ops_sampler.images_to_u8(x.to(DEV)).cpu()
    assert torch.equal(got, _u8_reference(x))
    assert int(got[0].max()) == 0 and int(got[2].max()) == 0 and sorted(set(got[1].reshape(-1).tolist())) == [0, 97]


@pytest.mark.parametrize("shape", [(6, 3, 8, 8), (3, 3, 5, 5)])
def test_images_to_u8_with_a_given_range_matches_the_torch_sequence(shape):
    """The visualization grid: one (lo, hi) over all images, from the fixed-order `salun_minmax`."""
    x = _u8_inputs((1,) + (shape[0] * shape[1],) + shape[2:], 400, 0.0625, 0.9375).reshape(shape)
    lohi = ops_sampler.minmax(x.to(DEV))
    assert torch.equal(lohi.cpu(), torch.stack([x.min(), x.max()]))
    v = torch.clamp((x + 1.0) / 2.0, 0.0, 1.0)
    got = ops_sampler.images_to_u8(x.to(DEV), value_range=lohi).cpu()
    want = _u8_reference(x, (float(v.min()), float(v.max())))
    per_image = _u8_reference(x, off_boundary=False)
    assert not torch.equal(want, per_image)  # the images' own ranges differ from the grid's
    assert torch.equal(got, want), int((got.int() - want.int()).abs().max())


@pytest.mark.parametrize("n", [1, 5, 1023, 4099, 300_001])
def test_minmax_matches_torch(n):
    x = _normal((n,), 500 + n)
    for t in (x, x[1:] if n > 1 else x):  # the second view starts one float in: not 16-byte aligned
        assert torch.equal(ops_sampler.minmax(t).cpu(), torch.stack([t.min(), t.max()]).cpu())


# --------------------------------------------------------------------------------------------- the modes, end to end
def _runner(tmp, bs, **over):
    from unlearn_saliency_amd.DDPM.runners.diffusion import Diffusion
    config = ddpm_small_config()
    config.sampling.batch_size = bs
    args = SimpleNamespace(ckpt_folder=str(tmp), synthetic=False, seed=1234, sample_type="generalized",
                           skip_type="uniform", timesteps=4, eta=1.0, cond_scale=2.0, classes_to_generate="1,4",
                           n_samples_per_class=5, mode="sample_classes")
    args.__dict__.update(over)
    return Diffusion(args, config)


def _write_checkpoint(folder, prefix):
    """ckpts/ckpt.pth = [model_state, ...] of the reduced U-Net, keys with or without the DataParallel prefix."""
    from unlearn_saliency_amd.DDPM.models.diffusion import Conditional_Model
    from unlearn_saliency_amd.DDPM.runners.diffusion import add_prefix
    state = fill_params(Conditional_Model(ddpm_small_config()), 7000).state_dict()
    os.makedirs(os.path.join(folder, "ckpts"), exist_ok=True)
    torch.save([add_prefix(state) if prefix else state, None, 0], os.path.join(folder, "ckpts", "ckpt.pth"))


def _read_tree(root):
    from PIL import Image
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".png"):
                out[os.path.relpath(os.path.join(d, f), root)] = np.asarray(Image.open(os.path.join(d, f))).astype(np.int32)
    return out


def test_sample_classes_does_not_depend_on_the_batch_size(tmp_path):
    """`--mode sample_classes`, 5 images per class, `sampling.batch_size` 4 (rounds of 4 + 1) and 3 (3 + 2): same tree
    `class_samples/<class>/<id>.png` with contiguous ids, and the same images.  The start noise and every step's noise
    are functions of (seed, image id) alone — asserted bit for bit on the start noise — but the decoded images are
    compared within 1/255 per channel, not for equality: the U-Net's convolution and GEMM kernels choose their tiling
    (and with it the summation order) by the batch size, so eps differs in the last bits between a round of 4 and a
    round of 3, and a last-bit difference can move a normalised pixel across a rounding boundary."""
    trees = []
    for bs, prefix in ((4, True), (3, False)):
        folder = tmp_path / f"bs{bs}"
        _write_checkpoint(str(folder), prefix)
        r = _runner(folder, bs)
        r.sample()
        root = folder / "class_samples"
        assert sorted(os.listdir(root)) == ["1", "4"]
        assert sorted(os.listdir(root / "1"), key=lambda f: int(f[:-4])) == [f"{i}.png" for i in range(0, 5)]
        assert sorted(os.listdir(root / "4"), key=lambda f: int(f[:-4])) == [f"{i}.png" for i in range(5, 10)]
        trees.append(_read_tree(str(root)))
    a, b = trees
    assert set(a) == set(b) and len(a) == 10
    for k in a:
        assert a[k].shape == (16, 16, 3) and a[k].min() == 0 and a[k].max() == 255  # normalised per image
        assert np.abs(a[k] - b[k]).max() <= 1, k
    assert len({v.tobytes() for v in a.values()}) == 10  # ten different images
    ids4 = torch.tensor([0, 1, 2, 3], dtype=torch.int64, device=DEV)
    ids3 = torch.tensor([3, 4, 5], dtype=torch.int64, device=DEV)
    z4, z3 = ops_sampler.sampler_noise(ids4, (3, 16, 16), 1234), ops_sampler.sampler_noise(ids3, (3, 16, 16), 1234)
    assert torch.equal(_bits(z4[3]), _bits(z3[0]))  # image 3: last of a round of 4, first of a round of 3


def test_sample_fid_with_an_excluded_class(tmp_path):
    _write_checkpoint(str(tmp_path), True)
    r = _runner(tmp_path, 4, mode="sample_fid", classes_to_generate="x3", n_samples_per_class=1, timesteps=2)
    r.sample()
    folder = tmp_path / "fid_samples_guidance_2.0_excluded_class_3"
    assert folder.is_dir()
    assert sorted(os.listdir(folder), key=lambda f: int(f[:-4])) == [f"{i}.png" for i in range(9)]
    assert all(v.shape == (16, 16, 3) for v in _read_tree(str(folder)).values())


def test_visualization_writes_one_grid(tmp_path):
    _write_checkpoint(str(tmp_path), True)
    r = _runner(tmp_path, 8, mode="visualization", timesteps=2, cond_scale=1.5)
    r.config.training.visualization_samples = 20  # 10 classes x 2, in 20 // 8 = 2 rounds of 10
    r.sample()
    tree = _read_tree(str(tmp_path))
    assert list(tree) == ["sample-1.5.png"]
    grid = tree["sample-1.5.png"]
    assert grid.shape == (10 * 16, 2 * 16, 3)  # one row per class, k = 2 tiles per row, no padding
    assert grid.min() == 0 and grid.max() == 255
    # tile (row r, column k) is image 2 r + k of class r, normalised over the range of ALL twenty images: the same rounds
    # again (ids 0..9 and 10..19, labels by row), one min / max over their concatenation.  (Within 1/255: see above.)
    model, _ = r.load_ema_model()
    with torch.no_grad():
        x = torch.cat([r._sample_round(model, list(range(lo, lo + 10)), [i // 2 for i in range(lo, lo + 10)], 1.5)
                       for lo in (0, 10)])
    want = ops_sampler.images_to_u8(x, value_range=ops_sampler.minmax(x)).cpu().numpy().astype(np.int32)
    tiles = grid.reshape(10, 16, 2, 16, 3).transpose(0, 2, 1, 3, 4).reshape(20, 16, 16, 3)
    assert np.abs(tiles - want).max() <= 1


def test_default_sample_image_path_is_the_tensor_op_loop():
    """`sample_image` without `fused` still runs `ddpm_step_conditional` / `generalized_steps_conditional` on torch's
    generator: the same tensor as calling them directly under the same torch seed."""
    from unlearn_saliency_amd.DDPM.runners.diffusion import Diffusion
    r = Diffusion.__new__(Diffusion)
    r.num_timesteps = 1000
    r.betas = torch.linspace(1e-4, 0.02, 1000, device=DEV)
    x = _normal((2, 3, 8, 8), 31)
    c = torch.tensor([2, 7], device=DEV)
    model = StubEps().to(DEV)
    r.args = SimpleNamespace(sample_type="ddpm_noisy", skip_type="quad", timesteps=6, eta=0.0, seed=1234)
    torch.manual_seed(5)
    out = r.sample_image(x, model, c, 1.5)
    seq = [int(s) for s in list(np.linspace(0, np.sqrt(800.0), 6) ** 2)]
    torch.manual_seed(5)
    ref, _ = DN.ddpm_step_conditional(x, c, seq, model, r.betas, 1.5)
    assert torch.equal(_bits(out), _bits(ref[-1].to(DEV)))
    r.args = SimpleNamespace(sample_type="generalized", skip_type="uniform", timesteps=8, eta=1.0, seed=1234)
    torch.manual_seed(6)
    out = r.sample_image(x, model, c, 2.0)
    torch.manual_seed(6)
    ref, _ = DN.generalized_steps_conditional(x, c, range(0, 1000, 125), model, r.betas, 2.0, eta=1.0)
    assert torch.equal(_bits(out), _bits(ref[-1].to(DEV)))
    with pytest.raises(ValueError, match="image ids"):
        r.sample_image(x, model, c, 2.0, fused=True)
