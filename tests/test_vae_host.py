"""The host side of the first-stage encoder (SD/autoencoder.py, SD/images.py, SD/train-scripts/encode_images.py):
module tree and checkpoint loading against the reference-run golden, the image transform against Pillow called
directly, the manifest and the command line.  No GPU."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import vae_fixture as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    d = os.path.join(ROOT, "unlearn_saliency_amd", "SD", "train-scripts")
    if d not in sys.path:
        sys.path.insert(0, d)
    spec = importlib.util.spec_from_file_location("sd_cli_" + name.replace("-", "_"), os.path.join(d, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


# ------------------------------------------------------------------------------------------ module tree
def test_state_dict_keys_and_shapes_are_the_reference_encoder_side():
    from unlearn_saliency_amd.SD.autoencoder import V1_DDCONFIG, AutoencoderKLLite
    g = X.golden()
    assert _shapes(AutoencoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM)) == X.unpack_keys(g["tiny_keys"], g["tiny_shapes"])
    assert V1_DDCONFIG == X.V1_DDCONFIG
    v1 = _shapes(AutoencoderKLLite())
    assert v1 == X.unpack_keys(g["v1_keys"], g["v1_shapes"])
    assert len(g["tiny_keys"]) == 64 and v1["encoder.conv_in.weight"] == (128, 3, 3, 3) and v1["quant_conv.weight"] == (8, 8, 1, 1)
    assert all(k.startswith(("encoder.", "quant_conv.")) for k in v1)


def test_library_forward_equals_the_reference_run():
    """Our module tree on library ops, in float64 and in fp32, against what the reference's Encoder computed."""
    from unlearn_saliency_amd.SD.autoencoder import AutoencoderKLLite
    g = X.golden()
    m = X.load_filled(AutoencoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM))
    x = torch.from_numpy(g["x"])
    assert np.array_equal(X.tiny_input(), g["x"])
    with torch.no_grad():
        y32 = m(x)
        y64 = m.double()(x.double())
    err64 = float((y64 - torch.from_numpy(g["moments64"])).abs().max())
    ref32 = float(np.abs(g["moments32"].astype(np.float64) - g["moments64"]).max())
    assert err64 <= 1e-12 * float(np.abs(g["moments64"]).max())
    assert float((y32.double() - torch.from_numpy(g["moments64"])).abs().max()) <= X.DEVICE_FACTOR * ref32
    assert np.array_equal(g["mode64"], g["moments64"][:, :4])                  # mode() is the mean half


def test_load_compvis():
    from unlearn_saliency_amd.SD.autoencoder import AutoencoderKLLite
    src = X.load_filled(AutoencoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM))
    sd = src.state_dict()
    ckpt = {"state_dict": {"first_stage_model." + k: v.clone() for k, v in sd.items()}}
    ckpt["state_dict"].update({"first_stage_model.decoder.conv_in.weight": torch.zeros(3),
                               "first_stage_model.post_quant_conv.weight": torch.zeros(3),
                               "first_stage_model.loss.logvar": torch.zeros(()),
                               "first_stage_model.model_ema.decay": torch.zeros(()),
                               "model.diffusion_model.out.2.bias": torch.zeros(4),
                               "cond_stage_model.transformer.x": torch.zeros(1)})
    dst = AutoencoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM).load_compvis(ckpt)
    assert all(torch.equal(v, sd[k]) for k, v in dst.state_dict().items())
    bare = dict(sd, **{"decoder.conv_out.bias": torch.zeros(3)})
    dst = AutoencoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM).load_compvis(bare)
    assert all(torch.equal(v, sd[k]) for k, v in dst.state_dict().items())
    missing = {k: v for k, v in ckpt["state_dict"].items() if not k.endswith("encoder.mid.attn_1.k.bias")}
    with pytest.raises(KeyError, match=r"encoder\.mid\.attn_1\.k\.bias"):
        AutoencoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM).load_compvis({"state_dict": missing})
    bad = dict(sd, **{"quant_conv.weight": torch.zeros(8, 4, 1, 1)})
    with pytest.raises(ValueError, match=r"quant_conv\.weight"):
        AutoencoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM).load_compvis(bad)
    assert not any(p.requires_grad for p in dst.parameters()) and not dst.training


def test_load_compvis_from_a_file(tmp_path):
    from unlearn_saliency_amd.SD.autoencoder import AutoencoderKLLite
    src = X.load_filled(AutoencoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM))
    p = tmp_path / "tiny.ckpt"
    torch.save({"state_dict": {"first_stage_model." + k: v for k, v in src.state_dict().items()}}, p)
    dst = AutoencoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM).load_compvis(str(p))
    assert all(torch.equal(v, src.state_dict()[k]) for k, v in dst.state_dict().items())


# ------------------------------------------------------------------------------------------ images
def _synthetic(w, h, mode="RGB"):
    from PIL import Image
    r = np.random.default_rng(w * 1000 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(xx * 5 + yy * 3 + 40 * c) % 256 for c in range(3)], -1) + r.integers(-20, 20, (h, w, 3))
    im = Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))
    return im.convert(mode)


@pytest.mark.parametrize("interpolation", ["bicubic", "bilinear", "lanczos"])
@pytest.mark.parametrize("wh,resized,box", [((48, 80), (32, 53), (0, 10, 32, 42)), ((80, 48), (53, 32), (10, 0, 42, 32))])
def test_transform_equals_pillow_called_directly(interpolation, wh, resized, box):
    """Resize(32): the shorter side becomes 32, the other int(32 * 80 / 48) = 53; CenterCrop(32) starts at
    int(round((53 - 32) / 2)) = 10; then convert("RGB")."""
    from PIL import Image
    from unlearn_saliency_amd.SD import images
    im = _synthetic(*wh)
    assert images.resized_size(*wh, 32) == resized and images.crop_box(*resized, 32) == box
    flt = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "lanczos": Image.LANCZOS}[interpolation]
    want = np.asarray(im.resize(resized, flt).crop(box).convert("RGB"))
    got = images.transform(im, 32, interpolation)
    assert got.dtype == np.uint8 and got.shape == (32, 32, 3) and np.array_equal(got, want)
    grey = images.transform(_synthetic(*wh, mode="L"), 32, interpolation)        # a one-band file comes out as three
    assert grey.shape == (32, 32, 3) and np.array_equal(grey[..., 0], grey[..., 2])
    assert not np.array_equal(images.transform(im, 32, "bilinear"), images.transform(im, 32, "lanczos"))


def test_transform_rejects_an_unknown_interpolation_and_loads_files(tmp_path):
    from unlearn_saliency_amd.SD import images
    with pytest.raises(ValueError, match="nearest"):
        images.transform(_synthetic(48, 80), 32, "nearest")
    p = tmp_path / "a.png"
    _synthetic(80, 48).save(p)
    assert np.array_equal(images.load(str(p), 32, "bicubic"), images.transform(_synthetic(80, 48), 32, "bicubic"))


# ------------------------------------------------------------------------------------------ manifest
def test_manifest_and_prompts(tmp_path):
    from unlearn_saliency_amd.SD import images
    man = tmp_path / "rows.csv"
    man.write_text("# split,path,prompt,other\n"
                   "forget,img/a.png,a photo of a church\n"
                   "forget,img/b.png,\"a photo, of a dog\",a photo of a cat\n"
                   "\n"
                   f"remain,{tmp_path}/abs.png,a photo of a truck\n")
    rows = images.read_manifest(str(man))
    assert [r.split for r in rows] == ["forget", "forget", "remain"]
    assert rows[0] == images.Row("forget", str(tmp_path / "img" / "a.png"), "a photo of a church", "")
    assert rows[1].prompt == "a photo, of a dog" and rows[1].other_prompt == "a photo of a cat"
    assert rows[2].path == f"{tmp_path}/abs.png" and rows[2].other_prompt is None
    ctx = {p: torch.zeros(1, 77, 8) for p in ("a photo of a church", "a photo, of a dog", "a photo of a truck", "")}
    with pytest.raises(KeyError, match="a photo of a cat"):
        images.check_prompts(rows, ctx)
    ctx["a photo of a cat"] = torch.zeros(1, 77, 8)
    images.check_prompts(rows, ctx)
    for bad in ("train,x.png,p\n", "forget,x.png\n", "forget,x.png,a,b,c\n"):
        man.write_text(bad)
        with pytest.raises(ValueError, match="rows.csv:1"):
            images.read_manifest(str(man))


# ------------------------------------------------------------------------------------------ the command line
def test_encode_images_parser():
    ap = _script("encode_images").build_parser()
    a = ap.parse_args(["--out", "z.pt"])
    assert (a.image_size, a.interpolation, a.posterior, a.seed, a.device, a.synthetic) == (512, "bicubic", "sample", 0, "0", 0)
    assert a.ckpt_path == "models/ldm/sd-v1-4-full-ema.ckpt" and a.manifest is None and a.contexts is None
    a = ap.parse_args("--manifest m.csv --contexts c.pt --ckpt_path x.ckpt --image_size 256 --interpolation lanczos "
                      "--batch_size 2 --posterior mode --seed 3 --device 1 --out o.pt --synthetic 2".split())
    assert (a.manifest, a.contexts, a.ckpt_path, a.image_size, a.interpolation, a.batch_size, a.posterior, a.seed, a.device,
            a.out, a.synthetic) == ("m.csv", "c.pt", "x.ckpt", 256, "lanczos", 2, "mode", 3, "1", "o.pt", 2)
    for bad in (["--out", "o", "--interpolation", "nearest"], ["--out", "o", "--posterior", "mean"], []):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
