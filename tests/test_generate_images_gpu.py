"""SD/eval-scripts/generate-images.py end to end with --synthetic: tiny U-Net and VAE, two CSV rows, two rounds of two
images, three LMS steps at 32 x 32."""
import csv
import importlib.util
import json
import os

import pytest

import fixtures

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a decoder with the first stage's factor of 8 (three Upsample layers): 4 x 4 latents -> 32 x 32 images
DDCONFIG = dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 1, 2, 2),
                num_res_blocks=1, attn_resolutions=(), dropout=0.0)
ROWS = [(3, "a photo of a tench", 11), (7, "a church", 12)]


def cli():
    path = os.path.join(ROOT, "unlearn_saliency_amd", "SD", "eval-scripts", "generate-images.py")
    spec = importlib.util.spec_from_file_location("sd_cli_generate_images", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def prompts_csv(tmp_path):
    path = tmp_path / "prompts.csv"
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["", "case_number", "prompt", "evaluation_seed", "class"])       # extra columns, as the reference's files
        for i, (case, prompt, seed) in enumerate(ROWS):
            w.writerow([i, case, prompt, seed, "x"])
    return str(path)


def argv(tmp_path, out, *more):
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in fixtures.sd_tiny_config().items()}
    dd = {k: (list(v) if isinstance(v, tuple) else v) for k, v in DDCONFIG.items()}
    return ["--model_name", "tiny", "--prompts_path", prompts_csv(tmp_path), "--save_path", str(tmp_path / out),
            "--synthetic", "--unet_config", json.dumps(cfg), "--ddconfig", json.dumps(dd), "--num_samples", "2",
            "--rounds", "2", "--ddim_steps", "3", "--image_size", "32", *more]


def png_bytes(folder):
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder))}


def test_synthetic_run_writes_the_references_file_names(tmp_path):
    from PIL import Image
    g = cli()
    written = g.main(argv(tmp_path, "a"))
    folder = tmp_path / "a" / "tiny"
    want = sorted(f"{case}_{i * 10 + num}.png" for case, _, _ in ROWS for i in range(2) for num in range(2))
    assert sorted(os.listdir(folder)) == want and sorted(os.path.basename(p) for p in written) == want
    pixels = []
    for n in want:
        im = Image.open(folder / n)
        assert im.size == (32, 32) and im.mode == "RGB"
        pixels.append(im.tobytes())
    assert len(set(pixels)) == len(pixels)                     # every image its own noise
    assert all(len(set(p)) > 8 for p in pixels)                # and not a flat field
    # a second run gives identical bytes
    g.main(argv(tmp_path, "b"))
    assert png_bytes(folder) == png_bytes(tmp_path / "b" / "tiny")
    # --from_case skips the rows below it
    g.main(argv(tmp_path, "c", "--from_case", "5"))
    assert sorted(os.listdir(tmp_path / "c" / "tiny")) == [n for n in want if n.startswith("7_")]
    first = png_bytes(folder)
    assert all(first[n] == b for n, b in png_bytes(tmp_path / "c" / "tiny").items())
    # the DDIM chain runs too, and gives other images
    g.main(argv(tmp_path, "d", "--sampler", "ddim", "--ddim_steps", "4", "--from_case", "5"))
    assert sorted(os.listdir(tmp_path / "d" / "tiny")) == [n for n in want if n.startswith("7_")]


def test_a_prompt_absent_from_contexts_is_an_error_naming_it(tmp_path):
    import torch
    g = cli()
    ctx = tmp_path / "contexts.pt"
    dim = fixtures.sd_tiny_config()["context_dim"]
    torch.save({"": torch.zeros(1, 77, dim), ROWS[0][1]: torch.zeros(1, 77, dim)}, ctx)
    with pytest.raises(SystemExit, match=ROWS[1][1]):
        g.main(argv(tmp_path, "e", "--contexts", str(ctx)))
    assert not os.path.exists(tmp_path / "e" / "tiny")
