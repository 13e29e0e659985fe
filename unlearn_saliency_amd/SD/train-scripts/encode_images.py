"""`python encode_images.py --manifest rows.csv --contexts ctx.pt --ckpt_path sd-v1-4-full-ema.ckpt --out latents.pt` —
image folders -> the `--latents` file generate_mask.py, random_label.py, nsfw_removal.py and the baselines read.

What the reference's loaders do on every fetch (SD/train-scripts/dataset.py -> model.get_input -> encode_first_stage ->
get_first_stage_encoding: the frozen AutoencoderKL's posterior, sampled, times 0.18215) is done here once, on the
device: the host transform of SD/images.py, then SD/autoencoder.py's EncoderPlan (K27 / K28 / K15) and the posterior
kernel.  The file is exactly the dict `_common.batches` loads:

    {"forget": [(z, c_forget, c_other), ...], "remain": [(z, c), ...]}     z already scaled by 0.18215

    --manifest FILE   CSV rows  split,path,prompt[,other_prompt]  with split in forget | remain (SD/images.py)
    --contexts FILE   torch.save'd dict {prompt: (1, 77, ctx) tensor}, as train-esd.py reads it (encode_prompts.py
                      writes one)
    --tokenizer DIR   instead: the folder with the CLIP tokenizer's vocab.json and merges.txt; the manifest's prompts are
                      encoded here by the text model of --ckpt_path (SD/clip_text.py: K29 and the K15 GEMM)
    --synthetic N     seeded encoder weights, `fill_u8` images and random contexts: N batches per split

A difference from the reference, by construction: a file freezes ONE posterior draw per image (keyed by --seed and
the image's row in the manifest, so it does not depend on --batch_size), where the reference redraws at every fetch.
`--posterior mode` stores the posterior mean instead.  The live path without that difference is
`EncoderPlan.first_stage(seed)` plugged into `LatentDiffusionLite(first_stage=...)`.
"""
import argparse
import json
import os

import _common


def build_parser():
    parser = argparse.ArgumentParser(prog="EncodeImages", description="Encode images to SD latents with the frozen VAE encoder")
    parser.add_argument("--manifest", type=str, default=None, help="CSV: split,path,prompt[,other_prompt]")
    parser.add_argument("--contexts", type=str, default=None, help="file with {prompt: (1, 77, ctx) tensor}")
    parser.add_argument("--tokenizer", type=str, default=None,
                        help="folder with the CLIP tokenizer's vocab.json and merges.txt: encode the prompts here")
    parser.add_argument("--ckpt_path", type=str, default="models/ldm/sd-v1-4-full-ema.ckpt",
                        help="SD-v1 CompVis checkpoint (or a bare autoencoder state dict)")
    parser.add_argument("--image_size", type=int, default=512)
    parser.add_argument("--interpolation", type=str, default="bicubic", choices=["bicubic", "bilinear", "lanczos"])
    parser.add_argument("--batch_size", type=int, default=4)
    parser.add_argument("--posterior", type=str, default="sample", choices=["sample", "mode"])
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--device", type=str, default="0")
    parser.add_argument("--out", type=str, required=True, help="the --latents file to write")
    parser.add_argument("--synthetic", type=int, default=0, help="this many synthetic batches per split instead")
    parser.add_argument("--ddconfig", type=str, default=None,
                        help="JSON (text or file) of the encoder's ddconfig; default: the v1 first_stage_config")
    parser.add_argument("--context_dim", type=int, default=768, help="width of the synthetic contexts")
    return parser


NO_SOURCE = ("give --manifest FILE and --contexts FILE, or --synthetic N.  --tokenizer DIR names the folder with the CLIP "
             "tokenizer's vocab.json and merges.txt; with it and --ckpt_path the script encodes its own prompts "
             "(SD/clip_text.py).")


def _ddconfig(arg):
    if arg is None:
        return None
    if os.path.exists(arg):
        with open(arg) as f:
            return json.load(f)
    return json.loads(arg)


def main(argv=None):
    import torch
    args = build_parser().parse_args(argv)
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be at least 1")
    if args.synthetic <= 0 and (not args.manifest or not (args.contexts or args.tokenizer)):
        raise SystemExit(NO_SOURCE)
    device = _common.device_of(args.device)
    from unlearn_saliency_amd import ops
    from unlearn_saliency_amd.SD import images
    from unlearn_saliency_amd.SD.autoencoder import SCALE_FACTOR, AutoencoderKLLite, EncoderPlan

    cfg = _ddconfig(args.ddconfig)
    torch.manual_seed(args.seed)
    model = AutoencoderKLLite(cfg, embed_dim=(cfg or {}).get("z_channels", 4))
    B, S = args.batch_size, args.image_size
    if args.synthetic > 0:
        g = torch.Generator().manual_seed(args.seed)
        n = args.synthetic * B
        rows = [images.Row(s, None, f"{s} {i}", "" if s == "forget" else None) for s in images.SPLITS for i in range(n)]
        contexts = {p: torch.randn(1, 77, args.context_dim, generator=g)
                    for p in sorted({r.prompt for r in rows} | {""})}
        pixels = lambda i, r: ops.fill_u8(S * S * 3, args.seed * 1000003 + i, device).view(S, S, 3)
    else:
        rows = images.read_manifest(args.manifest)
        if args.contexts:
            contexts = torch.load(args.contexts, map_location="cpu", weights_only=False)
        else:
            from unlearn_saliency_amd.SD import clip_text
            wanted = [p for r in rows for p in (r.prompt, r.other_prompt) if p is not None]
            contexts = clip_text.contexts_for(wanted, args.tokenizer, args.ckpt_path, device, batch=max(B, 8))
        try:
            images.check_prompts(rows, contexts)
        except KeyError as e:
            raise SystemExit(str(e.args[0]))
        model.load_compvis(args.ckpt_path)
        pixels = lambda i, r: torch.from_numpy(images.load(r.path, S, args.interpolation)).to(device)
    plan = EncoderPlan(model.to(device))

    out = {s: [] for s in images.SPLITS}
    ctx = lambda ps: torch.cat([contexts[p].reshape(1, *contexts[p].shape[-2:]) for p in ps]).to(device, torch.float32)
    for split in images.SPLITS:
        idx = [i for i, r in enumerate(rows) if r.split == split]
        for lo in range(0, len(idx), B):
            ids = idx[lo:lo + B]
            u8 = torch.stack([pixels(i, rows[i]) for i in ids])
            z = plan.encode(u8, ids, args.seed, 0, args.posterior == "mode", SCALE_FACTOR)
            cs = [ctx([rows[i].prompt for i in ids])]
            if split == "forget":
                cs.append(ctx([rows[i].other_prompt for i in ids]))
            out[split].append(tuple([z.cpu()] + [c.cpu() for c in cs]))
    torch.save(out, args.out)
    print("wrote", args.out, {k: len(v) for k, v in out.items()}, "batches of", B)


if __name__ == "__main__":
    main()
