"""`python encode_prompts.py --prompts_path prompts.csv --tokenizer DIR --ckpt_path sd-v1-4-full-ema.ckpt --out ctx.pt` —
prompts -> the `--contexts` file train-esd.py, encode_images.py and generate-images.py read:

    {prompt: (1, 77, W) fp32 tensor}     always holding ""

What the reference does on every fetch (FrozenCLIPEmbedder.forward: CLIPTokenizer, then CLIPTextModel's
last_hidden_state) is done here once, on the device: SD/clip_text.py's tokenizer on the host, then its TextPlan (K29 and
the K15 GEMM).

    --prompts_path CSV   every cell of the `prompt` column (the layout of SD/prompts/*.csv)
    --prompt TEXT ...    further prompts; each is also split by train-esd.py's own rule (--seperator, default ","), so
                         the file serves `train-esd.py --prompt "a, b"` as well
    --tokenizer DIR      the folder with the CLIP tokenizer's vocab.json and merges.txt (not part of this package)
    --ckpt_path CKPT     SD-v1 CompVis checkpoint: the text model is its `cond_stage_model.transformer.*` entries
    --synthetic          a seeded two-layer text model instead (--width, --seed): no checkpoint needed
"""
import argparse
import csv

import _common


def build_parser():
    parser = argparse.ArgumentParser(prog="EncodePrompts", description="Encode prompts to SD contexts with the CLIP text encoder")
    parser.add_argument("--prompts_path", type=str, default=None, help="CSV with a `prompt` column")
    parser.add_argument("--prompt", type=str, nargs="*", default=[], help="prompts given on the command line")
    parser.add_argument("--seperator", type=str, default=",", help="how train-esd.py splits a --prompt into words")
    parser.add_argument("--tokenizer", type=str, default=None, help="folder with vocab.json and merges.txt")
    parser.add_argument("--ckpt_path", type=str, default="models/ldm/sd-v1-4-full-ema.ckpt", help="SD-v1 CompVis checkpoint")
    parser.add_argument("--out", type=str, required=True, help="the --contexts file to write")
    parser.add_argument("--batch_size", type=int, default=8)
    parser.add_argument("--device", type=str, default="0")
    parser.add_argument("--synthetic", action="store_true", help="seeded text-model weights: no checkpoint needed")
    parser.add_argument("--width", type=int, default=768, help="--synthetic: the context width (a multiple of 64)")
    parser.add_argument("--seed", type=int, default=0, help="--synthetic: the seed of the weights")
    return parser


def collect(args):
    """"" first, then the CSV's prompt cells, then every --prompt and its words; each once, in that order."""
    from unlearn_saliency_amd.SD import train_scripts as TS
    prompts = [""]
    if args.prompts_path:
        with open(args.prompts_path, newline="", encoding="utf-8-sig") as f:
            rows = list(csv.DictReader(f))
        if rows and "prompt" not in rows[0]:
            raise SystemExit(f"{args.prompts_path}: no column `prompt`")
        prompts += [str(r["prompt"]) for r in rows]
    for p in args.prompt:
        prompts.append(p)
        prompts += TS.esd_words(p, None)[1] + TS.esd_words(p, args.seperator)[1]
    return list(dict.fromkeys(prompts))


def main(argv=None):
    import torch
    args = build_parser().parse_args(argv)
    if not args.tokenizer:
        from unlearn_saliency_amd.SD.clip_text import TOKENIZER_HINT
        raise SystemExit("give --tokenizer DIR.  " + TOKENIZER_HINT)
    if not args.prompts_path and not args.prompt:
        raise SystemExit("give --prompts_path CSV or --prompt TEXT ...")
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be at least 1")
    device = _common.device_of(args.device)
    from unlearn_saliency_amd.SD import clip_text
    prompts = collect(args)
    synthetic = clip_text.synthetic_config(args.width, 0) if args.synthetic else None
    ctx = clip_text.contexts_for(prompts, args.tokenizer, args.ckpt_path, device, synthetic, args.seed, args.batch_size)
    torch.save({p: c.cpu() for p, c in ctx.items()}, args.out)
    print("wrote", args.out, len(ctx), "contexts of", tuple(next(iter(ctx.values())).shape))
    return ctx


if __name__ == "__main__":
    main()
