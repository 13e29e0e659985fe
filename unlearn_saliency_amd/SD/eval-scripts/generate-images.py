"""`python generate-images.py --model_name NAME --prompts_path prompts.csv --save_path out` — the command line of the
reference's SD/eval-scripts/generate-images.py (same flags, same defaults) on this package: for every row of the CSV
(`case_number`, `prompt`, `evaluation_seed`) ten rounds of `--num_samples` images, written as
`<save_path>/<model_name>/<case>_<round * 10 + num>.png`.

What is kept from the reference: the initial noise (`torch.randn((B, 4, s / 8, s / 8), generator=torch.manual_seed(seed))`
on the host, one generator carried through the rounds, so the starting latents are the reference's), the LMS sampler
and its schedule (SD/lms.py), classifier-free guidance at `--guidance_scale`, `1 / 0.18215 * latents`, the decoder
(SD/autoencoder.py: DecoderPlan) and the byte rule `(image / 2 + 0.5).clamp(0, 1)`, `(image * 255).round()`.
The U-Net weights are `models/<model_name>/<model_name>.pt`, the CompVis file the train scripts write (the reference
loads the Diffusers twin next to it); when "SD" is in the model name the untouched `--ckpt_path` U-Net is used.

Additions:
    --ckpt_path FILE   SD-v1 checkpoint: the VAE decoder and the base U-Net       --config_path FILE  its YAML
    --contexts FILE    torch.save'd dict {prompt: (1, 77, 768) tensor} holding "" and every prompt of the CSV
                       (SD/train-scripts/encode_prompts.py writes one)
    --tokenizer DIR    instead of --contexts: the folder with the CLIP tokenizer's vocab.json and merges.txt; the prompts
                       are encoded here, by the text model of --ckpt_path (SD/clip_text.py: K29 and the K15 GEMM); with
                       --synthetic by a seeded two-layer text model of the U-Net's context width
    --sampler lms|ddim lms (default) or SD/ddim.py's DDIM chain with till_T = None
    --rounds N         rounds per row (default 10, as the reference)              --decode_batch N  latents per decode
    --bf16             the U-Net in the bf16 configuration (the decoder stays fp32)
    --synthetic        seeded U-Net and VAE weights and seeded contexts (--unet_config / --ddconfig JSON, --seed), so the
                       whole path runs without any file but the CSV
"""
import argparse
import csv
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

UNET_PREFIX = "model.diffusion_model."
NO_CONTEXTS = ("give --contexts FILE (context embeddings of \"\" and every prompt) or --synthetic: the text encoder runs "
               "only where it is asked for.  --tokenizer DIR names the folder with the CLIP tokenizer's vocab.json and "
               "merges.txt; with it and --ckpt_path the script encodes its own prompts (SD/clip_text.py).")


def build_parser():
    parser = argparse.ArgumentParser(prog="generateImages", description="Generate Images using Diffusers Code")
    parser.add_argument("--model_name", help="name of model", type=str, required=True)
    parser.add_argument("--prompts_path", help="path to csv file with prompts", type=str, required=True)
    parser.add_argument("--save_path", help="folder where to save images", type=str, required=True)
    parser.add_argument("--device", help="cuda device to run on", type=str, required=False, default="cuda:0")
    parser.add_argument("--guidance_scale", help="guidance to run eval", type=float, required=False, default=7.5)
    parser.add_argument("--image_size", help="image size used to train", type=int, required=False, default=512)
    parser.add_argument("--from_case", help="continue generating from case_number", type=int, required=False, default=0)
    parser.add_argument("--num_samples", help="number of samples per prompt", type=int, required=False, default=10)
    parser.add_argument("--ddim_steps", help="ddim steps of inference used to train", type=int, required=False, default=100)
    parser.add_argument("--ckpt_path", type=str, default="models/ldm/stable-diffusion-v1/sd-v1-4-full-ema.ckpt",
                        help="SD-v1 checkpoint: the VAE decoder and the base U-Net")
    parser.add_argument("--config_path", type=str, default="configs/stable-diffusion/v1-inference.yaml")
    parser.add_argument("--contexts", type=str, default=None,
                        help='file with the context embeddings: {prompt: (1, 77, ctx) tensor} holding "" and every prompt')
    parser.add_argument("--tokenizer", type=str, default=None,
                        help="folder with the CLIP tokenizer's vocab.json and merges.txt: encode the prompts here")
    parser.add_argument("--bf16", action="store_true", help="the U-Net in the bf16 configuration")
    parser.add_argument("--sampler", choices=("lms", "ddim"), default="lms")
    parser.add_argument("--rounds", type=int, default=10, help="rounds per row (the reference makes 10)")
    parser.add_argument("--decode_batch", type=int, default=0, help="latents per decoder call (default: --num_samples)")
    parser.add_argument("--synthetic", action="store_true", help="seeded weights and contexts: no checkpoint needed")
    parser.add_argument("--unet_config", type=str, default=None, help="--synthetic: the U-Net configuration as JSON")
    parser.add_argument("--ddconfig", type=str, default=None, help="--synthetic: the VAE ddconfig as JSON")
    parser.add_argument("--seed", type=int, default=0, help="--synthetic: the seed of the weights and contexts")
    return parser


def read_rows(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    for col in ("case_number", "prompt", "evaluation_seed"):
        if rows and col not in rows[0]:
            raise SystemExit(f"{path}: no column `{col}`")
    return [(int(r["case_number"]), str(r["prompt"]), int(r["evaluation_seed"])) for r in rows]


def _tuples(cfg):
    return {k: (tuple(v) if isinstance(v, list) else v) for k, v in cfg.items()}


def build_models(args, device):
    """-> (LatentDiffusionLite, DecoderPlan)"""
    import torch
    import yaml
    from unlearn_saliency_amd.SD.autoencoder import V1_DDCONFIG, DecoderKLLite, DecoderPlan
    from unlearn_saliency_amd.SD.ldm_lite import LatentDiffusionLite
    from unlearn_saliency_amd.SD.unet import V1_UNET_CONFIG
    ucfg, ddconfig, embed_dim = dict(V1_UNET_CONFIG), dict(V1_DDCONFIG), 4
    if args.synthetic:
        if args.unet_config:
            ucfg = _tuples(json.loads(args.unet_config))
        if args.ddconfig:
            ddconfig = _tuples(json.loads(args.ddconfig))
        torch.manual_seed(args.seed)
        model = LatentDiffusionLite(ucfg, bf16=args.bf16).to(device)
        model.fill_zero_initialised(seed=args.seed + 11)
        vae = DecoderKLLite(ddconfig, embed_dim)
    else:
        if os.path.exists(args.config_path):
            with open(args.config_path) as f:
                params = yaml.safe_load(f)["model"]["params"]
            ucfg.update(_tuples(params["unet_config"]["params"]))
            fs = params.get("first_stage_config", {}).get("params", {})
            ddconfig = _tuples(fs.get("ddconfig", ddconfig))
            embed_dim = int(fs.get("embed_dim", embed_dim))
        if not os.path.exists(args.ckpt_path):
            raise SystemExit(f"--ckpt_path {args.ckpt_path}: no such file (the VAE decoder and the base U-Net come from it; "
                             "--synthetic runs without one)")
        ckpt = torch.load(args.ckpt_path, map_location="cpu", weights_only=False)
        ckpt = ckpt.get("state_dict", ckpt)
        vae = DecoderKLLite(ddconfig, embed_dim).load_compvis(ckpt)
        if "SD" not in args.model_name:
            path = f"models/{args.model_name}/{args.model_name}.pt"
            if not os.path.exists(path):
                raise SystemExit(f"{path}: no such file (the CompVis state dict the train scripts write)")
            ckpt = torch.load(path, map_location="cpu", weights_only=False)
            ckpt = ckpt.get("state_dict", ckpt)
        model = LatentDiffusionLite(ucfg, bf16=args.bf16)
        model.model.diffusion_model.load_state_dict(
            {k[len(UNET_PREFIX):]: v for k, v in ckpt.items() if k.startswith(UNET_PREFIX)}, strict=True)
        model = model.to(device)
    model.requires_grad_(False).eval()
    model.use_mfma_convs()
    return model, DecoderPlan(vae.to(device))


def load_contexts(args, prompts, model, device):
    import torch
    if args.contexts:
        contexts = torch.load(args.contexts, map_location=device, weights_only=False)
    elif args.tokenizer:
        from unlearn_saliency_amd.SD import clip_text
        synthetic = clip_text.synthetic_config(model.model.diffusion_model.context_dim, 0) if args.synthetic else None
        contexts = clip_text.contexts_for(prompts, args.tokenizer, args.ckpt_path, device, synthetic, args.seed)
    elif args.synthetic:
        import zlib
        dim = model.model.diffusion_model.context_dim
        # keyed by the prompt's text alone: a prompt's context does not depend on the other rows
        draw = lambda p: torch.randn(1, 77, dim, generator=torch.Generator().manual_seed(
            (args.seed << 32) + zlib.crc32(p.encode())))
        contexts = {p: draw(p).to(device) for p in [""] + sorted(set(prompts))}
    else:
        raise SystemExit(NO_CONTEXTS)
    for p in [""] + prompts:
        if p not in contexts:
            raise SystemExit(f"--contexts: no embedding of the prompt `{p}`")
    return contexts


def generate_images(args):
    import torch
    from PIL import Image
    from unlearn_saliency_amd.SD.ddim import DDIMSampler
    from unlearn_saliency_amd.SD.lms import LMSSampler
    if not (args.contexts or args.tokenizer or args.synthetic):
        raise SystemExit(NO_CONTEXTS)
    if not torch.cuda.is_available():
        raise SystemExit("generate-images needs a ROCm device (no CPU fallback for the measured path)")
    device = args.device if ":" in args.device or not args.device.isdigit() else f"cuda:{int(args.device)}"
    rows = [r for r in read_rows(args.prompts_path) if r[0] >= args.from_case]
    # the contexts are checked before any model is built: a missing prompt costs nothing
    probe = None
    if args.contexts:
        probe = load_contexts(args, [p for _, p, _ in rows], None, device)
    model, plan = build_models(args, device)
    contexts = probe or load_contexts(args, [p for _, p, _ in rows], model, device)
    folder = f"{args.save_path}/{args.model_name}"
    os.makedirs(folder, exist_ok=True)
    B, side = args.num_samples, args.image_size // 8
    cin = model.model.diffusion_model.in_channels
    chunk = args.decode_batch if args.decode_batch > 0 else B
    sampler = LMSSampler(model) if args.sampler == "lms" else DDIMSampler(model).make_schedule(args.ddim_steps)
    written = []
    for case, prompt, seed in rows:
        print([prompt] * B)
        generator = torch.manual_seed(seed)
        cond = contexts[prompt].to(device).float().expand(B, -1, -1).contiguous()
        uncond = contexts[""].to(device).float().expand(B, -1, -1).contiguous()
        for i in range(args.rounds):
            noise = torch.randn((B, cin, side, side), generator=generator).to(device)
            if args.sampler == "lms":
                latents = sampler.sample(cond, uncond, args.guidance_scale, noise, args.ddim_steps)
            else:
                latents = sampler.sample(cond, uncond, args.guidance_scale, noise, till_T=None)
            images = torch.cat([plan.decode_u8(latents[j:j + chunk]) for j in range(0, B, chunk)]).cpu().numpy()
            for num, im in enumerate(images):
                path = f"{folder}/{case}_{i * 10 + num}.png"
                Image.fromarray(im).save(path)
                written.append(path)
    return written


def main(argv=None):
    args = build_parser().parse_args(argv)
    return generate_images(args)


if __name__ == "__main__":
    main()
