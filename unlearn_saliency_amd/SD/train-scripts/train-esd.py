"""`python train-esd.py --prompt "Van Gogh" --train_method xattn --devices 0,0` — command line of the reference's
SD/train-scripts/train-esd.py:381-511 in front of `unlearn_saliency_amd.SD.train_scripts.train_esd`: Erased Stable
Diffusion, and with `--mask_path` ESD restricted to a saliency mask written by generate_mask.py.

The prompts' context embeddings come from a file or from the text encoder of SD/clip_text.py:

    --contexts FILE   torch.save'd dict {prompt: (1, 77, ctx) tensor} holding "" and every word of the prompt
                      (encode_prompts.py writes one)
    --tokenizer DIR   instead: the folder with the CLIP tokenizer's vocab.json and merges.txt; "" and the words are
                      encoded here by the text model of --ckpt_path (K29 and the K15 GEMM)
    --synthetic N     (any N > 0) random contexts for "" and each word (benchmarks / smoke runs)

Reference quirks kept visible rather than reproduced: its `--lr` is declared `type=int` (so any `--lr 1e-5` on the
command line is rejected there; here it parses as float, default unchanged).  `--devices` keeps the reference's two
entries; both models live on the first (one MI355X holds the two U-Nets many times over)."""
import argparse

import _common
from random_label import save_compvis


def build_parser():
    parser = argparse.ArgumentParser(prog="TrainESD",
                                     description="Finetuning stable diffusion model to erase concepts using ESD method")
    parser.add_argument("--prompt", help="prompt corresponding to concept to erase", type=str, required=True)
    parser.add_argument("--train_method", help="method of training", type=str, required=True)
    parser.add_argument("--start_guidance", help="guidance of start image used to train", type=float, required=False,
                        default=3)
    parser.add_argument("--negative_guidance", help="guidance of negative training used to train", type=float,
                        required=False, default=1)
    parser.add_argument("--iterations", help="iterations used to train", type=int, required=False, default=1000)
    parser.add_argument("--lr", help="learning rate used to train", type=float, required=False, default=1e-5)
    parser.add_argument("--config_path", help="config path for stable diffusion v1-4 inference", type=str, required=False,
                        default="configs/stable-diffusion/v1-inference.yaml")
    parser.add_argument("--ckpt_path", help="ckpt path for stable diffusion v1-4", type=str, required=False,
                        default="models/ldm/stable-diffusion-v1/epoch=000050.ckpt")
    parser.add_argument("--mask_path", help="mask path for stable diffusion v1-4", type=str, required=False, default=None)
    parser.add_argument("--diffusers_config_path", help="diffusers unet config json path", type=str, required=False,
                        default="diffusers_unet_config.json")
    parser.add_argument("--devices", help="cuda devices to train on", type=str, required=False, default="0,0")
    parser.add_argument("--seperator", help="separator if you want to train bunch of words separately", type=str,
                        required=False, default=None)
    parser.add_argument("--image_size", help="image size used to train", type=int, required=False, default=512)
    parser.add_argument("--ddim_steps", help="ddim steps of inference used to train", type=int, required=False, default=50)
    _common.add_batch_source_flags(parser)
    parser.add_argument("--contexts", type=str, default=None,
                        help='file with the context embeddings: {prompt: (1, 77, ctx) tensor} holding "" and every word')
    return parser


def full_parser():
    """build_parser() is the table pinned against the reference's (tests/golden/cli_sd_baselines.json: its flags plus
    the batch-source additions); the command line adds the text encoder's flag to it."""
    parser = build_parser()
    parser.add_argument("--tokenizer", type=str, default=None,
                        help="folder with the CLIP tokenizer's vocab.json and merges.txt: encode the words here")
    return parser


NO_CONTEXTS = ("give --contexts FILE (context embeddings of \"\" and every word) or --synthetic N: the text encoder runs "
               "only where it is asked for.  --tokenizer DIR names the folder with the CLIP tokenizer's vocab.json and "
               "merges.txt; with it and --ckpt_path the script encodes its own prompts (SD/clip_text.py).")


def main(argv=None):
    import torch
    args = full_parser().parse_args(argv)
    if not (args.contexts or args.tokenizer or args.synthetic > 0):
        raise SystemExit(NO_CONTEXTS)
    devices = [_common.device_of(d.strip()) for d in args.devices.split(",")]
    from unlearn_saliency_amd.SD import train_scripts as TS
    model = TS.setup_model(args.config_path, args.ckpt_path, devices[0], bf16=args.bf16,
                           resident_activations=args.resident_activations)
    _, words = TS.esd_words(args.prompt, args.seperator)
    if args.contexts:
        contexts = torch.load(args.contexts, map_location=devices[0], weights_only=False)
    elif args.tokenizer:
        from unlearn_saliency_amd.SD import clip_text
        contexts = clip_text.contexts_for(words, args.tokenizer, args.ckpt_path, devices[0])
    elif args.synthetic > 0:
        g = torch.Generator(device=devices[0]).manual_seed(0)
        dim = model.model.diffusion_model.context_dim
        contexts = {w: torch.randn(1, 77, dim, device=devices[0], generator=g) for w in [""] + words}
    else:
        raise SystemExit(NO_CONTEXTS)
    model, losses = TS.train_esd(args.prompt, args.train_method, args.start_guidance, args.negative_guidance,
                                 args.iterations, args.lr, args.config_path, args.ckpt_path, args.mask_path,
                                 args.diffusers_config_path, devices, args.seperator, args.image_size, args.ddim_steps,
                                 model=model, contexts=contexts, save=True)
    name = TS.esd_name(args.train_method, args.lr, args.mask_path)   # train-esd.py:259-263
    print("saved", save_compvis(model, name), "final loss", losses[-1] if losses else None)


if __name__ == "__main__":
    main()
