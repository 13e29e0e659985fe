"""`python imageclassify.py --folder_path FOLDER --prompts_path prompts.csv` — the command line of the reference's
SD/eval-scripts/imageclassify.py (same flags, same defaults, same file rule) on this package: torchvision's ResNet-50
over every image of FOLDER (SD/resnet50.py: InferencePlan50 on K26, K27, K30, the evaluation head and the row top-k),
and a CSV with the top-k categories, indices and scores per image joined to the prompt file on `case_number`.

What is kept from the reference: names with `.png` or `.jpg` in them are classified; `case_number` is
`int(name.split("_")[0])` with the extension removed (what generate-images.py writes); the preset
`ResNet50_Weights.DEFAULT.transforms()` (resize 232, centre crop 224, ImageNet mean / std); `softmax` and `torch.topk`;
the default `--save_path` `{folder}/{folder.split("/")[-1]}_classification.csv`; and the file itself, which is what
`pd.merge(df, df_results)` followed by `to_csv(save_path)` writes - an inner join on `case_number` (rows of the prompt
file in file order, a row's images in name order), a leading unnamed index column, the prompt file's columns, then
`category_top{k}`, `index_top{k}`, `scores_top{k}`, the scores formatted as pandas formats a float32 column - written
here without importing pandas.  Cells of the prompt file are passed through as text: a float cell pandas would
re-format (`1.50` -> `1.5`) is written as read.

What differs: names are taken in SORTED order (the reference takes `os.listdir` order, which is not defined), and an
image is read with Pillow and `convert("RGB")`, so a grey or RGBA file is classified instead of failing.

Additions:
    --classifier_path FILE   torchvision's `resnet50-11ad3fa6.pth` (ResNet50_Weights.DEFAULT); a bare name is looked for in
                             the working directory, then $TORCH_HOME/hub/checkpoints, then ~/.cache/torch/hub/checkpoints
                             (where the reference leaves it).  Nothing is fetched.
    --categories FILE        1000 lines, one category name each (`weights.meta["categories"]`; see README.md)
    --synthetic              seeded stand-in weights (--seed) and the names class_0000 .. class_0999: no file but the images
"""
import argparse
import csv
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_CLASSIFIER = "resnet50-11ad3fa6.pth"
NUM_CLASSES = 1000
NO_CATEGORIES = ("give --categories FILE (1000 lines, one ImageNet category name each: the list torchvision keeps in "
                 "ResNet50_Weights.DEFAULT.meta[\"categories\"]; README.md has the one-liner that writes it) or --synthetic")


def build_parser():
    parser = argparse.ArgumentParser(prog="ImageClassification",
                                     description="Takes the path of images and generates classification scores")
    parser.add_argument("--folder_path", help="path to images", type=str, required=True)
    parser.add_argument("--prompts_path", help="path to prompts", type=str, required=True)
    parser.add_argument("--save_path", help="path to save results", type=str, required=False, default=None)
    parser.add_argument("--device", type=str, required=False, default="cuda:0")
    parser.add_argument("--topk", type=int, required=False, default=5)
    parser.add_argument("--batch_size", type=int, required=False, default=250)
    parser.add_argument("--classifier_path", type=str, default=DEFAULT_CLASSIFIER,
                        help="torchvision's ResNet-50 checkpoint (ResNet50_Weights.DEFAULT)")
    parser.add_argument("--categories", type=str, default=None, help="file with the 1000 category names, one per line")
    parser.add_argument("--synthetic", action="store_true", help="seeded stand-in weights and names: no checkpoint needed")
    parser.add_argument("--seed", type=int, default=0, help="--synthetic: the seed of the weights")
    return parser


def default_save_path(folder: str) -> str:
    return f"{folder}/{folder.split('/')[-1]}_classification.csv"


def image_names(folder: str):
    return sorted(name for name in os.listdir(folder) if ".png" in name or ".jpg" in name)


def case_number(name: str) -> int:
    return int(name.split("/")[-1].split("_")[0].replace(".png", "").replace(".jpg", ""))


def checkpoint_candidates(path: str, cwd=None, env=None, home=None):
    """Where `path` is looked for, in order.  A path with a directory in it is taken as given."""
    env = os.environ if env is None else env
    if os.path.dirname(path):
        return [path]
    out = [os.path.join(cwd if cwd is not None else os.getcwd(), path)]
    if env.get("TORCH_HOME"):
        out.append(os.path.join(env["TORCH_HOME"], "hub", "checkpoints", path))
    home = os.path.expanduser("~") if home is None else home
    out.append(os.path.join(home, ".cache", "torch", "hub", "checkpoints", path))
    return out


def find_checkpoint(path: str, cwd=None, env=None, home=None) -> str:
    tried = checkpoint_candidates(path, cwd, env, home)
    for p in tried:
        if os.path.isfile(p):
            return p
    raise SystemExit(f"--classifier_path {path}: not found; looked in " + ", ".join(tried) + ".  Nothing is downloaded: "
                     "copy torchvision's resnet50-11ad3fa6.pth to one of them, or run with --synthetic.")


def read_categories(path):
    if path is None:
        raise SystemExit(NO_CATEGORIES)
    with open(path, encoding="utf-8") as f:
        names = [ln.rstrip("\r\n") for ln in f]
    while names and names[-1] == "":
        names.pop()
    if len(names) != NUM_CLASSES:
        raise SystemExit(f"--categories {path}: {len(names)} lines, expected {NUM_CLASSES}")
    return names


def synthetic_categories():
    return [f"class_{i:04d}" for i in range(NUM_CLASSES)]


def format_scores(values):
    """The text pandas' to_csv writes for a float32 column: numpy's shortest round-trip form of each float32."""
    import numpy as np
    return [str(s) for s in np.asarray(values, dtype=np.float32).astype(str)]


def merged_rows(header, rows, case_numbers, categories, indices, scores, topk):
    """`pd.merge(df, df_results)` as lists of text cells: -> (header, rows).  `rows` are the prompt file's rows (lists of
    cells under `header`), `case_numbers` / `categories` / `indices` / `scores` are per image, the last three [n][topk]."""
    if "case_number" not in header:
        raise SystemExit("the prompt file has no column `case_number`")
    col = header.index("case_number")
    by_case: dict = {}
    for i, c in enumerate(case_numbers):
        by_case.setdefault(int(c), []).append(i)
    text = [format_scores([s[k] for s in scores]) for k in range(topk)]
    out_header = [""] + list(header)
    for k in range(1, topk + 1):
        out_header += [f"category_top{k}", f"index_top{k}", f"scores_top{k}"]
    out = []
    for row in rows:
        case = int(float(row[col]))                 # df["case_number"].astype("int")
        for i in by_case.get(case, ()):
            cells = list(row)
            cells[col] = str(case)
            for k in range(topk):
                cells += [str(categories[i][k]), str(int(indices[i][k])), text[k][i]]
            out.append([str(len(out))] + cells)
    return out_header, out


def read_prompts(path):
    with open(path, newline="", encoding="utf-8") as f:
        table = list(csv.reader(f))
    if not table:
        raise SystemExit(f"{path}: empty prompt file")
    return table[0], [r for r in table[1:] if r]


def write_csv(path, header, rows):
    with open(path, "w", newline="", encoding="utf-8") as f:
        w = csv.writer(f, lineterminator="\n", quoting=csv.QUOTE_MINIMAL)
        w.writerow(header)
        w.writerows(rows)


def load_images(folder, names):
    """-> list of uint8 (h, w, 3) arrays, decoded on the host."""
    import numpy as np
    from PIL import Image
    out = []
    for name in names:
        with Image.open(os.path.join(folder, name)) as im:
            out.append(np.asarray(im.convert("RGB")))
    return out


def classify(plan, images, topk, batch_size, device):
    """-> (scores [n, topk] float32, indices [n, topk] int64) as numpy arrays.  Images are grouped by size, so that a
    group is one K26 launch per batch."""
    import numpy as np
    import torch
    n = len(images)
    scores, indices = np.zeros((n, topk), np.float32), np.zeros((n, topk), np.int64)
    groups: dict = {}
    for i, im in enumerate(images):
        groups.setdefault(im.shape[:2], []).append(i)
    for ids in groups.values():
        for s in range(0, len(ids), batch_size):
            chunk = ids[s:s + batch_size]
            u8 = torch.from_numpy(np.stack([images[i] for i in chunk])).to(device)
            v, ix = plan.classify_u8(u8, topk)
            scores[chunk], indices[chunk] = v.cpu().numpy(), ix.cpu().numpy()
    return scores, indices


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    folder = args.folder_path
    save_path = args.save_path if args.save_path is not None else default_save_path(folder)
    if not 1 <= args.topk <= NUM_CLASSES:
        raise SystemExit("--topk must be in [1, 1000]")
    names_of = synthetic_categories() if args.synthetic else read_categories(args.categories)
    ckpt = None if args.synthetic else find_checkpoint(args.classifier_path)

    import torch
    from unlearn_saliency_amd.SD import resnet50 as R50
    model = R50.resnet50()
    if args.synthetic:
        model.load_state_dict(R50.standin_state_dict(args.seed))
    else:
        model.load_state_dict(torch.load(ckpt, map_location="cpu"))
    device = torch.device(args.device)
    if device.type == "cuda":
        torch.cuda.set_device(device)
    plan = R50.InferencePlan50(model.eval(), device)

    names = image_names(folder)
    if not names:
        raise SystemExit(f"{folder}: no .png or .jpg file")
    batch_size = len(names) if args.batch_size is None else max(1, min(args.batch_size, len(names)))
    scores, indices = classify(plan, load_images(folder, names), args.topk, batch_size, device)
    categories = [[names_of[j] for j in row] for row in indices]
    header, rows = read_prompts(args.prompts_path)
    out_header, out_rows = merged_rows(header, rows, [case_number(n) for n in names], categories, indices, scores, args.topk)
    write_csv(save_path, out_header, out_rows)
    print(f"{len(names)} images, {len(out_rows)} rows -> {save_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
