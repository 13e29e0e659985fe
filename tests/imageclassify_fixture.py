"""What test_imageclassify_host.py (CPU), test_imageclassify_gpu.py and tools/make_imageclassify_golden.py share: the
numpy model of the row top-k rule, the merge fixture of the CSV writer, the seeded stand-in ResNet-50 with its float64
copy on the CPU, and the end-to-end images.  Everything is computed once per process and left unchanged.

The tolerance of the network comparison is the project's rule (classifier_eval_fixture.py): the device's logits may be
DEVICE_FACTOR = 8 times as far from float64 as the SAME module tree in fp32 on the CPU library is.  A (row, rank) of
the top-5 is compared only where the float64 PROBABILITY gap to the next rank exceeds the logits' bound e: logits that
move by at most e move p_i by at most p_i (exp(2 e) - 1), so the difference of two probabilities moves by at most
(exp(2 e) - 1) (p_i + p_j) < e while p_i + p_j < 0.49 - which a 1000-way stand-in head with logits of a few units is
far inside - and a gap above e cannot be reversed.  At most MAX_LEFT_OUT of the pairs may be left out on that ground
(asserted on the CPU for the fp32 library in test_imageclassify_host.py)."""
import functools
import io

import numpy as np
import torch

WEIGHT_SEED = 0
DEVICE_FACTOR = 8
MAX_LEFT_OUT = 0.10
TOPK = 5
NETWORK_CASES = [(3, 64), (2, 224)]


# ------------------------------------------------------------------------------------------ the top-k rule
def topk_model(p: np.ndarray, k: int):
    """values [B, k], indices [B, k] by the rule of include/salun.h: larger first, NaN above every number, equal values
    (NaNs among themselves, -0 and +0) by ascending index."""
    p = np.asarray(p, np.float32)
    vals, idx = np.empty((p.shape[0], k), np.float32), np.empty((p.shape[0], k), np.int64)
    for b, row in enumerate(p):
        key = np.where(np.isnan(row), np.inf, row.astype(np.float64))      # NaN above +inf: give +inf a lower key
        key = np.where(np.isposinf(row), np.finfo(np.float64).max, key)
        order = sorted(range(row.size), key=lambda i: (-key[i], i))[:k]
        idx[b], vals[b] = order, row[order]
    return vals, idx


def topk_rows(K: int, kind: str, seed: int = 0) -> np.ndarray:
    """[4, K] fp32 rows: `free` has no two equal values; `ties` has few distinct values, +-0, +-inf and NaNs."""
    r = np.random.default_rng(seed + K)
    if kind == "free":
        return np.stack([r.permutation(K).astype(np.float32) / K - 0.3 for _ in range(4)])
    pool = np.array([0.0, -0.0, 1.0, 1.0, -2.5, np.nan, np.nan, np.inf, -np.inf, 3e-40], np.float32)
    return pool[r.integers(0, pool.size, (4, K))]


# ------------------------------------------------------------------------------------------ the CSV writer
PROMPTS_CSV = ('case_number,prompt,evaluation_seed,class,note\n'
               '3,"a photo of a tench, in a lake",2915,tench,1.50\n'
               '1,an image of a church,4054,church,\n'
               '7,nothing was generated for this row,11,none,x\n'
               '3,"a second row with case ""3""",77,tench,2\n'
               '0,Image of a cassette player,3186,cassette player,0.25\n')
MERGE_NAMES = ["0_0.png", "0_1.png", "1_0.png", "3_0.png", "3_10.png", "3_2.jpg", "9_0.png"]      # sorted; 9: no prompt row
MERGE_TOPK = 2


@functools.lru_cache(None)
def merge_results():
    """(case_numbers, categories, indices, scores) for MERGE_NAMES: float32 scores with 1.0, a denormal, a 9-digit
    value, and ordinary ones."""
    n = len(MERGE_NAMES)
    scores = np.array([[1.0, 0.0], [0.123456789, 1e-45], [0.5, 0.25], [0.99999994, 5.9604645e-08],
                       [0.7, 0.1], [3.0000001e-05, 1.17549435e-38], [0.33333334, 0.2]], np.float32)
    indices = np.array([[0, 482], [217, 1], [497, 999], [0, 391], [0, 758], [571, 2], [5, 6]], np.int64)
    categories = [[f"name {j}" if j != 482 else 'cassette player, "deck"' for j in row] for row in indices]
    cases = [int(nm.split("_")[0]) for nm in MERGE_NAMES]
    assert scores.shape == (n, MERGE_TOPK)
    return cases, categories, indices, scores


def merge_with_pandas() -> bytes:
    """The reference's statements on the fixture: pd.read_csv, astype("int"), pd.DataFrame, pd.merge, to_csv."""
    import pandas as pd
    cases, categories, indices, scores = merge_results()
    df = pd.read_csv(io.StringIO(PROMPTS_CSV), dtype=str, keep_default_na=False)     # cells as text: the script's rule
    df["case_number"] = df["case_number"].astype("int")
    d = {"case_number": cases}
    for k in range(1, MERGE_TOPK + 1):
        d[f"category_top{k}"] = [c[k - 1] for c in categories]
        d[f"index_top{k}"] = list(indices[:, k - 1])
        d[f"scores_top{k}"] = list(scores[:, k - 1])
    buf = io.StringIO()
    pd.merge(df, pd.DataFrame(d)).to_csv(buf)
    return buf.getvalue().encode()


# ------------------------------------------------------------------------------------------ the network
@functools.lru_cache(None)
def state_dict():
    from unlearn_saliency_amd.SD.resnet50 import standin_state_dict
    return standin_state_dict(WEIGHT_SEED)


@functools.lru_cache(None)
def models():
    """(fp32 module, float64 module) with the same state_dict, both in eval mode on the CPU."""
    from unlearn_saliency_amd.SD.resnet50 import resnet50
    m32, m64 = resnet50(), resnet50().double()
    m32.load_state_dict(state_dict())
    m64.load_state_dict(state_dict())
    return m32.eval(), m64.eval()


@functools.lru_cache(None)
def network_inputs(n, side):
    g = torch.Generator().manual_seed(200 + side)
    return torch.randn((n, 3, side, side), generator=g, dtype=torch.float32)


@functools.lru_cache(None)
def network_reference(n, side):
    """-> dict(l64, l32, figure = the library's max |logit - f64| / max |f64 logit|, bound = the device's absolute logit
    bound, p64, top = float64 top-5 indices, decided = [n, 5] bool: the float64 probability gap to the next rank exceeds
    the bound)."""
    m32, m64 = models()
    x = network_inputs(n, side)
    with torch.no_grad():
        l32, l64 = m32(x).double(), m64(x.double())
    peak = float(l64.abs().max())
    figure = float((l32 - l64).abs().max()) / peak
    bound = DEVICE_FACTOR * figure * peak
    p64 = torch.softmax(l64, -1)
    v, i = p64.topk(TOPK + 1, -1)
    return dict(l64=l64, l32=l32, figure=figure, bound=bound, p64=p64, top=i[:, :TOPK],
                decided=(v[:, :TOPK] - v[:, 1:]) > bound)


# ------------------------------------------------------------------------------------------ end to end
CLI_NAMES = ["0_0.png", "0_1.png", "2_0.png", "2_3.png", "5_0.png", "5_12.png"]
CLI_PROMPTS = ("case_number,prompt,evaluation_seed\n0,first prompt,1\n2,\"second, with a comma\",2\n"
               "4,a row without images,3\n5,third prompt,4\n")


@functools.lru_cache(None)
def cli_images():
    """Six uint8 images: four of 40 x 40 and two of 36 x 52 (two size groups), smooth random fields."""
    r = np.random.default_rng(7)
    out = []
    for i in range(6):
        h, w = (40, 40) if i % 3 != 2 else (36, 52)
        coarse = r.integers(0, 256, (-(-h // 8), -(-w // 8), 3)).astype(np.float64)
        img = np.kron(coarse, np.ones((8, 8, 1)))[:h, :w] + r.normal(0, 12, (h, w, 3))
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out
