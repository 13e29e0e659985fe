"""The text side of the Stable-Diffusion front-ends: prompts -> (B, 77, 768) contexts, as the reference's
`FrozenCLIPEmbedder.forward` (SD/ldm/modules/encoders/modules.py) computes them on every fetch —
`CLIPTokenizer(text, truncation=True, max_length=77, padding="max_length")` and then
`CLIPTextModel(input_ids=tokens).last_hidden_state`.

  ClipTokenizerLite(dir_or_files)  the byte-level BPE tokenizer of CLIP from the user's `vocab.json` and `merges.txt`
                                   (standard library only).  The two files are not bundled: they are the user's to name.
  ClipTextLite(config)             the module tree under transformers' names, so an SD-v1 checkpoint's
                                   `cond_stage_model.transformer.*` entries load with `load_compvis`.  Its `forward`
                                   runs the library's ops (any device, any dtype): the yardstick of the tests and of
                                   tools/clip_text_bench.py, not the path a user runs.
  TextPlan(model)                  that path: fp32, forward only, on K29 (ops_clip.py) and the K15 GEMM.  Per layer
                                     LN -> qkv GEMM (one job on a [3W, W] weight image built here, once)
                                        -> causal attention (reads the fused buffer in place)
                                        -> out_proj GEMM, accumulate=True into the residual stream
                                     LN -> fc1 GEMM -> quick-GELU in place -> fc2 GEMM, accumulate=True
                                   then the final LayerNorm: 8 launches a layer, no residual-add launch, no copy.
                                   The plan copies q / k / v weights: re-plan after loading other weights.
  contexts_for(...)                the helper the command lines share: {prompt: (1, 77, W)} for a list of prompts.

Out of scope: the OpenCLIP / SD-v2 text tower, the T5 embedder, `ftfy`-style text repair, literal special-token strings
inside a prompt, training the text encoder, bf16.
"""
from __future__ import annotations

import json
import os
import unicodedata
from typing import Dict, Iterable, List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

MAX_LENGTH = 77
BOS, EOS = "<|startoftext|>", "<|endoftext|>"
V1_TEXT_CONFIG = dict(vocab_size=49408, width=768, layers=12, heads=12, mlp=3072, positions=77, eps=1e-5)
CKPT_PREFIX = "cond_stage_model.transformer."
# How many layers of a TextPlan pass went to a library op instead of a kernel of this package.  No layer has such a
# route — outside a kernel's domain the plan raises — so every entry stays 0; tests and front-ends assert that.
LIBRARY_TEXT_CALLS = {"embed": 0, "layer_norm": 0, "linear": 0, "attention": 0, "quick_gelu": 0}
TOKENIZER_HINT = ("--tokenizer DIR names the folder with the CLIP tokenizer's vocab.json and merges.txt; with it and "
                  "--ckpt_path the script encodes its own prompts (SD/clip_text.py).")


# ------------------------------------------------------------------------------------------------------ the tokenizer
def bytes_to_unicode() -> Dict[int, str]:
    """The byte -> printable character table of byte-level BPE: printable Latin-1 bytes stand for themselves, the
    other 68 are moved to U+0100 onward in byte order."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    table, n = {b: chr(b) for b in keep}, 0
    for b in range(256):
        if b not in table:
            table[b] = chr(256 + n)
            n += 1
    return table


# the White_Space property (what `\s` means in the tokenizer's regular expressions)
_SPACE = frozenset("\t\n\x0b\x0c\r \x85\xa0\u1680\u2028\u2029\u202f\u205f\u3000" + "".join(chr(c) for c in range(0x2000, 0x200B)))
_CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")   # in the pattern's order (leftmost alternative wins)


def _kind(ch: str) -> str:
    if ch in _SPACE:
        return "s"
    cat = unicodedata.category(ch)[0]
    return cat if cat in "LN" else "o"


def split_words(text: str) -> List[str]:
    """The matches of  's|'t|'re|'ve|'m|'ll|'d|[\\p{L}]+|[\\p{N}]|[^\\s\\p{L}\\p{N}]+  in `text`, scanned by hand from
    the Unicode categories (`re` has no \\p): a contraction, a run of letters, ONE digit, or a run of anything else that
    is not white space."""
    out, i, n = [], 0, len(text)
    while i < n:
        hit = next((c for c in _CONTRACTIONS if text.startswith(c, i)), None)
        if hit:
            out.append(hit)
            i += len(hit)
            continue
        k = _kind(text[i])
        if k == "s":
            i += 1
        elif k == "N":
            out.append(text[i])
            i += 1
        else:
            j = i + 1
            while j < n and _kind(text[j]) == k:
                j += 1
            out.append(text[i:j])
            i = j
    return out


class ClipTokenizerLite:
    """`CLIPTokenizer` of transformers on the user's files: NFC, white-space runs -> one space (and strip), lower case,
    the split above, bytes -> characters, BPE with the `</w>` end-of-word suffix (merge rank = line order of merges.txt),
    unknown tokens -> `<|endoftext|>`."""

    def __init__(self, source, merges: Optional[str] = None):
        if merges is None:
            vocab_path, merges_path = os.path.join(os.fspath(source), "vocab.json"), os.path.join(os.fspath(source), "merges.txt")
        else:
            vocab_path, merges_path = os.fspath(source), os.fspath(merges)
        for p in (vocab_path, merges_path):
            if not os.path.isfile(p):
                raise FileNotFoundError(f"{p}: no such file.  The CLIP tokenizer needs two files, vocab.json and merges.txt "
                                        "(they are not part of this package; a transformers cache keeps them under "
                                        "models--openai--clip-vit-large-patch14/snapshots/*/)")
        with open(vocab_path, encoding="utf-8") as f:
            self.vocab: Dict[str, int] = json.load(f)
        with open(merges_path, encoding="utf-8") as f:
            lines = f.read().split("\n")
        if lines and lines[0].startswith("#version"):
            lines = lines[1:]
        pairs = [tuple(ln.split()) for ln in lines if ln.strip()]
        self.ranks = {p: i for i, p in enumerate(pairs) if len(p) == 2}
        for name in (BOS, EOS):
            if name not in self.vocab:
                raise ValueError(f"{vocab_path}: no `{name}` entry")
        self.bos_id, self.eos_id = self.vocab[BOS], self.vocab[EOS]
        self.vocab_size = max(self.vocab.values()) + 1
        self._bytes = bytes_to_unicode()
        self._cache: Dict[str, List[int]] = {}

    def _bpe(self, word: str) -> List[int]:
        got = self._cache.get(word)
        if got is not None:
            return got
        sym = list(word[:-1]) + [word[-1] + "</w>"]
        while len(sym) > 1:
            best, at = None, -1
            for i in range(len(sym) - 1):
                r = self.ranks.get((sym[i], sym[i + 1]))
                if r is not None and (best is None or r < best):
                    best, at = r, i
            if best is None:
                break
            a, b = sym[at], sym[at + 1]
            merged, i = [], 0
            while i < len(sym):
                if i < len(sym) - 1 and sym[i] == a and sym[i + 1] == b:
                    merged.append(a + b)
                    i += 2
                else:
                    merged.append(sym[i])
                    i += 1
            sym = merged
        ids = [self.vocab.get(s, self.eos_id) for s in sym]
        self._cache[word] = ids
        return ids

    def tokenize(self, text: str) -> List[int]:
        """The ids of `text` without BOS / EOS, not truncated."""
        text = unicodedata.normalize("NFC", text)
        text = "".join(" " if c in _SPACE else c for c in text)
        text = " ".join(p for p in text.split(" ") if p).lower()
        ids: List[int] = []
        for w in split_words(text):
            ids.extend(self._bpe("".join(self._bytes[b] for b in w.encode("utf-8"))))
        return ids

    def encode(self, texts, max_length: int = MAX_LENGTH) -> torch.Tensor:
        """-> int64 [B, max_length] on the host: BOS, at most max_length - 2 ids, EOS, then padding with the EOS id."""
        if isinstance(texts, str):
            texts = [texts]
        out = torch.full((len(texts), max_length), self.eos_id, dtype=torch.int64)
        for b, t in enumerate(texts):
            ids = [self.bos_id] + self.tokenize(t)[:max_length - 2] + [self.eos_id]
            out[b, :len(ids)] = torch.tensor(ids, dtype=torch.int64)
        return out


# ------------------------------------------------------------------------------------------------------ the module tree
class _Attention(nn.Module):
    def __init__(self, w: int):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(w, w) for _ in range(4))


class _MLP(nn.Module):
    def __init__(self, w: int, m: int):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(w, m), nn.Linear(m, w)


class _Layer(nn.Module):
    def __init__(self, w: int, m: int, eps: float):
        super().__init__()
        self.self_attn = _Attention(w)
        self.layer_norm1 = nn.LayerNorm(w, eps=eps)
        self.mlp = _MLP(w, m)
        self.layer_norm2 = nn.LayerNorm(w, eps=eps)


class _Embeddings(nn.Module):
    def __init__(self, vocab: int, w: int, positions: int):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab, w)
        self.position_embedding = nn.Embedding(positions, w)


class _Encoder(nn.Module):
    def __init__(self, n: int, w: int, m: int, eps: float):
        super().__init__()
        self.layers = nn.ModuleList(_Layer(w, m, eps) for _ in range(n))


class _TextModel(nn.Module):
    def __init__(self, c: dict):
        super().__init__()
        self.embeddings = _Embeddings(c["vocab_size"], c["width"], c["positions"])
        self.encoder = _Encoder(c["layers"], c["width"], c["mlp"], c["eps"])
        self.final_layer_norm = nn.LayerNorm(c["width"], eps=c["eps"])


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


class ClipTextLite(nn.Module):
    """transformers' CLIPTextModel (pre-LayerNorm blocks, causal self-attention, quick-GELU) under its parameter names:
    `text_model.embeddings.token_embedding.weight`, ..., `text_model.final_layer_norm.bias`."""

    def __init__(self, config: Optional[dict] = None):
        super().__init__()
        self.config = dict(V1_TEXT_CONFIG, **(config or {}))
        c = self.config
        if c["width"] % c["heads"]:
            raise ValueError(f"ClipTextLite: width {c['width']} is no multiple of {c['heads']} heads")
        self.text_model = _TextModel(c)

    @classmethod
    def v1(cls) -> "ClipTextLite":
        """The ViT-L/14 text tower of SD v1: 123,060,480 parameters."""
        return cls(V1_TEXT_CONFIG)

    def forward(self, ids: torch.Tensor) -> torch.Tensor:
        """ids int64 [B, T] -> last_hidden_state [B, T, W], on the library's ops."""
        tm, c = self.text_model, self.config
        B, T = ids.shape
        H, D = c["heads"], c["width"] // c["heads"]
        x = tm.embeddings.token_embedding(ids) + tm.embeddings.position_embedding.weight[:T]
        for lyr in tm.encoder.layers:
            a = lyr.self_attn
            h = lyr.layer_norm1(x)
            q, k, v = (p(h).view(B, T, H, D).transpose(1, 2) for p in (a.q_proj, a.k_proj, a.v_proj))
            o = F.scaled_dot_product_attention(q, k, v, is_causal=True, scale=D ** -0.5)
            x = x + a.out_proj(o.transpose(1, 2).reshape(B, T, H * D))
            x = x + lyr.mlp.fc2(quick_gelu(lyr.mlp.fc1(lyr.layer_norm2(x))))
        return tm.final_layer_norm(x)

    def load_compvis(self, source) -> "ClipTextLite":
        """`source`: a path or a dict; an SD-v1 CompVis checkpoint (["state_dict"], keys under
        `cond_stage_model.transformer.`) or a bare CLIPTextModel state dict.  The `position_ids` buffer old checkpoints
        carry is ignored; a missing or mis-shaped key is an error that names it."""
        sd = torch.load(source, map_location="cpu", weights_only=False) if isinstance(source, (str, bytes)) or \
            hasattr(source, "__fspath__") else source
        sd = sd.get("state_dict", sd)
        if any(k.startswith(CKPT_PREFIX) for k in sd):
            sd = {k[len(CKPT_PREFIX):]: v for k, v in sd.items() if k.startswith(CKPT_PREFIX)}
        sd = {k: v for k, v in sd.items() if not k.endswith("embeddings.position_ids")}
        own = self.state_dict()
        for k, t in own.items():
            if k not in sd:
                raise KeyError(f"load_compvis: the checkpoint has no `{k}`")
            if tuple(sd[k].shape) != tuple(t.shape):
                raise ValueError(f"load_compvis: `{k}` has shape {tuple(sd[k].shape)}, the text model needs {tuple(t.shape)}")
        extra = sorted(k for k in set(sd) - set(own) if k.startswith("text_model."))
        if extra:
            raise KeyError(f"load_compvis: unexpected key `{extra[0]}`" + (f" (and {len(extra) - 1} more)" if len(extra) > 1 else ""))
        self.load_state_dict({k: sd[k] for k in own})
        return self


# ------------------------------------------------------------------------------------------------------ the plan
class TextPlan:
    """The forward of `model` (a ClipTextLite on a ROCm device, fp32) on K29 and K15.  Heads must be 64 wide (K29's
    attention) and the width a multiple of 4; anything else is an error, never a library call."""

    def __init__(self, model: ClipTextLite):
        from .. import ops_clip
        p = next(model.parameters())
        if not p.is_cuda or p.dtype != torch.float32:
            raise RuntimeError("TextPlan: the model must be fp32 on a ROCm device (no CPU path)")
        c = model.config
        self.model, self.device = model, p.device
        self.W, self.H, self.F = c["width"], c["heads"], c["mlp"]
        if self.W // self.H != ops_clip.ATTN_D:
            raise ValueError(f"TextPlan: heads of {self.W // self.H} channels; the attention kernel serves {ops_clip.ATTN_D}")
        if c["positions"] > ops_clip.ATTN_MAX_T:
            raise ValueError(f"TextPlan: {c['positions']} positions; the attention kernel serves {ops_clip.ATTN_MAX_T}")
        # the fused projection: rows [0, W) = q_proj, [W, 2W) = k_proj, [2W, 3W) = v_proj
        self._qkv = []
        with torch.no_grad():
            for lyr in model.text_model.encoder.layers:
                a = lyr.self_attn
                self._qkv.append((torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]).contiguous(),
                                  torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]).contiguous()))
        self.launches = 0          # kernel calls of the last forward (the GEMM may add a fold launch of its own)

    @torch.no_grad()
    def forward(self, ids: torch.Tensor) -> torch.Tensor:
        """ids int64 [B, T] (host or device) -> last_hidden_state [B, T, W] on the device."""
        from .. import gemm, ops_clip
        tm, c = self.model.text_model, self.model.config
        B, T = (int(v) for v in ids.shape)
        if T > c["positions"]:
            raise ValueError(f"TextPlan: {T} tokens, the model has {c['positions']} positions")
        if ids.is_cuda:
            ops_clip.check_ids(ids, c["vocab_size"])
        M, W, dev = B * T, self.W, self.device
        x = ops_clip.clip_embed(ids, tm.embeddings.token_embedding.weight, tm.embeddings.position_embedding.weight).view(M, W)
        h = torch.empty((M, W), dtype=torch.float32, device=dev)
        qkv = torch.empty((M, 3 * W), dtype=torch.float32, device=dev)
        o = torch.empty((M, W), dtype=torch.float32, device=dev)
        u = torch.empty((M, self.F), dtype=torch.float32, device=dev)
        scale = float(ops_clip.ATTN_D) ** -0.5
        n = 1
        for lyr, (wqkv, bqkv) in zip(tm.encoder.layers, self._qkv):
            ops_clip.ln_f32_forward(x, lyr.layer_norm1.weight, lyr.layer_norm1.bias, lyr.layer_norm1.eps, out=h)
            gemm.mm_nt(h, wqkv, out=qkv, bias=bqkv)
            ops_clip.attn_causal_f32(qkv, B, T, self.H, scale, out=o)
            gemm.mm_nt(o, lyr.self_attn.out_proj.weight, out=x, bias=lyr.self_attn.out_proj.bias, accumulate=True)
            ops_clip.ln_f32_forward(x, lyr.layer_norm2.weight, lyr.layer_norm2.bias, lyr.layer_norm2.eps, out=h)
            gemm.mm_nt(h, lyr.mlp.fc1.weight, out=u, bias=lyr.mlp.fc1.bias)
            ops_clip.quick_gelu_(u)
            gemm.mm_nt(u, lyr.mlp.fc2.weight, out=x, bias=lyr.mlp.fc2.bias, accumulate=True)
            n += 8
        y = ops_clip.ln_f32_forward(x, tm.final_layer_norm.weight, tm.final_layer_norm.bias, tm.final_layer_norm.eps, out=h)
        self.launches = n + 1
        return y.view(B, T, W)

    def encode(self, texts: Sequence[str], tokenizer: ClipTokenizerLite) -> torch.Tensor:
        """prompts -> (B, 77, W) on the device."""
        return self.forward(tokenizer.encode(list(texts), MAX_LENGTH))

    def cond_stage(self, tokenizer: ClipTokenizerLite):
        """A callable for LatentDiffusionLite(cond_stage=...): a batch's "txt" entry (a string or a list of strings) ->
        its contexts, computed on every fetch as the reference does."""
        def encode(txt):
            return self.encode([txt] if isinstance(txt, str) else list(txt), tokenizer)
        return encode


# ------------------------------------------------------------------------------------------------------ front-ends
def synthetic_config(width: int, vocab_size: int) -> dict:
    """The text model of the `--synthetic` runs: seeded weights, two layers, 64-wide heads, the given context width."""
    return dict(vocab_size=int(vocab_size), width=int(width), layers=2, heads=max(1, int(width) // 64), mlp=4 * int(width),
                positions=MAX_LENGTH, eps=1e-5)


def build_plan(tokenizer_dir: str, ckpt_path: Optional[str], device, synthetic: Optional[dict] = None, seed: int = 0):
    """-> (TextPlan, ClipTokenizerLite).  With `synthetic` (a config, see synthetic_config) the weights are seeded and
    no checkpoint is read; else the text model comes from the SD-v1 checkpoint at `ckpt_path`."""
    tok = ClipTokenizerLite(tokenizer_dir)
    if synthetic is not None:
        cfg = dict(synthetic)
        cfg["vocab_size"] = max(int(cfg.get("vocab_size", 0)), tok.vocab_size)
        with torch.random.fork_rng():
            torch.manual_seed(seed)
            model = ClipTextLite(cfg)
    else:
        if not ckpt_path or not os.path.exists(ckpt_path):
            raise SystemExit(f"--ckpt_path {ckpt_path}: no such file (the text model's weights are its "
                             f"`{CKPT_PREFIX}*` entries)")
        model = ClipTextLite.v1().load_compvis(ckpt_path)
        if tok.vocab_size > model.config["vocab_size"]:
            raise SystemExit(f"--tokenizer: a vocabulary of {tok.vocab_size} entries, the text model embeds "
                             f"{model.config['vocab_size']}")
    model = model.to(device).float().requires_grad_(False).eval()
    return TextPlan(model), tok


def contexts_for(prompts: Iterable[str], tokenizer_dir: str, ckpt_path: Optional[str], device,
                 synthetic: Optional[dict] = None, seed: int = 0, batch: int = 8) -> Dict[str, torch.Tensor]:
    """{prompt: (1, 77, W) device tensor} for "" and every prompt, in the form the `--contexts` files have."""
    plan, tok = build_plan(tokenizer_dir, ckpt_path, device, synthetic, seed)
    todo = [""] + [p for p in dict.fromkeys(prompts) if p != ""]
    out: Dict[str, torch.Tensor] = {}
    for i in range(0, len(todo), batch):
        part = todo[i:i + batch]
        ctx = plan.encode(part, tok)
        for j, p in enumerate(part):
            out[p] = ctx[j:j + 1].clone()
    if any(LIBRARY_TEXT_CALLS.values()):
        raise RuntimeError(f"the text encoder left the package's kernels: {LIBRARY_TEXT_CALLS}")
    return out
