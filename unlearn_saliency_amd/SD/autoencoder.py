"""The encoder side of the Stable-Diffusion first stage (the reference's `AutoencoderKL`, ldm/models/autoencoder.py, with
the `Encoder` of ldm/modules/diffusionmodules/model.py:379-493) and its posterior, on this package's kernels.

`AutoencoderKLLite` is the module tree: the same attribute names, so `state_dict()` has the reference's keys
(`encoder.*`, `quant_conv.*`) and a CompVis checkpoint loads with `load_compvis`.  Its own `forward` runs the library's
ops (any device, any dtype): it is the yardstick of the tests and of tools/vae_bench.py, not the path a user runs.

`EncoderPlan(model)` is that path.  It is forward only and fp32, as the reference runs its frozen first stage:
  * every Conv2d is one K27 launch (conv_infer.conv_bn_act, shift = bias); the residual add rides as conv2's addend,
    the 1 x 1 nin_shortcut is computed first;
  * every GroupNorm(32, eps 1e-6) (+ SiLU) is one K28 call (norm.gn_split_act: two launches);
  * Downsample (F.pad(x, (0, 1, 0, 1)) + conv 3 x 3 / 2, padding 0) is one K27 launch with pad = 0 and P = H / 2: the
    taps past the high edge read zero;
  * three layers are outside K27's domain and are brought inside by zero-padding operands once, when the plan is made:
        conv_in     C = 3  -> 8   (weight columns; the input is written into a zeroed 8-channel buffer)
        conv_out    K = 8  -> 32  (weight rows and bias)
        quant_conv  K = 8  -> 32, C = 8 -> 32 (it reads conv_out's padded output in place)
    the posterior kernel reads the moments from the padded tensor;
  * mid.attn_1 (one head, d = C, scale C^-0.5): q / k / v / proj_out on K27, the product by the rule of
    DDPM/models/diffusion.py — gemm.attention_f32 (K15) up to 512 x 512 scores, the library's fused attention past
    that (64 x 64 latents = 4096 tokens take the library route; gemm.py measured it faster there).
The plan copies the weights it pads: re-plan after loading other weights into the model.

Out of scope: bf16 (the decoder is below; the CLIP text encoder is SD/clip_text.py).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

V1_DDCONFIG = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=(1, 2, 4, 4),
                   num_res_blocks=2, attn_resolutions=(), dropout=0.0)
V1_EMBED_DIM = 4
SCALE_FACTOR = 0.18215
GN_GROUPS, GN_EPS = 32, 1e-6
IGNORED_PREFIXES = ("decoder.", "post_quant_conv.", "loss.", "model_ema.")
# how many attention products of EncoderPlan went to "k15" (gemm.attention_f32) and to the "library" (fused attention)
ATTENTION_ROUTES = {"k15": 0, "library": 0}


def _norm(c: int) -> nn.GroupNorm:
    return nn.GroupNorm(GN_GROUPS, c, eps=GN_EPS, affine=True)


def _swish(x):
    return x * torch.sigmoid(x)


class ResnetBlock(nn.Module):
    """norm1 -> swish -> conv1 -> norm2 -> swish -> conv2, plus the input (through a 1 x 1 conv when the width changes)."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.norm1, self.conv1 = _norm(cin), nn.Conv2d(cin, cout, 3, 1, 1)
        self.norm2, self.conv2 = _norm(cout), nn.Conv2d(cout, cout, 3, 1, 1)
        if cin != cout:
            self.nin_shortcut = nn.Conv2d(cin, cout, 1)

    def forward(self, x):
        h = self.conv2(_swish(self.norm2(self.conv1(_swish(self.norm1(x))))))
        return (self.nin_shortcut(x) if hasattr(self, "nin_shortcut") else x) + h


class AttnBlock(nn.Module):
    """One-head self-attention over the H * W positions, width C."""

    def __init__(self, c: int):
        super().__init__()
        self.norm = _norm(c)
        self.q, self.k, self.v, self.proj_out = (nn.Conv2d(c, c, 1) for _ in range(4))

    def forward(self, x):
        b, c, hh, ww = x.shape
        h = self.norm(x)
        q, k, v = (m(h).reshape(b, c, hh * ww) for m in (self.q, self.k, self.v))
        p = torch.softmax(torch.bmm(q.transpose(1, 2), k) * (int(c) ** -0.5), dim=2)
        return x + self.proj_out(torch.bmm(v, p.transpose(1, 2)).reshape(b, c, hh, ww))


class Downsample(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 2, 0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1)))


class _Bag(nn.Module):
    """A container for the attribute names of the reference (.block, .attn, .downsample; .block_1, .attn_1, .block_2)."""


class Encoder(nn.Module):
    def __init__(self, *, ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions=(), in_channels=3, resolution,
                 z_channels, double_z=True, **ignored):
        super().__init__()
        self.ch, self.in_channels, self.resolution = ch, in_channels, resolution
        self.num_resolutions, self.num_res_blocks = len(ch_mult), num_res_blocks
        self.conv_in = nn.Conv2d(in_channels, ch, 3, 1, 1)
        self.down = nn.ModuleList()
        res, cin = resolution, ch
        for i, m in enumerate(ch_mult):
            lvl = _Bag()
            lvl.block, lvl.attn = nn.ModuleList(), nn.ModuleList()
            for _ in range(num_res_blocks):
                lvl.block.append(ResnetBlock(cin, ch * m))
                cin = ch * m
                if res in attn_resolutions:
                    lvl.attn.append(AttnBlock(cin))
            if i != len(ch_mult) - 1:
                lvl.downsample = Downsample(cin)
                res //= 2
            self.down.append(lvl)
        self.mid = _Bag()
        self.mid.block_1, self.mid.attn_1, self.mid.block_2 = ResnetBlock(cin, cin), AttnBlock(cin), ResnetBlock(cin, cin)
        self.norm_out = _norm(cin)
        self.conv_out = nn.Conv2d(cin, 2 * z_channels if double_z else z_channels, 3, 1, 1)

    def forward(self, x):
        h = self.conv_in(x)
        for i, lvl in enumerate(self.down):
            for j, blk in enumerate(lvl.block):
                h = blk(h)
                if len(lvl.attn):
                    h = lvl.attn[j](h)
            if i != self.num_resolutions - 1:
                h = lvl.downsample(h)
        h = self.mid.block_2(self.mid.attn_1(self.mid.block_1(h)))
        return self.conv_out(_swish(self.norm_out(h)))


class AutoencoderKLLite(nn.Module):
    """`encoder` + `quant_conv` of AutoencoderKL.  `forward(x)` = the moments [B, 2 embed_dim, h, w] on library ops."""

    def __init__(self, ddconfig: Optional[dict] = None, embed_dim: int = V1_EMBED_DIM):
        super().__init__()
        self.ddconfig = dict(ddconfig or V1_DDCONFIG)
        if not self.ddconfig.get("double_z", True):
            raise ValueError("AutoencoderKLLite: the KL autoencoder has double_z = True")
        self.embed_dim = int(embed_dim)
        self.encoder = Encoder(**self.ddconfig)
        self.quant_conv = nn.Conv2d(2 * self.ddconfig["z_channels"], 2 * self.embed_dim, 1)
        self.requires_grad_(False).eval()

    def forward(self, x):
        return self.quant_conv(self.encoder(x))

    def load_compvis(self, source) -> "AutoencoderKLLite":
        """`source`: a path or a dict; an SD-v1 CompVis checkpoint (["state_dict"], keys under `first_stage_model.`) or
        a bare autoencoder state dict.  Decoder, post_quant_conv, loss and EMA keys are ignored; a missing or mis-shaped
        encoder key is an error that names it."""
        sd = torch.load(source, map_location="cpu", weights_only=False) if isinstance(source, (str, bytes)) or \
            hasattr(source, "__fspath__") else source
        sd = sd.get("state_dict", sd)
        pre = "first_stage_model."
        if any(k.startswith(pre) for k in sd):
            sd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        sd = {k: v for k, v in sd.items() if not k.startswith(IGNORED_PREFIXES)}
        own = self.state_dict()
        for k, t in own.items():
            if k not in sd:
                raise KeyError(f"load_compvis: the checkpoint has no `{k}`")
            if tuple(sd[k].shape) != tuple(t.shape):
                raise ValueError(f"load_compvis: `{k}` has shape {tuple(sd[k].shape)}, the encoder needs {tuple(t.shape)}")
        extra = sorted(set(sd) - set(own))
        if extra:
            raise KeyError(f"load_compvis: unexpected key `{extra[0]}`" + (f" (and {len(extra) - 1} more)" if len(extra) > 1 else ""))
        self.load_state_dict({k: sd[k] for k in own})
        return self


def _ceil_to(n: int, m: int) -> int:
    return -(-n // m) * m


class EncoderPlan:
    """The encoder of `model` (an AutoencoderKLLite on a ROCm device, fp32) on K27 / K28 / K15 and the posterior kernel.
    Owns zero-padded copies of the three weights K27 needs padded (see the module docstring), made once here."""

    def __init__(self, model: AutoencoderKLLite):
        p = next(model.parameters())
        if not p.is_cuda or p.dtype != torch.float32:
            raise RuntimeError("EncoderPlan: the model must be fp32 on a ROCm device (no CPU path)")
        self.model, self.device = model, p.device
        enc = model.encoder
        self.zc = model.embed_dim
        self.cin, self.cin_pad = enc.in_channels, _ceil_to(enc.in_channels, 8)
        self.factor = 2 ** (enc.num_resolutions - 1)
        km = _ceil_to(enc.conv_out.out_channels, 32)
        self.cm = _ceil_to(model.quant_conv.out_channels, 32)
        self._padded = {id(enc.conv_in): self._pad(enc.conv_in, self.cin_pad, enc.conv_in.out_channels),
                        id(enc.conv_out): self._pad(enc.conv_out, enc.conv_out.in_channels, km),
                        id(model.quant_conv): self._pad(model.quant_conv, km, self.cm)}
        self._table = None
        self._counter = 0

    @staticmethod
    def _pad(conv: nn.Conv2d, C: int, K: int):
        w = torch.zeros((K, C) + tuple(conv.weight.shape[2:]), dtype=torch.float32, device=conv.weight.device)
        w[:conv.out_channels, :conv.in_channels] = conv.weight.detach()
        b = torch.zeros(K, dtype=torch.float32, device=conv.weight.device)
        b[:conv.out_channels] = conv.bias.detach()
        return w, b

    # ---- layers
    def _conv(self, conv: nn.Conv2d, x, addend=None, stride=1, pad=None, out_size=None):
        from .. import conv_infer
        w, b = self._padded.get(id(conv)) or (conv.weight, conv.bias)
        pad = conv.padding[0] if pad is None else pad
        return conv_infer.conv_bn_act(x, w, None, b, addend, False, stride, pad, out_size=out_size)

    @staticmethod
    def _gn(gn: nn.GroupNorm, x, silu: bool):
        from .. import norm
        return norm.gn_split_act(x, gn, silu)

    def _res(self, blk: ResnetBlock, x):
        h = self._conv(blk.conv1, self._gn(blk.norm1, x, True))
        h = self._gn(blk.norm2, h, True)
        skip = self._conv(blk.nin_shortcut, x) if hasattr(blk, "nin_shortcut") else x
        return self._conv(blk.conv2, h, addend=skip)

    def _attn(self, blk: AttnBlock, x):
        b, c, hh, ww = x.shape
        h = self._gn(blk.norm, x, False)
        tok = lambda t: t.reshape(b, 1, c, hh * ww).transpose(2, 3)       # [b, 1, hw, c] views of the NCHW outputs
        q, k, v = (tok(self._conv(m, h)) for m in (blk.q, blk.k, blk.v))
        o = self._product(q, k, v, float(c) ** -0.5).transpose(2, 3).reshape(b, c, hh, ww).contiguous()
        return self._conv(blk.proj_out, o, addend=x)

    @staticmethod
    def _product(q, k, v, scale: float):
        """softmax(scale q k^T) v of [b, 1, hw, c] views: K15 up to 512 x 512 scores, the library's fused attention past it."""
        from .. import gemm
        if gemm.attention_supported(q, k, v):
            ATTENTION_ROUTES["k15"] += 1
            return gemm.attention_f32(q, k, v, scale)
        ATTENTION_ROUTES["library"] += 1
        return F.scaled_dot_product_attention(q, k, v, scale=scale)

    # ---- inputs
    def _input(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 [B, cin, H, W] or uint8 [B, H, W, cin] -> the zero-padded fp32 [B, cin_pad, H, W] conv_in reads."""
        from .. import conv_infer, ops_infer
        if x.dtype == torch.uint8:
            B, H, W, C = x.shape
        else:
            B, C, H, W = x.shape
        if C != self.cin:
            raise ValueError(f"EncoderPlan: {C} input channels, the encoder takes {self.cin}")
        if H % self.factor or W % self.factor:
            raise ValueError(f"EncoderPlan: {H} x {W} is no multiple of the encoder's down-sampling factor {self.factor}")
        buf = torch.zeros((B, self.cin_pad, H, W), dtype=torch.float32, device=self.device)
        if x.dtype == torch.uint8:
            if self._table is None:
                self._table = ops_infer.u8_norm_table([0.5] * C, [0.5] * C).to(self.device)
            x = x.to(self.device)
            for i in range(B):                     # an image's first planes are contiguous in the padded buffer
                conv_infer.u8_to_chw_norm(x[i:i + 1], self._table, out=buf[i, :C])
        else:
            buf[:, :C] = x.to(self.device, torch.float32)
        return buf

    # ---- public
    @torch.no_grad()
    def encode_moments_padded(self, x: torch.Tensor) -> torch.Tensor:
        """-> [B, Cm, h, w], Cm = 2 embed_dim rounded up to K27's multiple of 32; channels past 2 embed_dim are zero."""
        m, enc = self.model, self.model.encoder
        h = self._conv(enc.conv_in, self._input(x))
        for i, lvl in enumerate(enc.down):
            for j, blk in enumerate(lvl.block):
                h = self._res(blk, h)
                if len(lvl.attn):
                    h = self._attn(lvl.attn[j], h)
            if i != enc.num_resolutions - 1:
                h = self._conv(lvl.downsample.conv, h, stride=2, pad=0, out_size=(h.shape[2] // 2, h.shape[3] // 2))
        h = self._res(enc.mid.block_2, self._attn(enc.mid.attn_1, self._res(enc.mid.block_1, h)))
        h = self._conv(enc.conv_out, self._gn(enc.norm_out, h, True))
        return self._conv(m.quant_conv, h)

    def encode_moments(self, x: torch.Tensor) -> torch.Tensor:
        """-> [B, 2 embed_dim, h, w]: mean and log-variance of the posterior."""
        return self.encode_moments_padded(x)[:, :2 * self.zc].contiguous()

    @torch.no_grad()
    def encode(self, x: torch.Tensor, image_ids, seed: int, draw: int = 0, deterministic: bool = False,
               scale: float = SCALE_FACTOR) -> torch.Tensor:
        """x: fp32 [B, 3, H, W] in [-1, 1] or uint8 [B, H, W, 3] -> z [B, embed_dim, H / f, W / f] = scale * a sample of
        the posterior (its mode with `deterministic`).  The noise of image b is keyed by (seed, image_ids[b], draw)."""
        from .. import ops_infer
        mom = self.encode_moments_padded(x)
        ids = None
        if not deterministic:
            ids = torch.as_tensor(image_ids, dtype=torch.int64).to(self.device).contiguous()
            if ids.numel() != mom.shape[0]:
                raise ValueError("encode: one image id per image")
        return ops_infer.vae_posterior_sample(mom, self.zc, ids, seed, draw, scale, deterministic)

    def first_stage(self, seed: int):
        """A callable for LatentDiffusionLite(first_stage=...): the UNSCALED posterior sample (get_input multiplies by
        scale_factor itself).  Image ids come from a running counter, so every fetch draws afresh, as the reference."""
        def encode(x):
            B = int(x.shape[0])
            ids = torch.arange(self._counter, self._counter + B, dtype=torch.int64)
            self._counter += B
            return self.encode(x, ids, seed, 0, False, 1.0)
        return encode


# ------------------------------------------------------------------------------------------------------ the decoder
# The other half of the first stage (the reference's `Decoder`, ldm/modules/diffusionmodules/model.py:496-625, behind
# `post_quant_conv`, as AutoencoderKL.decode chains them): what SD/eval-scripts/generate-images.py turns latents into
# images with.  `DecoderKLLite` is the module tree under the reference's names (`decoder.*`, `post_quant_conv.*`); its
# `forward` runs library ops and is the yardstick.  `DecoderPlan(model)` is the path a user runs, fp32 and forward only:
#   * Conv2d, GroupNorm(+SiLU), ResnetBlock and mid.attn_1 exactly as EncoderPlan runs them (K27 / K28 / K15);
#   * Upsample (F.interpolate(scale_factor=2, mode="nearest") + conv 3 x 3) is ONE launch of K27's up2 form
#     (conv_infer.conv_up2_bn_act): the gather reads x[ih >> 1][iw >> 1]; the four-fold tensor is never written;
#   * zero-padding, once, when the plan is made:
#         post_quant_conv  C = 4 -> 8, K = 4 -> 32  (the scaled latent is written into a zeroed 8-channel buffer)
#         conv_in          C = 4 -> 32              (it reads post_quant_conv's padded output in place)
#         conv_out         K = 3 -> 32              (decode_u8 reads the first three planes in place)
IGNORED_PREFIXES_DECODER = ("encoder.", "quant_conv.", "loss.", "model_ema.")


class Upsample(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 1, 1)

    def forward(self, x):
        return self.conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))


class Decoder(nn.Module):
    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions=(), in_channels=3,
                 resolution, z_channels, **ignored):
        super().__init__()
        self.ch, self.in_channels, self.resolution = ch, in_channels, resolution
        self.num_resolutions, self.num_res_blocks = len(ch_mult), num_res_blocks
        cin = ch * ch_mult[-1]
        res = resolution // 2 ** (self.num_resolutions - 1)
        self.conv_in = nn.Conv2d(z_channels, cin, 3, 1, 1)
        self.mid = _Bag()
        self.mid.block_1, self.mid.attn_1, self.mid.block_2 = ResnetBlock(cin, cin), AttnBlock(cin), ResnetBlock(cin, cin)
        levels = []
        for i in reversed(range(self.num_resolutions)):
            lvl = _Bag()
            lvl.block, lvl.attn = nn.ModuleList(), nn.ModuleList()
            for _ in range(num_res_blocks + 1):
                lvl.block.append(ResnetBlock(cin, ch * ch_mult[i]))
                cin = ch * ch_mult[i]
                if res in attn_resolutions:
                    lvl.attn.append(AttnBlock(cin))
            if i != 0:
                lvl.upsample = Upsample(cin)
                res *= 2
            levels.insert(0, lvl)                    # up[0] is the finest level, as in the reference
        self.up = nn.ModuleList(levels)
        self.norm_out = _norm(cin)
        self.conv_out = nn.Conv2d(cin, out_ch, 3, 1, 1)

    def forward(self, z):
        h = self.conv_in(z)
        h = self.mid.block_2(self.mid.attn_1(self.mid.block_1(h)))
        for i in reversed(range(self.num_resolutions)):
            lvl = self.up[i]
            for j, blk in enumerate(lvl.block):
                h = blk(h)
                if len(lvl.attn):
                    h = lvl.attn[j](h)
            if i != 0:
                h = lvl.upsample(h)
        return self.conv_out(_swish(self.norm_out(h)))


class DecoderKLLite(nn.Module):
    """`post_quant_conv` + `decoder` of AutoencoderKL.  `forward(z)` = the image [B, out_ch, f h, f w] of an UNSCALED
    latent on library ops."""

    def __init__(self, ddconfig: Optional[dict] = None, embed_dim: int = V1_EMBED_DIM):
        super().__init__()
        self.ddconfig = dict(ddconfig or V1_DDCONFIG)
        self.embed_dim = int(embed_dim)
        self.decoder = Decoder(**self.ddconfig)
        self.post_quant_conv = nn.Conv2d(self.embed_dim, self.ddconfig["z_channels"], 1)
        self.requires_grad_(False).eval()

    def forward(self, z):
        return self.decoder(self.post_quant_conv(z))

    def load_compvis(self, source) -> "DecoderKLLite":
        """`source`: a path or a dict; an SD-v1 CompVis checkpoint (["state_dict"], keys under `first_stage_model.`) or
        a bare autoencoder state dict.  Encoder, quant_conv, loss and EMA keys are ignored; a missing or mis-shaped
        decoder key is an error that names it."""
        sd = torch.load(source, map_location="cpu", weights_only=False) if isinstance(source, (str, bytes)) or \
            hasattr(source, "__fspath__") else source
        sd = sd.get("state_dict", sd)
        pre = "first_stage_model."
        if any(k.startswith(pre) for k in sd):
            sd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        sd = {k: v for k, v in sd.items() if not k.startswith(IGNORED_PREFIXES_DECODER)}
        own = self.state_dict()
        for k, t in own.items():
            if k not in sd:
                raise KeyError(f"load_compvis: the checkpoint has no `{k}`")
            if tuple(sd[k].shape) != tuple(t.shape):
                raise ValueError(f"load_compvis: `{k}` has shape {tuple(sd[k].shape)}, the decoder needs {tuple(t.shape)}")
        extra = sorted(set(sd) - set(own))
        if extra:
            raise KeyError(f"load_compvis: unexpected key `{extra[0]}`" + (f" (and {len(extra) - 1} more)" if len(extra) > 1 else ""))
        self.load_state_dict({k: sd[k] for k in own})
        return self


class DecoderPlan:
    """The decoder of `model` (a DecoderKLLite on a ROCm device, fp32) on K27 (plain and up2) / K28 / K15 and the
    byte kernel.  Owns zero-padded copies of the three weights K27 needs padded, made once here: re-plan after loading
    other weights into the model."""

    _pad = staticmethod(EncoderPlan._pad)
    _conv = EncoderPlan._conv
    _gn = staticmethod(EncoderPlan._gn)
    _res = EncoderPlan._res
    _attn = EncoderPlan._attn
    _product = staticmethod(EncoderPlan._product)

    def __init__(self, model: DecoderKLLite):
        p = next(model.parameters())
        if not p.is_cuda or p.dtype != torch.float32:
            raise RuntimeError("DecoderPlan: the model must be fp32 on a ROCm device (no CPU path)")
        self.model, self.device = model, p.device
        dec, pq = model.decoder, model.post_quant_conv
        self.zc, self.zc_pad = model.embed_dim, _ceil_to(model.embed_dim, 8)
        self.out_ch = dec.conv_out.out_channels
        self.factor = 2 ** (dec.num_resolutions - 1)
        kq = _ceil_to(pq.out_channels, 32)
        self._padded = {id(pq): self._pad(pq, self.zc_pad, kq),
                        id(dec.conv_in): self._pad(dec.conv_in, kq, dec.conv_in.out_channels),
                        id(dec.conv_out): self._pad(dec.conv_out, dec.conv_out.in_channels, _ceil_to(self.out_ch, 32))}

    def _up(self, up: Upsample, x):
        from .. import conv_infer
        return conv_infer.conv_up2_bn_act(x, up.conv.weight, None, up.conv.bias)

    @torch.no_grad()
    def decode_padded(self, z: torch.Tensor, scale: float = SCALE_FACTOR) -> torch.Tensor:
        """z [B, embed_dim, h, w] -> [B, Kp, f h, f w], Kp = out_ch rounded up to K27's multiple of 32; channels past
        out_ch are zero."""
        m, dec = self.model, self.model.decoder
        if z.dim() != 4 or z.shape[1] != self.zc:
            raise ValueError(f"DecoderPlan: a latent of shape {tuple(z.shape)}, the decoder takes [B, {self.zc}, h, w]")
        B, _, hh, ww = z.shape
        buf = torch.zeros((B, self.zc_pad, hh, ww), dtype=torch.float32, device=self.device)
        torch.mul(z.to(self.device, torch.float32), 1.0 / scale, out=buf[:, :self.zc])     # 1 / scale * z: one rounding
        h = self._conv(dec.conv_in, self._conv(m.post_quant_conv, buf))
        h = self._res(dec.mid.block_2, self._attn(dec.mid.attn_1, self._res(dec.mid.block_1, h)))
        for i in reversed(range(dec.num_resolutions)):
            lvl = dec.up[i]
            for j, blk in enumerate(lvl.block):
                h = self._res(blk, h)
                if len(lvl.attn):
                    h = self._attn(lvl.attn[j], h)
            if i != 0:
                h = self._up(lvl.upsample, h)
        return self._conv(dec.conv_out, self._gn(dec.norm_out, h, True))

    def decode(self, z: torch.Tensor, scale: float = SCALE_FACTOR) -> torch.Tensor:
        """z = scale * (a latent of the first stage) -> the image, fp32 [B, out_ch, f h, f w] in about [-1, 1]."""
        return self.decode_padded(z, scale)[:, :self.out_ch].contiguous()

    def decode_u8(self, z: torch.Tensor, scale: float = SCALE_FACTOR) -> torch.Tensor:
        """-> uint8 [B, f h, f w, out_ch] = round(clamp(image / 2 + 0.5, 0, 1) * 255), read from the padded output in place."""
        from .. import ops_infer
        return ops_infer.decoded_to_u8(self.decode_padded(z, scale), self.out_ch)
