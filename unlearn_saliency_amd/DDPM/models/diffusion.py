"""Class-conditional DDPM U-Net with classifier-free guidance, state_dict-compatible with the
reference's `Conditional_Model` (DDPM/models/diffusion.py:195-413).

Rebuilt from a level table so that `named_parameters()` yields the same 334 names, shapes and ORDER as
the reference — `null_classes_emb` first, then `temb.dense.*`, `classes_emb`,
`cemb.dense.*`, `conv_in`, `down.*`, `mid.*`, `up.*`, `norm_out`, `conv_out` — because that order is the
flat index the saliency ranking and the mask files are defined on, and so reference checkpoints
(`module.`-prefixed, saved from nn.DataParallel) load unchanged.

MI355X notes: spatial self-attention (256 tokens, one head of width C) goes through
`scaled_dot_product_attention` (one fused kernel on MFMA instead of bmm + softmax + bmm with a
materialised 256x256 score matrix per sample); everything else is MIOpen / rocBLAS via PyTorch-ROCm.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import draws
from ...norm import fused_gn_act


def prob_mask_like(shape, prob, device):
    """Bernoulli(prob) boolean mask; exact all-True / all-False at prob 1 / 0 (no RNG consumed)."""
    if prob == 1:
        return torch.ones(shape, device=device, dtype=torch.bool)
    if prob == 0:
        return torch.zeros(shape, device=device, dtype=torch.bool)
    return torch.zeros(shape, device=device).float().uniform_(0, 1) < prob


def get_timestep_embedding(timesteps: torch.Tensor, embedding_dim: int) -> torch.Tensor:
    """Sinusoidal embedding [sin | cos] with frequencies exp(-log(1e4) * i / (half-1))."""
    assert timesteps.dim() == 1
    half = embedding_dim // 2
    freq = torch.exp(torch.arange(half, dtype=torch.float32, device=timesteps.device) * -(math.log(10000) / (half - 1)))
    arg = timesteps.float()[:, None] * freq[None, :]
    emb = torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)
    if embedding_dim % 2 == 1:
        emb = F.pad(emb, (0, 1, 0, 0))
    return emb


def swish(x):
    return x * torch.sigmoid(x)


def group_norm(channels):
    return nn.GroupNorm(num_groups=32, num_channels=channels, eps=1e-6, affine=True)


class Upsample(nn.Module):
    def __init__(self, channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        if with_conv:
            self.conv = nn.Conv2d(channels, channels, 3, 1, 1)

    def forward(self, x):
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
        return self.conv(x) if self.with_conv else x


class Downsample(nn.Module):
    def __init__(self, channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        self.use_mfma = False  # set by conv.use_salun_convs(model)
        if with_conv:
            self.conv = nn.Conv2d(channels, channels, 3, 2, 0)  # asymmetric (0,1,0,1) padding applied by hand

    def forward(self, x):
        if not self.with_conv:
            return F.avg_pool2d(x, 2, 2)
        if self.use_mfma and x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled():
            x = x.contiguous()
            # the (0,1,0,1) zero padding is folded into the kernel: low-side pad 0, output size fixes the rest
            from ...conv import conv2d_lowpad
            return conv2d_lowpad(x, self.conv.weight, self.conv.bias, 2, 0, x.shape[2] // 2, x.shape[3] // 2)
        return self.conv(F.pad(x, (0, 1, 0, 1), mode="constant", value=0))


class ResnetBlock(nn.Module):
    """GN-swish-conv3x3, + Linear(swish([temb ‖ cemb])), GN-swish-dropout-conv3x3, 1x1 skip if widths differ."""

    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout, temb_channels=512,
                 cemb_channels=512):
        super().__init__()
        out_channels = in_channels if out_channels is None else out_channels
        self.in_channels, self.out_channels, self.use_conv_shortcut = in_channels, out_channels, conv_shortcut
        self.norm1 = group_norm(in_channels)
        self.conv1 = nn.Conv2d(in_channels, out_channels, 3, 1, 1)
        self.temb_cemb_proj = nn.Linear(temb_channels + cemb_channels, out_channels)
        self.norm2 = group_norm(out_channels)
        self.dropout = draws.CounterDropout(dropout)  # nn.Dropout whose draws follow the GLOBAL sample index (draws.py)
        self.conv2 = nn.Conv2d(out_channels, out_channels, 3, 1, 1)
        self.fused_node = False  # set by conv.use_salun_convs(model): the whole block as one autograd node
        if in_channels != out_channels:
            if conv_shortcut:
                self.conv_shortcut = nn.Conv2d(in_channels, out_channels, 3, 1, 1)
            else:
                self.nin_shortcut = nn.Conv2d(in_channels, out_channels, 1, 1, 0)

    def forward(self, x, emb_act, proj=None):
        """emb_act = swish([temb ‖ cemb]) — identical for every block, computed once per forward.
        proj: `self.temb_cemb_proj(emb_act)` when the model computed all blocks' projections in one grouped launch."""
        if self.fused_node:
            from ...resblock import fused_diffusion_resnet_block
            out = fused_diffusion_resnet_block(self, x, emb_act, proj)
            if out is not None:
                return out
        if proj is None:
            proj = self.temb_cemb_proj(emb_act)
        h = self.conv1(fused_gn_act(x, self.norm1, silu=True))  # swish(norm1(x)) as one kernel
        h = h + proj[:, :, None, None]
        h = self.conv2(self.dropout(fused_gn_act(h, self.norm2, silu=True)))
        if self.in_channels != self.out_channels:
            x = self.conv_shortcut(x) if self.use_conv_shortcut else self.nin_shortcut(x)
        return x + h


class AttnBlock(nn.Module):
    """Single-head spatial self-attention over H*W tokens of width C (1x1-conv projections)."""

    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        self.own_gemm = False  # set by conv.use_salun_convs(model): attention on this package's fp32 GEMM (K15)
        self.norm = group_norm(in_channels)
        self.q = nn.Conv2d(in_channels, in_channels, 1)
        self.k = nn.Conv2d(in_channels, in_channels, 1)
        self.v = nn.Conv2d(in_channels, in_channels, 1)
        self.proj_out = nn.Conv2d(in_channels, in_channels, 1)

    def forward(self, x):
        b, c, hh, ww = x.shape
        h = fused_gn_act(x, self.norm, silu=False)
        tok = lambda t: t.reshape(b, 1, c, hh * ww).transpose(2, 3)  # (b, 1, hw, c): channel-major memory, tokens contiguous
        q, k, v = tok(self.q(h)), tok(self.k(h)), tok(self.v(h))
        if self.own_gemm:
            from ... import gemm
            if gemm.attention_supported(q, k, v):
                # GEMM -> row softmax -> GEMM on the fp32 matrix-core kernel, reading q / k / v where the 1x1
                # convolutions left them and writing o straight back in NCHW (no transposing copy either side)
                o = gemm.attention_f32(q, k, v, float(c) ** -0.5)
                return x + self.proj_out(o.transpose(2, 3).reshape(b, c, hh, ww))
        o = F.scaled_dot_product_attention(q, k, v, scale=float(c) ** -0.5)
        o = o.transpose(2, 3).reshape(b, c, hh, ww).contiguous()  # back to NCHW (the reshape alone is a channels-last view)
        return x + self.proj_out(o)


class _Level(nn.Module):
    """Container with the attribute names the reference uses: .block, .attn, (.downsample | .upsample)."""


class Conditional_Model(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        mc, dc = config.model, config.data
        ch, out_ch, ch_mult = mc.ch, mc.out_ch, tuple(mc.ch_mult)
        nrb, attn_res, dropout = mc.num_res_blocks, mc.attn_resolutions, mc.dropout
        if mc.type == "bayesian":
            self.logvar = nn.Parameter(torch.zeros(config.diffusion.num_diffusion_timesteps))
        self.ch = ch
        self.temb_ch = self.cemb_ch = ch * 4
        self.num_resolutions, self.num_res_blocks = len(ch_mult), nrb
        self.resolution, self.in_channels = dc.image_size, mc.in_channels
        self.cond_drop_prob = mc.cond_drop_prob
        self.own_gemm = False  # set by conv.use_salun_convs(model): Linear layers on K15, projections grouped

        def dense_pair(n_in, n_hidden):
            holder = nn.Module()
            holder.dense = nn.ModuleList([nn.Linear(n_in, n_hidden), nn.Linear(n_hidden, n_hidden)])
            return holder

        self.temb = dense_pair(ch, self.temb_ch)
        self.classes_emb = nn.Embedding(dc.n_classes, ch)
        self.null_classes_emb = nn.Parameter(torch.randn(ch))
        self.cemb = dense_pair(ch, self.cemb_ch)
        self.conv_in = nn.Conv2d(mc.in_channels, ch, 3, 1, 1)

        def res(cin, cout):
            # cemb_channels stays at its 512 default exactly as in the reference, which is why only
            # ch = 128 (temb_ch = 512) yields a consistent network
            return ResnetBlock(in_channels=cin, out_channels=cout, temb_channels=self.temb_ch, dropout=dropout)

        curr_res = dc.image_size
        in_mult = (1,) + ch_mult
        self.down = nn.ModuleList()
        block_in = None
        for lvl in range(self.num_resolutions):
            level = _Level()
            level.block, level.attn = nn.ModuleList(), nn.ModuleList()
            block_in, block_out = ch * in_mult[lvl], ch * ch_mult[lvl]
            for _ in range(nrb):
                level.block.append(res(block_in, block_out))
                block_in = block_out
                if curr_res in attn_res:
                    level.attn.append(AttnBlock(block_in))
            if lvl != self.num_resolutions - 1:
                level.downsample = Downsample(block_in, mc.resamp_with_conv)
                curr_res //= 2
            self.down.append(level)

        self.mid = nn.Module()
        self.mid.block_1 = res(block_in, block_in)
        self.mid.attn_1 = AttnBlock(block_in)
        self.mid.block_2 = res(block_in, block_in)

        self.up = nn.ModuleList()
        for lvl in reversed(range(self.num_resolutions)):
            level = _Level()
            level.block, level.attn = nn.ModuleList(), nn.ModuleList()
            block_out = ch * ch_mult[lvl]
            for i in range(nrb + 1):
                skip_in = ch * (in_mult[lvl] if i == nrb else ch_mult[lvl])
                level.block.append(res(block_in + skip_in, block_out))
                block_in = block_out
                if curr_res in attn_res:
                    level.attn.append(AttnBlock(block_in))
            if lvl != 0:
                level.upsample = Upsample(block_in, mc.resamp_with_conv)
                curr_res *= 2
            self.up.insert(0, level)  # index == resolution level

        self.norm_out = group_norm(block_in)
        self.conv_out = nn.Conv2d(block_in, out_ch, 3, 1, 1)

    # ---------------------------------------------------------------- forward modes
    def forward(self, x, t, c, mode, **kwargs):
        """mode="train": one pass with label dropout `cond_drop_prob`;  mode="test": classifier-free
        guidance (1+s)·eps(x,c) − s·eps(x,∅) with s = `cond_scale` (reference :329-355)."""
        assert mode in ("train", "test")
        if mode == "train":
            return self._forward(x, t, c, cond_drop_prob=kwargs.get("cond_drop_prob"))
        return self._forward_with_cond_scale(x, t, c, cond_scale=kwargs.get("cond_scale"))

    def _forward_with_cond_scale(self, x, t, c, cond_scale=1.0):
        logits = self._forward(x, t, c, cond_drop_prob=0.0)
        if cond_scale == 0:
            return logits
        null_logits = self._forward(x, t, c, cond_drop_prob=1.0)
        return (1 + cond_scale) * logits - cond_scale * null_logits

    def eps_pair(self, x, t, c, null=True):
        """The two raw predictions of classifier-free guidance, (eps(x, c), eps(x, ∅)), uncombined: the fused sampler
        step does the combine itself (functions/denoising.py:fused_steps_conditional).  `null=False`: (eps(x, c), None)."""
        return self._forward(x, t, c, cond_drop_prob=0.0), (self._forward(x, t, c, cond_drop_prob=1.0) if null else None)

    def _projections(self, emb_act):
        """Every ResnetBlock adds Linear(emb_act) of the SAME activation (reference models/diffusion.py:120): with the
        own GEMM all 22 are one grouped launch (and one / one / 22-in-one in backward) instead of 22 library GEMMs with
        their bias adds, bias-gradient sums and AccumulateGrad launches.  -> {block: projection}, {} otherwise."""
        if not (self.own_gemm and emb_act.is_cuda and emb_act.dtype == torch.float32) or torch.is_autocast_enabled():
            return {}
        from ... import gemm
        blocks = self.__dict__.get("_resblocks")
        if blocks is None:
            blocks = [m for m in self.modules() if isinstance(m, ResnetBlock)]
            self.__dict__["_resblocks"] = blocks
        outs = gemm.grouped_linear(emb_act, [b.temb_cemb_proj for b in blocks])
        return dict(zip(blocks, outs))

    def _forward(self, x, t, c, cond_drop_prob=None):
        assert x.shape[2] == x.shape[3] == self.resolution
        batch = x.shape[0]
        cond_drop_prob = self.cond_drop_prob if cond_drop_prob is None else cond_drop_prob

        temb = self.temb.dense[1](swish(self.temb.dense[0](get_timestep_embedding(t, self.ch))))
        cemb = self.classes_emb(c.to(x.device))
        if cond_drop_prob > 0:
            # one draw per sample of the GLOBAL batch, sliced to this rank's shard under data parallel (draws.py)
            keep = draws.batch_draw(batch, lambda n: prob_mask_like((n,), 1 - cond_drop_prob, device=x.device))
            cemb = torch.where(keep[:, None], cemb, self.null_classes_emb[None, :].expand(batch, -1))
        cemb = self.cemb.dense[1](swish(self.cemb.dense[0](cemb)))
        emb_act = swish(torch.cat([temb, cemb], dim=-1))
        proj = self._projections(emb_act)

        hs = [self.conv_in(x)]
        for lvl, level in enumerate(self.down):
            for i, blk in enumerate(level.block):
                h = blk(hs[-1], emb_act, proj.get(blk))
                if len(level.attn) > 0:
                    h = level.attn[i](h)
                hs.append(h)
            if lvl != self.num_resolutions - 1:
                hs.append(level.downsample(hs[-1]))

        h = self.mid.block_2(self.mid.attn_1(self.mid.block_1(hs[-1], emb_act, proj.get(self.mid.block_1))), emb_act,
                             proj.get(self.mid.block_2))

        for lvl in reversed(range(self.num_resolutions)):
            level = self.up[lvl]
            for i, blk in enumerate(level.block):
                h = blk(torch.cat([h, hs.pop()], dim=1), emb_act, proj.get(blk))
                if len(level.attn) > 0:
                    h = level.attn[i](h)
            if lvl != 0:
                h = level.upsample(h)
        return self.conv_out(fused_gn_act(h, self.norm_out, silu=True))
