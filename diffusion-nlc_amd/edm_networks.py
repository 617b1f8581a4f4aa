"""EDM DDPM++ ``SongUNet`` and its sigma net on the HIP kernels (drop-in for src/edm_networks.py).

Only the configuration ``create_edm_sigma_eps_model`` builds is implemented
(src/script_util.py:243-262): positional embedding, 'standard' encoder/decoder,
resample_filter [1,1] (so down = 2x2 mean, up = nearest 2x), adaptive_scale False, one
attention head, skip_scale sqrt(1/2), GroupNorm(min(32,C/4) groups, eps 1e-6).

    UNetBlock (src/edm_networks.py:183-205)  GN+SiLU -> [2x2 mean | nearest-2x folded into the gather]
        -> 3x3 conv whose epilogue adds affine(emb) per (image, channel) -> GN+SiLU -> 3x3 conv with
        (+skip, * sqrt(1/2)) in its epilogue; attention: GN -> 1x1 qkv GEMM (interleaved q,k,v channel
        order and k/sqrt(C) folded into the weights) -> flash attention -> 1x1 proj (+x, * sqrt(1/2)).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import ops
from ._ext import ACT_SILU
from .hipnet import (EmbBank, HipModule, Norm, ResBlock, SelfAttention, SigmaNet, SpecBuilder, as_f32_cuda, first_conv_weight, pack, pack_opt,
                     qkv_row_scale)

GN_EPS = 1e-6
SKIP_SCALE = float(np.sqrt(0.5))


def _groups(c):
    return min(32, c // 4)               # GroupNorm.__init__ (src/edm_networks.py:108)


def _spec_block(sb: SpecBuilder, p, cin, cout, emb_ch, attention, up=False, down=False):
    sb.norm(p + ".norm0", cin)
    sb.conv(p + ".conv0", cout, cin, 3)
    if up or down:
        sb.add(p + ".conv0.resample_filter", (1, 1, 2, 2))
    if emb_ch:
        sb.linear(p + ".affine", cout, emb_ch)
    sb.norm(p + ".norm1", cout)
    sb.conv(p + ".conv1", cout, cout, 3)
    if cout != cin or up or down:
        sb.conv(p + ".skip", cout, cin, 1)
        if up or down:
            sb.add(p + ".skip.resample_filter", (1, 1, 2, 2))
    if attention:
        _spec_attention(sb, p, cout)


def _spec_attention(sb: SpecBuilder, p, c):
    sb.norm(p + ".norm2", c)
    sb.conv(p + ".qkv", 3 * c, c, 1)
    sb.conv(p + ".proj", c, c, 1)


def _unet_block(sd, p, dtype, device, bank: Optional[EmbBank], up=False, down=False, pure=False) -> ResBlock:
    """UNetBlock without its attention (src/edm_networks.py:183-197); ``pure``: PureUNetBlock.forward feeds conv0's output straight into
    conv1 (:944-945).  An up / down block always has the skip 1x1 (:176): up reads x through that launch's folded upsample.  Known
    difference from ADM: the down block does not use the fused pool (``fused_pool`` stays off) - norm -> pool -> conv and a second pool
    of x for the skip; switching it would change 16-bit results, so it is not this block's to fix."""
    cin, cout = sd[p + ".norm0.weight"].shape[0], sd[p + ".conv0.weight"].shape[0]
    return ResBlock(Norm(sd, p + ".norm0", device, _groups(cin), GN_EPS), pack(sd, p + ".conv0", dtype, device),
                    None if pure else Norm(sd, p + ".norm1", device, _groups(cout), GN_EPS), pack(sd, p + ".conv1", dtype, device),
                    pack_opt(sd, p + ".skip", dtype, device),
                    None if bank is None else bank.add(sd[p + ".affine.weight"], sd[p + ".affine.bias"])[0],
                    up=up, down=down, out_scale=SKIP_SCALE)


def _attention(sd, p, dtype, device) -> SelfAttention:
    """The attention half of a UNetBlock (:198-203), keys under the block's own prefix."""
    c = sd[p + ".proj.weight"].shape[0]
    idx = torch.arange(3 * c)
    perm = (idx % c) * 3 + idx // c             # reshape(n, C, 3, T).unbind(2): channel = c*3 + {q,k,v} (:199-200)
    scale, base2 = qkv_row_scale(c, float(c) ** -0.25, dtype)      # k / sqrt(C) (:127) split evenly over q and k
    return SelfAttention(Norm(sd, p + ".norm2", device, _groups(c), GN_EPS), pack(sd, p + ".qkv", dtype, device, row_perm=perm, row_scale=scale),
                         pack(sd, p + ".proj", dtype, device), 1, base2, out_scale=SKIP_SCALE)


class SongUNet(HipModule):
    """src/edm_networks.py:732-909 (the second, plain-nn.Module definition that carries ``encode``)."""

    def __init__(self, img_resolution, in_channels, out_channels, label_dim=0, augment_dim=0, model_channels=128,
                 channel_mult=[1, 2, 2, 2], channel_mult_emb=4, num_blocks=4, attn_resolutions=[16], dropout=0.10,
                 label_dropout=0, embedding_type="positional", channel_mult_noise=1, encoder_type="standard",
                 decoder_type="standard", resample_filter=[1, 1], **kwargs):
        if embedding_type != "positional" or encoder_type != "standard" or decoder_type != "standard" \
                or list(resample_filter) != [1, 1] or label_dim != 0 or channel_mult_noise != 1:
            raise NotImplementedError("HIP SongUNet: only the DDPM++ configuration of create_edm_sigma_eps_model")
        self.img_resolution, self.in_channels, self.out_channels = img_resolution, in_channels, out_channels
        self.augment_dim, self.model_channels = augment_dim, model_channels
        self.channel_mult, self.num_blocks = tuple(channel_mult), num_blocks
        self.attn_resolutions = tuple(attn_resolutions)
        self.emb_channels = model_channels * channel_mult_emb
        super().__init__()

    def _layout(self):
        enc, dec = [], []
        cout = self.in_channels
        mc = self.model_channels
        for level, mult in enumerate(self.channel_mult):
            res = self.img_resolution >> level
            if level == 0:
                cin, cout = cout, mc
                enc.append((f"enc.{res}x{res}_conv", "conv", cin, cout, {}))
            else:
                enc.append((f"enc.{res}x{res}_down", "block", cout, cout, {"down": True}))
            for idx in range(self.num_blocks):
                cin, cout = cout, mc * mult
                enc.append((f"enc.{res}x{res}_block{idx}", "block", cin, cout, {"attention": res in self.attn_resolutions}))
        skips = [e[3] for e in enc]
        nlev = len(self.channel_mult)
        for level, mult in reversed(list(enumerate(self.channel_mult))):
            res = self.img_resolution >> level
            if level == nlev - 1:
                dec.append((f"dec.{res}x{res}_in0", "block", cout, cout, {"attention": True}))
                dec.append((f"dec.{res}x{res}_in1", "block", cout, cout, {}))
            else:
                dec.append((f"dec.{res}x{res}_up", "block", cout, cout, {"up": True}))
            for idx in range(self.num_blocks + 1):
                cin = cout + skips.pop()
                cout = mc * mult
                dec.append((f"dec.{res}x{res}_block{idx}", "block", cin, cout,
                            {"attention": idx == self.num_blocks and res in self.attn_resolutions, "cat": True}))
            if level == 0:
                dec.append((f"dec.{res}x{res}_aux_norm", "aux_norm", cout, cout, {}))
                dec.append((f"dec.{res}x{res}_aux_conv", "aux_conv", cout, self.out_channels, {}))
        return enc, dec

    def param_spec(self):
        sb = SpecBuilder()
        mc, E = self.model_channels, self.emb_channels
        if self.augment_dim:
            sb.linear("map_augment", mc, self.augment_dim, bias=False)
        sb.linear("map_layer0", E, mc)
        sb.linear("map_layer1", E, E)
        enc, dec = self._layout()
        for p, kind, cin, cout, kw in enc + dec:
            if kind in ("conv", "aux_conv"):
                sb.conv(p, cout, cin, 3)
            elif kind == "aux_norm":
                sb.norm(p, cin)
            else:
                _spec_block(sb, p, cin, cout, E, kw.get("attention", False), up=kw.get("up", False), down=kw.get("down", False))
        return sb.spec

    def _build(self, sd, device, dtype):
        P = SimpleNamespace()
        half = self.model_channels // 2
        fr = torch.arange(0, half, dtype=torch.float32) / (half - 1)         # endpoint=True (:220-222)
        P.freqs = ((1 / 10000) ** fr).to(device)
        P.m0 = pack(sd, "map_layer0", torch.float32, device)
        P.m1 = pack(sd, "map_layer1", torch.float32, device)
        bank = EmbBank()
        enc, dec = self._layout()
        P.enc, P.dec = [], []

        def block(p, kw):                       # (UNetBlock's two halves: residual block, attention or None)
            return (_unet_block(sd, p, dtype, device, bank, up=kw.get("up", False), down=kw.get("down", False)),
                    _attention(sd, p, dtype, device) if kw.get("attention") else None)
        for p, kind, cin, cout, kw in enc:
            if kind == "conv":
                P.enc.append(("conv",) + first_conv_weight(sd, p, device))
            else:
                P.enc.append(("block",) + block(p, kw))
        for p, kind, cin, cout, kw in dec:
            if kind == "aux_norm":
                P.aux_norm = Norm(sd, p, device, _groups(cin), GN_EPS)
            elif kind == "aux_conv":
                P.aux_conv = pack(sd, p, dtype, device)
            else:
                P.dec.append((bool(kw.get("cat")),) + block(p, kw))
        bank.finalize(device, allow_split=ops.is16(dtype))
        P.bank = bank
        return P

    def run(self, x_nchw, noise_labels, mode="forward", in_scale=None, feat_nhwc=False):
        P = self.plan()
        with torch.cuda.device(self.device):
            # map_noise + the sin/cos swap (:837-838) == [sin || cos]; augment_labels is None on this path
            pe = ops.timestep_embedding(noise_labels, P.freqs, sin_first=True)
            e = ops.conv2d(pe, P.m0, act=ACT_SILU)
            e = ops.conv2d(e, P.m1, act=ACT_SILU)
            emb_all = P.bank(e)
            skips = []
            x = None
            for item in P.enc:
                if item[0] == "conv":
                    x = ops.conv_first(x_nchw, item[1], item[2], self.compute_dtype, in_scale=in_scale)
                else:
                    x = item[1](x, None, emb_all)
                    if item[2] is not None:
                        x = item[2](x)
                skips.append(x)
            if mode == "encode":
                return x if feat_nhwc else ops.nhwc_to_nchw_f32(x)
            for cat, blk, attn in P.dec:
                x = blk(x, skips.pop() if cat else None, emb_all)
                if attn is not None:
                    x = attn(x)
            return ops.conv2d(P.aux_norm(x, silu=True), P.aux_conv, out_nchw_f32=True)

    def _prep(self, x, noise_labels):
        self._require_gpu()
        return as_f32_cuda(x, self.device), as_f32_cuda(noise_labels, self.device).reshape(-1)

    def forward(self, x, noise_labels, class_labels=None, augment_labels=None):
        assert class_labels is None and augment_labels is None
        return self.run(*self._prep(x, noise_labels), mode="forward")

    def encode(self, x, noise_labels, class_labels=None, augment_labels=None):
        assert class_labels is None and augment_labels is None
        return self.run(*self._prep(x, noise_labels), mode="encode")


class SigmaModel(SigmaNet):
    """src/edm_networks.py:979-1022: PureUNetBlock (attention on even blocks) + pad/conv-s2 downsample, SiLU head."""

    ATTENTION_OWN_INDEX = False
    HEAD_ACT = ACT_SILU

    def __init__(self, dim=4, channels=64, n_blocks=2, out_dim=1, dropout=0.1, resample_filter=[1, 1]):
        super().__init__(dim, channels, n_blocks, out_dim)

    def _has_attention(self, i):
        return i % 2 == 0

    def _spec_block(self, sb, p, c):
        _spec_block(sb, p, c, c, 0, False)

    _spec_attention = staticmethod(_spec_attention)

    def _make_block(self, sd, p, dtype, device):
        return _unet_block(sd, p, dtype, device, None, pure=True)

    _make_attention = staticmethod(_attention)
