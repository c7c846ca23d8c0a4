"""UNet3DConditionModel on MI355X: drop-in for the reference's
/root/reference/models/unet_3d_condition_mask.py:54-526 (module) and the five block classes of
/root/reference/models/unet_3d_blocks.py:234-842, inference branches.

Same constructor arguments, same `forward` signature / return type, same diffusers state-dict keys
(SURVEY.md Appendix C); the arithmetic is the HIP token path of `layers.py`.  The whole denoising
forward between the NC(T)HW boundary tensors is a chain of libaa_mi355.so launches on torch's
current stream, so it can be captured in a hipGraph (`enable_graph`).
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn

from . import ops
from ._model import GraphModel, Session
from .layers import (Attention, Conv2d, Downsample2D, Grid, GroupNorm, Linear, ResnetBlock2D, TemporalConvLayer,
                     TimestepEmbedding, Transformer2DModel, TransformerTemporalModel, Upsample2D)


@dataclass
class UNet3DConditionOutput:
    """reference unet_3d_condition_mask.py:43-51."""
    sample: torch.Tensor


class _Stage(nn.Module):
    """One resolution stage; per-layer order of the reference inference branches:
    resnet -> temp_conv -> spatial transformer -> temporal transformer
    (unet_3d_blocks.py:514-526, 747-759; without attention :606-609, :833-836)."""

    def __init__(self, res_io, temb_channels, eps, groups, heads=None, head_dim=None, cross_attention_dim=None,
                 down=None, up=False):
        super().__init__()
        self.has_cross_attention = heads is not None
        self.gradient_checkpointing = False
        self.resnets = nn.ModuleList([ResnetBlock2D(i, o, temb_channels, eps=eps, groups=groups) for i, o in res_io])
        self.temp_convs = nn.ModuleList([TemporalConvLayer(o, o, dropout=0.1) for _, o in res_io])
        if self.has_cross_attention:
            self.attentions = nn.ModuleList(
                [Transformer2DModel(heads, head_dim, o, cross_attention_dim, groups) for _, o in res_io])
            self.temp_attentions = nn.ModuleList(
                [TransformerTemporalModel(heads, head_dim, o, groups) for _, o in res_io])
        out_ch = res_io[-1][1]
        self.downsamplers = nn.ModuleList([Downsample2D(out_ch, out_ch, padding=down)]) if down is not None else None
        self.upsamplers = nn.ModuleList([Upsample2D(out_ch, out_ch)]) if up else None

    def _layer(self, i, x, g, temb_silu, text, text_len, skip=None, dup=1):
        """`dup` > 1: x / g hold one copy of `dup` identical groups of clips (guidance); everything in front of the first
        text cross-attention is computed once, the result covers all groups."""
        x = self.resnets[i].tokens(x, g, temb_silu, x1=skip)
        if g.frames > 1:
            x = self.temp_convs[i].tokens(x, g)
        if self.has_cross_attention:
            x = self.attentions[i].tokens(x, g, text, text_len, dup=dup)
            if dup > 1:
                g = Grid(g.clips * dup, g.frames, g.h, g.w)
            if g.frames > 1:
                x = self.temp_attentions[i].tokens(x, g)
        return x


class _DownStage(_Stage):
    def tokens(self, x, g, temb_silu, text, text_len, dup=1):
        outs = []
        for i in range(len(self.resnets)):
            x = self._layer(i, x, g, temb_silu, text, text_len, dup=dup if i == 0 else 1)
            if i == 0 and dup > 1:
                g = Grid(g.clips * dup, g.frames, g.h, g.w)
            outs.append((x, g))
        if self.downsamplers is not None:
            x, g = self.downsamplers[0].tokens(x, g)
            outs.append((x, g))
        return x, g, outs


class CrossAttnDownBlock3D(_DownStage):
    """reference unet_3d_blocks.py:389-536."""


class DownBlock3D(_DownStage):
    """reference unet_3d_blocks.py:539-619."""


class _UpStage(_Stage):
    resolution_idx = None                       # position in up_blocks (diffusers); FreeU acts on 0 and 1
    s1 = s2 = b1 = b2 = None                    # FreeU scalars (UNet3DConditionModel.enable_freeu)

    def _freeu(self):
        """(b, s) of this block when FreeU is on for it - diffusers' condition: the four attributes set and non-zero, resolution_idx 0 / 1."""
        if self.resolution_idx not in (0, 1) or not (self.s1 and self.s2 and self.b1 and self.b2):
            return None
        return (self.b1, self.s1) if self.resolution_idx == 0 else (self.b2, self.s2)

    def tokens(self, x, g, skips, temb_silu, text, text_len, upsample_size=None):
        freeu = self._freeu()
        for i in range(len(self.resnets)):
            skip, _ = skips.pop()
            if freeu is not None:
                # in front of the implicit cat([x, skip]); in place: every reader of the two tensors (the down path, the mid block,
                # the layer before) has run, and a step recomputes both
                x, skip = ops.freeu(x, skip, g.images, g.h, g.w, freeu[0], freeu[1], hidden_out=x, skip_out=skip)
            x = self._layer(i, x, g, temb_silu, text, text_len, skip=skip)     # cat([x, skip]) is implicit
        if self.upsamplers is not None:
            x, g = self.upsamplers[0].tokens(x, g, upsample_size)
        return x, g


class CrossAttnUpBlock3D(_UpStage):
    """reference unet_3d_blocks.py:622-765."""


class UpBlock3D(_UpStage):
    """reference unet_3d_blocks.py:768-842."""


class UNetMidBlock3DCrossAttn(nn.Module):
    """reference unet_3d_blocks.py:234-386."""

    def __init__(self, channels, temb_channels, eps, groups, heads, head_dim, cross_attention_dim,
                 output_scale_factor=1.0):
        super().__init__()
        self.has_cross_attention = True
        self.gradient_checkpointing = False
        self.resnets = nn.ModuleList([ResnetBlock2D(channels, channels, temb_channels, eps=eps, groups=groups,
                                                    output_scale_factor=output_scale_factor) for _ in range(2)])
        self.temp_convs = nn.ModuleList([TemporalConvLayer(channels, channels, dropout=0.1) for _ in range(2)])
        self.attentions = nn.ModuleList([Transformer2DModel(heads, head_dim, channels, cross_attention_dim, groups)])
        self.temp_attentions = nn.ModuleList([TransformerTemporalModel(heads, head_dim, channels, groups)])

    def tokens(self, x, g, temb_silu, text, text_len):
        x = self.resnets[0].tokens(x, g, temb_silu)
        x = self.temp_convs[0].tokens(x, g)             # unconditional in the reference (:353-354)
        x = self.attentions[0].tokens(x, g, text, text_len)
        if g.frames > 1:
            x = self.temp_attentions[0].tokens(x, g)
        x = self.resnets[1].tokens(x, g, temb_silu)
        if g.frames > 1:
            x = self.temp_convs[1].tokens(x, g)
        return x


_DOWN = {"CrossAttnDownBlock3D": CrossAttnDownBlock3D, "DownBlock3D": DownBlock3D}
_UP = {"CrossAttnUpBlock3D": CrossAttnUpBlock3D, "UpBlock3D": UpBlock3D}


class UNet3DConditionModel(GraphModel):
    """Constructor arguments / defaults: reference unet_3d_condition_mask.py:87-110.  Loading, saving, `enable_graph`,
    `invalidate_caches` and the session store: _model.GraphModel."""

    class_name = "UNet3DConditionModel"
    config_extra = {"_class_name": "UNet3DConditionModel"}
    _packs = GraphModel._packs + ("_co_pack",)
    _supports_gradient_checkpointing = True

    def __init__(self, sample_size=None, in_channels=4, out_channels=4,
                 down_block_types=("CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "DownBlock3D"),
                 up_block_types=("UpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D"),
                 block_out_channels=(320, 640, 1280, 1280), layers_per_block=2, downsample_padding=1,
                 mid_block_scale_factor=1, act_fn="silu", norm_num_groups=32, norm_eps=1e-5,
                 cross_attention_dim=1024, attention_head_dim=64, motion_mask=False, motion_strength=False):
        super().__init__()
        if len(down_block_types) != len(up_block_types):
            raise ValueError(f"Must provide the same number of `down_block_types` as `up_block_types`. "
                             f"`down_block_types`: {down_block_types}. `up_block_types`: {up_block_types}.")
        if len(block_out_channels) != len(down_block_types):
            raise ValueError(f"Must provide the same number of `block_out_channels` as `down_block_types`. "
                             f"`block_out_channels`: {block_out_channels}. `down_block_types`: {down_block_types}.")
        if not isinstance(attention_head_dim, int) and len(attention_head_dim) != len(down_block_types):
            raise ValueError(f"Must provide the same number of `attention_head_dim` as `down_block_types`. "
                             f"`attention_head_dim`: {attention_head_dim}. `down_block_types`: {down_block_types}.")
        if act_fn not in ("silu", "swish"):
            raise ValueError("only act_fn='silu' is implemented")
        self.config = SimpleNamespace(
            sample_size=sample_size, in_channels=in_channels, out_channels=out_channels,
            down_block_types=tuple(down_block_types), up_block_types=tuple(up_block_types),
            block_out_channels=tuple(block_out_channels), layers_per_block=layers_per_block,
            downsample_padding=downsample_padding, mid_block_scale_factor=mid_block_scale_factor, act_fn=act_fn,
            norm_num_groups=norm_num_groups, norm_eps=norm_eps, cross_attention_dim=cross_attention_dim,
            attention_head_dim=attention_head_dim, motion_mask=motion_mask, motion_strength=motion_strength)
        self.motion_mask, self.motion_strength, self.sample_size = motion_mask, motion_strength, sample_size
        self.gradient_checkpointing = False
        ch0 = block_out_channels[0]
        temb = ch0 * 4
        n = len(block_out_channels)
        hd = (attention_head_dim,) * n if isinstance(attention_head_dim, int) else tuple(attention_head_dim)
        if any(d != 64 for d in hd):
            raise ValueError("the MI355X attention kernel implements attention_head_dim == 64 (the v1.02 architecture)")

        self.conv_in = Conv2d(in_channels, ch0, 3, padding=1)
        self.conv_in2 = Conv2d(5, ch0, 3, padding=1)
        self.time_embedding = TimestepEmbedding(ch0, temb, cond_proj_dim=ch0)
        self.motion_embedding = nn.Sequential(nn.Linear(ch0, temb), nn.SiLU(), nn.Linear(temb, temb))  # unused by forward, kept for checkpoints
        nn.init.zeros_(self.motion_embedding[-1].weight)
        nn.init.zeros_(self.motion_embedding[-1].bias)
        self.transformer_in = TransformerTemporalModel(8, hd[0], ch0, norm_num_groups)

        self.down_blocks = nn.ModuleList()
        out_c = ch0
        for i, kind in enumerate(down_block_types):
            if kind not in _DOWN:
                raise ValueError(f"{kind} does not exist.")
            in_c, out_c = out_c, block_out_channels[i]
            io = [(in_c if j == 0 else out_c, out_c) for j in range(layers_per_block)]
            attn = dict(heads=out_c // hd[i], head_dim=hd[i], cross_attention_dim=cross_attention_dim) \
                if kind.startswith("CrossAttn") else {}
            self.down_blocks.append(_DOWN[kind](io, temb, norm_eps, norm_num_groups,
                                                down=downsample_padding if i < n - 1 else None, **attn))

        # (registered ahead of mid_block like the reference - unet_3d_condition_mask.py:171-172,202: LoRA files address
        # layers by their position in named_modules(), so down_blocks -> up_blocks -> mid_block is part of the file format)
        self.up_blocks = nn.ModuleList()
        cm = block_out_channels[-1]
        self.mid_block = UNetMidBlock3DCrossAttn(cm, temb, norm_eps, norm_num_groups, cm // hd[-1], hd[-1],
                                                 cross_attention_dim, mid_block_scale_factor)

        rev, rhd = list(reversed(block_out_channels)), list(reversed(hd))
        out_c = rev[0]
        self.num_upsamplers = 0
        for i, kind in enumerate(up_block_types):
            if kind not in _UP:
                raise ValueError(f"{kind} does not exist.")
            prev_c, out_c = out_c, rev[i]
            skip_c = rev[min(i + 1, n - 1)]
            L = layers_per_block + 1
            io = [((prev_c if j == 0 else out_c) + (skip_c if j == L - 1 else out_c), out_c) for j in range(L)]
            up = i < n - 1
            self.num_upsamplers += int(up)
            attn = dict(heads=out_c // rhd[i], head_dim=rhd[i], cross_attention_dim=cross_attention_dim) \
                if kind.startswith("CrossAttn") else {}
            self.up_blocks.append(_UP[kind](io, temb, norm_eps, norm_num_groups, up=up, **attn))
            self.up_blocks[-1].resolution_idx = i

        self.conv_norm_out = GroupNorm(norm_num_groups, ch0, eps=norm_eps)
        self.conv_act = nn.SiLU()
        self.conv_out = Conv2d(ch0, out_channels, 3, padding=1)
        self._graph = None
        from . import layers as _layers
        if _layers.AA_FP8_FF:                                  # (the module-level knob: see enable_fp8_feedforward)
            self.enable_fp8_feedforward()

    # ------------------------------------------------------------------ batched small projections (_model.GraphModel)
    def _project_text(self, text_tokens):
        """K | V of the text for every cross-attention layer as ONE contraction; each layer receives its column slice."""
        self._project_batched(text_tokens, "_text_pack", lambda m: isinstance(m, Attention) and m.is_cross,
                              lambda a: (a.to_k, a.to_v), "kv")                          # [clips*L, sum of 2*inner]

    def _project_time_embeddings(self, temb_silu):
        """All ResnetBlock2D.time_emb_proj of the network as ONE contraction (31 two-row GEMMs otherwise, each a
        latency-bound launch): rows of the weights concatenated, every block receives its column slice."""
        self._project_batched(temb_silu, "_temb_pack", lambda m: isinstance(m, ResnetBlock2D) and m.time_emb_proj is not None,
                              lambda b: (b.time_emb_proj,), "tproj")                     # [clips, sum of Cout]

    def enable_gradient_checkpointing(self):       # inference-only implementation: accepted, no effect
        self.gradient_checkpointing = True

    def disable_gradient_checkpointing(self):
        self.gradient_checkpointing = False

    def enable_xformers_memory_efficient_attention(self, *a, **k):   # flash attention is always on
        return None

    def set_attention_slice(self, slice_size):     # scores never leave the chip: slicing is moot
        return None

    # ------------------------------------------------------------------ hot path
    def _core(self, sample, cond, mask, t, motion_t, cond_emb, text_tokens, g: Grid, text_len: int, upsample_sizes, cfg_dup=False):
        """Everything between the boundary tensors: only libaa_mi355 launches (graph-capturable).
        `cfg_dup`: the caller guarantees that the two halves of the batch differ ONLY in the text (classifier-free guidance,
        models/pipeline.py:160-168: same latents, condition frame, mask, timestep and motion for the unconditional and the
        text half).  Everything the text cannot reach - conv_in, transformer_in, the first resnet / temporal conv and the
        first spatial self-attention - is then computed for ONE half and replicated in front of the first text
        cross-attention: the same arithmetic per element (results equal to the strict form within the fp16 noise floor - the shared part runs
        other tile shapes), the redundant half of that prefix is not recomputed.
        sample [Bs,C,T,h,w] (fp32 or storage dtype), cond [Bc,C,1,h,w], mask [Bm,1,1,h,w] | None, t fp32 [B], motion_t fp32 [B] |
        None (or a ready [B, ch0] `cond_emb`), text_tokens [B*L, D]; returns the token matrix [B*(T+1)*h*w, 8]: columns [0, out_channels) are
        conv_out's channels, the rest zero filters (`_conv_out_pack`) - consumers take the row pitch (`stride(0)`) or slice."""
        dt = text_tokens.dtype
        ch0 = self.conv_in.out_channels
        t_sin = ops.timestep_embedding(t, ch0, dt)                                       # :408-413
        cond_sin = ops.timestep_embedding(motion_t, ch0, dt) if motion_t is not None else cond_emb   # :414-416
        dup = 2 if (cfg_dup and g.clips % 2 == 0 and self.down_blocks[0].has_cross_attention) else 1
        g0 = Grid(g.clips // dup, g.frames, g.h, g.w)
        x8 = ops.pack_latents(sample, cond, mask, g0.clips, dt)                           # :376, :424-428
        temb_silu = self.time_embedding.tokens(t_sin, cond_sin, final_silu=True)       # [clips, 4*ch0]
        self._project_time_embeddings(temb_silu)
        self._project_text(text_tokens)
        conv_in = self.conv_in2 if mask is not None else self.conv_in
        x = conv_in.tokens(x8, ops.conv3x3_geom(g0.images, g0.h, g0.w))
        if g.frames > 1:
            x = self.transformer_in.tokens(x, g0)
        skips = [(torch.cat([x] * dup) if dup > 1 else x, g)]
        for i, blk in enumerate(self.down_blocks):
            if i == 0:
                x, _, outs = blk.tokens(x, g0, temb_silu, text_tokens, text_len, dup=dup)
            else:
                x, g, outs = blk.tokens(x, g, temb_silu, text_tokens, text_len)
            if i == 0:
                g = outs[-1][1]
            skips += outs
        x = self.mid_block.tokens(x, g, temb_silu, text_tokens, text_len)
        for i, blk in enumerate(self.up_blocks):
            x, g = blk.tokens(x, g, skips, temb_silu, text_tokens, text_len, upsample_size=upsample_sizes[i])
        x = self.conv_norm_out.tokens(x, g.images, g.hw, silu=True)
        return ops.conv_gemm(x, self._conv_out_pack(), ops.conv3x3_geom(g.images, g.h, g.w))

    def _conv_out_pack(self):
        """conv_out (320 -> 4 channels, 3x3) with zero filters appended up to 8 output channels: 16-byte output rows are what the
        LDS-DMA contraction kernels store, so the head leaves the generic gather kernel (156 us at 20 TF/s at the 64x64 level,
        the slowest launch of a step per FLOP) for the tiled path; consumers read the first `out_channels` columns of the
        [tokens, 8] result (the solver kernel takes the row pitch, `forward` slices)."""
        from .layers import weights_key
        w, b = self.conv_out.weight, self.conv_out.bias
        n = w.shape[0]
        if n % 8 == 0 or w.shape[1] % 64:
            return self.conv_out.packed()
        key = weights_key(w, b)
        if getattr(self, "_co_pack", None) is None or self._co_key != key:
            pad = (-n) % 8
            wp = torch.cat([w.detach(), torch.zeros((pad,) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)])
            bp = None if b is None else torch.cat([b.detach(), torch.zeros(pad, dtype=b.dtype, device=b.device)])
            self._co_pack, self._co_key = ops.pack_weight(wp, bp), key
        return self._co_pack

    def forward(self, sample, timestep, encoder_hidden_states, condition_latent, mask, class_labels=None,
                timestep_cond=None, attention_mask=None, cross_attention_kwargs=None,
                down_block_additional_residuals=None, mid_block_additional_residual=None, motion=None,
                return_dict=True, image_embeds=None):
        """reference unet_3d_condition_mask.py:338-526.  `attention_mask`, `class_labels`,
        `cross_attention_kwargs`, `image_embeds` are accepted and unused, as in the reference."""
        if down_block_additional_residuals is not None or mid_block_additional_residual is not None:
            raise NotImplementedError("ControlNet residual hooks are not part of the MI355X hot path")
        self.require_device(sample)
        dt, dev = self.dtype, sample.device
        b, _, frames, h, w = sample.shape
        t = timestep
        if not torch.is_tensor(t):
            t = torch.tensor([float(t)], dtype=torch.float32, device=dev)
        t = t.to(device=dev, dtype=torch.float32).reshape(-1).expand(b).contiguous()
        motion_t = cond_emb = None
        if self.motion_strength and motion is not None:                                 # :414-416
            motion_t = torch.as_tensor(motion, device=dev).to(torch.float32).reshape(-1).expand(b).contiguous()
        elif timestep_cond is not None:
            cond_emb = timestep_cond.to(dt).expand(b, self.conv_in.out_channels).contiguous()
        use_mask = bool(self.motion_mask and mask is not None)
        if sample.dtype not in (torch.float32, dt):
            sample = sample.to(dt)
        sess = self.session(b, frames, h, w, tuple(encoder_hidden_states.shape[1:]), use_mask, motion_t is not None,
                            cond_emb is not None, sample.dtype, sample.shape[0], condition_latent.shape[0],
                            mask.shape[0] if use_mask else 0, dev)
        sess.load(sample=sample, cond=condition_latent, mask=mask if use_mask else None, t=t, motion=motion_t,
                  cond_emb=cond_emb, text=encoder_hidden_states)
        y = sess.run()
        y = y.reshape(b, frames + 1, h, w, -1)[..., :self.conv_out.out_channels].permute(0, 4, 1, 2, 3)[:, :, 1:]       # :521-522 (columns past out_channels: _conv_out_pack)
        return UNet3DConditionOutput(sample=y) if return_dict else (y,)

    # ------------------------------------------------------------------ opt-in paths
    def enable_fp8_feedforward(self, min_dim=None):
        """Opt in to the W8A8 (OCP e4m3) FeedForward path: every spatial and temporal transformer FeedForward with `dim >= min_dim` (default
        layers.FP8_FF_MIN_DIM = 640; the 320-channel ones keep their fused kernel) runs quantise -> GEGLU contraction -> quantise -> ff-out
        contraction on the block-scaled fp8 matrix form.  The e4m3 weights are derived from the parameters on first use (after a LoRA merge
        they are derived again).  The output differs from the 16-bit path by the quantisation error: off by default.  Returns the number of
        FeedForwards flagged."""
        from .layers import FP8_FF_MIN_DIM, FeedForward
        min_dim = FP8_FF_MIN_DIM if min_dim is None else min_dim
        n = 0
        for m in self.modules():
            if isinstance(m, FeedForward):
                m.fp8 = m.dim >= min_dim
                n += int(m.fp8)
        self.invalidate_caches()                               # (captured graphs replay the other path's launches)
        return n

    def disable_fp8_feedforward(self):
        from .layers import FeedForward
        for m in self.modules():
            if isinstance(m, FeedForward):
                m.fp8 = False
                m._pw8 = None
        self.invalidate_caches()

    def enable_freeu(self, s1, s2, b1, b2):
        """diffusers `enable_freeu` (FreeU, Si et al.): in the up blocks with resolution_idx 0 / 1 (the 8x8 and 16x16 levels of the v1.02
        architecture) every resnet sees the first half of the backbone channels scaled by b1 / b2 and the skip connection with its lowest
        Fourier modes scaled by s1 / s2 (`ops.freeu`, one launch per layer).  Off by default; the scalars are baked into captured graphs,
        so the sessions are dropped."""
        for blk in self.up_blocks:
            blk.s1, blk.s2, blk.b1, blk.b2 = s1, s2, b1, b2
        self.invalidate_caches()

    def disable_freeu(self):
        for blk in self.up_blocks:
            blk.s1 = blk.s2 = blk.b1 = blk.b2 = None
        self.invalidate_caches()

    # ------------------------------------------------------------------ sessions: static inputs (+ hipGraph replay)
    def session(self, batch, frames, h, w, text_shape, use_mask, has_motion, has_cond_emb, sample_dtype, sample_batch,
                cond_batch, mask_batch, device, cfg_dup=False):
        """The static input buffers (and, when graphs are enabled, the captured hipGraph) of one input signature.
        A caller that owns the denoising loop (LatentToVideoPipeline.denoise) writes its inputs straight into
        `sess.inputs[...]` once and then only calls `sess.run()` per step."""
        key = (batch, frames, h, w, tuple(text_shape), use_mask, has_motion, has_cond_emb, sample_dtype, sample_batch,
               cond_batch, mask_batch, self.dtype, str(device), bool(cfg_dup))
        return self._session(key, device, _Session)


class _Session(Session):
    def __init__(self, net, key, device):
        super().__init__(net)
        (b, frames, h, w, text_shape, use_mask, has_motion, has_cond_emb, sample_dtype, sample_batch, cond_batch, mask_batch,
         dt, _dev, self.cfg_dup) = key
        self.b, self.frames, self.h, self.w = b, frames, h, w
        z = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=device)
        c = net.config.in_channels
        self.inputs = dict(sample=z(sample_batch, c, frames, h, w, dtype=sample_dtype), cond=z(cond_batch, c, 1, h, w),
                           mask=z(mask_batch, 1, 1, h, w) if use_mask else None, t=z(b, dtype=torch.float32),
                           motion=z(b, dtype=torch.float32) if has_motion else None,
                           cond_emb=z(b, net.conv_in.out_channels) if has_cond_emb else None, text=z(b, *text_shape))
        self.text_len = text_shape[0]
        self.grid = Grid(b, frames + 1, h, w)
        # sizes the up path must hit when H or W is not a multiple of 2**num_upsamplers (:381-383, :490-491)
        up_factor = 2 ** net.num_upsamplers
        sizes = [(h, w)]
        for _ in range(net.num_upsamplers):
            ph, pw = sizes[-1]
            sizes.append(((ph - 1) // 2 + 1, (pw - 1) // 2 + 1))
        ups = [None] * len(net.up_blocks)
        if (h % up_factor != 0) or (w % up_factor != 0):
            for i in range(net.num_upsamplers):
                ups[i] = sizes[net.num_upsamplers - 1 - i]
        self.upsample_sizes = tuple(ups)

    def _core(self):
        i = self.inputs
        return self.net._core(i["sample"], i["cond"], i["mask"], i["t"], i["motion"], i["cond_emb"],
                              i["text"].reshape(-1, i["text"].shape[-1]), self.grid, self.text_len, self.upsample_sizes,
                              cfg_dup=self.cfg_dup)
