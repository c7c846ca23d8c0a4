"""LatentToVideoPipeline on MI355X: drop-in for /root/reference/models/pipeline.py:12-214
(`LatentToVideoPipeline.__call__`, a diffusers `TextToVideoSDPipeline` subclass) and the latent
helpers of /root/reference/utils/common.py:12-48,296-300.

Same keyword arguments, same return convention (`(frames, latents)` when `return_dict=False`,
pipeline.py:211-212).  Per denoising step the device work is: one UNet3D forward on the CFG-doubled
batch (hipGraph replay when enabled) and one fused guidance + solver update kernel
(`aa_cfg_dpm_step_tokens`, `aa_cfg_ddim_step_tokens` or `aa_cfg_unipc_step_tokens`) -- the reference's
cat / chunk / permute / scheduler.step chain (pipeline.py:165-192) collapses into those two.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from ._model import PretrainedPipeline, read_scheduler_config
from .schedulers import (CONTEXT_WEIGHTS, DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler, check_free_init,
                         context_windows, free_init_filter, free_init_steps)


class TextToVideoSDPipelineOutput(SimpleNamespace):
    pass


def _variance_noise(latents, generator):
    """The noise of one stochastic (eta > 0) scheduler step: fp32, drawn in the shape the reference hands the scheduler,
    [clips*frames, C, h, w] (reference models/pipeline.py:187-189), on the latents' device.  A generator living on another device
    draws there and the result is moved, as diffusers' randn_tensor does."""
    b, c, f, h, w = latents.shape
    dev = latents.device
    gdev = generator.device if generator is not None else dev
    if gdev.type == dev.type:
        return torch.randn((b * f, c, h, w), generator=generator, device=dev, dtype=torch.float32)
    return torch.randn((b * f, c, h, w), generator=generator, device=gdev, dtype=torch.float32).to(dev)


def _free_init_noise(latents, generator):
    """The fresh noise of one FreeInit re-initialisation: fp32 in the latents' own shape (diffusers `randn_tensor(latents.shape)`), with
    the generator-device handling of `_variance_noise`."""
    dev = latents.device
    gdev = generator.device if generator is not None else dev
    if gdev.type == dev.type:
        return torch.randn(tuple(latents.shape), generator=generator, device=dev, dtype=torch.float32)
    return torch.randn(tuple(latents.shape), generator=generator, device=gdev, dtype=torch.float32).to(dev)


def _latent_layout(flat, latents):
    """[clips*frames, C, h, w] -> the latents' [clips, C, frames, h, w]."""
    b, c, f, h, w = latents.shape
    return flat.reshape(b, f, c, h, w).permute(0, 2, 1, 3, 4).contiguous()


def tensor_to_vae_latent(t, vae):
    """reference utils/common.py:12-20."""
    b, f = t.shape[:2]
    lat = vae.encode(t.reshape((b * f,) + tuple(t.shape[2:]))).latent_dist.mode()
    lat = lat.reshape((b, f) + tuple(lat.shape[1:])).permute(0, 2, 1, 3, 4)
    return lat * 0.18215


def DDPM_forward(x0, step, num_frames, scheduler, generator=None):
    """reference utils/common.py:22-30 (what app.py:91 starts from): x0 repeated over frames and noised with
    prod(scheduler.alphas[t:]), t = scheduler.timesteps[-1]; needs a scheduler with `alphas` (DDIMScheduler).  `step` is
    unused, as in the reference; returns (xt, None)."""
    t = int(scheduler.timesteps[-1])
    xt = x0.repeat(1, 1, num_frames, 1, 1) if x0.shape[2] == 1 else x0
    eps = torch.randn(xt.shape, dtype=xt.dtype, device=xt.device, generator=generator)
    alpha_vec = torch.prod(scheduler.alphas[t:]).to(device=xt.device, dtype=xt.dtype)
    return torch.sqrt(alpha_vec) * xt + torch.sqrt(1 - alpha_vec) * eps, None


def DDPM_forward_timesteps(x0, step, num_frames, scheduler, generator=None):
    """reference utils/common.py:32-48: x0 repeated over frames, noised to timesteps[len-step]."""
    timesteps = scheduler.timesteps[len(scheduler.timesteps) - step:]
    xt = x0.repeat(1, 1, num_frames, 1, 1) if x0.shape[2] == 1 else x0
    noise = torch.randn(xt.shape, dtype=xt.dtype, device=xt.device, generator=generator)
    t = torch.tensor([int(timesteps[0])] * xt.shape[0], device=xt.device)
    return scheduler.add_noise(xt, noise, t), timesteps


def calculate_latent_motion_score(latents):
    """reference utils/common.py:296-300."""
    diff = (latents[:, :, 1:] - latents[:, :, :-1]).abs()
    return diff.mean(dim=[2, 3, 4]).sum(dim=1) * 10


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    """diffusers `rescale_noise_cfg` (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4): the guided
    prediction scaled per sample to the deviation of the text prediction, blended with weight `guidance_rescale`; evaluated in fp32
    (float64 operands stay float64).  guidance_rescale = 0 returns `noise_cfg` itself.  A sample whose guided prediction is constant
    (deviation 0: NaN in diffusers) is left unscaled, as aa_cfg_rescale_tokens leaves it."""
    if guidance_rescale == 0:
        return noise_cfg
    wide = torch.float64 if noise_cfg.dtype == torch.float64 else torch.float32
    cfg, text = noise_cfg.to(wide), noise_pred_text.to(wide)
    dims = list(range(1, cfg.dim()))
    std_text, std_cfg = text.std(dim=dims, keepdim=True), cfg.std(dim=dims, keepdim=True)
    ratio = torch.where(std_cfg > 0, std_text / std_cfg, torch.ones_like(std_cfg))
    noise_pred_rescaled = cfg * ratio
    return guidance_rescale * noise_pred_rescaled + (1 - guidance_rescale) * cfg


def _check_guidance_rescale(guidance_rescale):
    r = float(guidance_rescale)
    if not 0.0 <= r <= 1.0:                                   # (NaN fails both comparisons)
        raise ValueError(f"guidance_rescale {guidance_rescale!r}: a number in [0, 1]")
    return r


APG_DEFAULTS = dict(eta=0.0, norm_threshold=0.0, momentum=0.0)


def check_apg(apg):
    """The `apg` argument (Adaptive Projected Guidance: Sadat, Hilliges, Weber, "Eliminating Oversaturation and Artifacts of High
    Guidance Scales in Diffusion Models", 2024): None (off), or a mapping with the keys of APG_DEFAULTS - `eta` (the weight left to the
    part of the guidance update parallel to the text prediction; 1 is plain guidance, default 0), `norm_threshold` (the update's norm
    is clipped to it; 0, the default: no clipping) and `momentum` (of the running update, |momentum| < 1; 0, the default: none) - any
    of them left out taking its default.  An unknown key, a value that is no finite number, a negative threshold or |momentum| >= 1
    raises ValueError.  Returns the completed dict, or None.
    The paper's recommended ranges: eta in [0, 1) (0 in most of its experiments), a negative momentum between -0.75 and -0.25 (-0.5
    for most models) and a norm_threshold between 2.5 and 15 at ITS models' latent sizes; the threshold is a norm over the whole clip
    (channels * frames * h * w elements here), so it does not carry over from an image model.  Nobody has tuned any of the three for
    this model."""
    if apg is None:
        return None
    if not hasattr(apg, "keys"):
        raise ValueError(f"apg {apg!r}: None, or a mapping with keys from {sorted(APG_DEFAULTS)}")
    unknown = sorted(set(apg.keys()) - set(APG_DEFAULTS))
    if unknown:
        raise ValueError(f"apg: unknown key(s) {unknown} (known: {sorted(APG_DEFAULTS)})")
    a = dict(APG_DEFAULTS)
    for key in apg.keys():
        v = apg[key]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v):
            raise ValueError(f"apg.{key} = {v!r}: a finite number")
        a[key] = float(v)
    if a["norm_threshold"] < 0.0:
        raise ValueError(f"apg.norm_threshold = {a['norm_threshold']}: not negative (0: no clipping)")
    if abs(a["momentum"]) >= 1.0:
        raise ValueError(f"apg.momentum = {a['momentum']}: |momentum| < 1")
    return a


def adaptive_projected_guidance(pred_uncond, pred_text, guidance_scale, eta=0.0, norm_threshold=0.0, momentum=0.0, running=None):
    """Adaptive Projected Guidance as a torch expression (the definition of aa_apg_tokens, include/aa_mi355.h), per sample, reduced over
    every dimension but the first: d = text - uncond; with momentum != 0, d = running = d + momentum * running (`running`: the state
    of the previous call, None: zeros); s = min(1, norm_threshold / |d|) (norm_threshold 0: 1); p = s <d, text> / <text, text> (0 for a
    text prediction of zeros); the result is (1 + (g - 1)(eta - 1) p) text + (g - 1) s d.  Evaluated in float64; returned as fp32 for
    16- and 32-bit operands, float64 for float64.  Returns (guided, running) - running is None while momentum == 0."""
    ret = torch.float64 if pred_text.dtype == torch.float64 else torch.float32
    u, t = pred_uncond.to(torch.float64), pred_text.to(torch.float64)
    dims = list(range(1, t.dim()))
    d = t - u
    if momentum != 0:
        d = d + momentum * running.to(torch.float64) if running is not None else d
        running = d.to(ret)
    else:
        running = None
    dd, dt, tt = ((x * y).sum(dim=dims, keepdim=True) for x, y in ((d, d), (d, t), (t, t)))
    s = torch.ones_like(dd)
    if norm_threshold > 0:
        clip = dd > float(norm_threshold) ** 2
        s = torch.where(clip, float(norm_threshold) / torch.sqrt(torch.where(clip, dd, torch.ones_like(dd))), s)
    p = torch.where(tt > 0, s * dt / torch.where(tt > 0, tt, torch.ones_like(tt)), torch.zeros_like(tt))
    g1 = float(guidance_scale) - 1.0
    guided = (1.0 + g1 * (float(eta) - 1.0) * p) * t + g1 * s * d
    return guided.to(ret), running


def _apg_setup(apg, guidance_rescale):
    """check_apg for a sampling call: the completed dict or None; together with guidance_rescale > 0 ValueError (the two remedies are
    not combined: each rewrites the guided prediction from the raw halves)."""
    a = check_apg(apg)
    if a is not None and _check_guidance_rescale(guidance_rescale) > 0.0:
        raise ValueError("apg and guidance_rescale > 0 cannot be combined: choose one remedy for the guidance scale")
    return a


CONTEXT_DEFAULTS = dict(frames=16, overlap=4, weights="pyramid", closed_loop=False)
CONTEXT_MAX_FRAMES = 64                                       # AA_WINDOW_MAX: the slots a window descriptor carries by value


def check_context(context):
    """The `context` argument (context windows: sampling clips longer than the UNet's frame window): None (off), or a mapping with the
    keys of CONTEXT_DEFAULTS - `frames` (window length, 1 .. 64), `overlap` (0 <= overlap < frames), `weights` ("flat" / "pyramid"),
    `closed_loop` - any of them left out taking its default; an unknown key or a value out of range raises ValueError.  Returns the
    completed dict, or None."""
    if context is None:
        return None
    if not hasattr(context, "keys"):
        raise ValueError(f"context {context!r}: a mapping with keys from {sorted(CONTEXT_DEFAULTS)}")
    unknown = sorted(set(context.keys()) - set(CONTEXT_DEFAULTS))
    if unknown:
        raise ValueError(f"context: unknown key(s) {unknown} (known: {sorted(CONTEXT_DEFAULTS)})")
    c = dict(CONTEXT_DEFAULTS)
    c.update({k: context[k] for k in context.keys()})
    for k in ("frames", "overlap"):
        if isinstance(c[k], bool) or not isinstance(c[k], int):
            raise ValueError(f"context.{k} = {c[k]!r}: an integer")
    if not 1 <= c["frames"] <= CONTEXT_MAX_FRAMES:
        raise ValueError(f"context.frames = {c['frames']}: a window of 1 .. {CONTEXT_MAX_FRAMES} frames")
    if not 0 <= c["overlap"] < c["frames"]:
        raise ValueError(f"context.overlap = {c['overlap']}: 0 <= overlap < frames ({c['frames']})")
    if c["weights"] not in CONTEXT_WEIGHTS:
        raise ValueError(f"context.weights = {c['weights']!r}: one of {CONTEXT_WEIGHTS}")
    if not isinstance(c["closed_loop"], bool):
        raise ValueError(f"context.closed_loop = {c['closed_loop']!r}: true or false")
    return c


def _context_schedule(context, num_frames):
    """The step's windows (schedulers.context_windows) when `context` asks for a window shorter than the clip, else None: the
    unwindowed loop."""
    c = check_context(context)
    if c is None or c["frames"] >= num_frames:
        return None
    return context_windows(num_frames, c["frames"], c["overlap"], c["closed_loop"], c["weights"])


KEEP_KEYS = ("latents", "mask", "noise", "image", "image_mask")


def check_keep(keep, condition_latent=None, mask=None):
    """The `keep` argument (the known-region blend of inpainting samplers: what the mask holds still stays on the input image while
    sampling): None or False (off), True, or a mapping with keys from KEEP_KEYS -
      `latents`     the known latents [1 | b, C, 1 | T, h, w]; default `condition_latent`
      `mask`        [1 | b, 1, 1 | T, h, w] in the motion mask's convention, 1 = free, 0 = held; default the call's `mask`
      `noise`       fp32 in the latents' shape; default None: one torch.randn per call, drawn by the pipeline
      `image`       pixel-space known frames in [-1, 1], [b, 3, H, W] or [b, 3, 1 | f, H, W], pasted back after decoding; default None
      `image_mask`  [H, W] or [1 | b, 1, 1 | f, H, W], required with `image` (and only then)
    An unknown key, known latents or a mask that neither the mapping nor the call supplies, and `image` without `image_mask` (or the
    reverse) raise ValueError.  Returns the completed dict (every key present), or None."""
    if keep is None or keep is False:
        return None
    if keep is True:
        keep = {}
    if not hasattr(keep, "keys"):
        raise ValueError(f"keep {keep!r}: None, true / false, or a mapping with keys from {sorted(KEEP_KEYS)}")
    unknown = sorted(set(keep.keys()) - set(KEEP_KEYS))
    if unknown:
        raise ValueError(f"keep: unknown key(s) {unknown} (known: {sorted(KEEP_KEYS)})")
    k = {key: keep[key] if key in keep.keys() else None for key in KEEP_KEYS}
    if k["latents"] is None:
        k["latents"] = condition_latent
    if k["mask"] is None:
        k["mask"] = mask
    if k["latents"] is None:
        raise ValueError("keep: no known latents - neither keep.latents nor `condition_latent` is given")
    if k["mask"] is None:
        raise ValueError("keep: no mask - neither keep.mask nor the call's `mask` is given")
    if (k["image"] is None) != (k["image_mask"] is None):
        raise ValueError("keep.image and keep.image_mask go together: the known frames and where they are pasted back")
    return k


def _keep_operands(k, x):
    """The tensors of a completed `keep` dict as ops.keep_blend takes them for the fp32 latents `x` [b, C, T, h, w]: (known, mask,
    noise) on x's device, contiguous, shapes checked (ValueError)."""
    b, c, frames, h, w = x.shape
    known = torch.as_tensor(k["latents"]).to(x.device)
    m = torch.as_tensor(k["mask"]).to(x.device)
    if not known.is_floating_point() or known.dtype not in ops._DT:
        known = known.to(torch.float32)
    if not m.is_floating_point() or m.dtype not in ops._DT:
        m = m.to(torch.float32)
    if known.dim() != 5 or known.shape[0] not in (1, b) or known.shape[1] != c or known.shape[2] not in (1, frames) or tuple(known.shape[3:]) != (h, w):
        raise ValueError(f"keep.latents {tuple(known.shape)}: [1 | {b}, {c}, 1 | {frames}, {h}, {w}]")
    if m.dim() != 5 or m.shape[0] not in (1, b) or m.shape[1] != 1 or m.shape[2] not in (1, frames) or tuple(m.shape[3:]) != (h, w):
        raise ValueError(f"keep.mask {tuple(m.shape)}: [1 | {b}, 1, 1 | {frames}, {h}, {w}]")
    noise = k["noise"]
    if noise is not None:
        noise = torch.as_tensor(noise)
        if noise.dtype != torch.float32 or tuple(noise.shape) != tuple(x.shape):
            raise ValueError(f"keep.noise: fp32 in the latents' shape {tuple(x.shape)}")
        noise = noise.to(x.device).contiguous()
    return known.contiguous(), m.contiguous(), noise


def _keep_image_operands(k, video):
    """(image, image_mask) of a completed `keep` dict for the decoded fp32 video [b, 3, f, H, W]: fp32 on its device, the image as
    [b, 3, 1 | f, H, W], the mask as [1 | b, 1, 1 | f, H, W]."""
    b, c, f, H, W = video.shape
    img = torch.as_tensor(k["image"]).to(device=video.device, dtype=torch.float32)
    if img.dim() == 4:
        img = img[:, :, None]
    m = torch.as_tensor(k["image_mask"]).to(device=video.device, dtype=torch.float32)
    if m.dim() == 2:
        m = m[None, None, None]
    if img.dim() != 5 or img.shape[0] not in (1, b) or img.shape[1] != c or img.shape[2] not in (1, f) or tuple(img.shape[3:]) != (H, W):
        raise ValueError(f"keep.image {tuple(img.shape)}: [{b}, {c}, {H}, {W}] or [{b}, {c}, 1 | {f}, {H}, {W}]")
    if m.dim() != 5 or m.shape[0] not in (1, b) or m.shape[1] != 1 or m.shape[2] not in (1, f) or tuple(m.shape[3:]) != (H, W):
        raise ValueError(f"keep.image_mask {tuple(m.shape)}: [{H}, {W}] or [1 | {b}, 1, 1 | {f}, {H}, {W}]")
    return img.contiguous(), m.contiguous()


def _keep_scalars(sched, ts, i):
    """(a, s) of the blend behind step i of the schedule `ts`: (sqrt(abar), sqrt(1 - abar)) at ts[i + 1], the level the solver has just
    reached, in float64 from `scheduler.alphas_cumprod`; (1, 0) behind the last step (the known latents themselves, no noise read)."""
    if i + 1 >= len(ts):
        return 1.0, 0.0
    abar = float(sched.alphas_cumprod[int(ts[i + 1])])
    return abar ** 0.5, (1.0 - abar) ** 0.5


def tensor2vid(video):
    """diffusers 0.24 tensor2vid (mean = std = 0.5): [b,c,f,h,w] -> list of f uint8 [h, b*w, c] frames."""
    video = (video.float() * 0.5 + 0.5).clamp(0, 1)
    b, c, f, h, w = video.shape
    frames = (video.permute(2, 3, 0, 4, 1).reshape(f, h, b * w, c) * 255).to(torch.uint8).cpu().numpy()
    return [fr for fr in frames]


class LatentToVideoPipeline(PretrainedPipeline):
    """`save_pretrained` (reference train.py:298-299; text_encoder/ + tokenizer/ through transformers when present) and `to`:
    _model.PretrainedPipeline."""

    class_name = "LatentToVideoPipeline"
    components = ("unet", "vae", "text_encoder", "tokenizer")
    on_device = ("vae", "unet", "text_encoder")
    cfg_shared_prefix = True     # compute the text-independent prefix of the UNet once per guidance pair: the same arithmetic per element, but
                                 # other tile shapes / summation orders in the shared part - the two forms differ inside the fp16 noise floor
                                 # (0.013-0.029 of the latents' range over three steps at guidance 9, tests/test_gpu_fullsize.py), not bit for bit
    guidance_group = None        # (role, process group) of distributed.guidance_pair: the two guidance halves on two GPUs

    def __init__(self, vae=None, text_encoder=None, tokenizer=None, unet=None, scheduler=None):
        self.vae, self.text_encoder, self.tokenizer, self.unet = vae, text_encoder, tokenizer, unet
        self.scheduler = scheduler if scheduler is not None else DPMSolverMultistepScheduler()
        self.vae_scale_factor = 2 ** (len(vae.config.block_out_channels) - 1) if vae is not None else 8

    @classmethod
    def from_pretrained(cls, path, text_encoder=None, vae=None, unet=None, tokenizer=None, scheduler=None,
                        scheduler_from_config=False, **_):
        """diffusers directory layout (reference train.py:799-804).  Components passed by the caller
        are used as they are; the scheduler is rebuilt from `scheduler/scheduler_config.json`: as DPM-Solver++ (what the
        reference's train / eval path installs over it, train.py:806-808), or with `scheduler_from_config=True` as the class
        the file names when that is `DDIMScheduler` (what the reference's app samples with) or `UniPCMultistepScheduler`."""
        from .unet3d import UNet3DConditionModel
        from .vae import AutoencoderKL
        if unet is None:
            unet = UNet3DConditionModel.from_pretrained(path, subfolder="unet")
        if vae is None:
            vae = AutoencoderKL.from_pretrained(path, subfolder="vae")
        if scheduler is None:
            cfg = read_scheduler_config(path)
            named = {"DDIMScheduler": DDIMScheduler, "UniPCMultistepScheduler": UniPCMultistepScheduler}
            kind = named.get(cfg.get("_class_name"), DPMSolverMultistepScheduler) if scheduler_from_config else DPMSolverMultistepScheduler
            scheduler = kind.from_config(cfg)
        if tokenizer is None or text_encoder is None:
            try:                   # the tokenizer is transformers' (host-side string processing), the text tower is clip.py
                from transformers import CLIPTokenizer
                from .clip import CLIPTextModel
                tokenizer = tokenizer or CLIPTokenizer.from_pretrained(path, subfolder="tokenizer")
                text_encoder = text_encoder or CLIPTextModel.from_pretrained(path, subfolder="text_encoder")
            except Exception:      # text encoder is optional: callers may pass prompt_embeds
                pass
        return cls(vae, text_encoder, tokenizer, unet, scheduler)

    def enable_freeu(self, s1, s2, b1, b2):
        """diffusers `TextToVideoSDPipeline.enable_freeu`: forwards to the UNet (UNet3DConditionModel.enable_freeu)."""
        self.unet.enable_freeu(s1=s1, s2=s2, b1=b1, b2=b2)

    def disable_freeu(self):
        self.unet.disable_freeu()

    free_init = None             # the completed dict of check_free_init while FreeInit is enabled on the pipeline

    def enable_free_init(self, num_iters=3, use_fast_sampling=False, method="butterworth", order=4, spatial_stop_frequency=0.25,
                         temporal_stop_frequency=0.25):
        """diffusers `FreeInitMixin.enable_free_init` (Wu et al., "FreeInit: Bridging Initialization Gap in Video Diffusion Models"):
        every call samples `num_iters` times, each later iteration starting from the previous result re-noised to the last training
        timestep, low-passed over (frames, h, w) and filled up with the high frequencies of fresh noise (`__call__`).  A per-call
        `free_init=dict(...)` overrides what is set here."""
        self.free_init = check_free_init(dict(num_iters=num_iters, use_fast_sampling=use_fast_sampling, method=method, order=order,
                                              spatial_stop_frequency=spatial_stop_frequency, temporal_stop_frequency=temporal_stop_frequency))

    def disable_free_init(self):
        self.free_init = None

    def free_init_scalars(self):
        """(sqrt(abar), sqrt(1 - abar)) at the last training timestep: the re-noising `scheduler.add_noise(x, n0, N - 1)` of FreeInit."""
        abar = float(self.scheduler.alphas_cumprod[self.scheduler.config.num_train_timesteps - 1])
        return abar ** 0.5, (1.0 - abar) ** 0.5

    @staticmethod
    def free_init_tables(free_init, latents):
        """The kernel tables (ops.free_init_tables) of the filter `free_init` describes, for the latents' whole [frames, h, w]."""
        T, h, w = latents.shape[-3:]
        mask = free_init_filter(T, h, w, free_init["method"], free_init["order"], free_init["spatial_stop_frequency"],
                                free_init["temporal_stop_frequency"])
        return ops.free_init_tables(T, h, w, mask, latents.device)

    # ------------------------------------------------------------------ helpers (diffusers TextToVideoSDPipeline)
    def check_inputs(self, prompt, height, width, callback_steps, negative_prompt=None, prompt_embeds=None,
                     negative_prompt_embeds=None):
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_steps is None or not isinstance(callback_steps, int) or callback_steps <= 0:
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps}.")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError("Cannot forward both `prompt` and `prompt_embeds`.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")

    def _encode_prompt(self, prompt, device, do_cfg, negative_prompt=None, prompt_embeds=None,
                       negative_prompt_embeds=None):
        def clip(texts):
            ids = self.tokenizer(texts, padding="max_length", max_length=self.tokenizer.model_max_length,
                                 truncation=True, return_tensors="pt").input_ids.to(device)
            return self.text_encoder(ids)[0]

        if prompt_embeds is None:
            if self.text_encoder is None or self.tokenizer is None:
                raise ValueError("no text encoder loaded: pass `prompt_embeds` / `negative_prompt_embeds`")
            texts = [prompt] if isinstance(prompt, str) else list(prompt)
            prompt_embeds = clip(texts)
        if do_cfg and negative_prompt_embeds is None:
            if self.text_encoder is None or self.tokenizer is None:
                raise ValueError("classifier-free guidance needs `negative_prompt_embeds` when no text encoder is loaded")
            neg = [negative_prompt or ""] * prompt_embeds.shape[0] if not isinstance(negative_prompt, list) else negative_prompt
            negative_prompt_embeds = clip(neg)
        if do_cfg:
            prompt_embeds = torch.cat([negative_prompt_embeds.to(prompt_embeds), prompt_embeds])
        return prompt_embeds

    def decode_latents(self, latents):
        latents = latents / self.vae.config.scaling_factor
        b, c, f, h, w = latents.shape
        img = self.vae.decode(latents.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)).sample
        return img.reshape((b, f) + tuple(img.shape[1:])).permute(0, 2, 1, 3, 4).float()

    # ------------------------------------------------------------------ denoising
    def denoise(self, latents, prompt_embeds, condition_latent, mask, motion, timesteps, guidance_scale,
                callback=None, callback_steps=1, eta=0.0, generator=None, guidance_rescale=0.0, context=None, keep=None, apg=None):
        """The hot loop (reference pipeline.py:163-198).  `prompt_embeds` already holds [uncond; text]
        when guidance is on.  Latents are kept in fp32.

        With the DPM-Solver++, the DDIM or the UniPC scheduler one step is exactly two device submissions: the UNet session (a hipGraph
        replay holding timestep embedding + input packing + the whole forward when graphs are enabled) and the fused
        guidance + solver kernel, which reads the UNet's token-layout output, updates the fp32 latents in place - they ARE
        the session's `sample` input, duplicated for guidance by the packing kernel - and deposits the next timestep.
        `eta` / `generator` reach the scheduler as in the reference (pipeline.py:156,189): DDIM with eta > 0 adds one
        torch.randn per step, DPM-Solver++ and UniPC take neither.  UniPC keeps four fp32 buffers of the latents' size for
        the length of the call (the corrected sample and three data predictions).
        `guidance_rescale` > 0 under guidance (diffusers' argument, `rescale_noise_cfg`): the step becomes session run,
        ops.cfg_rescale_tokens - the rescaled guided prediction written over the unconditional half of the token matrix, two
        launches - and the same solver kernel with guidance off.  With 0, the default, a step issues what it issued before.
        `context` (check_context; context windows) with `frames` below the clip's length: the session is built for `frames` frames and
        the fp32 latents of the whole clip live in a buffer of their own; per step every window of schedulers.context_windows runs
        ops.window_gather_latents into the session's `sample`, the session, (ops.cfg_rescale_tokens, per window,) and
        ops.window_merge_tokens, which blends the window's prediction into one token matrix of the clip's length (both guidance halves:
        a frame held by one window keeps the UNet's bits); then the same solver kernel runs once on that matrix with the same guidance.  The solver state is sized from the long latents.  None, or a window
        that holds the whole clip: the loop of before, no window op.
        `keep` (check_keep; the known-region blend of inpainting samplers): behind the solver kernel of step i one ops.keep_blend, in
        place on the whole clip's fp32 latents (under context windows: the long buffer), overwrites what the mask holds still with
        a_i * known + s_i * noise, (a_i, s_i) = (sqrt(abar), sqrt(1 - abar)) at the NEXT timestep - the level the solver has just
        reached - and (1, 0) behind the last step, so the held region ends as the known latents bit for bit; where the mask is 1 the
        launch hands the latents through untouched.  One noise tensor serves the whole call (and every FreeInit iteration).  The
        callback sees the blended latents; nothing is blended before the first step.  Under a guidance pair both ranks blend alike
        (their generators must agree, as for eta > 0).  UniPC is refused (`_keep_setup`).  None / False: no launch, no randn.
        `apg` (check_apg; Adaptive Projected Guidance) under guidance: the step becomes session run, ops.apg_tokens - the projected
        guided prediction written over the unconditional half of the token matrix, two launches - and the same solver kernel with
        guidance off: the path `guidance_rescale` takes, for all three solvers.  With momentum the fp32 buffer of the running update
        (the size of the latents) is allocated and zeroed here, so every `denoise` - every FreeInit iteration - starts afresh.  Under
        context windows APG runs per window, in front of the merge, with one momentum buffer per window of the schedule (a
        departure, as for guidance_rescale: the merge writes a blended frame to both halves, so the merged matrix cannot be guided
        afterwards; norms and projections are the window's).  Under a guidance pair both ranks run it on the gathered matrix alike.
        Together with guidance_rescale > 0: ValueError.  None, or guidance_scale <= 1: no launch, no buffer, the loop of before."""
        k = self._keep_setup(keep, condition_latent, mask, latents, generator)
        cfg = guidance_scale > 1.0
        rescale = _check_guidance_rescale(guidance_rescale) if cfg else 0.0
        apg = _apg_setup(apg, guidance_rescale) if cfg else None
        windows = _context_schedule(context, latents.shape[2])
        sched = self.scheduler
        unet = self.unet
        if not (isinstance(sched, (DPMSolverMultistepScheduler, DDIMScheduler, UniPCMultistepScheduler)) and hasattr(unet, "session")):
            return self._denoise_generic(latents, prompt_embeds, condition_latent, mask, motion, timesteps, guidance_scale,
                                         callback, callback_steps, eta, generator, guidance_rescale=guidance_rescale, context=context, keep=k,
                                         apg=apg)
        dev = latents.device
        b0, _, frames, h, w = latents.shape
        wf = frames if windows is None else len(windows[0][0])  # frames the UNet sees at a time
        use_mask = bool(unet.motion_mask and mask is not None)
        has_motion = bool(unet.motion_strength and motion is not None)
        pair = self.guidance_group if cfg else None
        if pair is not None:
            # Latency mode: this rank runs ONE half of the guidance batch (role 0: unconditional context = first half of `prompt_embeds`,
            # role 1: the text half), the pair exchanges the UNet outputs with one all-gather per step (RCCL over xGMI) and both ranks
            # apply the identical guidance + solver update to their copy of the latents.  Same arithmetic per element (the two halves of
            # a guidance batch never interact inside the UNet); eta > 0: both ranks must hold generators in the same state.
            from . import distributed as D
            role, group = pair
            b, text, shared = b0, prompt_embeds[role * b0:(role + 1) * b0], False
        else:
            # under guidance both halves of the UNet batch see the same latents / condition frame / mask / timestep / motion and
            # differ only in the text: the UNet computes the text-independent prefix once (UNet3DConditionModel._core cfg_dup)
            b, text = 2 * b0 if cfg else b0, prompt_embeds
            shared = cfg and self.cfg_shared_prefix and b0 % condition_latent.shape[0] == 0 and (not use_mask or b0 % mask.shape[0] == 0)
        sess = unet.session(b, wf, h, w, tuple(text.shape[1:]), use_mask, has_motion, False, torch.float32, b0,
                            condition_latent.shape[0], mask.shape[0] if use_mask else 0, dev, cfg_dup=shared)
        tokens = sess.run                                       # [b*(T+1)*h*w, 8], columns [0, out_channels) valid (row pitch = stride(0))
        if pair is not None:
            # (the token matrix is padded to 8 columns: only conv_out's channels travel - 0.28 MB per rank at 16x64x64)
            tokens = lambda: D.all_gather_cat(sess.run()[:, :unet.conv_out.out_channels], group)   # [uncond clips | text clips], the layout the solver kernel reads
        mot = None
        if has_motion:
            mot = torch.as_tensor(motion, device=dev).to(torch.float32).reshape(-1).expand(b).contiguous()
        ts = [int(t) for t in timesteps]
        sess.load(sample=latents if windows is None else None, cond=condition_latent, mask=mask if use_mask else None, text=text, motion=mot,
                  t=torch.full((b,), float(ts[0]) if ts else 0.0, dtype=torch.float32, device=dev))
        pre = rescale > 0.0 or apg is not None                  # the token matrix is guided in front of the solver kernel, which runs with guidance off
        guidance = guidance_scale if cfg and not pre else None
        if windows is None:
            x = sess.inputs["sample"]                           # fp32 [b0,C,T,h,w]: updated in place by the solver kernel
        else:
            # the clip's latents in a buffer of their own; the session's `sample` holds one window at a time (the gather fills it)
            x = latents.to(torch.float32).contiguous().clone()
            descs = [ops.window_desc(win) for win in windows]
            acc = torch.empty((b0, frames, h * w, x.shape[1]), dtype=torch.float32, device=dev)
            halves = 2 if cfg and not pre else 1                # a UNet output of the clip's length: [uncond clips | text clips]
            merged = torch.zeros((halves * b0 * (frames + 1) * h * w, 8), dtype=unet.dtype, device=dev)
        step = self._solver_step(x, eta, generator)
        if k is not None:
            known, held, knoise = _keep_operands(k, x)
        if apg is not None:                                     # the running update r, zero before the first step: one buffer per UNet run of a step
            runs = 1 if windows is None else len(windows)
            running = [torch.zeros(b0 * wf * h * w * x.shape[1], dtype=torch.float32, device=dev) if apg["momentum"] != 0.0 else None
                       for _ in range(runs)]

        def guide(tok, j):
            """The guided prediction over the unconditional half of `tok`, the output of the step's j-th UNet run (in place: the next
            session run, or gather, rewrites the matrix)."""
            if rescale > 0.0:
                ops.cfg_rescale_tokens(tok, b0, x.shape[1], wf, h * w, guidance_scale, rescale)
            elif apg is not None:
                ops.apg_tokens(tok, b0, x.shape[1], wf, h * w, guidance_scale, apg["eta"], apg["norm_threshold"], apg["momentum"],
                               momentum_buf=running[j])
        for i, t in enumerate(ts):
            if windows is None:
                tok = tokens()
                if pre:
                    guide(tok, 0)
            else:
                for j, win in enumerate(descs):                 # schedule order: a frame's first window writes `acc`, its last `merged`
                    ops.window_gather_latents(x, win, out=sess.inputs["sample"])
                    wtok = tokens()
                    if pre:                                     # per window (a departure: deviations, norms and projections are the window's, not the clip's)
                        guide(wtok, j)
                    ops.window_merge_tokens(wtok, acc, merged, win, guidance)
                tok = merged
            step(tok, guidance, t, i, sess.inputs["t"], float(ts[i + 1]) if i + 1 < len(ts) else float(t))
            if k is not None:
                a, s = _keep_scalars(sched, ts, i)
                ops.keep_blend(x, known, held, a, s, noise=knoise if i + 1 < len(ts) else None)
            if callback is not None and i % callback_steps == 0:
                callback(i, t, x)
        return x.clone()

    def _solver_step(self, x, eta, generator):
        """The scheduler's part of the fused loop: returns step(tokens, guidance, t, i, next_t, next_t_value), one fused guidance +
        solver update of the fp32 latents `x` from the UNet's token-layout output (`i` counts the steps of this run before it).  The
        closure owns the solver state: the previous x0 for DPM-Solver++, the four buffers of `_unipc_state` (history rotated per step)
        for UniPC, none for DDIM, where eta > 0 draws the step's variance noise first (one torch.randn + the relayout into the
        latents' order; eta = 0 launches nothing else)."""
        sched = self.scheduler
        if isinstance(sched, DDIMScheduler):
            def step(tokens, guidance, t, i, next_t, next_t_value):
                k = sched.coefficients(sched.index_for_timestep(t), eta)
                noise = _latent_layout(_variance_noise(x, generator), x) if eta > 0 else None
                ops.cfg_ddim_step_tokens(tokens, x, None, guidance, k, noise=noise if k["c_n"] != 0.0 else None,
                                         next_t=next_t, next_t_value=next_t_value)
        elif isinstance(sched, UniPCMultistepScheduler):
            state = self._unipc_state(x)

            def step(tokens, guidance, t, i, next_t, next_t_value):
                k = sched.coefficients(sched.index_for_timestep(t), i)
                state[1:] = ops.cfg_unipc_step_tokens(tokens, x, None, guidance, k, state[0], state[1:],
                                                      next_t=next_t, next_t_value=next_t_value)
        else:
            x0_prev = torch.zeros_like(x)

            def step(tokens, guidance, t, i, next_t, next_t_value):
                k = sched.coefficients(sched.index_for_timestep(t), i > 0)
                ops.cfg_dpm_step_tokens(tokens, x, x0_prev, None, guidance, k, next_t=next_t, next_t_value=next_t_value)
        return step

    def _keep_setup(self, keep, condition_latent, mask, latents, generator):
        """check_keep for this pipeline and these latents: the completed dict with its `noise` in place - left out, it is drawn here,
        one torch.randn of the latents' shape (fp32, the caller's generator, a generator on another device handled as
        `_free_init_noise` handles it) - or None (off: nothing is drawn).  A completed dict passes through unchanged, so `__call__`
        draws once and every `denoise` of the call blends with the same noise.  Raises ValueError, before any device work, for a
        scheduler the blend cannot serve."""
        k = check_keep(keep, condition_latent, mask)
        if k is None:
            return None
        if isinstance(self.scheduler, UniPCMultistepScheduler):
            raise ValueError("keep: not available with UniPCMultistepScheduler - its corrector rebuilds the sample from its own `last_sample` "
                             "and never reads the sample it is handed, so the blend would be dropped from the trajectory while still "
                             "steering the UNet; sample with DPM-Solver++ or DDIM")
        if not hasattr(self.scheduler, "alphas_cumprod"):
            raise ValueError(f"keep: {type(self.scheduler).__name__} has no `alphas_cumprod` to take the noise level of a step from")
        if k["noise"] is None:
            k["noise"] = _free_init_noise(latents, generator)
        return k

    @staticmethod
    def _unipc_state(x):
        """The four fp32 buffers a UniPC run keeps next to the latents: [corrected sample, m of the previous step, of the second
        previous, of the third previous] (zeroed: a coefficient of zero must not meet a NaN)."""
        return [torch.zeros_like(x) for _ in range(4)]

    def _denoise_generic(self, latents, prompt_embeds, condition_latent, mask, motion, timesteps, guidance_scale,
                         callback=None, callback_steps=1, eta=0.0, generator=None, guidance_rescale=0.0, context=None, keep=None, apg=None):
        """Any scheduler with a diffusers-style `step()`: the UNet through its module `forward`, guidance and the update as
        torch expressions (the reference's own sequence, pipeline.py:165-192).  `eta` / `generator` go to a `step()` that
        names them (diffusers' prepare_extra_step_kwargs, pipeline.py:156); DDIM's variance noise is drawn here exactly as
        the fused loop draws it, so both consume the generator alike.  `guidance_rescale` > 0 under guidance applies
        `rescale_noise_cfg` to the guided prediction.  `context` with a window shorter than the clip (check_context): per step the
        module forward, guidance and `rescale_noise_cfg` run per window of schedulers.context_windows, the guided predictions are
        summed in fp32 with the windows' per-frame weights, and `step()` is applied once to the whole clip.  `keep` (check_keep): the
        blend of `denoise` behind every `step()`, as torch expressions with the same selection at the mask's endpoints.  `apg`
        (check_apg) under guidance: `adaptive_projected_guidance` in the place of the guidance expression, its running update kept per
        UNet run of a step - one for the clip, or one per window of the schedule - and zero before the first step."""
        import inspect
        k = self._keep_setup(keep, condition_latent, mask, latents, generator)
        cfg = guidance_scale > 1.0
        rescale = _check_guidance_rescale(guidance_rescale) if cfg else 0.0
        apg = _apg_setup(apg, guidance_rescale) if cfg else None
        running = {}                                            # window number -> the running update of APG's momentum
        windows = _context_schedule(context, latents.shape[2])
        dt = self.unet.dtype
        sched = self.scheduler
        accepted = set(inspect.signature(sched.step).parameters)
        extra = {}
        if "eta" in accepted:
            extra["eta"] = eta
        if "generator" in accepted and not isinstance(sched, DDIMScheduler):
            extra["generator"] = generator
        x = latents.float().contiguous()
        cond = torch.cat([condition_latent, condition_latent]) if cfg else condition_latent     # :160-161
        if k is not None:
            known, held, knoise = _keep_operands(k, x)
            known, held, ts = known.float(), held.float(), [int(t) for t in timesteps]

        def predict(xs, t, j=0):
            """The (guided, rescaled) fp32 prediction for the latents `xs` - the clip, or window `j` of it."""
            x_lp = xs.to(dt)
            model_in = torch.cat([x_lp, x_lp]) if cfg else x_lp                                  # :165
            eps = self.unet(model_in, t, encoder_hidden_states=prompt_embeds, condition_latent=cond, mask=mask,
                            motion=None if motion is None else torch.as_tensor(motion, device=x.device)).sample
            e_u, e_t = (eps[: xs.shape[0]], eps[xs.shape[0]:]) if cfg else (eps, eps)
            if apg is not None:
                e, running[j] = adaptive_projected_guidance(e_u.float(), e_t.float(), guidance_scale, apg["eta"], apg["norm_threshold"],
                                                            apg["momentum"], running.get(j))
                return e
            e = e_u.float() + guidance_scale * (e_t.float() - e_u.float()) if cfg else eps.float()
            if rescale > 0.0:
                e = rescale_noise_cfg(e, e_t.float(), rescale)
            return e

        for i, t in enumerate(timesteps):
            if windows is None:
                e = predict(x, t)
            else:
                e = torch.zeros_like(x)
                for j, (idx, wn, _first, _last) in enumerate(windows):
                    idx = torch.as_tensor(idx, device=x.device)
                    wn = torch.tensor(wn, dtype=torch.float64).to(device=x.device, dtype=torch.float32).reshape(1, 1, -1, 1, 1)
                    e[:, :, idx] += wn * predict(x[:, :, idx], t, j)
            b, c, f, h, w = x.shape
            if isinstance(sched, DDIMScheduler) and eta > 0:
                extra["variance_noise"] = _variance_noise(x, generator)
            flat = sched.step(e.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w), t,
                              x.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w), **extra).prev_sample
            x = flat.reshape(b, f, c, h, w).permute(0, 2, 1, 3, 4).contiguous()
            if k is not None:
                a, s = _keep_scalars(sched, ts, i)
                kn = a * known + s * knoise if i + 1 < len(ts) else a * known
                x = torch.where(held >= 1, x, torch.where(held <= 0, kn, held * x + (1 - held) * kn)).contiguous()
            if callback is not None and i % callback_steps == 0:
                callback(i, t, x)
        return x

    @torch.no_grad()
    def __call__(self, prompt=None, height=None, width=None, num_frames=16, num_inference_steps=50,
                 guidance_scale=9.0, negative_prompt=None, eta=0.0, generator=None, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, output_type="np", return_dict=True,
                 callback=None, callback_steps=1, cross_attention_kwargs=None, condition_latent=None,
                 mask=None, timesteps=None, motion=None, guidance_rescale=0.0, context=None, free_init=None, keep=None, apg=None):
        """`apg` (check_apg; None: off, the default): Adaptive Projected Guidance in the place of plain guidance at guidance_scale > 1
        (`denoise`): the guidance update's part parallel to the text prediction damped by `eta`, its norm clipped to `norm_threshold`,
        a `momentum` across the steps of one `denoise`.  DEPARTURES: applied to the model output as it comes (the paper argues on the
        denoised prediction), per window under context windows, refused together with guidance_rescale > 0 (ValueError).
        `keep` (check_keep; None / False: off, the default): the known-region blend of inpainting samplers - what the mask holds still
        (mask 0) is put back on the known latents, noised to the step's level, behind every solver step (`denoise`), and with
        keep.image / keep.image_mask the known pixels are pasted over the decoded fp32 video by one more ops.keep_blend in front of
        `tensor2vid`.  The noise of the call is drawn once, here, in front of the first FreeInit iteration.  Off: no launch, no randn.
        `free_init` (a mapping, check_free_init; None: what `enable_free_init` set, off by default) with num_iters > 1 - FreeInit:
        the clip is sampled num_iters times.  Iteration 0 starts from the caller's latents n0; iteration i >= 1 from
        ops.freeinit_mix(x, n0, z): the previous result x re-noised with n0 to the last training timestep, low-passed over the clip's
        whole (frames, h, w), the high frequencies taken from z = one torch.randn of the latents' shape (fp32, the caller's generator).
        `set_timesteps` runs before every iteration (a multistep scheduler's state starts afresh), under `use_fast_sampling` with
        free_init_steps(...) steps - which a caller's own `timesteps` cannot follow: ValueError.  The mix sits outside `denoise`, so
        guidance_rescale, context windows and FreeU compose with it unchanged.  DEPARTURE from diffusers: the latents stay fp32 between
        iterations (diffusers rounds them to the model dtype).  num_iters = 1, or off: one `denoise`, no extra launch, no extra randn."""
        if latents is None:
            raise ValueError("LatentToVideoPipeline expects caller-prepared `latents` (reference pipeline.py:153)")
        apg = _apg_setup(apg, guidance_rescale)
        keep = self._keep_setup(keep, condition_latent, mask, latents, generator)
        fi = check_free_init(free_init) if free_init is not None else self.free_init
        iters = fi["num_iters"] if fi is not None else 1
        fast = iters > 1 and fi["use_fast_sampling"]
        if fast and timesteps is not None:
            raise ValueError("free_init.use_fast_sampling shortens the schedule per iteration: it cannot be combined with `timesteps`")
        height = height or latents.shape[-2] * self.vae_scale_factor
        width = width or latents.shape[-1] * self.vae_scale_factor
        self.check_inputs(prompt, height, width, callback_steps, negative_prompt, prompt_embeds, negative_prompt_embeds)
        device = latents.device
        do_cfg = guidance_scale > 1.0
        prompt_embeds = self._encode_prompt(prompt, device, do_cfg, negative_prompt, prompt_embeds, negative_prompt_embeds)
        x = latents
        if iters > 1:
            n0 = latents.to(torch.float32).contiguous()         # the run's initial noise, kept for every re-initialisation
            a, s = self.free_init_scalars()
            tables = self.free_init_tables(fi, latents)
        for it in range(iters):
            if it > 0:
                x = ops.freeinit_mix(x, n0, _free_init_noise(n0, generator), a, s, tables, out=x)
            self.scheduler.set_timesteps(free_init_steps(num_inference_steps, iters, it, fast), device=device)
            ts = self.scheduler.timesteps if timesteps is None else timesteps
            x = self.denoise(x, prompt_embeds, condition_latent, mask, motion, [int(t) for t in ts],
                             guidance_scale, callback, callback_steps, eta=eta, generator=generator, guidance_rescale=guidance_rescale,
                             context=context, keep=keep, apg=apg)
        latents = x.to(self.unet.dtype)
        if self.vae is None or output_type == "latent":
            video = None
        else:
            video_tensor = self.decode_latents(latents)
            if keep is not None and keep["image"] is not None:  # (decode_latents returns a permuted view: the kernel wants the planes dense)
                image, image_mask = _keep_image_operands(keep, video_tensor)
                video_tensor = ops.keep_blend(video_tensor.contiguous(), image, image_mask, 1.0, 0.0)
            video = video_tensor if output_type == "pt" else tensor2vid(video_tensor)
        if not return_dict:
            return (video, latents)
        return TextToVideoSDPipelineOutput(frames=video)
