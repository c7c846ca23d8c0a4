"""DDIM on the host: `schedulers.DDIMScheduler` against a float64 restatement of the DDIM update kept in this file (`RefDDIM`; diffusers
is not installed, the formulas are the published ones: Song et al. 2021, eq. 12 and 16), against the existing DPM-Solver++ class
where the two samplers coincide, `DDPM_forward`, `from_pretrained(scheduler_from_config=...)`, and the product denoising loops - the
fused one (UNet session + aa_cfg_ddim_step_tokens on the emulator) and the generic one - against the oracle loop driving `RefDDIM`."""
import json
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle
from animate_anything_amd import ops
from animate_anything_amd.pipeline import DDPM_forward, LatentToVideoPipeline
from animate_anything_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler


class RefDDIM:
    """float64 DDIM: `set_timesteps`, `timesteps`, `step(e, t, x) -> tensor` (what oracle.LatentToVideoPipeline drives).  Holds
    `eta`, `use_clipped_model_output` and the generator of the variance noise itself; the noise is drawn in fp32 in the shape of
    the model output (so that a product loop seeded alike sees the same numbers) and used in float64."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 clip_sample=False, clip_sample_range=1.0, set_alpha_to_one=False, steps_offset=1, prediction_type="epsilon",
                 timestep_spacing="leading", eta=0.0, use_clipped_model_output=False, generator=None):
        self.N, self.spacing, self.offset, self.pred = num_train_timesteps, timestep_spacing, steps_offset, prediction_type
        self.clip = clip_sample_range if clip_sample else None
        self.eta, self.recompute, self.generator = eta, use_clipped_model_output, generator
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32).double() ** 2
        else:
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32).double()
        self.abar = torch.cumprod(1.0 - betas, 0)
        self.abar_final = 1.0 if set_alpha_to_one else self.abar[0].item()

    def set_timesteps(self, n, device=None):
        N = self.N
        if self.spacing == "leading":
            ts = [int(round(i * (N // n))) + self.offset for i in range(n)][::-1]
        elif self.spacing == "linspace":
            ts = [int(v) for v in np.round(np.linspace(0, N - 1, n))][::-1]
        else:
            ts = [int(v) - 1 for v in np.round(np.arange(N, 0, -N / n))]
        self.n, self.timesteps = n, torch.tensor(ts)

    def step(self, e, t, x):
        t = int(t)
        t_prev = t - self.N // self.n
        a = self.abar[t].item()
        a_prev = self.abar[t_prev].item() if t_prev >= 0 else self.abar_final
        x, m = x.double(), e.double()
        if self.pred == "epsilon":
            x0, eps = (x - math.sqrt(1 - a) * m) / math.sqrt(a), m
        elif self.pred == "sample":
            x0, eps = m, (x - math.sqrt(a) * m) / math.sqrt(1 - a)
        else:
            x0, eps = math.sqrt(a) * x - math.sqrt(1 - a) * m, math.sqrt(a) * m + math.sqrt(1 - a) * x
        if self.clip is not None:
            x0 = x0.clamp(-self.clip, self.clip)
        sigma = self.eta * math.sqrt((1 - a_prev) / (1 - a) * (1 - a / a_prev))
        if self.recompute:
            eps = (x - math.sqrt(a) * x0) / math.sqrt(1 - a)
        out = math.sqrt(a_prev) * x0 + math.sqrt(1 - a_prev - sigma ** 2) * eps
        if self.eta > 0:
            out = out + sigma * torch.randn(e.shape, generator=self.generator, dtype=torch.float32).double()
        return out


# ---- (a) schedule and chained step against RefDDIM ----
@pytest.mark.parametrize("steps_offset", [0, 1])
@pytest.mark.parametrize("spacing", ["leading", "trailing", "linspace"])
@pytest.mark.parametrize("steps", [10, 25, 50])
def test_timesteps_match_the_restatement(steps, spacing, steps_offset):
    a = DDIMScheduler(timestep_spacing=spacing, steps_offset=steps_offset)
    b = RefDDIM(timestep_spacing=spacing, steps_offset=steps_offset)
    a.set_timesteps(steps)
    b.set_timesteps(steps)
    assert a.timesteps.tolist() == b.timesteps.tolist()
    assert a.num_inference_steps == steps and len(a.timesteps) == steps and a.timesteps.dtype == torch.int64
    if spacing == "leading":
        assert a.timesteps[0] == (1000 // steps) * (steps - 1) + steps_offset and a.timesteps[-1] == steps_offset
    if spacing == "trailing":
        assert a.timesteps[0] == 999


@pytest.mark.parametrize("recompute", [False, True], ids=["eps_model", "eps_clipped"])
@pytest.mark.parametrize("eta", [0.0, 0.7])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("steps", [10, 25, 50])
def test_chained_step_matches_the_restatement(steps, prediction_type, clip, eta, recompute):
    """All steps chained on [3,4,8,8] randn inputs, within 1e-4 of the float64 restatement (the bound of
    test_pipeline_host.test_dpm_solver_matches_oracle); both draw the variance noise from generators seeded alike."""
    kw = dict(prediction_type=prediction_type, clip_sample=clip, clip_sample_range=1.0)
    a = DDIMScheduler(**kw)
    b = RefDDIM(eta=eta, use_clipped_model_output=recompute, generator=torch.Generator().manual_seed(7), **kw)
    a.set_timesteps(steps)
    b.set_timesteps(steps)
    ga = torch.Generator().manual_seed(7)
    g = torch.Generator().manual_seed(0)
    xa = xb = torch.randn(3, 4, 8, 8, generator=g)
    worst = 0.0
    for t in a.timesteps:
        e = torch.randn(3, 4, 8, 8, generator=g)
        out = a.step(e, t, xa, eta=eta, use_clipped_model_output=recompute, generator=ga)
        xa, xb = out.prev_sample, b.step(e, t, xb)
        assert xa.dtype == torch.float32 and out.pred_original_sample.shape == xa.shape
        worst = max(worst, (xa.double() - xb).abs().max().item())
        assert (xa.double() - xb).abs().max() < 1e-4
    print(f"worst distance over the chain {worst:.3g}")


def test_config_surface():
    s = DDIMScheduler()
    assert s.order == 1 and s.init_noise_sigma == 1.0 and s.betas.shape == s.alphas.shape == s.alphas_cumprod.shape == (1000,)
    assert torch.equal(s.alphas, 1.0 - s.betas) and torch.allclose(s.alphas_cumprod, torch.cumprod(s.alphas, 0))
    assert s.final_alpha_cumprod == float(s.alphas_cumprod[0])
    assert DDIMScheduler(set_alpha_to_one=True).final_alpha_cumprod == 1.0
    assert DDIMScheduler(beta_schedule="linear", beta_start=1e-4, beta_end=2e-2).betas[-1].item() == pytest.approx(2e-2, rel=1e-6)
    for bad in (dict(thresholding=True), dict(rescale_betas_zero_snr=True)):
        with pytest.raises(NotImplementedError):
            DDIMScheduler(**bad)
    cfg = {"_class_name": "DDIMScheduler", "_diffusers_version": "0.24.0", "beta_end": 0.013, "clip_sample": True,
           "clip_sample_range": 2.0, "prediction_type": "v_prediction", "timestep_spacing": "trailing", "skip_prk_steps": True}
    c = DDIMScheduler.from_config(cfg, steps_offset=0)
    assert (c.config.beta_end, c.config.clip_sample, c.config.clip_sample_range, c.config.prediction_type, c.config.timestep_spacing,
            c.config.steps_offset) == (0.013, True, 2.0, "v_prediction", "trailing", 0)
    again = DDIMScheduler.from_config(c.config)
    assert vars(again.config) == vars(c.config)
    x = torch.randn(2, 4, 3, 3)
    assert s.scale_model_input(x, 5) is x
    s.set_timesteps(10)
    assert [s.index_for_timestep(t) for t in s.timesteps] == list(range(10))
    n, t = torch.randn(2, 4, 3, 3), torch.tensor([501, 1])
    acp = s.alphas_cumprod[t].reshape(2, 1, 1, 1).float()
    assert torch.allclose(s.add_noise(x, n, t), acp.sqrt() * x + (1 - acp).sqrt() * n, atol=1e-6)
    with pytest.raises(ValueError):
        s.step(x, 501, x, eta=0.5, generator=torch.Generator(), variance_noise=n)


# ---- (b) independent cross-check against the DPM-Solver++ class ----
@pytest.mark.parametrize("steps", [10, 25])
def test_deterministic_ddim_is_first_order_dpm_solver(steps):
    """eta = 0, no clipping, epsilon prediction: one DDIM step from alpha_bar_s to alpha_bar_t IS the first-order DPM-Solver++
    update (Lu et al. 2022, sec. 4.1).  The DPM side comes from the existing class: `_alpha_sigma` of its sigmas and the closed form
    x' = (sigma_t / sigma_s) x - alpha_t (exp(-h) - 1) x0, and - where its grid allows - its own `coefficients`.  1e-6 relative, float64."""
    dpm = DPMSolverMultistepScheduler()
    dpm.set_timesteps(steps)
    ddim = DDIMScheduler(clip_sample=False, prediction_type="epsilon")
    ddim.set_timesteps(steps)
    acp = ddim.alphas_cumprod.double()
    g = torch.Generator().manual_seed(3)
    x, e = torch.randn(64, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
    for i, t in enumerate(ddim.timesteps.tolist()):
        k = ddim.coefficients(i)
        assert k["c_n"] == 0.0 and k["clip"] is None and not k["eps_from_x0"]
        x0 = k["a_x"] * x + k["a_m"] * e
        got = k["c_0"] * x0 + k["c_e"] * (k["e_x"] * x + k["e_m"] * e)
        t_prev = t - 1000 // steps
        a_s = acp[t].item()
        a_t = acp[t_prev].item() if t_prev >= 0 else ddim.final_alpha_cumprod
        al_s, sg_s = DPMSolverMultistepScheduler._alpha_sigma(math.sqrt((1 - a_s) / a_s))
        al_t, sg_t = DPMSolverMultistepScheduler._alpha_sigma(math.sqrt((1 - a_t) / a_t))
        assert al_s == pytest.approx(math.sqrt(a_s), rel=1e-12) and sg_t == pytest.approx(math.sqrt(1 - a_t), rel=1e-12)
        h = (math.log(al_t) - math.log(sg_t)) - (math.log(al_s) - math.log(sg_s))
        want = (sg_t / sg_s) * x - al_t * (math.exp(-h) - 1.0) * ((x - sg_s * e) / al_s)
        assert (got - want).abs().max().item() <= 1e-6 * want.abs().max().item()
    # the class's own first-order coefficients at its own grid points, replayed through DDIM's closed form between the same two noise levels
    for i in range(steps):
        kd = dpm.coefficients(i, have_prev=False)
        al_t, sg_t = DPMSolverMultistepScheduler._alpha_sigma(dpm.sigmas[i + 1])
        x0 = (x - kd["sigma_s"] * e) / kd["alpha_s"]
        want = kd["c_x"] * x - kd["c_d0"] * x0
        got = al_t * x0 + sg_t * e                                   # DDIM, eta = 0: sqrt(abar_prev) x0 + sqrt(1 - abar_prev) eps
        assert not kd["second_order"] and (got - want).abs().max().item() <= 1e-6 * want.abs().max().item()


# ---- (c) DDPM_forward ----
def test_ddpm_forward_is_its_formula():
    s = DDIMScheduler()
    s.set_timesteps(25)
    x0 = torch.randn(2, 4, 1, 5, 6, generator=torch.Generator().manual_seed(4))
    xt, ts = DDPM_forward(x0, 25, 3, s, generator=torch.Generator().manual_seed(5))
    assert ts is None and xt.shape == (2, 4, 3, 5, 6) and xt.dtype == x0.dtype
    eps = torch.randn(2, 4, 3, 5, 6, generator=torch.Generator().manual_seed(5))
    a = torch.prod(s.alphas[int(s.timesteps[-1]):]).float()
    assert int(s.timesteps[-1]) == 1 and 0.0 < a.item() < 1e-2
    assert torch.allclose(xt, a.sqrt() * x0.repeat(1, 1, 3, 1, 1) + (1 - a).sqrt() * eps, atol=1e-6, rtol=0)


# ---- (d) from_pretrained(scheduler_from_config=...) ----
def test_from_pretrained_scheduler_from_config(tmp_path):
    (tmp_path / "scheduler").mkdir()
    cfg = {"_class_name": "DDIMScheduler", "_diffusers_version": "0.24.0", "beta_start": 0.00085, "beta_end": 0.0125,
           "beta_schedule": "scaled_linear", "clip_sample": False, "set_alpha_to_one": False, "steps_offset": 1,
           "num_train_timesteps": 1000, "prediction_type": "epsilon", "skip_prk_steps": True, "trained_betas": None}
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(cfg))
    parts = dict(unet=object(), vae=None, tokenizer=object(), text_encoder=object())
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 2, 3, 4)))
    default = LatentToVideoPipeline.from_pretrained(str(tmp_path), **dict(parts, vae=vae))
    assert type(default.scheduler) is DPMSolverMultistepScheduler and default.scheduler.config.beta_end == 0.0125
    ddim = LatentToVideoPipeline.from_pretrained(str(tmp_path), scheduler_from_config=True, **dict(parts, vae=vae))
    assert type(ddim.scheduler) is DDIMScheduler and ddim.scheduler.config.beta_end == 0.0125 and not ddim.scheduler.config.clip_sample
    cfg["_class_name"] = "PNDMScheduler"                 # any other class name: the default scheduler, as today
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(cfg))
    other = LatentToVideoPipeline.from_pretrained(str(tmp_path), scheduler_from_config=True, **dict(parts, vae=vae))
    assert type(other.scheduler) is DPMSolverMultistepScheduler


# ---- (e) the denoising loops on the emulator ----
class _StubUNet:                                        # tests/test_pipeline_host.py::_StubUNet
    def __init__(self, dtype):
        self.dtype = dtype

    def __call__(self, x, t, encoder_hidden_states=None, condition_latent=None, mask=None, motion=None, **_):
        txt = encoder_hidden_states.float().mean(dim=(1, 2)).reshape(-1, 1, 1, 1, 1)
        y = 0.3 * x.float() * float(np.cos(int(t) / 300.0)) + 0.1 * condition_latent.float() + txt \
            + 0.05 * mask.float() * float(motion.float().sum())
        return SimpleNamespace(sample=y.to(x.dtype))


class _SessionStubUNet(_StubUNet):
    """The same stand-in behind the session interface `LatentToVideoPipeline.denoise` drives (unet3d._Session: static input buffers,
    `run()` returning the token matrix [batch*(frames+1)*h*w, 8] with the condition frame in front), so that the fused loop runs on
    the CPU: guidance and the DDIM update are then aa_cfg_ddim_step_tokens on the emulator."""
    motion_mask = True
    motion_strength = True

    def session(self, batch, frames, h, w, text_shape, use_mask, has_motion, has_cond_emb, sample_dtype, sample_batch, cond_batch,
                mask_batch, device, cfg_dup=False):
        net, dt = self, self.dtype
        z = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype)

        class Session:
            runs = 0
            inputs = dict(sample=z(sample_batch, 4, frames, h, w, dtype=sample_dtype), cond=z(cond_batch, 4, 1, h, w),
                          mask=z(mask_batch, 1, 1, h, w), t=z(batch, dtype=torch.float32), motion=z(batch, dtype=torch.float32),
                          text=z(batch, *text_shape))

            def load(self, **tensors):
                for k, v in tensors.items():
                    if v is not None and self.inputs[k].data_ptr() != v.data_ptr():
                        dst = self.inputs[k]
                        dst.copy_(v.reshape(dst.shape) if v.numel() == dst.numel() else v.expand(dst.shape))

            def run(self):
                i = self.inputs
                assert len(set(i["t"].tolist())) == 1, "every batch entry sees the step's timestep"
                rep = batch // sample_batch
                x = i["sample"].to(dt).repeat(rep, 1, 1, 1, 1)
                y = net(x, i["t"][0].item(), encoder_hidden_states=i["text"], condition_latent=i["cond"].repeat(batch // cond_batch, 1, 1, 1, 1),
                        mask=i["mask"], motion=i["motion"][:1]).sample                     # [batch, 4, frames, h, w]
                full = torch.cat([torch.full_like(y[:, :, :1], 77.0), y], dim=2)             # frame 0: the slot the step kernel must skip
                tok = torch.full((batch * (frames + 1) * h * w, 8), -55.0, dtype=dt)         # columns 4..7: padding it must not read
                tok[:, :4] = full.permute(0, 2, 3, 4, 1).reshape(-1, 4)
                Session.runs += 1
                return tok

        self.last_session = Session()
        return self.last_session


def _loop_case(guidance, eta, seed=2):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    lat, cond, mask = r(1, 4, 3, 4, 4), r(1, 4, 1, 4, 4), (r(1, 1, 1, 4, 4) > 0).float()
    pos, neg = r(1, 7, 16), r(1, 7, 16)
    want = oracle.LatentToVideoPipeline(None, _StubUNet(torch.float32), RefDDIM(eta=eta, generator=torch.Generator().manual_seed(11)))(
        latents=lat, prompt_embeds=pos, negative_prompt_embeds=neg, condition_latent=cond, mask=mask, motion=[3.0],
        num_inference_steps=6, guidance_scale=guidance, return_dict=False)[1]
    call = dict(latents=lat, prompt_embeds=pos.half(), negative_prompt_embeds=neg.half(), condition_latent=cond.half(), mask=mask.half(),
                motion=[3.0], num_inference_steps=6, guidance_scale=guidance, eta=eta, return_dict=False)
    return want, call


@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("guidance", [9.0, 1.0])
def test_fused_denoise_loop_matches_oracle(emu, monkeypatch, guidance, eta):
    """6 DDIM steps through `denoise`'s fused branch: one session run + one aa_cfg_ddim_step_tokens per step (counted), within
    2e-2 * max|want| of the float64 oracle loop (the bound of test_pipeline_host.test_denoise_loop_matches_oracle)."""
    want, call = _loop_case(guidance, eta)
    unet = _SessionStubUNet(torch.float16)
    pipe = LatentToVideoPipeline(vae=None, unet=unet, scheduler=DDIMScheduler())
    launches = []
    real = ops.cfg_ddim_step_tokens
    monkeypatch.setattr(ops, "cfg_ddim_step_tokens", lambda *a, **k: (launches.append(k.get("next_t_value")), real(*a, **k))[1])
    monkeypatch.setattr(pipe, "_denoise_generic", lambda *a, **k: pytest.fail("the fused loop was not selected"))
    frames, got = pipe(generator=torch.Generator().manual_seed(11), **call)
    assert frames is None and got.shape == want.shape
    ts = pipe.scheduler.timesteps.tolist()
    assert unet.last_session.runs == 6 and launches == [float(t) for t in ts[1:]] + [float(ts[-1])]
    err = (got.double() - want).abs().max().item()
    print(f"fused loop: distance {err:.3g}, bound {2e-2 * want.abs().max().item():.3g}")
    assert err < 2e-2 * want.abs().max().item()


@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("guidance", [9.0, 1.0])
def test_generic_denoise_loop_matches_oracle(guidance, eta):
    """The same case through `_denoise_generic` (module forward + DDIMScheduler.step), same bound; with equal seeds both product
    loops draw the same variance noise as the oracle's scheduler."""
    want, call = _loop_case(guidance, eta)
    pipe = LatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=DDIMScheduler())
    frames, got = pipe(generator=torch.Generator().manual_seed(11), **call)
    err = (got.double() - want).abs().max().item()
    print(f"generic loop: distance {err:.3g}, bound {2e-2 * want.abs().max().item():.3g}")
    assert frames is None and err < 2e-2 * want.abs().max().item()


def test_dpm_solver_ignores_eta_and_generator():
    """`__call__` hands eta / generator on; DPM-Solver++ takes neither (diffusers' prepare_extra_step_kwargs): same latents."""
    _, call = _loop_case(9.0, 0.0)
    pipe = LatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=DPMSolverMultistepScheduler())
    base = pipe(**call)[1]
    g = torch.Generator().manual_seed(1)
    state = g.get_state()
    again = pipe(**dict(call, eta=0.9), generator=g)[1]
    assert torch.equal(base, again) and torch.equal(g.get_state(), state)
