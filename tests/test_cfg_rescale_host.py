"""guidance_rescale without a GPU: `pipeline.rescale_noise_cfg` against diffusers' expression, the keyword's way from `__call__` (both
pipelines) into `denoise`, the eval key, and the fused loop of the product TINY_UNET on the SIMT emulator - session run,
aa_cfg_rescale_tokens, the sampler's step kernel with guidance off - against the oracle's UNet driven by a loop written here.

Fused loop against the oracle loop, three steps at guidance 9, max|fused - oracle| / max|oracle| of the final latents; rescale 0.7 is
allowed twice what the same test measures with rescale off (the parent's path), the margin DDIM and UniPC were given.  Measured on the
emulator (rescale off, rescale 0.7):
  DPM-Solver++   2.506e-3  2.039e-3
  DDIM           3.104e-3  2.099e-3
  UniPC order 2  3.163e-3  2.342e-3"""
import pytest
import torch

import oracle
from animate_anything_amd import ops
from animate_anything_amd.pipeline import LatentToVideoPipeline, rescale_noise_cfg
from animate_anything_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler
from animate_anything_amd.unet3d import UNet3DConditionModel
from test_ddim_host import _SessionStubUNet, _StubUNet
from util import TINY_UNET, rel_err, seeded_state


def diffusers_rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    """diffusers 0.24 `rescale_noise_cfg`, written out."""
    std_text = noise_pred_text.std(dim=list(range(1, noise_pred_text.ndim)), keepdim=True)
    std_cfg = noise_cfg.std(dim=list(range(1, noise_cfg.ndim)), keepdim=True)
    noise_pred_rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * noise_pred_rescaled + (1 - guidance_rescale) * noise_cfg


def test_rescale_noise_cfg_is_the_diffusers_expression():
    g = torch.Generator().manual_seed(3)
    for mean in (0.0, 50.0):
        u = torch.randn(3, 4, 5, 6, 7, generator=g, dtype=torch.float64) * torch.tensor([1.0, 0.01, 3.0]).reshape(3, 1, 1, 1, 1) + mean
        t = torch.randn(3, 4, 5, 6, 7, generator=g, dtype=torch.float64) * torch.tensor([1.0, 0.01, 3.0]).reshape(3, 1, 1, 1, 1) + mean
        for guidance in (1.5, 9.0):
            cfg = u + guidance * (t - u)
            for phi in (0.3, 0.7, 1.0):
                want, got = diffusers_rescale_noise_cfg(cfg, t, phi), rescale_noise_cfg(cfg, t, phi)
                assert got.dtype == torch.float64 and (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
                assert (got - cfg).abs().max().item() > 1e-3                      # it does something
            per_clip = rescale_noise_cfg(cfg, t, 1.0).reshape(3, -1).std(dim=1)       # phi = 1: every clip takes the text prediction's deviation
            assert torch.allclose(per_clip, t.reshape(3, -1).std(dim=1), rtol=1e-12)
    half = rescale_noise_cfg(cfg.half(), t.half(), 0.7)                              # 16-bit operands are evaluated in fp32
    assert half.dtype == torch.float32 and rel_err(half, diffusers_rescale_noise_cfg(cfg, t, 0.7)) < 2e-3


def test_rescale_zero_returns_its_input_and_a_constant_clip_is_left_unscaled():
    g = torch.Generator().manual_seed(4)
    cfg, t = torch.randn(2, 4, 3, 5, 5, generator=g), torch.randn(2, 4, 3, 5, 5, generator=g)
    assert rescale_noise_cfg(cfg, t, 0.0) is cfg and rescale_noise_cfg(cfg, t) is cfg
    cfg[1] = 0.75                                                                    # std == 0: diffusers divides by zero
    assert not torch.isfinite(diffusers_rescale_noise_cfg(cfg, t, 0.7)[1]).any()
    got = rescale_noise_cfg(cfg, t, 0.7)
    assert torch.equal(got[1], cfg[1]) and torch.allclose(got[0], diffusers_rescale_noise_cfg(cfg, t, 0.7)[0], rtol=1e-6, atol=1e-6)


def _call_args(guidance):
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g)
    lat, cond, mask = r(1, 4, 3, 4, 4), r(1, 4, 1, 4, 4), (r(1, 1, 1, 4, 4) > 0).float()
    return dict(latents=lat, prompt_embeds=r(1, 7, 16).half(), negative_prompt_embeds=r(1, 7, 16).half(), condition_latent=cond.half(),
                mask=mask.half(), motion=[3.0], num_inference_steps=3, guidance_scale=guidance, return_dict=False)


def test_the_keyword_reaches_denoise_from_both_pipelines(monkeypatch):
    from animate_anything_amd import layerdiffuse
    seen = []

    def fake_denoise(self, latents, *a, **k):
        seen.append(k.get("guidance_rescale", "absent"))
        return latents.float()
    monkeypatch.setattr(LatentToVideoPipeline, "denoise", fake_denoise)
    pipe = LatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=DPMSolverMultistepScheduler())
    pipe(**_call_args(9.0))
    pipe(guidance_rescale=0.7, **_call_args(9.0))
    assert seen == [0.0, 0.7]
    rgba = layerdiffuse.MaskedLatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=DPMSolverMultistepScheduler())
    monkeypatch.setattr(rgba, "decode_latents", lambda latents: latents)
    monkeypatch.setattr(layerdiffuse, "decode_rgba", lambda *a: (None, None, None))
    rgba(output_type="pt", guidance_rescale=0.4, **_call_args(9.0))
    rgba(output_type="pt", **_call_args(9.0))
    assert seen == [0.0, 0.7, 0.4, 0.0]


@pytest.mark.parametrize("scheduler", [DPMSolverMultistepScheduler, DDIMScheduler, UniPCMultistepScheduler])
def test_both_loops_apply_it_under_guidance_only(emu, monkeypatch, scheduler):
    """The fused loop (stub session on the emulator): one aa_cfg_rescale_tokens per step, in place on the session's matrix, and the
    step kernel with guidance off; the generic loop: rescale_noise_cfg; guidance_scale <= 1 and rescale 0 leave both as they were,
    a rescale outside [0, 1] is refused."""
    from animate_anything_amd import pipeline as P
    calls, guided = [], []
    real = ops.cfg_rescale_tokens
    monkeypatch.setattr(ops, "cfg_rescale_tokens", lambda *a, **k: (calls.append((a[1:], k)), real(*a, **k))[1])
    for name, at in (("cfg_dpm_step_tokens", 4), ("cfg_ddim_step_tokens", 3), ("cfg_unipc_step_tokens", 3)):     # where `guidance` stands
        monkeypatch.setattr(ops, name, lambda *a, _s=getattr(ops, name), _at=at, **k: (guided.append(a[_at]), _s(*a, **k))[1])
    torch_calls = []
    real_torch = P.rescale_noise_cfg
    monkeypatch.setattr(P, "rescale_noise_cfg", lambda *a: (torch_calls.append(a[2]), real_torch(*a))[1])
    outs = {}
    for guidance, phi in ((9.0, 0.0), (9.0, 0.7), (1.0, 0.7), (1.0, 0.0)):
        del calls[:], guided[:], torch_calls[:]
        fused = LatentToVideoPipeline(vae=None, unet=_SessionStubUNet(torch.float16), scheduler=scheduler())
        monkeypatch.setattr(fused, "_denoise_generic", lambda *a, **k: pytest.fail("the fused loop was not selected"))
        got = fused(guidance_rescale=phi, **_call_args(guidance))[1]
        assert len(calls) == (3 if guidance > 1 and phi > 0 else 0) and torch_calls == []
        assert all(c[0] == (1, 4, 3, 16, 9.0, 0.7) and c[1] == {} for c in calls)      # in place: no `out`
        assert guided == ([None] * 3 if guidance == 1.0 or phi > 0 else [9.0] * 3)
        generic = LatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=scheduler())(guidance_rescale=phi, **_call_args(guidance))[1]
        assert torch_calls == ([0.7] * 3 if guidance > 1 and phi > 0 else [])
        assert rel_err(got, generic) < 2e-2
        outs[guidance, phi] = got
    assert torch.equal(outs[1.0, 0.7], outs[1.0, 0.0]) and not torch.equal(outs[9.0, 0.7], outs[9.0, 0.0])
    pipe = LatentToVideoPipeline(vae=None, unet=_SessionStubUNet(torch.float16), scheduler=scheduler())
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            pipe(guidance_rescale=bad, **_call_args(9.0))
        with pytest.raises(ValueError, match="guidance_rescale"):
            LatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=scheduler())(guidance_rescale=bad, **_call_args(9.0))


def test_eval_validates_the_key_before_any_model_is_loaded(tmp_path):
    from animate_anything_amd import eval as aa_eval
    missing = str(tmp_path / "no_such_checkpoint")
    for bad in (1.5, -0.2, "strong", True, None, [0.7], float("nan")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            aa_eval.main_eval(missing, {"guidance_rescale": bad})
        with pytest.raises(ValueError, match="guidance_rescale"):
            aa_eval.batch_eval(None, None, None, None, {}, {"guidance_rescale": bad}, str(tmp_path), False)
    assert aa_eval._check_guidance_rescale({}) == 0.0                                # absent: off
    assert aa_eval._check_guidance_rescale({"guidance_rescale": 1}) == 1.0 and aa_eval._check_guidance_rescale({"guidance_rescale": 0}) == 0.0
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text("pretrained_model_path: x\nvalidation_data: {guidance_scale: 9}\n")
    assert aa_eval._check_guidance_rescale(aa_eval.load_config(str(cfg_path))["validation_data"]) == 0.0
    cfg = aa_eval.load_config(str(cfg_path), ["validation_data.guidance_rescale=0.7"])
    assert aa_eval._check_guidance_rescale(cfg["validation_data"]) == 0.7
    cfg = aa_eval.load_config(str(cfg_path), ["validation_data.guidance_rescale=2"])
    cfg["pretrained_model_path"] = missing
    with pytest.raises(ValueError, match="guidance_rescale"):
        aa_eval.main_eval(**cfg)


# ---- the product UNet's fused loop on the emulator against the oracle's UNet ----
STEPS, GUIDANCE, RESCALE = 3, 9.0, 0.7
SAMPLERS = {"dpm": lambda: DPMSolverMultistepScheduler(), "ddim": lambda: DDIMScheduler(), "unipc": lambda: UniPCMultistepScheduler(solver_order=2)}


@pytest.fixture(scope="module")
def tiny_pair():
    torch.manual_seed(0)
    ref = oracle.UNet3DConditionModel(**TINY_UNET).eval()
    state = seeded_state(ref)
    ref.load_state_dict(state)
    net = UNet3DConditionModel(**TINY_UNET).eval()
    net.load_state_dict(state)
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g)
    case = dict(lat=r(1, 4, 2, 5, 6), cond=r(1, 4, 1, 5, 6), pos=r(1, 9, 64), neg=r(1, 9, 64), mask=torch.zeros(1, 1, 1, 5, 6))
    case["mask"][..., 1:4, 2:5] = 1
    return ref, net.half(), case


def oracle_loop(ref, case, scheduler, rescale):
    """The reference's sequence (batch the halves, guidance, the scheduler's step on [b*f, c, h, w]) around the oracle's UNet in fp32,
    with diffusers' rescale between guidance and step."""
    scheduler.set_timesteps(STEPS)
    x = case["lat"].clone()
    text, cond = torch.cat([case["neg"], case["pos"]]), torch.cat([case["cond"], case["cond"]])
    with torch.no_grad():
        for t in scheduler.timesteps:
            eps = ref(torch.cat([x, x]), int(t), text, cond, case["mask"], motion=torch.tensor([3.0])).sample
            e_u, e_t = eps[:1], eps[1:]
            e = e_u + GUIDANCE * (e_t - e_u)
            if rescale > 0:
                e = diffusers_rescale_noise_cfg(e, e_t, rescale)
            b, c, f, h, w = x.shape
            flat = scheduler.step(e.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w), t, x.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)).prev_sample
            x = flat.reshape(b, f, c, h, w).permute(0, 2, 1, 3, 4).contiguous()
    return x


@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_fused_loop_of_the_tiny_unet_matches_the_oracle_loop(emu, monkeypatch, tiny_pair, sampler):
    ref, net, case = tiny_pair
    calls = []
    real = ops.cfg_rescale_tokens
    monkeypatch.setattr(ops, "cfg_rescale_tokens", lambda *a, **k: (calls.append(a[1:]), real(*a, **k))[1])
    dist, finals = {}, {}
    for rescale in (0.0, RESCALE):
        want = oracle_loop(ref, case, SAMPLERS[sampler](), rescale)
        pipe = LatentToVideoPipeline(vae=None, unet=net, scheduler=SAMPLERS[sampler]())
        monkeypatch.setattr(pipe, "_denoise_generic", lambda *a, **k: pytest.fail("the fused loop was not selected"))
        pipe.scheduler.set_timesteps(STEPS)
        with torch.no_grad():
            got = pipe.denoise(case["lat"], torch.cat([case["neg"], case["pos"]]).half(), case["cond"].half(), case["mask"].half(), [3.0],
                               [int(t) for t in pipe.scheduler.timesteps], GUIDANCE, guidance_rescale=rescale)
        assert torch.isfinite(got).all()
        dist[rescale], finals[rescale] = rel_err(got, want), (got, want)
    print(f"{sampler}: fused vs oracle, rescale off {dist[0.0]:.4g}, rescale {RESCALE} {dist[RESCALE]:.4g} (bound {2 * dist[0.0]:.4g})")
    assert calls == [(1, 4, 2, 30, GUIDANCE, RESCALE)] * STEPS
    assert rel_err(finals[RESCALE][1], finals[0.0][1]) > 0.05                        # the rescale moves the oracle's result: no no-op passes
    assert dist[0.0] > 0.0 and dist[RESCALE] <= 2 * dist[0.0]
