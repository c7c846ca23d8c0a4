"""`keep` (the known-region blend of inpainting samplers) without a GPU: `check_keep`, the generic loop against a loop written here, the
fused loop on the emulator (stub session; one ops.keep_blend behind every solver kernel) against the generic loop and against its own
exactness properties, `keep=None` / `False` against the call without the keyword (no launch, no randn), the UniPC refusal, the keyword's
way from `__call__`, the pixel composite after decoding, context windows and FreeInit on top, and the eval key."""
import math
from types import SimpleNamespace

import pytest
import torch

from animate_anything_amd import ops
from animate_anything_amd.pipeline import KEEP_KEYS, LatentToVideoPipeline, check_keep
from animate_anything_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler
from test_ddim_host import _SessionStubUNet, _StubUNet
from util import rel_err

EPS = 2.0 ** -24
H, W = 4, 6
SCHEDULERS = [DPMSolverMultistepScheduler, DDIMScheduler]


def _case(frames=3, guidance=9.0, seed=2, steps=3):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    lat, cond, mask = r(1, 4, frames, H, W), r(1, 4, 1, H, W), (r(1, 1, 1, H, W) > 0).float()
    return dict(latents=lat, prompt_embeds=r(1, 7, 16).half(), negative_prompt_embeds=r(1, 7, 16).half(), condition_latent=cond.half(),
                mask=mask.half(), motion=[3.0], num_inference_steps=steps, guidance_scale=guidance, return_dict=False)


def _held_mask(kind="mixed"):
    """[1, 1, 1, H, W] fp16: the left half 0 (held), the right half 1 (free), one column of 0.5 between them; or all 0 / all 1."""
    m = torch.zeros(1, 1, 1, H, W)
    if kind == "ones":
        m += 1.0
    elif kind == "mixed":
        m[..., W // 2] = 0.5
        m[..., W // 2 + 1:] = 1.0
    return m.half()


def _noise(case, seed=31):
    return torch.randn(case["latents"].shape, generator=torch.Generator().manual_seed(seed))


def _run(make_unet, scheduler, case, **kw):
    """One call; returns (final fp32 latents as `denoise` left them, the callback's latents per step)."""
    seen = []
    pipe = LatentToVideoPipeline(vae=None, unet=make_unet(), scheduler=scheduler())
    final = []
    real = pipe.denoise
    pipe.denoise = lambda *a, **k: (final.append(real(*a, **k)), final[-1])[1]
    pipe(callback=lambda i, t, x: seen.append(x.clone()), **kw, **case)
    return final[-1], seen


FUSED = lambda: _SessionStubUNet(torch.float16)
GENERIC = lambda: _StubUNet(torch.float16)


def test_check_keep():
    cond, mask = torch.zeros(1, 4, 1, H, W), torch.ones(1, 1, 1, H, W)
    assert check_keep(None) is None and check_keep(False) is None and check_keep(None, cond, mask) is None
    k = check_keep(True, cond, mask)
    assert sorted(k) == sorted(KEEP_KEYS) and k["latents"] is cond and k["mask"] is mask
    assert k["noise"] is None and k["image"] is None and k["image_mask"] is None
    assert check_keep({}, cond, mask) == k
    other, noise = torch.ones(1, 4, 1, H, W), torch.zeros(1, 4, 3, H, W)
    k = check_keep(dict(latents=other, mask=_held_mask(), noise=noise), cond, mask)
    assert k["latents"] is other and k["noise"] is noise and k["mask"] is not mask
    assert check_keep(dict(latents=other, mask=mask))["latents"] is other                 # nothing needed from the call
    again = check_keep(k, None, None)                                                      # a completed dict passes through
    assert all(again[key] is k[key] for key in KEEP_KEYS)
    img, im = torch.zeros(1, 3, 8, 8), torch.ones(8, 8)
    k = check_keep(dict(image=img, image_mask=im), cond, mask)
    assert k["image"] is img and k["image_mask"] is im
    for bad in (dict(latent=cond), dict(strength=0.5), dict(mask=mask, keep=True)):
        with pytest.raises(ValueError, match="unknown key"):
            check_keep(bad, cond, mask)
    for bad in (1, "on", [cond, mask], 0.5):
        with pytest.raises(ValueError, match="keep"):
            check_keep(bad, cond, mask)
    with pytest.raises(ValueError, match="no mask"):
        check_keep(True, cond, None)
    with pytest.raises(ValueError, match="no mask"):
        check_keep(dict(latents=cond), None, None)
    with pytest.raises(ValueError, match="no known latents"):
        check_keep(True, None, mask)
    with pytest.raises(ValueError, match="image_mask"):
        check_keep(dict(image=img), cond, mask)
    with pytest.raises(ValueError, match="image_mask"):
        check_keep(dict(image_mask=im), cond, mask)


def test_operand_shapes_are_refused_before_any_launch(emu, monkeypatch):
    monkeypatch.setattr(ops, "keep_blend", lambda *a, **k: pytest.fail("launched"))
    case = _case()
    for make in (FUSED, GENERIC):
        for bad, what in ((dict(mask=torch.ones(1, 1, 1, H, W + 1)), "keep.mask"), (dict(mask=torch.ones(H, W)), "keep.mask"),
                          (dict(mask=torch.ones(1, 1, 2, H, W)), "keep.mask"), (dict(latents=torch.ones(1, 3, 1, H, W)), "keep.latents"),
                          (dict(latents=torch.ones(2, 4, 1, H, W)), "keep.latents"), (dict(noise=torch.zeros(1, 4, 2, H, W)), "keep.noise"),
                          (dict(noise=_noise(case).double()), "keep.noise")):
            with pytest.raises(ValueError, match=what):
                _run(make, DDIMScheduler, case, keep=bad)


def _by_hand(unet, scheduler, case, known, mask, noise):
    """The keep loop written out: the reference's step, then the blend as plain arithmetic at the level of the NEXT timestep."""
    x = case["latents"].float().clone()
    g = case["guidance_scale"]
    text = torch.cat([case["negative_prompt_embeds"], case["prompt_embeds"]])
    cond = torch.cat([case["condition_latent"]] * 2)
    scheduler.set_timesteps(case["num_inference_steps"])
    ts = [int(t) for t in scheduler.timesteps]
    m, known = mask.double(), known.double()
    for i, t in enumerate(scheduler.timesteps):
        xl = x.to(unet.dtype)
        eps = unet(torch.cat([xl, xl]), t, encoder_hidden_states=text, condition_latent=cond, mask=case["mask"], motion=torch.as_tensor(case["motion"])).sample.float()
        e = eps[:1] + g * (eps[1:] - eps[:1])
        b, c, f, h, w = x.shape
        flat = scheduler.step(e.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w), t, x.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)).prev_sample
        x = flat.reshape(b, f, c, h, w).permute(0, 2, 1, 3, 4).contiguous()
        if i + 1 < len(ts):
            abar = float(scheduler.alphas_cumprod[ts[i + 1]])
            kn = math.sqrt(abar) * known + math.sqrt(1.0 - abar) * noise.double()
        else:
            kn = known.expand(x.shape)
        x = (m * x.double() + (1.0 - m) * kn).float()
    return x


@pytest.mark.parametrize("scheduler", SCHEDULERS)
def test_generic_loop_is_the_loop_written_by_hand(scheduler):
    unet = _StubUNet(torch.float32)
    case = _case()
    noise, mask = _noise(case), _held_mask()
    got, _ = _run(lambda: unet, scheduler, case, keep=dict(mask=mask, noise=noise))
    want = _by_hand(unet, scheduler(), case, case["condition_latent"].float(), mask.float(), noise)
    plain, _ = _run(lambda: unet, scheduler, case)
    assert rel_err(got, want) <= 1e-5, rel_err(got, want)
    assert rel_err(got, plain) > 1e-2, "the blend changes the result"
    other = torch.randn(1, 4, 3, H, W, generator=torch.Generator().manual_seed(9))      # known latents of the mapping's own, per frame
    got, _ = _run(lambda: unet, scheduler, case, keep=dict(latents=other, mask=mask, noise=noise))
    assert rel_err(got, _by_hand(unet, scheduler(), case, other, mask.float(), noise)) <= 1e-5


@pytest.mark.parametrize("scheduler", SCHEDULERS)
def test_fused_loop_on_the_emulator(emu, monkeypatch, scheduler):
    blends = []
    real = ops.keep_blend
    monkeypatch.setattr(ops, "keep_blend", lambda *a, **k: (blends.append((a, k)), real(*a, **k))[1])
    case = _case()
    steps = case["num_inference_steps"]
    noise, mask = _noise(case), _held_mask()
    known = case["condition_latent"].float().expand(case["latents"].shape)
    held, free = (mask.float() <= 0).expand(known.shape), (mask.float() >= 1).expand(known.shape)
    bits = lambda t: t.contiguous().view(torch.int32)
    sched = scheduler()
    sched.set_timesteps(steps)
    ts = [int(t) for t in sched.timesteps]
    plain = {}
    for name, make in (("fused", FUSED), ("generic", GENERIC)):
        del blends[:]
        final, seen = _run(make, scheduler, case, keep=dict(mask=mask, noise=noise))
        assert len(blends) == (steps if name == "fused" else 0), "one launch behind every solver kernel; the generic loop blends in torch"
        if name == "fused":
            for i, (a, k) in enumerate(blends):
                abar = float(sched.alphas_cumprod[ts[i + 1]]) if i + 1 < steps else 1.0
                assert a[0].shape == case["latents"].shape and a[0].dtype == torch.float32 and k.get("out") is None, "in place, on the whole clip"
                assert a[1].dtype == torch.float16 and a[2].dtype == torch.float16, "the condition latent and the mask as they are stored"
                assert (a[3], a[4]) == (math.sqrt(abar), math.sqrt(1.0 - abar)) if i + 1 < steps else (a[3], a[4]) == (1.0, 0.0)
                assert (k["noise"] is None) == (i + 1 == steps)
        assert len(seen) == steps and torch.equal(bits(seen[-1]), bits(final)), "the callback sees the blended latents"
        assert torch.equal(bits(final)[held], bits(known)[held]), f"{name}: the held region ends as the known latents"
        for i in range(steps - 1):
            abar = float(sched.alphas_cumprod[ts[i + 1]])
            a32, s32 = (float(torch.tensor(v, dtype=torch.float32)) for v in (math.sqrt(abar), math.sqrt(1.0 - abar)))
            want = a32 * known.double() + s32 * noise.double()
            bound = 8 * EPS * ((a32 * known.double()).abs() + (s32 * noise.double()).abs())
            assert ((seen[i].double() - want).abs() <= bound)[held].all(), f"{name}: step {i} holds a_i known + s_i noise"
        plain[name] = _run(make, scheduler, case)
        assert torch.equal(bits(seen[0])[free], bits(plain[name][1][0])[free]), f"{name}: the free region after the first step is the plain run's"
        assert not torch.equal(bits(seen[0])[held], bits(plain[name][1][0])[held])
        # an all-ones mask: the plain run bit for bit, every step; an all-zeros mask: the known latents
        ones_final, ones_seen = _run(make, scheduler, case, keep=dict(mask=_held_mask("ones"), noise=noise))
        assert torch.equal(bits(ones_final), bits(plain[name][0])) and all(torch.equal(bits(a), bits(b)) for a, b in zip(ones_seen, plain[name][1]))
        zeros_final, _ = _run(make, scheduler, case, keep=dict(mask=_held_mask("zeros"), noise=noise))
        assert torch.equal(bits(zeros_final), bits(known))
        plain[name + " keep"] = final
    d = rel_err(plain["fused keep"], plain["generic keep"])
    print(f"{scheduler.__name__}: fused vs generic with keep {d:.3g}, without {rel_err(plain['fused'][0], plain['generic'][0]):.3g}")
    assert torch.isfinite(plain["fused keep"]).all() and d < 2e-2


@pytest.mark.parametrize("scheduler", SCHEDULERS + [UniPCMultistepScheduler])
def test_off_launches_nothing_and_draws_nothing(emu, monkeypatch, scheduler):
    case = _case()
    want = {name: _run(make, scheduler, case)[0] for name, make in (("fused", FUSED), ("generic", GENERIC))}
    monkeypatch.setattr(ops, "keep_blend", lambda *a, **k: pytest.fail("keep_blend was launched with the feature off"))
    monkeypatch.setattr(torch, "randn", lambda *a, **k: pytest.fail("torch.randn was called with the feature off"))
    for name, make in (("fused", FUSED), ("generic", GENERIC)):
        for off in (None, False):
            assert torch.equal(_run(make, scheduler, case, keep=off)[0], want[name]), (name, off)


def test_unipc_is_refused_in_both_loops(emu, monkeypatch):
    case = _case()
    monkeypatch.setattr(ops, "keep_blend", lambda *a, **k: pytest.fail("launched"))
    for make in (FUSED, GENERIC):
        unet = make()
        pipe = LatentToVideoPipeline(vae=None, unet=unet, scheduler=UniPCMultistepScheduler())
        monkeypatch.setattr(pipe, "_encode_prompt", lambda *a, **k: pytest.fail("device work in front of the refusal"))
        with pytest.raises(ValueError, match="UniPC.*corrector.*last_sample"):
            pipe(keep=True, **case)
        pipe.scheduler.set_timesteps(3)
        text = torch.cat([case["negative_prompt_embeds"], case["prompt_embeds"]])
        for loop in (pipe.denoise, pipe._denoise_generic):
            with pytest.raises(ValueError, match="UniPC"):
                loop(case["latents"], text, case["condition_latent"], case["mask"], [3.0], pipe.scheduler.timesteps, 9.0, keep=dict(noise=_noise(case)))
        assert not hasattr(unet, "last_session"), "no session was built"


def test_the_keyword_reaches_denoise_from_call(monkeypatch):
    seen = []

    def fake_denoise(self, latents, *a, **k):
        seen.append(k.get("keep", "absent"))
        return latents.float()
    monkeypatch.setattr(LatentToVideoPipeline, "denoise", fake_denoise)
    pipe = LatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=DPMSolverMultistepScheduler())
    case = _case()
    pipe(**case)
    pipe(keep=False, **case)
    g = torch.Generator().manual_seed(4)
    pipe(keep=True, generator=g, **case)
    noise = _noise(case)
    pipe(keep=dict(noise=noise, mask=_held_mask()), **case)
    assert seen[0] is None and seen[1] is None
    drawn = torch.randn(case["latents"].shape, generator=torch.Generator().manual_seed(4))
    assert sorted(seen[2]) == sorted(KEEP_KEYS) and seen[2]["latents"] is case["condition_latent"] and seen[2]["mask"] is case["mask"]
    assert seen[2]["noise"].dtype == torch.float32 and torch.equal(seen[2]["noise"], drawn), "one randn of the latents' shape from the caller's generator"
    assert seen[3]["noise"] is noise and seen[3]["latents"] is case["condition_latent"] and seen[3]["mask"] is not case["mask"]


class _StubVAE:
    """decode: the first three latent channels, every pixel doubled along both axes (fp16, like the model)."""
    config = SimpleNamespace(block_out_channels=(1, 1, 1, 1), scaling_factor=1.0)
    dtype = torch.float16
    decodes = 0

    def decode(self, z):
        _StubVAE.decodes += 1
        return SimpleNamespace(sample=z[:, :3].repeat_interleave(2, dim=2).repeat_interleave(2, dim=3))


def test_the_image_composite_runs_once_after_decoding(emu, monkeypatch):
    blends = []
    real = ops.keep_blend
    monkeypatch.setattr(ops, "keep_blend", lambda *a, **k: (blends.append((a, k, _StubVAE.decodes)), real(*a, **k))[1])
    case = _case()
    steps, frames = case["num_inference_steps"], case["latents"].shape[2]
    g = torch.Generator().manual_seed(12)
    image = torch.rand(1, 3, 2 * H, 2 * W, generator=g) * 2 - 1
    image_mask = torch.ones(2 * H, 2 * W)
    image_mask[:, :W] = 0.0                                                           # the left half is held
    _StubVAE.decodes = 0
    make = lambda: LatentToVideoPipeline(vae=_StubVAE(), unet=FUSED(), scheduler=DDIMScheduler())
    plain = make()(output_type="pt", **case)[0]
    assert plain.shape == (1, 3, frames, 2 * H, 2 * W) and not blends
    for img, im in ((image, image_mask.numpy()), (image[:, :, None], image_mask[None, None, None]),
                    (image[:, :, None].expand(1, 3, frames, 2 * H, 2 * W), image_mask[None, None, None].expand(1, 1, frames, 2 * H, 2 * W))):
        del blends[:]
        before = _StubVAE.decodes
        video, latents = make()(output_type="pt", keep=dict(image=img, image_mask=im, noise=_noise(case)), **case)
        assert len(blends) == steps + 1 and [b[2] for b in blends] == [before] * steps + [before + 1], "one blend per step, one after decoding"
        a, k, _ = blends[-1]
        assert a[0].shape == (1, 3, frames, 2 * H, 2 * W) and a[0].is_contiguous() and a[0].dtype == torch.float32 and (a[3], a[4]) == (1, 0)
        assert k.get("noise") is None
        assert torch.equal(video[..., :W], image[:, :, None].expand(1, 3, frames, 2 * H, 2 * W)[..., :W]), "the known pixels, bit for bit"
        assert not torch.equal(video[..., W:], image[:, :, None].expand(1, 3, frames, 2 * H, 2 * W)[..., W:])
        # the free half is what the VAE made of the kept latents
        want = latents[:, :3].permute(0, 2, 1, 3, 4).repeat_interleave(2, dim=3).repeat_interleave(2, dim=4).permute(0, 2, 1, 3, 4).float()
        assert torch.equal(video[..., W:], want[..., W:])
    del blends[:]
    assert make()(output_type="latent", keep=dict(image=image, image_mask=image_mask), **case)[0] is None and len(blends) == steps
    with pytest.raises(ValueError, match="keep.image "):
        make()(output_type="pt", keep=dict(image=image[..., :-1], image_mask=image_mask), **case)
    with pytest.raises(ValueError, match="keep.image_mask"):
        make()(output_type="pt", keep=dict(image=image, image_mask=image_mask[:-1]), **case)


@pytest.mark.parametrize("scheduler", SCHEDULERS)
def test_it_composes_with_context_windows(emu, monkeypatch, scheduler):
    blends = []
    real = ops.keep_blend
    monkeypatch.setattr(ops, "keep_blend", lambda *a, **k: (blends.append(a[0].shape), real(*a, **k))[1])
    case = _case(10)
    context = dict(frames=4, overlap=2)
    noise, mask = _noise(case), _held_mask()
    known = case["condition_latent"].float().expand(case["latents"].shape)
    held = (mask.float() <= 0).expand(known.shape)
    unet = FUSED()
    fused, _ = _run(lambda: unet, scheduler, case, context=context, keep=dict(mask=mask, noise=noise))
    assert unet.last_session.inputs["sample"].shape == (1, 4, 4, H, W) and blends == [(1, 4, 10, H, W)] * 3, "one blend per step, on the long buffer"
    generic, _ = _run(GENERIC, scheduler, case, context=context, keep=dict(mask=mask, noise=noise))
    for got in (fused, generic):
        assert torch.equal(got[held], known[held])
    assert rel_err(fused, generic) < 2e-2, rel_err(fused, generic)
    assert rel_err(fused, _run(FUSED, scheduler, case, context=context)[0]) > 1e-2


def test_it_composes_with_free_init_on_one_noise_tensor(emu, monkeypatch):
    blends, draws = [], []
    real, real_randn = ops.keep_blend, torch.randn
    monkeypatch.setattr(ops, "keep_blend", lambda *a, **k: (blends.append(k.get("noise")), real(*a, **k))[1])
    monkeypatch.setattr(torch, "randn", lambda *a, **k: (draws.append(a), real_randn(*a, **k))[1])
    case = _case(4)
    steps = case["num_inference_steps"]
    mask = _held_mask()
    known = case["condition_latent"].float().expand(case["latents"].shape)
    held = (mask.float() <= 0).expand(known.shape)
    for make in (FUSED, GENERIC):
        del blends[:], draws[:]
        _run(make, DDIMScheduler, case, free_init=dict(num_iters=2), generator=torch.Generator().manual_seed(3))
        plain_draws = len(draws)
        del draws[:]
        got, _ = _run(make, DDIMScheduler, case, free_init=dict(num_iters=2), keep=dict(mask=mask), generator=torch.Generator().manual_seed(3))
        assert len(draws) == plain_draws + 1, "one randn for the whole call"
        assert torch.equal(got[held], known[held])
        if make is FUSED:
            used = [n for n in blends if n is not None]
            assert len(blends) == 2 * steps and len(used) == 2 * (steps - 1) and len({n.data_ptr() for n in used}) == 1, "every iteration blends with the same noise"


def test_eval_validates_the_key_before_any_model_is_loaded(tmp_path):
    from animate_anything_amd import eval as aa_eval
    missing = str(tmp_path / "no_such_checkpoint")
    for bad in (1, 0, "true", "yes", 0.5, {"on": True}, [True]):
        with pytest.raises(ValueError, match="keep_unmasked"):
            aa_eval.main_eval(missing, {"keep_unmasked": bad, "num_frames": 16})
        with pytest.raises(ValueError, match="keep_unmasked"):
            aa_eval.batch_eval(None, None, None, None, {}, {"keep_unmasked": bad}, str(tmp_path), False)
    with pytest.raises(ValueError, match="keep_unmasked.*unipc"):
        aa_eval.main_eval(missing, {"keep_unmasked": True, "num_frames": 16}, sampler="unipc")
    with pytest.raises(ValueError, match="keep_unmasked.*unipc"):
        aa_eval.batch_eval(None, None, None, None, {}, {"keep_unmasked": True}, str(tmp_path), False, sampler="unipc")
    assert aa_eval._check_keep_unmasked({}) is False and aa_eval._check_keep_unmasked(None) is False      # absent: off
    assert aa_eval._check_keep_unmasked({"keep_unmasked": False}, "unipc") is False
    assert aa_eval._check_keep_unmasked({"keep_unmasked": True}, "ddim") is True
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text("pretrained_model_path: x\nsampler: unipc\nvalidation_data: {guidance_scale: 9, num_frames: 16, keep_unmasked: true}\n")
    cfg = aa_eval.load_config(str(cfg_path))
    assert aa_eval._check_keep_unmasked(cfg["validation_data"]) is True
    cfg["pretrained_model_path"] = missing
    with pytest.raises(ValueError, match="keep_unmasked"):
        aa_eval.main_eval(**cfg)
    cfg = aa_eval.load_config(str(cfg_path), ["validation_data.keep_unmasked=maybe", "sampler=dpm"])
    cfg["pretrained_model_path"] = missing
    with pytest.raises(ValueError, match="keep_unmasked"):
        aa_eval.main_eval(**cfg)
