"""Context windows without a GPU: the schedule of `schedulers.context_windows` (coverage, distinct indices, per-frame weights, flags,
the refusals), `check_context`, the generic loop against a loop written here on a stub UNet whose output depends on the slot, the fused
loop on the emulator (stub session: gather, session run, merge per window, one solver kernel per step) against the generic loop,
`context=None` / a window that holds the whole clip against the call without the keyword, the keyword's way from `__call__`, and the
eval key."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from animate_anything_amd import ops
from animate_anything_amd.pipeline import CONTEXT_DEFAULTS, LatentToVideoPipeline, check_context
from animate_anything_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler, context_windows
from test_ddim_host import _SessionStubUNet, _StubUNet
from util import rel_err

GRID = [(n, length, overlap) for n in (1, 2, 5, 7, 10, 16, 17, 32, 48) for length in (1, 2, 3, 4, 16) for overlap in (0, 1, 2, 3, 4, 15)
        if overlap < length]


@pytest.mark.parametrize("weights", ["flat", "pyramid"])
@pytest.mark.parametrize("closed_loop", [False, True], ids=["open", "closed"])
def test_schedule_properties(closed_loop, weights):
    overlapping = 0
    for n, length, overlap in GRID:
        windows = context_windows(n, length, overlap, closed_loop=closed_loop, weights=weights)
        if n <= length:                                                               # "feature off": one window, the clip itself
            assert windows == [(list(range(n)), [1.0] * n, [True] * n, [True] * n)]
            continue
        total, holders = np.zeros(n, dtype=np.float64), [[] for _ in range(n)]
        raw = [1.0 if weights == "flat" else float(min(j + 1, length - j)) for j in range(length)]
        for k, (idx, wn, first, last) in enumerate(windows):
            assert len(idx) == len(wn) == len(first) == len(last) == length
            assert len(set(idx)) == length and all(0 <= f < n for f in idx), "indices inside a window are distinct and in range"
            assert all(isinstance(w, float) and 0.0 < w <= 1.0 for w in wn)
            for j, f in enumerate(idx):
                total[f] += wn[j]
                holders[f].append((k, j))
        assert all(holders), "every frame is covered"
        assert np.abs(total - 1.0).max() <= 1e-12
        for f, held in enumerate(holders):
            ks = [k for k, _ in held]
            assert ks == sorted(ks) and len(set(ks)) == len(ks)
            for k, j in held:
                idx, wn, first, last = windows[k]
                assert first[j] == (k == ks[0]) and last[j] == (k == ks[-1]), "first / last: no earlier / no later window holds the frame"
                assert wn[j] == raw[j] / sum(raw[jj] for _, jj in held)                 # float64, per frame
                if len(held) == 1:
                    assert wn[j] == 1.0 and first[j] and last[j], "a frame held by one window has weight exactly 1.0"
            overlapping += len(held) > 1
        stride = length - overlap
        if closed_loop:
            assert [w[0][0] for w in windows] == list(range(0, n, stride))
            assert all(w[0] == [(w[0][0] + j) % n for j in range(length)] for w in windows)
        else:
            starts = [w[0][0] for w in windows]
            assert all(w[0] == list(range(s, s + length)) for w, s in zip(windows, starts))
            assert windows[-1][0][-1] == n - 1, "the last open window ends at num_frames"
            assert starts == sorted(set(starts)) and starts[:-1] == list(range(0, n - length, stride))[:len(starts) - 1]
            assert all(b - a <= stride for a, b in zip(starts, starts[1:]))
    assert overlapping > 100


def test_schedule_examples_and_refusals():
    assert [w[0] for w in context_windows(10, 4, 2)] == [[0, 1, 2, 3], [2, 3, 4, 5], [4, 5, 6, 7], [6, 7, 8, 9]]
    assert [w[0] for w in context_windows(10, 4, 2, closed_loop=True)][-1] == [8, 9, 0, 1]
    assert [w[0][0] for w in context_windows(32, 16, 4)] == [0, 12, 16]
    assert [w[0] for w in context_windows(8, 4, 0)] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert context_windows(10, 4, 2)[0][1] == [1.0, 1.0, 2 / 3, 1 / 3] and context_windows(10, 4, 2, weights="flat")[1][1] == [0.5] * 4
    for bad in ((10, 0, 0), (10, 4, 4), (10, 4, 5), (10, 4, -1), (0, 4, 2), (-3, 4, 2)):
        with pytest.raises(ValueError, match="context_windows"):
            context_windows(*bad)
        with pytest.raises(ValueError, match="context_windows"):
            context_windows(*bad, closed_loop=True)
    for bad in ("gauss", None, 1):
        with pytest.raises(ValueError, match="weights"):
            context_windows(10, 4, 2, weights=bad)


def test_check_context():
    assert check_context(None) is None and check_context({}) == CONTEXT_DEFAULTS
    assert CONTEXT_DEFAULTS == dict(frames=16, overlap=4, weights="pyramid", closed_loop=False)
    assert check_context({"frames": 4, "overlap": 2}) == dict(frames=4, overlap=2, weights="pyramid", closed_loop=False)
    for bad in ({"frame": 4}, {"frames": 4, "stride": 2}, {"frames": 4.0, "overlap": 1}, {"frames": True, "overlap": 0}, {"frames": 0, "overlap": 0},
                {"frames": 65, "overlap": 4}, {"frames": 4, "overlap": 4}, {"frames": 4, "overlap": -1}, {"frames": 4}, {"weights": "gauss"},
                {"closed_loop": 1}, {"closed_loop": "yes"}, [16, 4], 16, "pyramid"):
        with pytest.raises(ValueError, match="context"):
            check_context(bad)


class _SlotStubUNet(_StubUNet):
    """The stand-in of test_ddim_host.py plus a term that depends on the SLOT a frame sits in: a loop that fed the windows' frames to
    the UNet in another order, or blended by frame instead of by slot, would not pass."""

    def __call__(self, x, t, **kw):
        y = super().__call__(x, t, **kw).sample.float()
        slot = torch.arange(x.shape[2], dtype=torch.float32).reshape(1, 1, -1, 1, 1)
        return SimpleNamespace(sample=(y + 0.07 * slot * (1.0 + x.float())).to(x.dtype))


def _case(frames, guidance=9.0, seed=2, steps=3):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    lat, cond, mask = r(1, 4, frames, 4, 4), r(1, 4, 1, 4, 4), (r(1, 1, 1, 4, 4) > 0).float()
    return dict(latents=lat, prompt_embeds=r(1, 7, 16).half(), negative_prompt_embeds=r(1, 7, 16).half(), condition_latent=cond.half(),
                mask=mask.half(), motion=[3.0], num_inference_steps=steps, guidance_scale=guidance, return_dict=False)


def _by_hand(unet, scheduler, case, context, guidance_rescale=0.0):
    """The windowed loop written out frame by frame: every window through the UNet, guidance, (rescale per window,) the prediction of
    frame f = sum of weight * the slot's prediction over the (window, slot) pairs that hold f, then the scheduler's step on the clip."""
    from animate_anything_amd.pipeline import rescale_noise_cfg
    x = case["latents"].float().clone()
    n = x.shape[2]
    g = case["guidance_scale"]
    text = torch.cat([case["negative_prompt_embeds"], case["prompt_embeds"]]) if g > 1 else case["prompt_embeds"]
    cond = torch.cat([case["condition_latent"]] * 2) if g > 1 else case["condition_latent"]
    windows = context_windows(n, context["frames"], context["overlap"], context.get("closed_loop", False), context.get("weights", "pyramid"))
    scheduler.set_timesteps(case["num_inference_steps"])
    for t in scheduler.timesteps:
        per_frame = [[] for _ in range(n)]
        for idx, wn, _, _ in windows:
            xw = torch.stack([x[:, :, f] for f in idx], dim=2).to(unet.dtype)
            eps = unet(torch.cat([xw, xw]) if g > 1 else xw, t, encoder_hidden_states=text, condition_latent=cond, mask=case["mask"],
                       motion=torch.as_tensor(case["motion"])).sample.float()
            e = eps[:1] + g * (eps[1:] - eps[:1]) if g > 1 else eps
            if g > 1 and guidance_rescale > 0:
                e = rescale_noise_cfg(e, eps[1:], guidance_rescale)
            for j, f in enumerate(idx):
                per_frame[f].append(np.float32(wn[j]).item() * e[:, :, j])
        e_clip = torch.stack([sum(parts[1:], parts[0]) for parts in per_frame], dim=2)
        b, c, f, h, w = x.shape
        flat = scheduler.step(e_clip.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w), t, x.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)).prev_sample
        x = flat.reshape(b, f, c, h, w).permute(0, 2, 1, 3, 4).contiguous()
    return x


@pytest.mark.parametrize("scheduler", [DPMSolverMultistepScheduler, DDIMScheduler, UniPCMultistepScheduler])
def test_generic_loop_is_the_loop_written_by_hand(scheduler):
    unet = _SlotStubUNet(torch.float32)
    for context, guidance, rescale in itertools.product(({"frames": 4, "overlap": 2}, {"frames": 3, "overlap": 1, "weights": "flat", "closed_loop": True},
                                                          {"frames": 4, "overlap": 0}), (9.0, 1.0), (0.0, 0.7)):
        case = _case(10, guidance)
        got = LatentToVideoPipeline(vae=None, unet=unet, scheduler=scheduler())(context=context, guidance_rescale=rescale, **case)[1]
        want = _by_hand(unet, scheduler(), case, context, rescale)
        plain = LatentToVideoPipeline(vae=None, unet=unet, scheduler=scheduler())(guidance_rescale=rescale, **case)[1]
        assert got.shape == (1, 4, 10, 4, 4) and rel_err(got, want) <= 1e-5, (context, guidance, rescale, rel_err(got, want))
        assert rel_err(got, plain) > 1e-2, "the windows change what the slot-dependent UNet predicts"


@pytest.mark.parametrize("scheduler", [DPMSolverMultistepScheduler, DDIMScheduler, UniPCMultistepScheduler])
def test_no_context_and_a_window_that_holds_the_clip_are_the_call_without_the_keyword(emu, monkeypatch, scheduler):
    for name in ("window_gather_latents", "window_merge_tokens", "window_desc"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: pytest.fail(f"{_n} was called with the feature off"))
    for make in (lambda: _SessionStubUNet(torch.float16), lambda: _SlotStubUNet(torch.float16)):       # the fused and the generic loop
        case = _case(6)
        want = LatentToVideoPipeline(vae=None, unet=make(), scheduler=scheduler())(**case)[1]
        for context in (None, {"frames": 6, "overlap": 2}, {"frames": 16}, {"frames": 7, "overlap": 0, "closed_loop": True}):
            got = LatentToVideoPipeline(vae=None, unet=make(), scheduler=scheduler())(context=context, **case)[1]
            assert torch.equal(got, want), context
        for bad in ({"frames": 4, "overlap": 4}, {"length": 4}, {"frames": 100}):                       # refused even where it would not act
            with pytest.raises(ValueError, match="context"):
                LatentToVideoPipeline(vae=None, unet=make(), scheduler=scheduler())(context=bad, **case)


@pytest.mark.parametrize("scheduler", [DPMSolverMultistepScheduler, DDIMScheduler, UniPCMultistepScheduler])
def test_fused_loop_on_the_emulator_matches_the_generic_loop(emu, monkeypatch, scheduler):
    """Stub session on the emulator: per step and window one gather into the session's `sample`, one session run, (one rescale,) one
    merge; then ONE solver kernel on the merged matrix - both halves and the step's guidance, or one half after a rescale or without
    guidance.  The session is built for the window's length."""
    calls = []
    for name in ("window_gather_latents", "window_merge_tokens", "cfg_rescale_tokens", "cfg_dpm_step_tokens", "cfg_ddim_step_tokens", "cfg_unipc_step_tokens"):
        monkeypatch.setattr(ops, name, lambda *a, _s=getattr(ops, name), _n=name, **k: (calls.append((_n, a, k)), _s(*a, **k))[1])
    for context, guidance, rescale in (({"frames": 4, "overlap": 2}, 9.0, 0.0), ({"frames": 4, "overlap": 2}, 9.0, 0.7), ({"frames": 4, "overlap": 2}, 1.0, 0.0),
                                       ({"frames": 3, "overlap": 1, "weights": "flat", "closed_loop": True}, 9.0, 0.0), ({"frames": 4, "overlap": 0}, 9.0, 0.0)):
        del calls[:]
        case = _case(10, guidance)
        windows = context_windows(10, context["frames"], context["overlap"], context.get("closed_loop", False), context.get("weights", "pyramid"))
        unet = _SessionStubUNet(torch.float16)
        fused = LatentToVideoPipeline(vae=None, unet=unet, scheduler=scheduler())
        monkeypatch.setattr(fused, "_denoise_generic", lambda *a, **k: pytest.fail("the fused loop was not selected"))
        got = fused(context=context, guidance_rescale=rescale, **case)[1]
        sess = unet.last_session
        assert sess.inputs["sample"].shape == (1, 4, context["frames"], 4, 4) and sess.runs == 3 * len(windows)
        per_window = ["window_gather_latents", "cfg_rescale_tokens", "window_merge_tokens"] if guidance > 1 and rescale > 0 else ["window_gather_latents", "window_merge_tokens"]
        names = [c[0] for c in calls]
        step = names[len(per_window) * len(windows)]
        assert step.startswith("cfg_") and step.endswith("_step_tokens")
        assert names == (per_window * len(windows) + [step]) * 3
        g = guidance if guidance > 1 and rescale == 0 else None                               # what merge and step kernel are handed
        rows = (2 if g is not None else 1) * 11 * 16
        for name, a, k in calls:
            if name == "window_gather_latents":
                assert a[0].shape == (1, 4, 10, 4, 4) and k["out"] is sess.inputs["sample"]
            elif name == "window_merge_tokens":
                assert a[1].shape == (1, 10, 16, 4) and a[2].shape == (rows, 8) and a[4] == g
            elif name == "cfg_rescale_tokens":
                assert a[1:] == (1, 4, context["frames"], 16, guidance, rescale)                       # per window
            else:
                assert a[0].shape == (rows, 8) and a[1].shape == (1, 4, 10, 4, 4)
                assert a[4 if name == "cfg_dpm_step_tokens" else 3] == g, "the step kernel guides the merged halves as the merge read them"
        generic = LatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=scheduler())(context=context, guidance_rescale=rescale, **case)[1]
        assert torch.isfinite(got).all() and rel_err(got, generic) < 2e-2, (context, guidance, rescale, rel_err(got, generic))


def test_the_keyword_reaches_denoise_from_both_pipelines(monkeypatch):
    from animate_anything_amd import layerdiffuse
    seen = []

    def fake_denoise(self, latents, *a, **k):
        seen.append(k.get("context", "absent"))
        return latents.float()
    monkeypatch.setattr(LatentToVideoPipeline, "denoise", fake_denoise)
    pipe = LatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=DPMSolverMultistepScheduler())
    pipe(**_case(6))
    pipe(context={"frames": 4}, **_case(6))
    rgba = layerdiffuse.MaskedLatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=DPMSolverMultistepScheduler())
    monkeypatch.setattr(rgba, "decode_latents", lambda latents: latents)
    monkeypatch.setattr(layerdiffuse, "decode_rgba", lambda *a: (None, None, None))
    rgba(output_type="pt", context={"frames": 3, "overlap": 1}, **_case(6))
    rgba(output_type="pt", **_case(6))
    assert seen == [None, {"frames": 4}, {"frames": 3, "overlap": 1}, None]


def test_eval_validates_the_key_before_any_model_is_loaded(tmp_path):
    from animate_anything_amd import eval as aa_eval
    missing = str(tmp_path / "no_such_checkpoint")
    for bad in ({"frames": 4, "overlap": 4}, {"frames": 4, "stride": 2}, {"frames": 0}, {"frames": "16"}, {"weights": "gauss"}, {"closed_loop": 1}, 16, [16, 4],
                "pyramid"):
        with pytest.raises(ValueError, match="context"):
            aa_eval.main_eval(missing, {"context": bad, "num_frames": 32})
        with pytest.raises(ValueError, match="context"):
            aa_eval.batch_eval(None, None, None, None, {}, {"context": bad}, str(tmp_path), False)
    assert aa_eval._check_context({}) is None and aa_eval._check_context(None) is None          # absent: off
    assert aa_eval._check_context({"context": {}}) == CONTEXT_DEFAULTS
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text("pretrained_model_path: x\nvalidation_data: {guidance_scale: 9, num_frames: 32, context: {frames: 16, overlap: 6, closed_loop: true}}\n")
    cfg = aa_eval.load_config(str(cfg_path))
    assert aa_eval._check_context(cfg["validation_data"]) == dict(frames=16, overlap=6, weights="pyramid", closed_loop=True)
    cfg = aa_eval.load_config(str(cfg_path), ["validation_data.context.overlap=16"])
    cfg["pretrained_model_path"] = missing
    with pytest.raises(ValueError, match="context.overlap"):
        aa_eval.main_eval(**cfg)
