"""Context windows on the MI355X: the fused loop (per step and window: aa_window_gather_latents, the UNet session at the window's
length, aa_window_merge_tokens; then one solver kernel on the merged matrix) against the generic loop (module forward per window, a
weighted fp32 sum, the scheduler's `step()`) on the tiny UNet of tests/test_gpu_ddim.py, 6 steps at guidance 9 on 6x6 latents, under
DPM-Solver++, DDIM and UniPC order 2, `ops.AUTOTUNE` off.

The yardstick is max|fused - generic| / max|generic| of the final latents.  10 frames in windows of 4 with overlap 2 (pyramid) may show
twice the larger of what the same sampler shows UNWINDOWED at 4 frames and at 10 frames in the same fixture (the parent's path; the
margin of tests/test_gpu_cfg_rescale.py).  Measured on one MI355X (unwindowed 4 frames, unwindowed 10 frames, windowed, windowed with
guidance_rescale 0.7; the windowed graph run equals the eager one bit for bit):
  DPM-Solver++   3.0292e-3  3.1915e-3  2.9436e-3  3.1838e-3   (bound 6.3829e-3)
  DDIM           3.4309e-3  3.5971e-3  3.1565e-3  3.4514e-3   (bound 7.1943e-3)
  UniPC order 2  3.8944e-3  3.2904e-3  3.3633e-3  3.0631e-3   (bound 7.7888e-3)
The windows move the final latents of this model by 0.13 / 0.16 / 0.17 of their range against the unwindowed 10-frame run.
Overlap 0 - 8 frames as two windows of 4 - is held against plain `denoise` runs of the two halves."""
import pytest
import torch

from animate_anything_amd import ops
from animate_anything_amd.pipeline import LatentToVideoPipeline
from animate_anything_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler
from test_gpu_ddim import model
from util import rel_err, unet_inputs

pytestmark = pytest.mark.gpu

STEPS, GUIDANCE, RESCALE = 6, 9.0, 0.7
SCHEDULERS = {"dpm": lambda: DPMSolverMultistepScheduler(), "ddim": lambda: DDIMScheduler(), "unipc": lambda: UniPCMultistepScheduler(solver_order=2)}
CONTEXT = dict(frames=4, overlap=2, weights="pyramid")


def loops(net, scheduler, frames, graph=False, fused=True, generic=True, first_frame=0, guidance=GUIDANCE, **kw):
    """(fused, generic) final latents of the same 6-step guided run on frames [first_frame, first_frame + frames) of the 10-frame
    inputs; `kw` goes to both loops."""
    i, neg = unet_inputs(frames=10), unet_inputs(seed=4321)["text"]
    dev = lambda x: x.half().cuda()
    text = torch.cat([neg, i["text"]]) if guidance > 1 else i["text"]
    net.enable_graph(graph)
    pipe = LatentToVideoPipeline(vae=None, unet=net, scheduler=scheduler)
    scheduler.set_timesteps(STEPS)
    args = (i["sample"][:, :, first_frame:first_frame + frames].contiguous().cuda(), dev(text), dev(i["cond"]), dev(i["mask"]), [3.0],
            [int(t) for t in scheduler.timesteps], guidance)
    autotune, ops.AUTOTUNE = ops.AUTOTUNE, False        # the library's own tile choice: timing-picked tiles would move the distance from run to run
    try:
        with torch.no_grad():
            a = pipe.denoise(*args, **kw).float().cpu() if fused else None
            scheduler.set_timesteps(STEPS)              # (a multistep scheduler's `step()` keeps state)
            b = pipe._denoise_generic(*args, **kw).float().cpu() if generic else None
        torch.cuda.synchronize()
    finally:
        ops.AUTOTUNE = autotune
    return a, b


@pytest.fixture(scope="module")
def net():
    return model()


@pytest.fixture(scope="module")
def runs(net):
    """Computed once, shared, never changed: per sampler the unwindowed runs at 4 and 10 frames and the windowed ones."""
    out = {}
    for name, make in SCHEDULERS.items():
        out[name, "plain4"] = loops(net, make(), 4)
        out[name, "plain10"] = loops(net, make(), 10)
        out[name, "windowed"] = loops(net, make(), 10, context=CONTEXT)
        out[name, "windowed graph"] = loops(net, make(), 10, graph=True, generic=False, context=CONTEXT)
        out[name, "rescale"] = loops(net, make(), 10, context=CONTEXT, guidance_rescale=RESCALE)
    return out


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_fused_loop_matches_the_generic_loop(runs, sampler):
    off4, off10 = rel_err(*runs[sampler, "plain4"]), rel_err(*runs[sampler, "plain10"])
    on, on_rescale = rel_err(*runs[sampler, "windowed"]), rel_err(*runs[sampler, "rescale"])
    bound = 2 * max(off4, off10)
    print(f"{sampler}: fused vs generic, unwindowed 4 frames {off4:.5g}, 10 frames {off10:.5g}, windowed {on:.5g}, "
          f"windowed with rescale {RESCALE} {on_rescale:.5g} (bound {bound:.5g})")
    assert torch.isfinite(runs[sampler, "windowed"][0]).all() and torch.isfinite(runs[sampler, "rescale"][0]).all()
    assert min(off4, off10) > 0.0 and on <= bound
    assert on_rescale <= bound
    assert not torch.equal(runs[sampler, "rescale"][0], runs[sampler, "windowed"][0])


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_graph_replay_is_bit_equal_to_eager_and_the_windows_act(runs, sampler):
    assert torch.equal(runs[sampler, "windowed graph"][0], runs[sampler, "windowed"][0])
    fused, generic = runs[sampler, "windowed"]
    plain_fused, plain_generic = runs[sampler, "plain10"]
    print(f"{sampler}: windowed vs unwindowed 10 frames, fused {rel_err(fused, plain_fused):.4g}, generic {rel_err(generic, plain_generic):.4g}")
    assert fused.shape == plain_fused.shape == (2, 4, 10, 6, 6)
    assert not torch.equal(fused, plain_fused) and not torch.equal(generic, plain_generic)
    assert rel_err(fused, plain_fused) > rel_err(fused, generic), "the windows move the result by more than the two loops differ"


def _halves(net, sampler, guidance):
    """8 frames in windows of 4 without overlap, and plain `denoise` of each half's latents: [(part of the windowed result, plain)]."""
    whole, _ = loops(net, SCHEDULERS[sampler](), 8, generic=False, guidance=guidance, context=dict(frames=4, overlap=0))
    return [(whole[:, :, 4 * half:4 * half + 4], loops(net, SCHEDULERS[sampler](), 4, generic=False, first_frame=4 * half, guidance=guidance)[0])
            for half in (0, 1)]


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_overlap_zero_is_a_plain_run_of_each_half(net, sampler):
    """8 frames in windows of 4 without overlap: every frame is held by one window, the two halves never meet, so each half of the
    result is what plain `denoise` gives for that half's latents - bit for bit, at guidance 9: the merged matrix keeps both guidance
    halves, a frame held by one window hands the UNet's u and t through, and the step kernel forms u + g (t - u) from the same bits
    with the same instructions as in the plain run.  (A merged matrix of ROUNDED guided values, one half, missed this by 1.4e-3 ...
    1.7e-3 of the latents' range after 6 steps.)"""
    for half, (part, plain) in enumerate(_halves(net, sampler, GUIDANCE)):
        print(f"{sampler}: half {half}: max|windowed - plain| {(part - plain).abs().max().item():.4g} "
              f"(relative {rel_err(part, plain):.4g}, {int((part != plain).sum())} of {plain.numel()} elements differ)")
        assert torch.equal(part, plain)


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_overlap_zero_without_guidance_is_a_plain_run_of_each_half(net, sampler):
    """The same with guidance off: the merge hands the UNet's bits through, so gather, session, merge and the solver kernel over 8
    frames give bit for bit what the plain loop gives for each half."""
    for part, plain in _halves(net, sampler, 1.0):
        assert torch.isfinite(part).all() and torch.equal(part, plain)


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_closed_loop_runs_and_stays_finite(runs, net, sampler):
    closed, _ = loops(net, SCHEDULERS[sampler](), 10, generic=False, context=dict(CONTEXT, closed_loop=True))
    assert closed.shape == (2, 4, 10, 6, 6) and torch.isfinite(closed).all()
    assert not torch.equal(closed, runs[sampler, "windowed"][0])                 # the fifth window, frames 8 9 0 1, changes the blend


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_a_window_that_holds_the_clip_launches_no_window_op(runs, net, monkeypatch, sampler):
    for name in ("window_gather_latents", "window_merge_tokens"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: pytest.fail(f"{_n} was launched with the feature off"))
    for context in (dict(frames=10, overlap=2), dict(frames=16), None):
        fused, _ = loops(net, SCHEDULERS[sampler](), 10, generic=False, context=context)
        assert torch.equal(fused, runs[sampler, "plain10"][0])


def test_eval_driver_with_context_windows(tmp_path, monkeypatch):
    """`python -m animate_anything_amd.eval` with `num_frames: 10` and `validation_data.context: {frames: 4, overlap: 2}` on a synthetic
    checkpoint (the flow of tests/test_gpu_cfg_rescale.py): 10 frames come out of the fused loop - four windows per step."""
    import json
    import os

    import numpy as np
    import yaml
    from PIL import Image

    from animate_anything_amd import eval as aa_eval
    from animate_anything_amd.unet3d import UNet3DConditionModel
    from animate_anything_amd.vae import AutoencoderKL
    from util import SMALL_UNET, SMALL_VAE
    torch.manual_seed(0)
    ckpt = tmp_path / "ckpt"
    UNet3DConditionModel(**SMALL_UNET).save_pretrained(str(ckpt / "unet"))
    AutoencoderKL(**SMALL_VAE).save_pretrained(str(ckpt / "vae"))
    os.makedirs(ckpt / "scheduler")
    json.dump({"_class_name": "DDIMScheduler", "beta_start": 0.00085, "beta_end": 0.012, "beta_schedule": "scaled_linear",
               "clip_sample": False, "set_alpha_to_one": False, "num_train_timesteps": 1000, "steps_offset": 1,
               "timestep_spacing": "leading"}, open(ckpt / "scheduler" / "scheduler_config.json", "w"))
    Image.fromarray(np.random.default_rng(0).integers(0, 255, (120, 160, 3), dtype=np.uint8)).save(tmp_path / "img.jpg")
    torch.save({"prompt_embeds": torch.randn(1, 77, 128), "negative_prompt_embeds": torch.randn(1, 77, 128)}, tmp_path / "embeds.pt")
    cfg = {"pretrained_model_path": str(ckpt), "motion_mask": True, "motion_strength": True, "seed": 7,
           "output_dir": str(tmp_path / "out"), "iters": 1,
           "validation_data": {"prompt": "", "prompt_image": str(tmp_path / "img.jpg"), "prompt_embeds": str(tmp_path / "embeds.pt"),
                               "num_frames": 10, "width": 128, "height": 128, "num_inference_steps": 3, "guidance_scale": 9, "fps": 8,
                               "context": {"frames": 4, "overlap": 2}}}
    yaml.safe_dump(cfg, open(tmp_path / "config.yaml", "w"))
    gathers, merges, guided = [], [], []
    real_gather, real_merge, real_step = ops.window_gather_latents, ops.window_merge_tokens, ops.cfg_dpm_step_tokens
    monkeypatch.setattr(ops, "window_gather_latents", lambda *a, **k: (gathers.append(tuple(k["out"].shape)), real_gather(*a, **k))[1])
    monkeypatch.setattr(ops, "window_merge_tokens", lambda *a, **k: (merges.append((tuple(a[1].shape), a[4], tuple(a[2].shape))), real_merge(*a, **k))[1])
    monkeypatch.setattr(ops, "cfg_dpm_step_tokens", lambda *a, **k: (guided.append((tuple(a[1].shape), a[4])), real_step(*a, **k))[1])
    monkeypatch.setattr(LatentToVideoPipeline, "_denoise_generic", lambda *a, **k: pytest.fail("the eval driver left the fused loop"))
    results = aa_eval.main(["--config", str(tmp_path / "config.yaml"), "--eval"])
    _, frames, latents = results[0]
    assert gathers == [(1, 4, 4, 14, 18)] * 12 and merges == [((1, 10, 14 * 18, 4), 9, (2 * 11 * 14 * 18, 8))] * 12   # 3 steps x 4 windows
    assert guided == [((1, 4, 10, 14, 18), 9)] * 3                                  # the step kernel guides the merged halves
    assert len(frames) == 10 and latents.shape == (1, 4, 10, 14, 18) and torch.isfinite(latents).all()
    assert os.path.exists(tmp_path / "out" / "img" / "0.gif")
    with pytest.raises(ValueError, match="context"):
        aa_eval.main(["--config", str(tmp_path / "config.yaml"), "--eval", "validation_data.context.overlap=4"])
