"""Adaptive Projected Guidance on the MI355X: the fused loop (UNet session, aa_apg_tokens in place, the sampler's step kernel with
guidance off) against the generic loop (module forward, `adaptive_projected_guidance`, the scheduler's `step()`) on the tiny UNet of
tests/test_gpu_ddim.py, 6 steps at guidance 9 as in tests/test_gpu_cfg_rescale.py, under DPM-Solver++, DDIM and UniPC order 2, eager
and graph; hipGraph replay against eager bit for bit; APG on against APG off; `apg=None` against the keyword left out; one run under
context windows (10 frames in windows of 4, momentum on: one buffer per window); one run of the eval driver.

APG runs with {eta: 0, norm_threshold: rho, momentum: -0.5}, rho = half the |t - u| of the generic loop's first step (fp32), so the
clip acts from the first step on.  The yardstick is max|fused - generic| / max|generic| of the final latents: APG may show twice what
the same sampler shows with APG off (the parent's path) in the same fixture.  Measured on one MI355X (eager and graph alike; APG
off, APG on with rho = 0.17829):
  DPM-Solver++     2.5265e-3  1.2459e-3   (bound 5.0531e-3)
  DDIM             2.7323e-3  1.5820e-3
  UniPC order 2    2.7533e-3  1.5305e-3
  context windows  2.4432e-3  1.3733e-3   (DPM-Solver++, 10 frames in windows of 4, rho = 0.23975)
APG moves the final latents of this model by 7.6e-2 / 9.0e-2 / 8.4e-2 (fused and generic loop alike to three digits)."""
import pytest
import torch

from animate_anything_amd import ops
from animate_anything_amd import pipeline as P
from animate_anything_amd.pipeline import LatentToVideoPipeline
from animate_anything_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler
from test_gpu_ddim import model
from util import rel_err, unet_inputs

pytestmark = pytest.mark.gpu

STEPS, GUIDANCE = 6, 9.0
SCHEDULERS = {"dpm": lambda: DPMSolverMultistepScheduler(), "ddim": lambda: DDIMScheduler(), "unipc": lambda: UniPCMultistepScheduler(solver_order=2)}
CONTEXT = dict(frames=4, overlap=2, weights="pyramid")


def loops(net, scheduler, graph, fused=True, generic=True, frames=None, steps=STEPS, **kw):
    """(fused, generic) final latents of the same guided run; `kw` goes to both loops."""
    i, neg = unet_inputs() if frames is None else unet_inputs(frames=frames), unet_inputs(seed=4321)["text"]
    dev = lambda x: x.half().cuda()
    net.enable_graph(graph)
    pipe = LatentToVideoPipeline(vae=None, unet=net, scheduler=scheduler)
    scheduler.set_timesteps(STEPS)
    args = (i["sample"].cuda(), dev(torch.cat([neg, i["text"]])), dev(i["cond"]), dev(i["mask"]), [3.0],
            [int(t) for t in scheduler.timesteps][:steps], GUIDANCE)
    autotune, ops.AUTOTUNE = ops.AUTOTUNE, False        # the library's own tile choice: timing-picked tiles would move the distance from run to run
    try:
        with torch.no_grad():
            one = pipe.denoise(*args, **kw).float().cpu() if fused else None
            scheduler.set_timesteps(STEPS)              # (a multistep scheduler's `step()` keeps state)
            other = pipe._denoise_generic(*args, **kw).float().cpu() if generic else None
        torch.cuda.synchronize()
    finally:
        ops.AUTOTUNE = autotune
    return one, other


def first_step_norm(net, monkeypatch, **kw):
    """|t - u| of the generic loop's first step (the smallest over its UNet runs), read off `adaptive_projected_guidance`."""
    seen = []
    real = P.adaptive_projected_guidance
    monkeypatch.setattr(P, "adaptive_projected_guidance",
                        lambda u, t, *a: (seen.append((t.double() - u.double()).reshape(t.shape[0], -1).norm(dim=1).min().item()), real(u, t, *a))[1])
    loops(net, DPMSolverMultistepScheduler(), False, fused=False, steps=1, apg=dict(eta=1.0), **kw)
    monkeypatch.setattr(P, "adaptive_projected_guidance", real)
    assert seen and min(seen) > 0.0
    return min(seen)


@pytest.fixture(scope="module")
def net():
    return model()


@pytest.fixture(scope="module")
def apg(net):
    mp = pytest.MonkeyPatch()
    try:
        rho = first_step_norm(net, mp)
    finally:
        mp.undo()
    return dict(eta=0.0, norm_threshold=float(torch.tensor(0.5 * rho, dtype=torch.float32)), momentum=-0.5)


@pytest.fixture(scope="module")
def runs(net, apg):
    """Computed once, shared, never changed."""
    out = {}
    for name, make in SCHEDULERS.items():
        for graph in (False, True):
            out[name, graph, False] = loops(net, make(), graph)
            out[name, graph, True] = loops(net, make(), graph, apg=apg)
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_fused_loop_matches_the_generic_loop(runs, apg, sampler, graph):
    off, on = rel_err(*runs[sampler, graph, False]), rel_err(*runs[sampler, graph, True])
    print(f"{sampler}: fused vs generic, APG off {off:.5g}, APG {apg} {on:.5g} (bound {2 * off:.5g})")
    assert torch.isfinite(runs[sampler, graph, True][0]).all()
    assert off > 0.0 and on <= 2 * off


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_graph_replay_is_bit_equal_to_eager_and_apg_acts(runs, sampler):
    assert torch.equal(runs[sampler, False, True][0], runs[sampler, True, True][0])
    for graph in (False, True):
        fused_on, generic_on = runs[sampler, graph, True]
        fused_off, generic_off = runs[sampler, graph, False]
        print(f"{sampler}: APG on vs APG off, fused {rel_err(fused_on, fused_off):.4g}, generic {rel_err(generic_on, generic_off):.4g}")
        assert rel_err(fused_on, fused_off) > 1e-3 and rel_err(generic_on, generic_off) > 1e-3


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_apg_none_is_the_path_without_the_keyword(runs, net, monkeypatch, sampler):
    monkeypatch.setattr(ops, "apg_tokens", lambda *a, **k: pytest.fail("apg=None launched aa_apg_tokens"))
    for graph in (False, True):
        fused, _ = loops(net, SCHEDULERS[sampler](), graph, generic=False, apg=None)
        assert torch.equal(fused, runs[sampler, graph, False][0])


def test_context_windows_keep_one_momentum_buffer_per_window(net, monkeypatch):
    """10 frames in windows of 4 with overlap 2 under DPM-Solver++, momentum on: four windows per step, each with its own running
    update, APG in front of the merge; held to twice the windowed distance with APG off."""
    rho = first_step_norm(net, monkeypatch, frames=10, context=CONTEXT)
    apg = dict(eta=0.0, norm_threshold=float(torch.tensor(0.5 * rho, dtype=torch.float32)), momentum=-0.5)
    off = rel_err(*loops(net, DPMSolverMultistepScheduler(), False, frames=10, context=CONTEXT))
    buffers, merges = [], []
    real, real_merge = ops.apg_tokens, ops.window_merge_tokens
    monkeypatch.setattr(ops, "apg_tokens", lambda *a, **k: (buffers.append(k["momentum_buf"].data_ptr()), real(*a, **k))[1])
    monkeypatch.setattr(ops, "window_merge_tokens", lambda *a, **k: (merges.append(a[4]), real_merge(*a, **k))[1])
    fused, generic = loops(net, DPMSolverMultistepScheduler(), False, frames=10, context=CONTEXT, apg=apg)
    on = rel_err(fused, generic)
    print(f"context windows: fused vs generic, APG off {off:.5g}, APG {apg} {on:.5g} (bound {2 * off:.5g})")
    assert len(buffers) == 4 * STEPS and len(set(buffers)) == 4 and buffers == buffers[:4] * STEPS
    assert merges == [None] * (4 * STEPS)                                        # the merge runs with guidance off
    assert torch.isfinite(fused).all() and off > 0.0 and on <= 2 * off


def test_eval_driver_with_apg(tmp_path, monkeypatch):
    """`python -m animate_anything_amd.eval` with `validation_data.apg` on a synthetic checkpoint (the flow of
    tests/test_gpu_cfg_rescale.py): every step of the fused loop runs aa_apg_tokens in place and the DPM-Solver++ kernel with guidance
    off; without the key no step does."""
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
                               "num_frames": 4, "width": 128, "height": 128, "num_inference_steps": 3, "guidance_scale": 9, "fps": 8}}
    yaml.safe_dump(cfg, open(tmp_path / "config.yaml", "w"))
    calls, guided = [], []
    real, real_step = ops.apg_tokens, ops.cfg_dpm_step_tokens
    monkeypatch.setattr(ops, "apg_tokens", lambda *a, **k: (calls.append((a[1:], sorted(k))), real(*a, **k))[1])
    monkeypatch.setattr(ops, "cfg_dpm_step_tokens", lambda *a, **k: (guided.append(a[4]), real_step(*a, **k))[1])
    monkeypatch.setattr(LatentToVideoPipeline, "_denoise_generic", lambda *a, **k: pytest.fail("the eval driver left the fused loop"))
    results = aa_eval.main(["--config", str(tmp_path / "config.yaml"), "--eval", "validation_data.apg.eta=0.25",
                            "validation_data.apg.norm_threshold=3", "validation_data.apg.momentum=-0.5"])
    _, frames, latents = results[0]
    assert calls == [((1, 4, 4, 14 * 18, 9, 0.25, 3.0, -0.5), ["momentum_buf"])] * 3 and guided == [None] * 3
    assert len(frames) == 4 and latents.shape == (1, 4, 4, 14, 18) and torch.isfinite(latents).all()
    del calls[:], guided[:]
    plain = aa_eval.main(["--config", str(tmp_path / "config.yaml"), "--eval"])[0][2]
    assert calls == [] and guided == [9] * 3 and not torch.equal(plain, latents)
