"""guidance_rescale on the MI355X: the fused loop (UNet session, aa_cfg_rescale_tokens, the sampler's step kernel with guidance off)
against the generic loop (module forward, `rescale_noise_cfg`, the scheduler's `step()`) on the tiny UNet of tests/test_gpu_ddim.py,
6 steps at guidance 9 as in tests/test_gpu_unipc.py, under DPM-Solver++, DDIM and UniPC order 2; hipGraph replay against eager bit
for bit; rescale 0.7 against rescale 0; `guidance_rescale=0.0` against the keyword left out; one run of the eval driver.

The yardstick is max|fused - generic| / max|generic| of the final latents: with rescale 0.7 it may be twice what the same sampler
shows with rescale off (the parent's path) in the same fixture.  Measured on one MI355X (eager and graph alike; rescale off, 0.7):
  DPM-Solver++   2.8495e-3  2.5483e-3
  DDIM           2.7537e-3  2.6364e-3
  UniPC order 2  2.2627e-3  2.5447e-3   (bound 4.5254e-3)
The rescale itself moves the final latents of this model by 7.3e-3 / 8.9e-3 / 1.0e-2 (fused loop; the generic loop 7.0e-3 / 8.9e-3 / 9.6e-3)."""
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


def loops(net, scheduler, graph, generic=True, **kw):
    """(fused, generic) final latents of the same 6-step guided run; `kw` goes to both loops."""
    i, neg = unet_inputs(), unet_inputs(seed=4321)["text"]
    dev = lambda x: x.half().cuda()
    net.enable_graph(graph)
    pipe = LatentToVideoPipeline(vae=None, unet=net, scheduler=scheduler)
    scheduler.set_timesteps(STEPS)
    args = (i["sample"].cuda(), dev(torch.cat([neg, i["text"]])), dev(i["cond"]), dev(i["mask"]), [3.0],
            [int(t) for t in scheduler.timesteps], GUIDANCE)
    autotune, ops.AUTOTUNE = ops.AUTOTUNE, False        # the library's own tile choice: timing-picked tiles would move the distance from run to run
    try:
        with torch.no_grad():
            fused = pipe.denoise(*args, **kw).float().cpu()
            scheduler.set_timesteps(STEPS)              # (a multistep scheduler's `step()` keeps state)
            other = pipe._denoise_generic(*args, **kw).float().cpu() if generic else None
        torch.cuda.synchronize()
    finally:
        ops.AUTOTUNE = autotune
    return fused, other


@pytest.fixture(scope="module")
def net():
    return model()


@pytest.fixture(scope="module")
def runs(net):
    out = {}
    for name, make in SCHEDULERS.items():
        for graph in (False, True):
            out[name, graph, 0.0] = loops(net, make(), graph)
            out[name, graph, RESCALE] = loops(net, make(), graph, guidance_rescale=RESCALE)
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_fused_loop_matches_the_generic_loop(runs, sampler, graph):
    off, on = rel_err(*runs[sampler, graph, 0.0]), rel_err(*runs[sampler, graph, RESCALE])
    print(f"{sampler}: fused vs generic, rescale off {off:.5g}, rescale {RESCALE} {on:.5g} (bound {2 * off:.5g})")
    assert torch.isfinite(runs[sampler, graph, RESCALE][0]).all()
    assert off > 0.0 and on <= 2 * off


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_graph_replay_is_bit_equal_to_eager_and_the_rescale_acts(runs, sampler):
    assert torch.equal(runs[sampler, False, RESCALE][0], runs[sampler, True, RESCALE][0])
    for graph in (False, True):
        fused_on, generic_on = runs[sampler, graph, RESCALE]
        fused_off, generic_off = runs[sampler, graph, 0.0]
        print(f"{sampler}: rescale {RESCALE} vs rescale off, fused {rel_err(fused_on, fused_off):.4g}, generic {rel_err(generic_on, generic_off):.4g}")
        assert not torch.equal(fused_on, fused_off) and not torch.equal(generic_on, generic_off)


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_rescale_zero_is_the_path_without_the_keyword(runs, net, monkeypatch, sampler):
    monkeypatch.setattr(ops, "cfg_rescale_tokens", lambda *a, **k: pytest.fail("guidance_rescale=0.0 launched the rescale"))
    for graph in (False, True):
        fused, _ = loops(net, SCHEDULERS[sampler](), graph, generic=False, guidance_rescale=0.0)
        assert torch.equal(fused, runs[sampler, graph, 0.0][0])


def test_eval_driver_with_guidance_rescale(tmp_path, monkeypatch):
    """`python -m animate_anything_amd.eval` with `validation_data.guidance_rescale=0.7` on a synthetic checkpoint (the flow of
    tests/test_gpu_unipc.py): every step of the fused loop runs aa_cfg_rescale_tokens in place and the DPM-Solver++ kernel with
    guidance off; without the key no step does."""
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
    rescales, guided = [], []
    real, real_step = ops.cfg_rescale_tokens, ops.cfg_dpm_step_tokens
    monkeypatch.setattr(ops, "cfg_rescale_tokens", lambda *a, **k: (rescales.append((a[1:], sorted(k))), real(*a, **k))[1])
    monkeypatch.setattr(ops, "cfg_dpm_step_tokens", lambda *a, **k: (guided.append(a[4]), real_step(*a, **k))[1])
    monkeypatch.setattr(LatentToVideoPipeline, "_denoise_generic", lambda *a, **k: pytest.fail("the eval driver left the fused loop"))
    results = aa_eval.main(["--config", str(tmp_path / "config.yaml"), "--eval", "validation_data.guidance_rescale=0.7"])
    _, frames, latents = results[0]
    assert rescales == [((1, 4, 4, 14 * 18, 9, 0.7), [])] * 3 and guided == [None] * 3
    assert len(frames) == 4 and latents.shape == (1, 4, 4, 14, 18) and torch.isfinite(latents).all()
    assert os.path.exists(tmp_path / "out" / "img" / "0.gif")
    del rescales[:], guided[:]
    plain = aa_eval.main(["--config", str(tmp_path / "config.yaml"), "--eval"])[0][2]
    assert rescales == [] and guided == [9] * 3 and not torch.equal(plain, latents)
