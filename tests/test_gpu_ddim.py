"""DDIM on the MI355X: the fused loop (UNet session + aa_cfg_ddim_step_tokens per step) against the generic loop (module forward +
DDIMScheduler.step) on the tiny UNet, hipGraph replay against eager bit for bit, and one kernel call at the benchmark's shape."""
import pytest
import torch

import oracle
from animate_anything_amd import ops
from animate_anything_amd.pipeline import LatentToVideoPipeline
from animate_anything_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
from animate_anything_amd.unet3d import UNet3DConditionModel
from util import TINY_UNET, rel_err, seeded_state, unet_inputs

pytestmark = pytest.mark.gpu

STEPS, GUIDANCE = 4, 9.0
# max|fused - generic| / max|generic| of the final latents under DPMSolverMultistepScheduler at this shape (same model, inputs, 4 steps,
# guidance 9), measured on an MI355X with this file's `loops`.  The two loops run the same arithmetic in another
# order (guidance halves sharing the UNet's text-independent prefix, fused scalars): DDIM, an update of the same length, gets twice that.
# Measured: DPM-Solver++ 2.46088e-3 (eager and graph alike); DDIM at the same time 3.247e-3, with eta = 0.5 3.433e-3.
DPM_DISTANCE = 2.46088e-3


def model():
    torch.manual_seed(0)
    ref = oracle.UNet3DConditionModel(**TINY_UNET).eval()
    net = UNet3DConditionModel(**TINY_UNET).eval()
    net.load_state_dict(seeded_state(ref))
    return net.half().cuda()


def loops(net, scheduler, graph, eta=0.0, seed=None):
    """(fused, generic) final latents of the same 4-step guided run."""
    i, neg = unet_inputs(), unet_inputs(seed=4321)["text"]
    dev = lambda x: x.half().cuda()
    net.enable_graph(graph)
    pipe = LatentToVideoPipeline(vae=None, unet=net, scheduler=scheduler)
    scheduler.set_timesteps(STEPS)
    args = (i["sample"].cuda(), dev(torch.cat([neg, i["text"]])), dev(i["cond"]), dev(i["mask"]), [3.0],
            [int(t) for t in scheduler.timesteps], GUIDANCE)
    gen = lambda: None if seed is None else torch.Generator(device="cuda").manual_seed(seed)
    autotune, ops.AUTOTUNE = ops.AUTOTUNE, False        # the library's own tile choice: timing-picked tiles would move the distance from run to run
    try:
        with torch.no_grad():
            fused = pipe.denoise(*args, eta=eta, generator=gen())
            scheduler.set_timesteps(STEPS)              # (a multistep scheduler's `step()` keeps state)
            generic = pipe._denoise_generic(*args, eta=eta, generator=gen())
        torch.cuda.synchronize()
    finally:
        ops.AUTOTUNE = autotune
    return fused.float().cpu(), generic.float().cpu()


@pytest.fixture(scope="module")
def runs():
    net = model()
    out = {}
    for graph in (False, True):
        out[graph] = loops(net, DDIMScheduler(), graph)
        out[graph, "eta"] = loops(net, DDIMScheduler(), graph, eta=0.5, seed=5)
    return out


def test_graph_replay_is_bit_equal_to_eager(runs):
    for eager, replay in ((runs[False], runs[True]), (runs[False, "eta"], runs[True, "eta"])):
        assert torch.isfinite(eager[0]).all() and torch.equal(eager[0], replay[0])


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_fused_loop_matches_the_generic_loop(runs, graph):
    fused, generic = runs[graph]
    d = rel_err(fused, generic)
    print(f"DDIM fused vs generic: {d:.4g} (bound {2 * DPM_DISTANCE:.4g})")
    assert d <= 2 * DPM_DISTANCE
    fused, generic = runs[graph, "eta"]                  # eta > 0: both loops draw the same variance noise from generators seeded alike
    d = rel_err(fused, generic)
    print(f"DDIM eta=0.5 fused vs generic: {d:.4g} (bound {2 * DPM_DISTANCE:.4g})")
    assert d <= 2 * DPM_DISTANCE
    assert not torch.equal(runs[graph][0], runs[graph, "eta"][0])


def test_eval_driver_with_sampler_ddim(tmp_path, monkeypatch):
    """`python -m animate_anything_amd.eval` with `sampler=ddim` on a synthetic checkpoint (the flow of tests/test_gpu_eval.py): the clip
    comes out of the fused loop - one aa_cfg_ddim_step_tokens per step, no DPM step, no generic loop."""
    import json
    import os

    import numpy as np
    import yaml
    from PIL import Image

    from animate_anything_amd import eval as aa_eval
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
    steps, real = [], ops.cfg_ddim_step_tokens
    monkeypatch.setattr(ops, "cfg_ddim_step_tokens", lambda *a, **k: (steps.append(k["next_t_value"]), real(*a, **k))[1])
    monkeypatch.setattr(ops, "cfg_dpm_step_tokens", lambda *a, **k: pytest.fail("sampler=ddim ran the DPM-Solver++ step"))
    monkeypatch.setattr(LatentToVideoPipeline, "_denoise_generic", lambda *a, **k: pytest.fail("sampler=ddim left the fused loop"))
    results = aa_eval.main(["--config", str(tmp_path / "config.yaml"), "--eval", "sampler=ddim"])
    _, frames, latents = results[0]
    assert steps == [334.0, 1.0, 1.0]                   # the next timestep deposited by each of the three steps (667 -> 334 -> 1)
    assert len(frames) == 4 and frames[0].shape == (112, 144, 3)
    assert latents.shape == (1, 4, 4, 14, 18) and torch.isfinite(latents).all()
    assert os.path.exists(tmp_path / "out" / "img" / "0.gif")
    with pytest.raises(ValueError, match="sampler"):
        aa_eval.main(["--config", str(tmp_path / "config.yaml"), "--eval", "sampler=plms"])


def test_ddim_step_kernel_at_the_benchmark_shape():
    """aa_cfg_ddim_step_tokens at 2 x 4 x 16 x 64 x 64 (guidance, clamp, epsilon from the clamped x0, noise) against the torch
    expression on the GPU, as test_gpu_svd.test_svd_glue_kernels_at_the_real_shapes does for the Euler kernel."""
    g = torch.Generator(device="cuda").manual_seed(0)
    clips, c, f, h, w = 2, 4, 16, 64, 64
    tok = torch.randn(2 * clips * (f + 1) * h * w, 8, generator=g, device="cuda").half()
    x = torch.randn(clips, c, f, h, w, generator=g, device="cuda")
    noise = torch.randn(clips, c, f, h, w, generator=g, device="cuda")
    s = DDIMScheduler(clip_sample=True, clip_sample_range=8.0)
    s.set_timesteps(10)
    k = s.coefficients(3, eta=0.7, use_clipped_model_output=True)
    m = tok.float().reshape(2 * clips, f + 1, h, w, 8).permute(0, 4, 1, 2, 3)[:, :c, 1:]
    m = m[:clips] + GUIDANCE * (m[clips:] - m[:clips])
    x0 = (k["a_x"] * x + k["a_m"] * m).clamp(-8.0, 8.0)
    share = (x0.abs() == 8.0).float().mean().item()
    want = k["c_0"] * x0 + k["c_e"] * (k["q_x"] * x + k["q_0"] * x0) + k["c_n"] * noise
    lp = torch.empty(clips, c, f, h, w, dtype=torch.float16, device="cuda")
    nt = torch.zeros(2 * clips, device="cuda")
    ops.cfg_ddim_step_tokens(tok, x, lp, GUIDANCE, k, noise=noise, next_t=nt, next_t_value=301.0)
    assert 0.05 < share < 0.95 and k["c_n"] > 0
    assert rel_err(x, want) < 1e-5 and rel_err(lp, x) < 2e-3 and torch.all(nt == 301.0)
