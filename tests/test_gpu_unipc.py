"""UniPC on the MI355X: the fused loop (UNet session + aa_cfg_unipc_step_tokens per step) against the generic loop (module forward +
UniPCMultistepScheduler.step) on the tiny UNet of tests/test_gpu_ddim.py, hipGraph replay against eager bit for bit, and one kernel
call at the benchmark's shape.

The two loops are not bit-equal under any sampler (guidance halves sharing the UNet's text-independent prefix, fused scalars): the
yardstick is max|fused - generic| / max|generic| of the final latents under DPMSolverMultistepScheduler - the parent's code path,
measured in the same fixture (same model, inputs, 6 steps, guidance 9, tile autotuning off) - and UniPC, the same arithmetic in
another order, is allowed twice that, the margin DDIM was given.
Measured on one MI355X in one process (eager and graph alike), after each of the 6 steps:
  DPM-Solver++    2.292e-3 2.679e-3 2.594e-3 2.722e-3 2.738e-3 2.8495e-3   (final 2.8495e-3: the bound is 5.699e-3)
  UniPC order 2   2.936e-3 2.839e-3 2.311e-3 2.358e-3 2.288e-3 2.2627e-3
  UniPC order 3   2.936e-3 2.839e-3 2.456e-3 2.454e-3 2.295e-3 2.3708e-3
The kernel at the benchmark's shape: x' 5.3e-6, xhat 1.1e-6, m 7.2e-6 against a bound of 1.06e-3."""
import pytest
import torch

from animate_anything_amd import ops
from animate_anything_amd.pipeline import LatentToVideoPipeline
from animate_anything_amd.schedulers import DPMSolverMultistepScheduler, UniPCMultistepScheduler
from test_gpu_ddim import model
from util import rel_err, unet_inputs

pytestmark = pytest.mark.gpu

STEPS, GUIDANCE = 6, 9.0


def loops(net, scheduler, graph):
    """(fused, generic): the latents after every step of the same 6-step guided run through both loops."""
    i, neg = unet_inputs(), unet_inputs(seed=4321)["text"]
    dev = lambda x: x.half().cuda()
    net.enable_graph(graph)
    pipe = LatentToVideoPipeline(vae=None, unet=net, scheduler=scheduler)
    scheduler.set_timesteps(STEPS)
    args = (i["sample"].cuda(), dev(torch.cat([neg, i["text"]])), dev(i["cond"]), dev(i["mask"]), [3.0],
            [int(t) for t in scheduler.timesteps], GUIDANCE)
    fused, generic = [], []
    autotune, ops.AUTOTUNE = ops.AUTOTUNE, False        # the library's own tile choice: timing-picked tiles would move the distance from run to run
    try:
        with torch.no_grad():
            pipe.denoise(*args, callback=lambda k, t, x: fused.append(x.float().cpu()))
            scheduler.set_timesteps(STEPS)              # (a multistep scheduler's `step()` keeps state)
            pipe._denoise_generic(*args, callback=lambda k, t, x: generic.append(x.float().cpu()))
        torch.cuda.synchronize()
    finally:
        ops.AUTOTUNE = autotune
    assert len(fused) == len(generic) == STEPS
    return fused, generic


SCHEDULERS = {"dpm": lambda: DPMSolverMultistepScheduler(), "order2": lambda: UniPCMultistepScheduler(solver_order=2),
              "order3": lambda: UniPCMultistepScheduler(solver_order=3)}


@pytest.fixture(scope="module")
def runs():
    net = model()
    return {(name, graph): loops(net, make(), graph) for graph in (False, True) for name, make in SCHEDULERS.items()}


@pytest.mark.parametrize("order", ["order2", "order3"])
def test_graph_replay_is_bit_equal_to_eager(runs, order):
    eager, replay = runs[order, False][0], runs[order, True][0]
    assert torch.isfinite(eager[-1]).all() and all(torch.equal(a, b) for a, b in zip(eager, replay))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("order", ["order2", "order3"])
def test_fused_loop_matches_the_generic_loop(runs, order, graph):
    per_step = lambda name: [rel_err(f, g) for f, g in zip(*runs[name, graph])]
    dpm, uni = per_step("dpm"), per_step(order)
    print("DPM-Solver++ fused vs generic after each step: " + " ".join(f"{d:.4g}" for d in dpm))
    print(f"UniPC {order} fused vs generic after each step: " + " ".join(f"{d:.4g}" for d in uni))
    print(f"final: UniPC {uni[-1]:.5g}, DPM-Solver++ {dpm[-1]:.5g}, bound {2 * dpm[-1]:.5g}")
    assert dpm[-1] > 0.0 and uni[-1] <= 2 * dpm[-1]
    assert not torch.equal(runs[order, graph][0][-1], runs["dpm", graph][0][-1])


def test_eval_driver_with_sampler_unipc(tmp_path, monkeypatch):
    """`python -m animate_anything_amd.eval` with `sampler=unipc` on a synthetic checkpoint that ships a DDIM scheduler config (the flow
    of tests/test_gpu_ddim.py): the clip comes out of the fused loop - one aa_cfg_unipc_step_tokens per step, no other solver step, no
    generic loop."""
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
    steps, real = [], ops.cfg_unipc_step_tokens
    monkeypatch.setattr(ops, "cfg_unipc_step_tokens", lambda *a, **k: (steps.append((a[4]["corr_on"], k["next_t_value"])), real(*a, **k))[1])
    monkeypatch.setattr(ops, "cfg_dpm_step_tokens", lambda *a, **k: pytest.fail("sampler=unipc ran the DPM-Solver++ step"))
    monkeypatch.setattr(ops, "cfg_ddim_step_tokens", lambda *a, **k: pytest.fail("sampler=unipc ran the DDIM step"))
    monkeypatch.setattr(LatentToVideoPipeline, "_denoise_generic", lambda *a, **k: pytest.fail("sampler=unipc left the fused loop"))
    results = aa_eval.main(["--config", str(tmp_path / "config.yaml"), "--eval", "sampler=unipc"])
    _, frames, latents = results[0]
    assert steps == [(False, 501.0), (True, 251.0), (True, 251.0)]      # leading spacing, offset 1: 751 -> 501 -> 251; corrector from step 1 on
    assert len(frames) == 4 and latents.shape == (1, 4, 4, 14, 18) and torch.isfinite(latents).all()
    assert os.path.exists(tmp_path / "out" / "img" / "0.gif")


def test_unipc_step_kernel_at_the_benchmark_shape():
    """aa_cfg_unipc_step_tokens at tokens [2*17*4096, 8] / latents [1, 4, 16, 64, 64] (corrector order 3, predictor order 3)
    against float64 on the GPU, at the bound of tests/test_unipc_step.py: 1e-5 * max(1, max sum|coefficient * operand|)."""
    g = torch.Generator(device="cuda").manual_seed(0)
    clips, c, f, h, w = 1, 4, 16, 64, 64
    r = lambda *s: torch.randn(*s, generator=g, device="cuda")
    tok = r(2 * clips * (f + 1) * h * w, 8).half()
    x, last, h1, h2, h3 = (r(clips, c, f, h, w) for _ in range(5))
    s = UniPCMultistepScheduler(solver_order=3)
    s.set_timesteps(10)
    k = s.coefficients(5)
    assert s.orders(5) == (3, 3)
    e = tok.double().reshape(2 * clips, f + 1, h, w, 8).permute(0, 4, 1, 2, 3)[:, :c, 1:]
    e_abs = e[:clips].abs() + GUIDANCE * (e[clips:].abs() + e[:clips].abs())
    e = e[:clips] + GUIDANCE * (e[clips:] - e[:clips])
    X, L, H1, H2, H3 = (v.double() for v in (x, last, h1, h2, h3))
    m = k["a_x"] * X + k["a_m"] * e
    m_abs = abs(k["a_x"]) * X.abs() + abs(k["a_m"]) * e_abs
    xh = k["q_l"] * L + k["q_1"] * H1 + k["q_2"] * H2 + k["q_3"] * H3 + k["q_n"] * m
    xh_abs = abs(k["q_l"]) * L.abs() + abs(k["q_1"]) * H1.abs() + abs(k["q_2"]) * H2.abs() + abs(k["q_3"]) * H3.abs() + abs(k["q_n"]) * m_abs
    want = k["p_x"] * xh + k["p_0"] * m + k["p_1"] * H1 + k["p_2"] * H2
    top = abs(k["p_x"]) * xh_abs + abs(k["p_0"]) * m_abs + abs(k["p_1"]) * H1.abs() + abs(k["p_2"]) * H2.abs()
    bound = 1e-5 * max(1.0, torch.maximum(top, torch.maximum(xh_abs, m_abs)).max().item())
    keep1, keep2 = h1.clone(), h2.clone()
    lp = torch.empty(clips, c, f, h, w, dtype=torch.float16, device="cuda")
    nt = torch.zeros(2 * clips, device="cuda")
    rotated = ops.cfg_unipc_step_tokens(tok, x, lp, GUIDANCE, k, last, (h1, h2, h3), next_t=nt, next_t_value=301.0)
    errs = [(got.double() - ref).abs().max().item() for got, ref in ((x, want), (last, xh), (h3, m))]
    print(f"x' / xhat / m errors {errs} (bound {bound:.3g})")
    assert max(errs) <= bound
    assert rotated[0] is h3 and rotated[1] is h1 and rotated[2] is h2 and torch.equal(h1, keep1) and torch.equal(h2, keep2)
    assert rel_err(lp, x) < 2e-3 and torch.all(nt == 301.0)
