"""`keep` (the known-region blend of inpainting samplers) on the MI355X: the fused loop (UNet session, solver kernel, aa_keep_blend in
place on the fp32 latents) against the generic loop (module forward, the scheduler's `step()`, the blend as torch expressions) in the
fixture of tests/test_gpu_context_windows.py - the tiny UNet of tests/test_gpu_ddim.py, 6 steps at guidance 9 on 6x6 latents, 4 frames,
`ops.AUTOTUNE` off - under DPM-Solver++ and DDIM, with a mask of the test's own handed over as keep["mask"]: the left half 0 (held), the
right half 1 (free), one column of 0.5 between them.

The yardstick is max|fused - generic| / max|generic| of the final latents: with `keep` on it may show twice what the same sampler
shows with `keep` off in the same fixture (the parent's path; the margin of tests/test_gpu_context_windows.py), and 10 frames in
windows of 4 / 2 with `keep` twice what the same windows show without.  Measured on one MI355X (keep off, keep on; windowed keep off,
windowed keep on; the graph run with `keep` equals the eager one bit for bit):
  DPM-Solver++   2.5705e-3  2.7518e-3  3.0866e-3  2.7759e-3   (bounds 5.1411e-3, 6.1733e-3)
  DDIM           3.0381e-3  3.5968e-3  3.2063e-3  4.2291e-3   (bounds 6.0762e-3, 6.4126e-3)
The held region ends as the known latents bit for bit in both loops, an all-ones mask is the plain run bit for bit, an all-zeros mask
gives the known latents, and with the feature off nothing is launched."""
import pytest
import torch

from animate_anything_amd import ops
from animate_anything_amd.pipeline import LatentToVideoPipeline
from animate_anything_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
from test_gpu_context_windows import CONTEXT, loops
from test_gpu_ddim import model
from util import rel_err, unet_inputs

pytestmark = pytest.mark.gpu

SCHEDULERS = {"dpm": lambda: DPMSolverMultistepScheduler(), "ddim": lambda: DDIMScheduler()}
H = W = 6


def held_mask(kind="mixed"):
    m = torch.zeros(1, 1, 1, H, W)
    if kind == "ones":
        m += 1.0
    elif kind == "mixed":
        m[..., W // 2] = 0.5
        m[..., W // 2 + 1:] = 1.0
    return m.half().cuda()


def keep_of(frames, kind="mixed"):
    noise = torch.randn((2, 4, frames, H, W), generator=torch.Generator().manual_seed(77)).cuda()
    return dict(mask=held_mask(kind), noise=noise)


def known_of(frames):
    """The condition latent as the loops hold it (fp16), widened and broadcast over the frames."""
    return unet_inputs(frames=10)["cond"].half().float().expand(2, 4, frames, H, W)


@pytest.fixture(scope="module")
def net():
    return model()


@pytest.fixture(scope="module")
def runs(net):
    """Computed once, shared, never changed: per sampler (fused, generic) final latents."""
    out = {}
    for name, make in SCHEDULERS.items():
        out[name, "plain"] = loops(net, make(), 4)
        out[name, "keep"] = loops(net, make(), 4, keep=keep_of(4))
        out[name, "keep graph"] = loops(net, make(), 4, graph=True, generic=False, keep=keep_of(4))
        out[name, "ones"] = loops(net, make(), 4, generic=False, keep=keep_of(4, "ones"))
        out[name, "zeros"] = loops(net, make(), 4, keep=keep_of(4, "zeros"))
        out[name, "windowed"] = loops(net, make(), 10, context=CONTEXT)
        out[name, "windowed keep"] = loops(net, make(), 10, context=CONTEXT, keep=keep_of(10))
    return out


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_fused_loop_matches_the_generic_loop(runs, sampler):
    off, on = rel_err(*runs[sampler, "plain"]), rel_err(*runs[sampler, "keep"])
    print(f"{sampler}: fused vs generic, keep off {off:.5g}, keep on {on:.5g} (bound {2 * off:.5g})")
    assert torch.isfinite(runs[sampler, "keep"][0]).all()
    assert off > 0.0 and on <= 2 * off
    assert not torch.equal(runs[sampler, "keep"][0], runs[sampler, "plain"][0]), "the blend acts"


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_graph_replay_is_bit_equal_to_eager(runs, sampler):
    assert torch.equal(runs[sampler, "keep graph"][0], runs[sampler, "keep"][0])


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_exactness(runs, sampler):
    known = known_of(4)
    held = (held_mask().float().cpu() <= 0).expand(known.shape)
    for got in runs[sampler, "keep"]:
        assert torch.equal(got[held], known[held]), "the held region ends as the known latents, bit for bit"
    assert not torch.equal(runs[sampler, "keep"][0][~held], known[~held])
    assert torch.equal(runs[sampler, "ones"][0], runs[sampler, "plain"][0]), "an all-ones mask is the plain run"
    for got in runs[sampler, "zeros"]:
        assert torch.equal(got, known), "an all-zeros mask gives the known latents"


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_it_composes_with_context_windows(runs, sampler):
    off, on = rel_err(*runs[sampler, "windowed"]), rel_err(*runs[sampler, "windowed keep"])
    print(f"{sampler}: 10 frames in windows of 4 / 2, fused vs generic, keep off {off:.5g}, keep on {on:.5g} (bound {2 * off:.5g})")
    known = known_of(10)
    held = (held_mask().float().cpu() <= 0).expand(known.shape)
    for got in runs[sampler, "windowed keep"]:
        assert got.shape == (2, 4, 10, H, W) and torch.isfinite(got).all() and torch.equal(got[held], known[held])
    assert off > 0.0 and on <= 2 * off
    assert not torch.equal(runs[sampler, "windowed keep"][0], runs[sampler, "windowed"][0])


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_off_launches_nothing(runs, net, monkeypatch, sampler):
    monkeypatch.setattr(ops, "keep_blend", lambda *a, **k: pytest.fail("keep_blend was launched with the feature off"))
    for off in (None, False):
        fused, _ = loops(net, SCHEDULERS[sampler](), 4, generic=False, keep=off)
        assert torch.equal(fused, runs[sampler, "plain"][0])


def test_eval_driver_keeps_the_unmasked_region(tmp_path, monkeypatch):
    """`python -m animate_anything_amd.eval` with `validation_data.keep_unmasked: true` and a PNG mask whose left half is 0, on the
    synthetic checkpoint of tests/test_gpu_context_windows.py: the fused loop, one blend per step and one after decoding, and every output
    frame shows the input image's own pixels where the mask is 0, byte for byte; without the key the region is re-rendered."""
    import json
    import os

    import numpy as np
    import yaml
    from PIL import Image

    from animate_anything_amd import eval as aa_eval
    from animate_anything_amd.pipeline import tensor2vid
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
    motion = np.zeros((120, 160), dtype=np.uint8)
    motion[:, 80:] = 255
    Image.fromarray(motion).save(tmp_path / "mask.png")
    torch.save({"prompt_embeds": torch.randn(1, 77, 128), "negative_prompt_embeds": torch.randn(1, 77, 128)}, tmp_path / "embeds.pt")
    cfg = {"pretrained_model_path": str(ckpt), "motion_mask": True, "motion_strength": True, "seed": 7,
           "output_dir": str(tmp_path / "out"), "iters": 1,
           "validation_data": {"prompt": "", "prompt_image": str(tmp_path / "img.jpg"), "prompt_embeds": str(tmp_path / "embeds.pt"),
                               "mask": str(tmp_path / "mask.png"), "num_frames": 4, "width": 128, "height": 128, "num_inference_steps": 3,
                               "guidance_scale": 9, "fps": 8, "keep_unmasked": True}}
    yaml.safe_dump(cfg, open(tmp_path / "config.yaml", "w"))
    blends = []
    real = ops.keep_blend
    monkeypatch.setattr(ops, "keep_blend", lambda *a, **k: (blends.append(tuple(a[0].shape)), real(*a, **k))[1])
    monkeypatch.setattr(LatentToVideoPipeline, "_denoise_generic", lambda *a, **k: pytest.fail("the eval driver left the fused loop"))
    _, frames, latents = aa_eval.main(["--config", str(tmp_path / "config.yaml"), "--eval"])[0]
    height, width = frames[0].shape[:2]
    assert (height, width) == (112, 144) and len(frames) == 4 and latents.shape == (1, 4, 4, 14, 18) and torch.isfinite(latents).all()
    assert blends == [(1, 4, 4, 14, 18)] * 3 + [(1, 3, 4, height, width)], "one blend per step, one after decoding"
    held = aa_eval.load_motion_mask(str(tmp_path / "mask.png"), width, height) == 0
    assert held.any() and not held.all()
    image = aa_eval.preprocess_image(Image.open(tmp_path / "img.jpg").convert("RGB"), height, width)
    want = tensor2vid(image[:, :, None])[0]
    for frame in frames:
        assert frame.shape == want.shape and (frame[held] == want[held]).all(), "the held pixels are the input image's, byte for byte"
    assert any((frame[~held] != want[~held]).any() for frame in frames)
    del blends[:]
    del cfg["validation_data"]["keep_unmasked"]                                          # absent: off
    yaml.safe_dump(cfg, open(tmp_path / "plain.yaml", "w"))
    _, plain_frames, _ = aa_eval.main(["--config", str(tmp_path / "plain.yaml"), "--eval"])[0]
    assert not blends
    assert any((frame[held] != want[held]).any() for frame in plain_frames), "without the key the held region is re-rendered"
    with pytest.raises(ValueError, match="keep_unmasked"):
        aa_eval.main(["--config", str(tmp_path / "config.yaml"), "--eval", "sampler=unipc"])
