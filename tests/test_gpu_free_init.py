"""FreeInit on the MI355X, on the tiny UNet of tests/test_gpu_ddim.py: 4 frames of 6x6 latents, 6 steps at guidance 9, two iterations
with a butterworth filter of stop frequency 0.6 / 0.6 (the default 0.25 leaves a mask of ~0 at this size), under DPM-Solver++, DDIM and
UniPC order 2, `ops.AUTOTUNE` off.

Wiring, exact: `pipe(..., free_init=dict(num_iters=2, ...), generator=seeded)` equals, bit for bit, the sequence written out here -
`denoise`, one torch.randn from an equally seeded generator, ops.freeinit_mix, `set_timesteps`, `denoise` - eager and with graphs on.

Parity: max|fused - generic| / max|generic| of the final latents, the fused loop being denoise / ops.freeinit_mix / denoise and the generic
one _denoise_generic / a float64 torch.fft mix on the CPU / _denoise_generic (the same fresh noise on both sides).  The two-iteration run
may show twice what ONE iteration of the same sampler shows in this fixture (the parent's path): the first iteration's difference enters the
second scaled by sqrt(abar) ~ 0.07 and low-passed, so the second iteration should sit near the single-run distance; the factor 2 is
the margin of tests/test_gpu_context_windows.py.  Measured on one MI355X (one iteration, two iterations, bound; share of the latents'
range by which the second iteration moves the result):
  DPM-Solver++   3.0251e-3  3.4850e-3  (bound 6.0502e-3)   0.620
  DDIM           2.9793e-3  4.5529e-3  (bound 5.9587e-3)   0.628
  UniPC order 2  3.1227e-3  3.1052e-3  (bound 6.2454e-3)   0.629
The effect is reported, not held to a value: it only has to exceed 0.01, or the test would not be exercising the feature."""
import pytest
import torch

from animate_anything_amd import ops
from animate_anything_amd.pipeline import LatentToVideoPipeline
from animate_anything_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler, check_free_init
from test_gpu_ddim import model
from util import rel_err, unet_inputs

pytestmark = pytest.mark.gpu

STEPS, GUIDANCE, FRAMES, SEED = 6, 9.0, 4, 2024
SCHEDULERS = {"dpm": lambda: DPMSolverMultistepScheduler(), "ddim": lambda: DDIMScheduler(), "unipc": lambda: UniPCMultistepScheduler(solver_order=2)}
FREE_INIT = dict(num_iters=2, method="butterworth", spatial_stop_frequency=0.6, temporal_stop_frequency=0.6)


def operands():
    i, neg = unet_inputs(frames=FRAMES), unet_inputs(seed=4321)["text"]
    dev = lambda x: x.half().cuda()
    return i["sample"].contiguous().cuda(), dev(i["text"]), dev(neg), dev(i["cond"]), dev(i["mask"])


def by_pipeline(net, scheduler, graph):
    lat, text, neg, cond, mask = operands()
    net.enable_graph(graph)
    pipe = LatentToVideoPipeline(vae=None, unet=net, scheduler=scheduler)
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    out = pipe(latents=lat, prompt_embeds=text, negative_prompt_embeds=neg, condition_latent=cond, mask=mask, motion=[3.0],
               num_inference_steps=STEPS, guidance_scale=GUIDANCE, free_init=FREE_INIT, generator=gen, output_type="latent", return_dict=False)[1]
    torch.cuda.synchronize()
    return out.cpu()


def by_hand(net, scheduler, graph, fused=True):
    """denoise -> randn -> mix -> set_timesteps -> denoise; returns (first iteration, second iteration in the model dtype, second in
    fp32).  fused: `denoise` and ops.freeinit_mix; else `_denoise_generic` and a float64 torch.fft mix on the CPU."""
    lat, text, neg, cond, mask = operands()
    net.enable_graph(graph)
    pipe = LatentToVideoPipeline(vae=None, unet=net, scheduler=scheduler)
    run = pipe.denoise if fused else pipe._denoise_generic
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    both = torch.cat([neg, text])
    scheduler.set_timesteps(STEPS)
    first = run(lat, both, cond, mask, [3.0], [int(t) for t in scheduler.timesteps], GUIDANCE)
    kept = first.float().cpu()
    z = torch.randn(tuple(lat.shape), generator=gen, device="cuda", dtype=torch.float32)
    a, s = pipe.free_init_scalars()
    tables = pipe.free_init_tables(check_free_init(FREE_INIT), lat)
    if fused:
        x = ops.freeinit_mix(first, lat, z, a, s, tables, out=first)
    else:
        dims = (-3, -2, -1)
        d = a * first.double().cpu() + s * lat.double().cpu() - z.double().cpu()
        lp = torch.fft.ifftn(tables.mask.double().cpu() * torch.fft.fftn(d, dim=dims), dim=dims).real
        x = (z.double().cpu() + lp).float().cuda()
    scheduler.set_timesteps(STEPS)
    second = run(x, both, cond, mask, [3.0], [int(t) for t in scheduler.timesteps], GUIDANCE)
    torch.cuda.synchronize()
    return kept, second.to(net.dtype).cpu(), second.float().cpu()


@pytest.fixture(scope="module")
def net():
    return model()


@pytest.fixture(scope="module")
def runs(net):
    """Computed once, shared, never changed."""
    out = {}
    autotune, ops.AUTOTUNE = ops.AUTOTUNE, False        # the library's own tile choice: timing-picked tiles would move the distance from run to run
    try:
        with torch.no_grad():
            for name, make in SCHEDULERS.items():
                out[name, "pipeline"] = by_pipeline(net, make(), False)
                out[name, "pipeline graph"] = by_pipeline(net, make(), True)
                out[name, "hand"] = by_hand(net, make(), False)
                out[name, "hand graph"] = by_hand(net, make(), True)
                out[name, "generic"] = by_hand(net, make(), False, fused=False)
    finally:
        ops.AUTOTUNE = autotune
        net.enable_graph(False)
    return out


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_the_pipeline_runs_the_sequence_written_by_hand(runs, sampler):
    bits = lambda v: v.contiguous().view(torch.int16)
    want = runs[sampler, "hand"][1]
    assert want.dtype == torch.float16 and want.shape == (2, 4, FRAMES, 6, 6) and torch.isfinite(want).all()
    assert torch.equal(bits(runs[sampler, "pipeline"]), bits(want))
    assert torch.equal(bits(runs[sampler, "pipeline graph"]), bits(want)), "a graph replay repeats the eager bits"
    assert torch.equal(bits(runs[sampler, "hand graph"][1]), bits(want))
    assert torch.equal(runs[sampler, "hand graph"][0], runs[sampler, "hand"][0])


@pytest.mark.parametrize("sampler", list(SCHEDULERS))
def test_fused_loop_matches_the_generic_loop_and_the_feature_acts(runs, sampler):
    first_f, _, second_f = runs[sampler, "hand"]
    first_g, _, second_g = runs[sampler, "generic"]
    one, two = rel_err(first_f, first_g), rel_err(second_f, second_g)
    moved = (second_f - first_f).abs().max().item() / (first_f.max() - first_f.min()).item()
    print(f"{sampler}: fused vs generic, one iteration {one:.5g}, two iterations {two:.5g} (bound {2 * one:.5g}); "
          f"the second iteration moves the latents by {moved:.3g} of their range")
    assert torch.isfinite(second_f).all() and one > 0.0
    assert two <= 2 * one
    assert moved > 0.01, "the second iteration does not move the result: the test is not exercising the feature"
