"""aa_cfg_ddim_step_tokens (guidance + DDIMScheduler.step from the UNet's token layout) against the float64 formula evaluated from
the same rounded inputs, on the emulator and on the GPU: every prediction type, eta = 0 and eta > 0 with a noise tensor, epsilon
from the model output and from the clamped x0, clamping that really clamps, both token pitches, f16 and bf16 tokens."""
import math

import pytest
import torch

from animate_anything_amd import ops
from animate_anything_amd.schedulers import DDIMScheduler

DEV = "cpu"


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    global DEV
    if request.param == "emu":
        DEV = "cpu"
        request.getfixturevalue("emu")
    else:
        assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
        DEV = "cuda"
    yield request.param
    DEV = "cpu"


CLIPS, C, FRAMES, H, W = 2, 4, 3, 2, 5
ABAR = 0.5041                                   # alpha_bar_t of the hand-made step (sqrt = 0.71)
ABAR_PREV = 0.64


def coefficients(prediction_type, eta, clip, eps_from_x0, abar=ABAR, abar_prev=ABAR_PREV):
    """The scalars of one step from alpha_bar_t = abar to abar_prev, written out from the formulas (not through DDIMScheduler)."""
    sa, sb = math.sqrt(abar), math.sqrt(1.0 - abar)
    a_x, a_m, e_x, e_m = {"epsilon": (1 / sa, -sb / sa, 0.0, 1.0), "sample": (0.0, 1.0, 1 / sb, -sa / sb),
                          "v_prediction": (sa, -sb, sb, sa)}[prediction_type]
    sigma = eta * math.sqrt((1 - abar_prev) / (1 - abar) * (1 - abar / abar_prev))
    return dict(a_x=a_x, a_m=a_m, e_x=e_x, e_m=e_m, q_x=1 / sb, q_0=-sa / sb, clip=clip, eps_from_x0=eps_from_x0,
                c_0=math.sqrt(abar_prev), c_e=math.sqrt(1 - abar_prev - sigma * sigma), c_n=sigma)


def operands(dt, cfg, ld, seed=161):
    g = torch.Generator().manual_seed(seed)
    b = 2 * CLIPS if cfg else CLIPS
    tok = torch.randn(b * (FRAMES + 1) * H * W, ld, generator=g).to(dt)
    x = torch.randn(CLIPS, C, FRAMES, H, W, generator=g)
    noise = torch.randn(CLIPS, C, FRAMES, H, W, generator=g)
    return tok, x, noise


def reference(tok, x, noise, guidance, k):
    """float64, from the rounded tokens; returns (x', share of elements the clamp changed)."""
    b = tok.shape[0] // ((FRAMES + 1) * H * W)
    m = tok.double().reshape(b, FRAMES + 1, H, W, -1).permute(0, 4, 1, 2, 3)[:, :C, 1:]
    if guidance is not None:
        m = m[:CLIPS] + guidance * (m[CLIPS:] - m[:CLIPS])
    x = x.double()
    x0 = k["a_x"] * x + k["a_m"] * m
    share = 0.0
    if k["clip"] is not None:
        share = (x0.abs() > k["clip"]).double().mean().item()
        x0 = x0.clamp(-k["clip"], k["clip"])
    e = k["q_x"] * x + k["q_0"] * x0 if k["eps_from_x0"] else k["e_x"] * x + k["e_m"] * m
    out = k["c_0"] * x0 + k["c_e"] * e
    if k["c_n"] != 0.0:
        out = out + k["c_n"] * noise.double()
    return out, share


def check(dt, cfg, ld, k, with_noise):
    """Tolerances of tests/test_kernels.py::test_cfg_dpm_step_tokens (f16: state 1e-5, 16-bit copy 2e-3) and of
    tests/test_kernels_bf16.py::test_cfg_dpm_step_tokens (state 1e-5, copy = the round-to-nearest of the state)."""
    tok, x, noise = operands(dt, cfg, ld)
    guidance = 9.0 if cfg else None
    want, share = reference(tok, x, noise, guidance, k)
    if k["clip"] is not None:
        assert 0.25 <= share <= 0.75, f"the reference clamps {share:.2f} of the elements: the case does not test the clamp"
    b = 2 * CLIPS if cfg else CLIPS
    xd = x.to(DEV)
    lp = torch.empty(CLIPS, C, FRAMES, H, W, dtype=dt, device=DEV)
    nt = torch.zeros(b, dtype=torch.float32, device=DEV)
    ops.cfg_ddim_step_tokens(tok.to(DEV), xd, lp, guidance, k, noise=noise.to(DEV) if with_noise else None, next_t=nt, next_t_value=913.0)
    got, ref = xd.double().cpu(), want
    err, top = (got - ref).abs().max().item(), max(1.0, ref.abs().max().item())
    print(f"state err {err:.3g} (bound {1e-5 * top:.3g}), clamped share {share:.2f}")
    assert err <= 1e-5 * top
    if dt == torch.float16:
        assert (lp.double().cpu() - got).abs().max().item() <= 2e-3 * max(1.0, got.abs().max().item())
    else:
        assert torch.equal(lp.cpu(), xd.cpu().to(dt))
    assert torch.equal(nt.cpu(), torch.full((b,), 913.0))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("cfg", [True, False], ids=["guided", "plain"])
@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("prediction_type", ["epsilon", "sample", "v_prediction"])
def test_prediction_types_and_pitches(backend, prediction_type, ld, cfg, dt):
    check(dt, cfg, ld, coefficients(prediction_type, 0.0, None, False), with_noise=False)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("cfg", [True, False], ids=["guided", "plain"])
@pytest.mark.parametrize("eps_from_x0", [False, True], ids=["eps_model", "eps_clipped"])
@pytest.mark.parametrize("eta", [0.0, 0.7])
@pytest.mark.parametrize("prediction_type", ["epsilon", "sample", "v_prediction"])
def test_eta_noise_and_clipped_epsilon(backend, prediction_type, eta, eps_from_x0, cfg, dt):
    """eta > 0 reads the noise tensor; eta = 0 is handed one too and must not read it into the result (c_n = 0)."""
    check(dt, cfg, 8, coefficients(prediction_type, eta, None, eps_from_x0), with_noise=True)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("cfg", [True, False], ids=["guided", "plain"])
@pytest.mark.parametrize("eps_from_x0", [False, True], ids=["eps_model", "eps_clipped"])
@pytest.mark.parametrize("prediction_type", ["epsilon", "sample", "v_prediction"])
def test_clamp(backend, prediction_type, eps_from_x0, cfg, dt):
    """clip_sample with a range the reference really clamps at (a middle share of the elements, asserted on the reference
    alone in `check`): 8.0 under guidance 9, 1.0 without, at alpha_bar = 0.5041."""
    check(dt, cfg, 4, coefficients(prediction_type, 0.7, 8.0 if cfg else 1.0, eps_from_x0), with_noise=True)


def test_coefficients_of_the_scheduler_are_the_formula():
    """DDIMScheduler.coefficients feeds the kernel: at a real step it returns what `coefficients` above writes out."""
    for pt in ("epsilon", "sample", "v_prediction"):
        s = DDIMScheduler(prediction_type=pt, clip_sample=True, clip_sample_range=2.5)
        s.set_timesteps(10)
        t = int(s.timesteps[4])
        want = coefficients(pt, 0.7, 2.5, True, float(s.alphas_cumprod[t]), float(s.alphas_cumprod[t - 100]))
        got = s.coefficients(4, eta=0.7, use_clipped_model_output=True)
        assert set(got) == set(want)
        for key in want:
            assert got[key] == pytest.approx(want[key], rel=1e-12, abs=0), key


def test_missing_noise_is_refused_and_nothing_is_written(backend):
    tok, x, _ = operands(torch.float16, True, 8)
    xd = x.to(DEV)
    with pytest.raises(RuntimeError, match="noise"):
        ops.cfg_ddim_step_tokens(tok.to(DEV), xd, None, 9.0, coefficients("epsilon", 0.7, None, False), noise=None)
    assert torch.equal(xd.cpu(), x)


def test_operand_validation(backend):
    tok, x, noise = operands(torch.float16, False, 8)
    k = coefficients("epsilon", 0.7, None, False)
    tok, xd, nd = tok.to(DEV), x.to(DEV), noise.to(DEV)
    with pytest.raises(RuntimeError, match="noise"):
        ops.cfg_ddim_step_tokens(tok, xd, None, None, k, noise=nd[:1])
    with pytest.raises(RuntimeError, match="noise"):
        ops.cfg_ddim_step_tokens(tok, xd, None, None, k, noise=nd.double())
    with pytest.raises(RuntimeError, match="latents_lp"):
        ops.cfg_ddim_step_tokens(tok, xd, torch.empty_like(xd, dtype=torch.bfloat16), None, k, noise=nd)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.cfg_ddim_step_tokens(tok, xd.half(), None, None, k, noise=nd)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.cfg_ddim_step_tokens(tok, xd.transpose(3, 4), None, None, k, noise=nd)
    with pytest.raises(RuntimeError, match="rows"):
        ops.cfg_ddim_step_tokens(tok, xd, None, 9.0, k, noise=nd)        # guidance needs twice the token rows
    assert torch.equal(xd.cpu(), x)
