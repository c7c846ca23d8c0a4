"""What aa_cfg_dpm_step_tokens, aa_cfg_ddim_step_tokens and aa_cfg_unipc_step_tokens share (glue.h guided_token(): the token
addressing with frame 0 dropped, the [uncond clips | text clips] batch order, u + g*(t - u)) and their grid-stride loop, on the
emulator and on the GPU (the large shape too: the emulator takes a fraction of a second for it).

(1) With scalars that make each solver return its model output, the three kernels must hand back the same bits, and those
within the step tests' bound 1e-5 * max(1, max|ref|) of the float64 guided value from the rounded tokens.
(2) At 786,432 elements the launch (at most 2048 blocks of 256 threads = 524,288) takes a second trip through
`for (i ...; i += gridDim.x * 256)`; each kernel against its float64 formula with real scalars, same bound."""
import functools

import pytest
import torch

import test_ddim_step
import test_unipc_step
from animate_anything_amd import ops
from test_ddim_step import backend  # noqa: F401  (the emulator / GPU fixture; it sets test_ddim_step.DEV)

SMALL = (2, 4, 3, 2, 5)                          # clips, C, frames, h, w
LARGE = (3, 4, 16, 64, 64)                       # 786,432 elements > 2048 * 256 threads
GUIDANCE = 9.0

# scalars under which a solver's x' is its (guided) model output e
DDIM_IDENTITY = dict(a_x=0.0, a_m=1.0, e_x=0.0, e_m=0.0, q_x=0.0, q_0=0.0, clip=None, eps_from_x0=False, c_0=1.0, c_e=0.0, c_n=0.0)
UNIPC_IDENTITY = dict(a_x=0.0, a_m=1.0, corr_on=False, q_l=0.0, q_1=0.0, q_2=0.0, q_3=0.0, q_n=0.0, p_x=0.0, p_0=1.0, p_1=0.0, p_2=0.0)
DPM_IDENTITY = dict(sigma_s=-1.0, alpha_s=1.0, c_x=0.0, c_d0=-1.0, c_d1=0.0)        # with latents of zeros
DPM_REAL = dict(sigma_s=0.7, alpha_s=0.71, c_x=0.9, c_d0=-0.2, c_d1=-0.05)          # (tests/test_kernels.py::test_cfg_dpm_step_tokens)


def dev():
    return test_ddim_step.DEV


def put(t):
    """A copy on the backend's device (on the emulator `.to("cpu")` alone would hand the kernel the reference's own tensor)."""
    return t.clone().to(dev())


@functools.lru_cache(maxsize=None)
def case(shape, dt, cfg, ld, seed=181):
    """(tokens, five fp32 tensors in the latents' shape, float64 guided model output from the rounded tokens); read-only."""
    clips, c, frames, h, w = shape
    g = torch.Generator().manual_seed(seed)
    b = 2 * clips if cfg else clips
    tok = torch.randn(b * (frames + 1) * h * w, ld, generator=g).to(dt)
    state = [torch.randn(*shape, generator=g) for _ in range(5)]
    e = tok.double().reshape(b, frames + 1, h, w, ld).permute(0, 4, 1, 2, 3)[:, :c, 1:]
    if cfg:
        e = e[:clips] + GUIDANCE * (e[clips:] - e[:clips])
    return tok, state, e.contiguous()


def dpm_reference(x, x0p, e, k):
    x0 = (x.double() - k["sigma_s"] * e) / k["alpha_s"]
    return k["c_x"] * x.double() - k["c_d0"] * x0 - k["c_d1"] * (x0 - x0p.double()), x0


def close(name, got, ref):
    err, bound = (got.double().cpu() - ref).abs().max().item(), 1e-5 * max(1.0, ref.abs().max().item())
    print(f"{name}: err {err:.3g} (bound {bound:.3g})")
    assert err <= bound, name


@pytest.mark.parametrize("cfg", [True, False], ids=["guided", "plain"])
def test_dpm_identity_scalars_give_the_guided_value_in_float64(cfg):
    """CPU check of the case below: with DPM_IDENTITY and latents of zeros the DPM form is the guided value exactly."""
    _, state, e = case(SMALL, torch.float16, cfg, 8)
    nx, x0 = dpm_reference(torch.zeros(SMALL), state[1], e, DPM_IDENTITY)
    assert torch.equal(nx, e) and torch.equal(x0, e)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("cfg", [True, False], ids=["guided", "plain"])
@pytest.mark.parametrize("ld", [4, 8])
def test_the_three_samplers_read_the_same_value(backend, ld, cfg, dt):
    tok, state, e = case(SMALL, dt, cfg, ld)
    guidance = GUIDANCE if cfg else None
    tokd = tok.to(dev())
    x_ddim, x_unipc, x_dpm = put(state[0]), put(state[0]), torch.zeros(SMALL, device=dev())
    ops.cfg_ddim_step_tokens(tokd, x_ddim, None, guidance, DDIM_IDENTITY)
    ops.cfg_unipc_step_tokens(tokd, x_unipc, None, guidance, UNIPC_IDENTITY, put(state[1]), (None, None, None))
    ops.cfg_dpm_step_tokens(tokd, x_dpm, put(state[1]), None, guidance, DPM_IDENTITY)
    assert torch.equal(x_ddim.cpu(), x_unipc.cpu()) and torch.equal(x_ddim.cpu(), x_dpm.cpu())
    close("guided value", x_ddim, e)


# ---- the second trip of the grid-stride loop ----
def large_operands():
    tok, state, e = case(LARGE, torch.float16, True, 8)
    return tok.to(dev()), [put(s) for s in state], state, e, torch.zeros(2 * LARGE[0], device=dev())


def test_grid_stride_wrap_dpm(backend):
    tok, (x, x0p, *_), state, e, nt = large_operands()
    ops.cfg_dpm_step_tokens(tok, x, x0p, None, GUIDANCE, DPM_REAL, next_t=nt, next_t_value=301.0)
    want, want_x0 = dpm_reference(state[0], state[1], e, DPM_REAL)
    close("x'", x, want)
    close("x0", x0p, want_x0)
    assert torch.equal(nt.cpu(), torch.full((2 * LARGE[0],), 301.0))


def test_grid_stride_wrap_ddim(backend):
    """eta = 0.7: the noise operand is read past the first trip too."""
    tok, (x, noise, *_), state, e, nt = large_operands()
    k = test_ddim_step.coefficients("epsilon", 0.7, None, False)
    ops.cfg_ddim_step_tokens(tok, x, None, GUIDANCE, k, noise=noise, next_t=nt, next_t_value=301.0)
    x0 = k["a_x"] * state[0].double() + k["a_m"] * e
    close("x'", x, k["c_0"] * x0 + k["c_e"] * (k["e_x"] * state[0].double() + k["e_m"] * e) + k["c_n"] * state[1].double())
    assert torch.equal(nt.cpu(), torch.full((2 * LARGE[0],), 301.0))


def test_grid_stride_wrap_unipc(backend):
    """Step 4 of the 6-step order-3 schedule of tests/test_unipc_step.py: corrector order 3, every buffer read and written.
    (|ref| <= the sum of |coefficient * operand| behind it, so this bound is no wider than that file's 1e-5 * max(1, max S).)"""
    tok, (x, last, h1, h2, h3), state, e, nt = large_operands()
    k = test_unipc_step.scalars(4)
    assert k["corr_on"] and k["q_3"] != 0.0
    ops.cfg_unipc_step_tokens(tok, x, None, GUIDANCE, k, last, (h1, h2, h3), next_t=nt, next_t_value=301.0)
    x0, l0, m1, m2, m3 = (s.double() for s in state)
    m = k["a_x"] * x0 + k["a_m"] * e
    xh = k["q_l"] * l0 + k["q_1"] * m1 + k["q_2"] * m2 + k["q_3"] * m3 + k["q_n"] * m
    close("x'", x, k["p_x"] * xh + k["p_0"] * m + k["p_1"] * m1 + k["p_2"] * m2)
    close("xhat", last, xh)
    close("m", h3, m)
    assert torch.equal(h1.cpu(), state[2]) and torch.equal(h2.cpu(), state[3])
    assert torch.equal(nt.cpu(), torch.full((2 * LARGE[0],), 301.0))
