"""aa_cfg_unipc_step_tokens (guidance + the corrector of the step before + the UniPC predictor, from the UNet's token layout) against
the float64 formula evaluated from the same rounded operands, on the emulator and on the GPU.  The scalars are those of real
steps of a 6-step order-3 schedule: step 0 (no corrector, predictor order 1), 1 (corrector 1, predictor 2), 2 (corrector 2,
predictor 3), 4 (corrector 3, predictor lowered to 2) and 5 (corrector 2, the final predictor lowered to 1).

Bound: the kernel spends at most 14 fp32 operations on an element (guidance 2, m 2, xhat 5, x' 4, one to spare), each within 2^-24 of its
result, and every intermediate is bounded by S = sum |coefficient * operand| expanded down to the inputs; 14 * 2^-24 = 8.3e-7,
the fp32 rounding of the ten scalars adds as much again, so 1e-5 * max(1, max S) holds with room and without a measurement."""
import pytest
import torch

import test_ddim_step
from animate_anything_amd import ops
from animate_anything_amd.schedulers import UniPCMultistepScheduler
from test_ddim_step import backend  # noqa: F401  (the emulator / GPU fixture; it sets test_ddim_step.DEV)

CLIPS, C, FRAMES, H, W = 2, 4, 3, 2, 5
SHAPE = (CLIPS, C, FRAMES, H, W)
STEP_ORDERS = {0: (1, 0), 1: (2, 1), 2: (3, 2), 4: (2, 3), 5: (1, 2)}        # step -> (predictor order, corrector order)


def dev():
    return test_ddim_step.DEV


def put(t):
    """A copy on the backend's device (on the emulator `.to("cpu")` alone would hand the kernel the reference's own tensor)."""
    return t.clone().to(dev())


def scalars(step, prediction_type="epsilon", solver_type="bh2"):
    s = UniPCMultistepScheduler(solver_order=3, prediction_type=prediction_type, solver_type=solver_type)
    s.set_timesteps(6)
    assert s.orders(step) == STEP_ORDERS[step]
    return s.coefficients(step)


def operands(dt, cfg, ld, seed=171):
    g = torch.Generator().manual_seed(seed)
    b = 2 * CLIPS if cfg else CLIPS
    tok = torch.randn(b * (FRAMES + 1) * H * W, ld, generator=g).to(dt)
    x, last, h1, h2, h3 = (torch.randn(*SHAPE, generator=g) for _ in range(5))
    return tok, x, last, [h1, h2, h3]


def reference(tok, x, last, hist, guidance, k):
    """float64 from the rounded tokens: (x', xhat, m, S) with S the elementwise sum of |coefficient * operand| behind x'."""
    b = tok.shape[0] // ((FRAMES + 1) * H * W)
    e = tok.double().reshape(b, FRAMES + 1, H, W, -1).permute(0, 4, 1, 2, 3)[:, :C, 1:]
    e_abs = e.abs()
    if guidance is not None:
        e_abs = e[:CLIPS].abs() + abs(guidance) * (e[CLIPS:].abs() + e[:CLIPS].abs())
        e = e[:CLIPS] + guidance * (e[CLIPS:] - e[:CLIPS])
    x, last, (h1, h2, h3) = x.double(), last.double(), [h.double() for h in hist]
    m = k["a_x"] * x + k["a_m"] * e
    m_abs = abs(k["a_x"]) * x.abs() + abs(k["a_m"]) * e_abs
    xh, xh_abs = x, x.abs()
    if k["corr_on"]:
        xh = k["q_l"] * last + k["q_1"] * h1 + k["q_2"] * h2 + k["q_3"] * h3 + k["q_n"] * m
        xh_abs = abs(k["q_l"]) * last.abs() + abs(k["q_1"]) * h1.abs() + abs(k["q_2"]) * h2.abs() + abs(k["q_3"]) * h3.abs() + abs(k["q_n"]) * m_abs
    out = k["p_x"] * xh + k["p_0"] * m + k["p_1"] * h1 + k["p_2"] * h2
    s = abs(k["p_x"]) * xh_abs + abs(k["p_0"]) * m_abs + abs(k["p_1"]) * h1.abs() + abs(k["p_2"]) * h2.abs()
    return out, xh, m, torch.maximum(s, torch.maximum(xh_abs, m_abs))


def check(dt, cfg, ld, k):
    tok, x, last, hist = operands(dt, cfg, ld)
    guidance = 9.0 if cfg else None
    want, want_hat, want_m, s = reference(tok, x, last, hist, guidance, k)
    b = 2 * CLIPS if cfg else CLIPS
    d = dev()
    xd, ld_, hd = put(x), put(last), [put(h) for h in hist]
    lp = torch.empty(*SHAPE, dtype=dt, device=d)
    nt = torch.zeros(b, dtype=torch.float32, device=d)
    rotated = ops.cfg_unipc_step_tokens(tok.to(d), xd, lp, guidance, k, ld_, hd, next_t=nt, next_t_value=913.0)
    bound = 1e-5 * max(1.0, s.max().item())
    for name, got, ref in (("x'", xd, want), ("xhat", ld_, want_hat), ("m", hd[2], want_m)):
        err = (got.double().cpu() - ref).abs().max().item()
        print(f"{name}: err {err:.3g} (bound {bound:.3g})")
        assert err <= bound, name
    # the history rotation: m went into the oldest buffer, the other two are bit-equal, and the caller gets (m, h1, h2) back
    assert torch.equal(hd[0].cpu(), hist[0]) and torch.equal(hd[1].cpu(), hist[1])
    assert [r.data_ptr() for r in rotated] == [hd[2].data_ptr(), hd[0].data_ptr(), hd[1].data_ptr()]
    if dt == torch.float16:                       # (the 16-bit copy at the tolerances of test_ddim_step.check)
        assert (lp.double().cpu() - xd.double().cpu()).abs().max().item() <= 2e-3 * max(1.0, xd.abs().max().item())
    else:
        assert torch.equal(lp.cpu(), xd.cpu().to(dt))
    assert torch.equal(nt.cpu(), torch.full((b,), 913.0))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("cfg", [True, False], ids=["guided", "plain"])
@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("step", list(STEP_ORDERS))
def test_steps_of_an_order_3_schedule(backend, step, ld, cfg, dt):
    check(dt, cfg, ld, scalars(step))


@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
@pytest.mark.parametrize("prediction_type", ["sample", "v_prediction"])
def test_prediction_types_and_b_choices(backend, prediction_type, solver_type):
    check(torch.float16, True, 8, scalars(4, prediction_type, solver_type))


def test_history_buffers_may_be_missing_where_their_coefficients_are_zero(backend):
    """Step 0 reads no history: with (h1, None, None) m goes into h1, with no history buffer at all it is not stored."""
    tok, x, last, hist = operands(torch.float16, True, 8)
    k = scalars(0)
    want, want_hat, want_m, s = reference(tok, x, last, hist, 9.0, k)
    bound = 1e-5 * max(1.0, s.max().item())
    d = dev()
    xd, ld_, h1 = put(x), put(last), put(hist[0])
    rotated = ops.cfg_unipc_step_tokens(tok.to(d), xd, None, 9.0, k, ld_, (h1, None, None))
    assert rotated[0] is h1 and rotated[1:] == (None, None)
    assert (xd.double().cpu() - want).abs().max().item() <= bound and (h1.double().cpu() - want_m).abs().max().item() <= bound
    assert torch.equal(ld_.cpu(), x)                                   # no corrector: xhat is the sample as handed in
    xd = put(x)
    assert ops.cfg_unipc_step_tokens(tok.to(d), xd, None, 9.0, k, ld_, (None, None, None)) == (None, None, None)
    assert (xd.double().cpu() - want).abs().max().item() <= bound


def test_operand_validation_leaves_every_buffer_untouched(backend):
    tok, x, last, hist = operands(torch.float16, False, 8)
    k = scalars(4)                                                     # corrector order 3: every coefficient but p_2 is non-zero
    assert all(k[name] != 0.0 for name in ("q_l", "q_1", "q_2", "q_3", "q_n", "p_x", "p_0", "p_1")) and k["p_2"] == 0.0
    d = dev()
    tok, xd, ld_, hd = tok.to(d), put(x), put(last), [put(h) for h in hist]
    call = lambda **kw: ops.cfg_unipc_step_tokens(kw.get("tok", tok), kw.get("x", xd), kw.get("lp"), kw.get("g"), kw.get("k", k),
                                                  kw.get("last", ld_), kw.get("hist", hd))
    # the entry point: a non-zero coefficient with a null buffer, overlapping buffers
    for missing in ((None, hd[1], hd[2]), (hd[0], None, hd[2]), (hd[0], hd[1], None)):
        with pytest.raises(RuntimeError, match="history"):
            call(hist=missing)
    with pytest.raises(RuntimeError, match="history"):
        call(k=scalars(2), hist=(hd[0], None, hd[2]))                  # predictor order 3: p_2 needs hist2 (q_2 too)
    for aliased in (dict(hist=(hd[0], hd[0], hd[2])), dict(hist=(hd[0], hd[1], ld_)), dict(last=xd), dict(hist=(xd, hd[1], hd[2]))):
        with pytest.raises(RuntimeError, match="overlap"):
            call(**aliased)
    n = xd.numel()
    big = torch.zeros(2 * n - 8, device=d)
    with pytest.raises(RuntimeError, match="overlap"):                 # two views of one allocation that share 8 elements
        call(hist=(hd[0], big[:n].view(SHAPE), big[n - 8:].view(SHAPE)))
    # the wrapper: dtypes, shapes, layout, token rows
    with pytest.raises(RuntimeError, match="three"):
        call(hist=hd[:2])
    with pytest.raises(RuntimeError, match="last_sample"):
        call(last=None)
    with pytest.raises(RuntimeError, match="last_sample"):
        call(last=ld_[:1])
    with pytest.raises(RuntimeError, match="history"):
        call(hist=(hd[0], hd[1].double(), hd[2]))
    with pytest.raises(RuntimeError, match="latents_lp"):
        call(lp=torch.empty_like(xd, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="fp32"):
        call(x=xd.half())
    with pytest.raises(RuntimeError, match="contiguous"):
        call(x=xd.transpose(3, 4))
    with pytest.raises(RuntimeError, match="rows"):
        call(g=9.0)                                                    # guidance needs twice the token rows
    assert torch.equal(xd.cpu(), x) and torch.equal(ld_.cpu(), last) and torch.equal(big.cpu(), torch.zeros(2 * n - 8))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(hd, hist))
