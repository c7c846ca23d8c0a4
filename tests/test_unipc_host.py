"""UniPC on the host: `schedulers.UniPCMultistepScheduler` (diffusers is not installed; the formulas are the published ones, Zhao et
al. 2023, "UniPC", in the data-prediction form with the B(h) choices bh1 / bh2) checked four ways: the order of accuracy of
`scalars` on an ODE with a closed-form solution, the predictor against the existing DPM-Solver++ class where the two coincide,
chained `step()` against a float64 restatement kept in this file (`RefUniPC`, written in the difference form D_k rather than
the folded linear one), and the fused product loops (session stand-in + aa_cfg_unipc_step_tokens on the emulator, single rank
and the guidance-parallel pair over gloo) against `_denoise_generic` and the oracle loop driving `RefUniPC`."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
from animate_anything_amd import ops
from animate_anything_amd.pipeline import LatentToVideoPipeline
from animate_anything_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler
from test_ddim_host import _SessionStubUNet, _StubUNet


# ---- (1) order of accuracy on an analytic ODE, through `scalars` ----
MU, SD, X_T = 0.7, 0.5, 1.3


def _alpha_sigma(t):
    abar = math.exp(-(0.1 * t + 9.95 * t * t))
    return math.sqrt(abar), math.sqrt(1.0 - abar)


def _eps(x, t):
    """The exact noise prediction for data ~ N(MU, SD^2): x_t ~ N(alpha MU, alpha^2 SD^2 + sigma^2)."""
    a, s = _alpha_sigma(t)
    return s * (x - a * MU) / (a * a * SD * SD + s * s)


def _exact(t):
    """The probability-flow ODE keeps the standardised coordinate: x_t = alpha MU + sqrt(v_t / v_1) (x_1 - alpha_1 MU)."""
    a, s = _alpha_sigma(t)
    a1, s1 = _alpha_sigma(1.0)
    return a * MU + math.sqrt((a * a * SD * SD + s * s) / (a1 * a1 * SD * SD + s1 * s1)) * (X_T - a1 * MU)


def _integrate(n, order, corrector, lower_order_final):
    ts = [1.0 - 0.9 * j / n for j in range(n + 1)]
    sig = [_alpha_sigma(t)[1] / _alpha_sigma(t)[0] for t in ts]
    x, last, hist, o_before = X_T, None, [0.0, 0.0, 0.0], 0
    for i in range(n):
        o = min(order, i + 1, n - i if lower_order_final else order)
        o_corr = o_before if corrector and i > 0 else 0
        k = UniPCMultistepScheduler.scalars(sig, i, o, o_corr, "bh2")
        m = k["a_x"] * x + k["a_m"] * _eps(x, ts[i])
        if o_corr:
            x = k["q_l"] * last + k["q_1"] * hist[0] + k["q_2"] * hist[1] + k["q_3"] * hist[2] + k["q_n"] * m
        last = x
        x = k["p_x"] * x + k["p_0"] * m + k["p_1"] * hist[0] + k["p_2"] * hist[1]
        hist, o_before = [m, hist[0], hist[1]], o
    return abs(x - _exact(0.1))


@pytest.mark.parametrize("order,corrector,lower_order_final,theory", [
    (1, False, False, 1), (1, True, False, 2), (3, False, False, 3), (3, True, False, 4), (2, True, False, 3), (2, True, True, 2)])
def test_order_of_accuracy(order, corrector, lower_order_final, theory):
    """Observed order between 80 and 160 uniform steps from t = 1 to t = 0.1 is at least theory - 0.5.  Measured on the CPU:
    1.00, 1.94, 3.07, 4.30, 2.73, 1.96.  (Order 2 without corrector is left out: it is superconvergent on this scalar problem.)"""
    e80, e160 = _integrate(80, order, corrector, lower_order_final), _integrate(160, order, corrector, lower_order_final)
    observed = math.log2(e80 / e160)
    print(f"order {order} corrector {corrector} lower_order_final {lower_order_final}: {e80:.3g} -> {e160:.3g}, observed {observed:.2f}")
    assert observed >= theory - 0.5


# ---- (2) the predictor against the existing DPM-Solver++ class ----
@pytest.mark.parametrize("steps", [6, 10, 14])
def test_predictor_is_dpm_solver_2m(steps):
    """Corrector disabled everywhere, order 2, bh2, fewer than 15 steps: x' = c_x x - c_d0 x0 - c_d1 (x0 - x0_prev)."""
    dpm = DPMSolverMultistepScheduler()
    uni = UniPCMultistepScheduler(solver_order=2, solver_type="bh2", disable_corrector=tuple(range(steps)),
                                  timestep_spacing=dpm.config.timestep_spacing, steps_offset=dpm.config.steps_offset)
    dpm.set_timesteps(steps)
    uni.set_timesteps(steps)
    assert uni.timesteps.tolist() == dpm.timesteps.tolist() and np.array_equal(uni.sigmas, dpm.sigmas)
    for i in range(steps):
        kd, ku = dpm.coefficients(i, have_prev=i > 0), uni.coefficients(i)
        assert not ku["corr_on"] and ku["p_2"] == 0.0
        assert ku["p_x"] == pytest.approx(kd["c_x"], rel=1e-12, abs=0)
        assert ku["p_0"] == pytest.approx(-(kd["c_d0"] + kd["c_d1"]), rel=1e-12, abs=0)
        assert ku["p_1"] == pytest.approx(kd["c_d1"], rel=1e-12, abs=0)
        assert ku["a_x"] == pytest.approx(1.0 / kd["alpha_s"], rel=1e-12) and ku["a_m"] == pytest.approx(-kd["sigma_s"] / kd["alpha_s"], rel=1e-12)


@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
def test_first_order_predictor_is_ddim(solver_type):
    """Order 1: x' = (sigma_t / sigma_s) x + (alpha_t - sigma_t alpha_s / sigma_s) m, whatever B(h)."""
    uni = UniPCMultistepScheduler(solver_order=1, solver_type=solver_type, disable_corrector=tuple(range(10)))
    uni.set_timesteps(10)
    for i in range(10):
        a_s, s_s = DPMSolverMultistepScheduler._alpha_sigma(uni.sigmas[i])
        a_t, s_t = DPMSolverMultistepScheduler._alpha_sigma(uni.sigmas[i + 1])
        k = uni.coefficients(i)
        assert k["p_x"] == pytest.approx(s_t / s_s, rel=1e-12, abs=0) and k["p_1"] == k["p_2"] == 0.0
        assert k["p_0"] == pytest.approx(a_t - s_t * a_s / s_s, rel=1e-12, abs=0)


# ---- (3) chained step() against a float64 restatement ----
class RefUniPC:
    """float64 UniPC in the difference form: `set_timesteps`, `timesteps`, `step(e, t, x) -> tensor` (what
    oracle.LatentToVideoPipeline drives)."""

    def __init__(self, solver_order=2, prediction_type="epsilon", solver_type="bh2", lower_order_final=True, disable_corrector=(),
                 timestep_spacing="linspace", steps_offset=0, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012):
        self.order, self.pred, self.kind, self.lof, self.off = solver_order, prediction_type, solver_type, lower_order_final, set(disable_corrector)
        self.N, self.spacing, self.offset = num_train_timesteps, timestep_spacing, steps_offset
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32).double() ** 2
        self.abar = torch.cumprod(1.0 - betas, 0)

    def set_timesteps(self, n, device=None):
        N = self.N
        if self.spacing == "linspace":
            ts = [int(v) for v in np.round(np.linspace(0, N - 1, n + 1))][::-1][:-1]
        elif self.spacing == "leading":
            ts = [int(round(i * (N // (n + 1)))) + self.offset for i in range(n + 1)][::-1][:-1]
        else:
            ts = [int(v) - 1 for v in np.round(np.arange(N, 0, -N / n))]
        ratio = ((1 - self.abar) / self.abar).sqrt()
        sig = [float(np.float32(ratio[t].item())) for t in ts] + [float(np.float32(ratio[0].item()))]
        self.alpha = [1.0 / math.sqrt(s * s + 1.0) for s in sig]
        self.sigma = [s * a for s, a in zip(sig, self.alpha)]
        self.lam = [math.log(a) - math.log(s) for a, s in zip(self.alpha, self.sigma)]
        self.n, self.timesteps, self._ts = n, torch.tensor(ts), ts
        self.m, self.last, self.lower, self.used = {}, None, 0, 0

    def _update(self, s0, target, x, order, m_new=None):
        """From index s0 to `target` with base prediction m[s0]; m_new: the corrector's extra difference (r = 1)."""
        h = self.lam[target] - self.lam[s0]
        hh = -h
        h_phi_1 = math.expm1(hh)
        B = h_phi_1 if self.kind == "bh2" else hh
        m0 = self.m[s0]
        rks, D = [], []
        for k in range(1, order):
            rks.append((self.lam[s0 - k] - self.lam[s0]) / h)
            D.append((self.m[s0 - k] - m0) / rks[-1])
        if m_new is not None:
            rks.append(1.0)
            D.append(m_new - m0)
        b, h_phi_k, fact = [], h_phi_1 / hh - 1.0, 1.0
        for j in range(1, len(rks) + 1):
            b.append(h_phi_k * fact / B)
            fact *= j + 1
            h_phi_k = h_phi_k / hh - 1.0 / fact
        if len(rks) == 1:
            rho = [0.5]
        elif rks:
            R = torch.tensor([[r ** j for r in rks] for j in range(len(rks))], dtype=torch.float64)
            rho = torch.linalg.solve(R, torch.tensor(b, dtype=torch.float64)).tolist()
        out = (self.sigma[target] / self.sigma[s0]) * x - self.alpha[target] * h_phi_1 * m0
        for r, d in zip(rho if rks else [], D):
            out = out - self.alpha[target] * B * r * d
        return out

    def step(self, e, t, x):
        i = self._ts.index(int(t))
        x, e = x.double(), e.double()
        if self.pred == "epsilon":
            m = (x - self.sigma[i] * e) / self.alpha[i]
        elif self.pred == "sample":
            m = e
        else:
            m = self.alpha[i] * x - self.sigma[i] * e
        if self.last is not None and (i - 1) not in self.off:
            x = self._update(i - 1, i, self.last, self.used, m_new=m)
        self.m[i], self.last = m, x
        o = min(self.order, self.n - i) if self.lof else self.order
        self.used = min(o, self.lower + 1)
        out = self._update(i, i + 1, x, self.used)
        self.lower = min(self.lower + 1, self.order)
        return out


@pytest.mark.parametrize("spacing", ["linspace", "leading", "trailing"])
@pytest.mark.parametrize("prediction_type", ["epsilon", "sample", "v_prediction"])
@pytest.mark.parametrize("lower_order_final", [True, False], ids=["lof", "nolof"])
@pytest.mark.parametrize("disable", [(), (1, 4)], ids=["corr_all", "corr_off_1_4"])
@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_chained_step_matches_the_restatement(order, solver_type, disable, lower_order_final, prediction_type, spacing):
    """7 chained steps on [3,4,8,8] randn inputs (the order-3 corrector reads three history entries from step 3 on) within
    1e-5 * max(1, max|ref|) of the float64 restatement: `step()` computes in fp32."""
    kw = dict(solver_order=order, solver_type=solver_type, disable_corrector=disable, lower_order_final=lower_order_final,
              prediction_type=prediction_type, timestep_spacing=spacing, steps_offset=1 if spacing == "leading" else 0)
    a, b = UniPCMultistepScheduler(**kw), RefUniPC(**kw)
    a.set_timesteps(7)
    b.set_timesteps(7)
    assert a.timesteps.tolist() == b.timesteps.tolist() and a.timesteps.dtype == torch.int64
    g = torch.Generator().manual_seed(0)
    xa = xb = torch.randn(3, 4, 8, 8, generator=g)
    worst = 0.0
    for i, t in enumerate(a.timesteps):
        e = torch.randn(3, 4, 8, 8, generator=g)
        want_pred, want_corr = a.orders(i)
        assert want_corr == (0 if i == 0 or (i - 1) in disable else b.used)
        xa, xb = a.step(e, t, xa).prev_sample, b.step(e, t, xb)
        assert want_pred == b.used and xa.dtype == torch.float32
        err, top = (xa.double() - xb).abs().max().item(), max(1.0, xb.abs().max().item())
        worst = max(worst, err / top)
        assert err <= 1e-5 * top, (i, err, top)
    print(f"worst distance over the chain {worst:.3g} of max(1, max|ref|)")


def test_a_run_that_starts_inside_the_schedule_builds_its_order_up_again():
    """DDPM_forward_timesteps hands the loop a tail of the schedule: the history is empty at its first step, so the orders
    come from the steps taken, not from the index."""
    kw = dict(solver_order=3, lower_order_final=True)
    a, b = UniPCMultistepScheduler(**kw), RefUniPC(**kw)
    a.set_timesteps(10)
    b.set_timesteps(10)
    assert [a.orders(i, i - 4) for i in range(4, 10)] == [(1, 0), (2, 1), (3, 2), (3, 3), (2, 3), (1, 2)]
    g = torch.Generator().manual_seed(1)
    xa = xb = torch.randn(2, 4, 5, 5, generator=g)
    for t in a.timesteps[4:]:
        e = torch.randn(2, 4, 5, 5, generator=g)
        xa, xb = a.step(e, t, xa).prev_sample, b.step(e, t, xb)
        assert (xa.double() - xb).abs().max().item() <= 1e-5 * max(1.0, xb.abs().max().item())


# ---- (5) config surface ----
def test_config_surface_and_refused_configurations():
    s = UniPCMultistepScheduler()
    assert s.order == 1 and s.init_noise_sigma == 1.0
    assert (s.config.solver_order, s.config.solver_type, s.config.timestep_spacing, s.config.steps_offset, s.config.predict_x0,
            s.config.lower_order_final, s.config.disable_corrector) == (2, "bh2", "linspace", 0, True, True, ())
    for bad in (dict(thresholding=True), dict(use_karras_sigmas=True), dict(predict_x0=False), dict(solver_p=object())):
        with pytest.raises(NotImplementedError):
            UniPCMultistepScheduler(**bad)
    for bad in (dict(solver_order=4), dict(solver_order=0), dict(prediction_type="flow"), dict(solver_type="bh3"),
                dict(timestep_spacing="karras")):
        with pytest.raises(ValueError):
            UniPCMultistepScheduler(**bad)
    with pytest.raises(NotImplementedError):
        UniPCMultistepScheduler(beta_schedule="squaredcos_cap_v2")
    for alias in ("midpoint", "heun", "logrho"):
        assert UniPCMultistepScheduler(solver_type=alias).config.solver_type == "bh2"
    with pytest.raises(ValueError, match="repeat"):
        UniPCMultistepScheduler().set_timesteps(1500)
    x = torch.randn(2, 4, 3, 3)
    assert s.scale_model_input(x, 5) is x
    s.set_timesteps(10)
    d = DPMSolverMultistepScheduler(timestep_spacing="linspace")
    d.set_timesteps(10)
    assert s.timesteps.tolist() == d.timesteps.tolist() and np.array_equal(s.sigmas, d.sigmas) and s.sigmas.dtype == np.float64
    assert len(s.sigmas) == 11 and s.sigmas[-1] == d.sigmas[-1]
    assert [s.index_for_timestep(t) for t in s.timesteps] == list(range(10))
    n, t = torch.randn(2, 4, 3, 3), s.timesteps[[2, 7]]
    assert torch.equal(s.add_noise(x, n, t), d.add_noise(x, n, t))
    out = s.step(n, s.timesteps[0], x)
    assert out.prev_sample.shape == x.shape and isinstance(s.step(n, s.timesteps[1], out.prev_sample, return_dict=False), tuple)


def test_from_config_of_a_dpm_and_of_a_ddim_scheduler():
    dpm = DPMSolverMultistepScheduler(beta_end=0.013, solver_order=2)
    u = UniPCMultistepScheduler.from_config(dpm.config)
    assert (u.config.beta_end, u.config.solver_order, u.config.solver_type, u.config.timestep_spacing, u.config.steps_offset,
            u.config.lower_order_final) == (0.013, 2, "bh2", "leading", 1, True)                       # midpoint -> bh2
    ddim = {"_class_name": "DDIMScheduler", "_diffusers_version": "0.24.0", "beta_start": 0.00085, "beta_end": 0.0125,
            "beta_schedule": "scaled_linear", "clip_sample": False, "set_alpha_to_one": False, "steps_offset": 1,
            "num_train_timesteps": 1000, "prediction_type": "v_prediction", "skip_prk_steps": True, "trained_betas": None}
    u = UniPCMultistepScheduler.from_config(ddim, solver_order=3)
    assert (u.config.beta_end, u.config.prediction_type, u.config.steps_offset, u.config.solver_order, u.config.timestep_spacing) == \
        (0.0125, "v_prediction", 1, 3, "linspace")
    u = UniPCMultistepScheduler.from_config(DDIMScheduler(timestep_spacing="trailing").config)
    assert u.config.timestep_spacing == "trailing"
    again = UniPCMultistepScheduler.from_config(u.config)
    assert vars(again.config) == vars(u.config)


def test_from_pretrained_scheduler_from_config(tmp_path):
    import json
    from types import SimpleNamespace
    (tmp_path / "scheduler").mkdir()
    cfg = {"_class_name": "UniPCMultistepScheduler", "_diffusers_version": "0.24.0", "beta_start": 0.00085, "beta_end": 0.0125,
           "beta_schedule": "scaled_linear", "solver_order": 3, "solver_type": "bh1", "disable_corrector": [0], "num_train_timesteps": 1000}
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(cfg))
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 2, 3, 4)))
    parts = dict(unet=object(), vae=vae, tokenizer=object(), text_encoder=object())
    named =LatentToVideoPipeline.from_pretrained(str(tmp_path), scheduler_from_config=True, **parts).scheduler
    assert type(named) is UniPCMultistepScheduler
    assert (named.config.beta_end, named.config.solver_order, named.config.solver_type, named.config.disable_corrector) == (0.0125, 3, "bh1", (0,))


def test_eval_validates_the_sampler_before_any_model_is_loaded(tmp_path):
    from animate_anything_amd import eval as aa_eval
    assert aa_eval.SAMPLERS["unipc"] is UniPCMultistepScheduler
    with pytest.raises(ValueError, match="sampler"):
        aa_eval.main_eval(str(tmp_path / "no_such_checkpoint"), {}, sampler="plms")
    with pytest.raises(ValueError, match="sampler"):
        aa_eval.batch_eval(None, None, None, None, {}, {}, str(tmp_path), False, sampler="plms")


# ---- (4) the denoising loops on the emulator ----
STEPS = 6
LOOP_CONFIGS = {"order2": dict(solver_order=2), "order3_bh1": dict(solver_order=3, solver_type="bh1", disable_corrector=(2,))}


def _loop_case(guidance, seed=2):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    lat, cond, mask = r(1, 4, 3, 4, 4), r(1, 4, 1, 4, 4), (r(1, 1, 1, 4, 4) > 0).float()
    pos, neg = r(1, 7, 16), r(1, 7, 16)
    return dict(latents=lat, prompt_embeds=pos.half(), negative_prompt_embeds=neg.half(), condition_latent=cond.half(), mask=mask.half(),
                motion=[3.0], num_inference_steps=STEPS, guidance_scale=guidance, return_dict=False)


def _oracle_loop(call, config):
    f = lambda v: v.float() if torch.is_tensor(v) else v
    return oracle.LatentToVideoPipeline(None, _StubUNet(torch.float32), RefUniPC(**config))(**{k: f(v) for k, v in call.items()})[1]


def _generic_loop(call, config):
    return LatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=UniPCMultistepScheduler(**config))(**call)[1]


@pytest.mark.parametrize("config", list(LOOP_CONFIGS))
@pytest.mark.parametrize("guidance", [9.0, 1.0])
def test_fused_denoise_loop_matches_the_generic_loop(emu, monkeypatch, guidance, config):
    """6 UniPC steps through `denoise`'s fused branch: one session run + one aa_cfg_unipc_step_tokens per step (counted), four
    fp32 buffers, the callback sees the latents of every step.  Against `_denoise_generic` and against the float64 oracle loop
    within 2e-2 * max|want| (the bound of test_ddim_host / test_pipeline_host for loops whose UNet computes in fp16)."""
    config = LOOP_CONFIGS[config]
    call = _loop_case(guidance)
    generic, want = _generic_loop(call, config), _oracle_loop(call, config)
    unet = _SessionStubUNet(torch.float16)
    pipe = LatentToVideoPipeline(vae=None, unet=unet, scheduler=UniPCMultistepScheduler(**config))
    launches, states, seen = [], [], []
    real, real_state = ops.cfg_unipc_step_tokens, pipe._unipc_state
    monkeypatch.setattr(ops, "cfg_unipc_step_tokens", lambda *a, **k: (launches.append(k.get("next_t_value")), real(*a, **k))[1])
    monkeypatch.setattr(pipe, "_unipc_state", lambda x: (states.append(real_state(x)), states[-1])[1])
    monkeypatch.setattr(pipe, "_denoise_generic", lambda *a, **k: pytest.fail("the fused loop was not selected"))
    frames, got = pipe(callback=lambda i, t, x: seen.append((i, int(t), x.clone())), **call)
    ts = pipe.scheduler.timesteps.tolist()
    assert frames is None and got.shape == want.shape
    assert unet.last_session.runs == STEPS and launches == [float(t) for t in ts[1:]] + [float(ts[-1])]
    assert len(states) == 1 and len(states[0]) == 4 and all(b.dtype == torch.float32 and b.shape == got.shape for b in states[0])
    assert [(i, t) for i, t, _ in seen] == list(enumerate(ts)) and torch.equal(seen[-1][2].to(got.dtype), got)
    for name, ref in (("generic", generic.double()), ("oracle", want)):
        err = (got.double() - ref).abs().max().item()
        print(f"fused loop vs {name}: distance {err:.3g}, bound {2e-2 * ref.abs().max().item():.3g}")
        assert err < 2e-2 * ref.abs().max().item()
    err = (generic.double() - want).abs().max().item()
    print(f"generic loop vs oracle: distance {err:.3g}")
    assert err < 2e-2 * want.abs().max().item()


def _pair_worker(rank, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      AA_EMU_THREADS="2")
    torch.set_num_threads(2)
    import build_emu
    from animate_anything_amd import _lib
    from animate_anything_amd import distributed as D
    r, w, _ = D.init("gloo")
    _, role, group = D.guidance_pair(r, w)
    unet = _SessionStubUNet(torch.float16)
    unet.conv_out = torch.nn.Conv2d(4, 4, 1)                    # (the pair loop sends conv_out.out_channels token columns)
    pipe = LatentToVideoPipeline(vae=None, unet=unet, scheduler=UniPCMultistepScheduler(**LOOP_CONFIGS["order3_bh1"]))
    pipe.guidance_group = (role, group)
    with _lib.use_library(_lib.bind(build_emu.build()), host_pointers=True):
        out = pipe(**_loop_case(9.0))[1]
    q.put((rank, role, unet.last_session.runs, out))
    dist.barrier()
    dist.destroy_process_group()


def test_guidance_parallel_loop_matches_the_generic_loop(emu):
    """The guidance-parallel loop (two gloo ranks, one half of the guidance batch each, one all-gather per step) takes the
    UniPC branch: both ranks end on the same latents, those of the single-rank fused loop, within the loops' bound of the
    generic loop."""
    config, call = LOOP_CONFIGS["order3_bh1"], _loop_case(9.0)
    generic = _generic_loop(call, config)
    single = LatentToVideoPipeline(vae=None, unet=_SessionStubUNet(torch.float16), scheduler=UniPCMultistepScheduler(**config))(**call)[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + ((os.getpid() + 271) % 500)
    procs = [ctx.Process(target=_pair_worker, args=(r, port, q)) for r in range(2)]
    [p.start() for p in procs]
    got = sorted((q.get(timeout=300) for _ in range(2)), key=lambda g: g[0])
    [p.join(60) for p in procs]
    assert [(g[0], g[1], g[2]) for g in got] == [(0, 0, STEPS), (1, 1, STEPS)]
    assert torch.equal(got[0][3], got[1][3])
    top = generic.abs().max().item()
    err_single, err = (got[0][3] - single).abs().max().item(), (got[0][3] - generic).abs().max().item()
    print(f"pair vs single-rank fused {err_single:.3g}, pair vs generic {err:.3g} (bound {2e-2 * top:.3g})")
    assert err_single <= 1e-6 * top and err < 2e-2 * top
