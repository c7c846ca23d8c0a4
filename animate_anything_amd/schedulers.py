"""Host-side samplers for the denoising loop.

`DPMSolverMultistepScheduler` mirrors the diffusers==0.24.0 scheduler the reference installs at
/root/reference/train.py:806-808 (`DPMSolverMultistepScheduler.from_config(pipeline.scheduler.config)`:
dpmsolver++, order 2, midpoint, epsilon prediction, lower_order_final) and
`DDPMScheduler.add_noise` as used by /root/reference/utils/common.py:32-48.

The schedule (timesteps, sigmas) and the per-step scalar coefficients are host float64 math; the
tensor update itself is either the torch expression of `step()` (API parity with diffusers) or the
fused HIP kernel `aa_cfg_dpm_step` fed by `coefficients()` (what the pipeline uses).

`DDIMScheduler` is the scheduler the checkpoints themselves ship and the reference's app samples with; same split
(host float64 scalars, torch `step()` or the fused kernel `aa_cfg_ddim_step_tokens`).

`UniPCMultistepScheduler` is the sampler for 8-12 steps: DPM-Solver++'s multistep predictor plus a corrector that costs no
extra UNet call; same split, fused kernel `aa_cfg_unipc_step_tokens`.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch


class SchedulerOutput(SimpleNamespace):
    pass


def _betas(num_train_timesteps, beta_start, beta_end, beta_schedule):
    if beta_schedule == "scaled_linear":
        return np.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=np.float32).astype(np.float64) ** 2
    if beta_schedule == "linear":
        return np.linspace(beta_start, beta_end, num_train_timesteps, dtype=np.float32).astype(np.float64)
    raise NotImplementedError(f"{beta_schedule} is not implemented")


def _alphas_cumprod(num_train_timesteps, beta_start, beta_end, beta_schedule):
    return np.cumprod(1.0 - _betas(num_train_timesteps, beta_start, beta_end, beta_schedule))


class _Scheduler:
    """What the samplers below share: `from_config`, the identity `scale_model_input`, the timestep lookup over `self._ts` and the
    sigma schedule of the multistep solvers."""
    order = 1

    @classmethod
    def from_config(cls, config, **overrides):
        cfg = dict(vars(config)) if isinstance(config, SimpleNamespace) else dict(config)
        cfg.update(overrides)
        return cls(**{k: v for k, v in cfg.items() if not k.startswith("_")})

    def scale_model_input(self, sample, timestep=None):
        return sample

    def index_for_timestep(self, timestep):
        return self._ts.index(int(timestep))

    def _set_sigma_schedule(self, ts, device):
        """The tail of `set_timesteps` of DPM-Solver++ and UniPC: `sigmas` (sigma/alpha form, rounded to float32 like diffusers)
        at the timesteps `ts` plus the final one, `timesteps` and the lookup list from `self._acp`."""
        sig = ((1 - self._acp) / self._acp) ** 0.5
        sigmas = np.concatenate([np.interp(ts, np.arange(len(sig)), sig), [sig[0]]]).astype(np.float32)
        self.sigmas = sigmas.astype(np.float64)
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)
        self._ts = [int(t) for t in ts]


class DDPMScheduler:
    """Only what the eval path needs: the forward-noising `add_noise`."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", **_):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start,
                                      beta_end=beta_end, beta_schedule=beta_schedule)
        self.alphas_cumprod = torch.from_numpy(_alphas_cumprod(num_train_timesteps, beta_start, beta_end, beta_schedule))

    def add_noise(self, original_samples, noise, timesteps):
        acp = self.alphas_cumprod.to(original_samples.device)[torch.as_tensor(timesteps).to(original_samples.device).long()]
        shape = (-1,) + (1,) * (original_samples.dim() - 1)
        a = acp.sqrt().reshape(shape).to(original_samples.dtype)
        s = (1 - acp).sqrt().reshape(shape).to(original_samples.dtype)
        return a * original_samples + s * noise


class DPMSolverMultistepScheduler(_Scheduler):
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 solver_order=2, prediction_type="epsilon", algorithm_type="dpmsolver++", solver_type="midpoint",
                 lower_order_final=True, timestep_spacing="leading", steps_offset=1, **_):
        if prediction_type != "epsilon" or algorithm_type != "dpmsolver++" or solver_type != "midpoint" or solver_order > 2:
            raise NotImplementedError("only epsilon / dpmsolver++ / midpoint / order<=2 (the reference's configuration)")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, solver_order=solver_order,
                                      prediction_type=prediction_type, algorithm_type=algorithm_type,
                                      solver_type=solver_type, lower_order_final=lower_order_final,
                                      timestep_spacing=timestep_spacing, steps_offset=steps_offset)
        self._acp = _alphas_cumprod(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.alphas_cumprod = torch.from_numpy(self._acp)
        self.init_noise_sigma = 1.0
        self.timesteps = None
        self.sigmas = None

    def set_timesteps(self, num_inference_steps, device=None):
        c, N = self.config, self.config.num_train_timesteps
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, N - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, num_inference_steps + 1) * (N // (num_inference_steps + 1))).round()[::-1][:-1].copy().astype(np.int64)
            ts = ts + c.steps_offset
        else:
            raise NotImplementedError(c.timestep_spacing)
        self._set_sigma_schedule(ts, device)
        self.num_inference_steps = num_inference_steps
        self.model_outputs = [None] * c.solver_order
        self.lower_order_nums = 0
        self._step_index = None

    @staticmethod
    def _alpha_sigma(sigma):
        alpha = 1.0 / math.sqrt(sigma * sigma + 1.0)
        return alpha, sigma * alpha

    def add_noise(self, original_samples, noise, timesteps):
        idx = [self._ts.index(int(t)) for t in timesteps]
        a = torch.tensor([self._alpha_sigma(self.sigmas[i])[0] for i in idx], dtype=torch.float32)
        s = torch.tensor([self._alpha_sigma(self.sigmas[i])[1] for i in idx], dtype=torch.float32)
        shape = (-1,) + (1,) * (original_samples.dim() - 1)
        a = a.reshape(shape).to(original_samples.device, original_samples.dtype)
        s = s.reshape(shape).to(original_samples.device, original_samples.dtype)
        return a * original_samples + s * noise

    # ---- scalar part of one step (shared by `step` and the fused kernel) -------------------------
    def coefficients(self, step_index: int, have_prev: bool):
        """x' = c_x*x - c_d0*x0 - c_d1*(x0 - x0_prev) with x0 = (x - sigma_s*eps)/alpha_s.
        Returns dict(sigma_s, alpha_s, c_x, c_d0, c_d1, second_order)."""
        n = len(self._ts)
        final_low = (step_index == n - 1) and self.config.lower_order_final and n < 15
        a_s, s_s = self._alpha_sigma(self.sigmas[step_index])
        a_t, s_t = self._alpha_sigma(self.sigmas[step_index + 1])
        lam_s, lam_t = math.log(a_s) - math.log(s_s), math.log(a_t) - math.log(s_t)
        h = lam_t - lam_s
        coef = a_t * (math.exp(-h) - 1.0)
        first = self.config.solver_order == 1 or not have_prev or final_low
        c_d1 = 0.0
        if not first:
            a_p, s_p = self._alpha_sigma(self.sigmas[step_index - 1])
            r0 = (lam_s - (math.log(a_p) - math.log(s_p))) / h
            c_d1 = 0.5 * coef / r0
        return dict(sigma_s=s_s, alpha_s=a_s, c_x=s_t / s_s, c_d0=coef, c_d1=c_d1, second_order=not first)

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        """diffusers-compatible tensor update (torch ops)."""
        if self._step_index is None:
            self._step_index = self.index_for_timestep(timestep)
        i = self._step_index
        k = self.coefficients(i, have_prev=self.lower_order_nums >= 1)
        x0 = (sample.float() - k["sigma_s"] * model_output.float()) / k["alpha_s"]
        prev = k["c_x"] * sample.float() - k["c_d0"] * x0
        if k["second_order"]:
            prev = prev - k["c_d1"] * (x0 - self.model_outputs[-1])
        self.model_outputs = self.model_outputs[1:] + [x0]
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1
        prev = prev.to(sample.dtype)
        return SchedulerOutput(prev_sample=prev) if return_dict else (prev,)


class DDIMScheduler(_Scheduler):
    """diffusers==0.24.0 DDIMScheduler, restated from memory like the rest of this file (diffusers is not a dependency): the
    scheduler the checkpoints of this model family carry in `scheduler/scheduler_config.json` and the one the reference's app
    samples with (reference app.py:64-113, start latents from utils/common.py:22-30 which reads `scheduler.alphas`).

    Schedule and per-step scalars are host float64 math; the tensor update is either the torch expression of `step()` (fp32,
    API parity with diffusers) or the fused HIP kernel `aa_cfg_ddim_step_tokens` fed by `coefficients()`.  Dynamic
    thresholding and zero-SNR beta rescaling are not implemented.  The argument defaults are the values those checkpoints
    ship (scaled_linear 0.00085-0.012, no clipping, set_alpha_to_one=False, steps_offset=1), like the sibling classes, not
    diffusers' own; a `scheduler_config.json` written by diffusers names every key, so `from_config` is unaffected."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 clip_sample=False, set_alpha_to_one=False, steps_offset=1, prediction_type="epsilon", thresholding=False,
                 clip_sample_range=1.0, timestep_spacing="leading", rescale_betas_zero_snr=False, **_):
        if thresholding or rescale_betas_zero_snr:
            raise NotImplementedError("DDIMScheduler: thresholding / rescale_betas_zero_snr are not implemented")
        if prediction_type not in ("epsilon", "v_prediction", "sample"):
            raise ValueError(f"prediction_type {prediction_type!r}: epsilon, v_prediction or sample")
        if timestep_spacing not in ("leading", "trailing", "linspace"):
            raise ValueError(f"timestep_spacing {timestep_spacing!r}: leading, trailing or linspace")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, clip_sample=clip_sample, set_alpha_to_one=set_alpha_to_one,
                                      steps_offset=steps_offset, prediction_type=prediction_type, thresholding=thresholding,
                                      clip_sample_range=clip_sample_range, timestep_spacing=timestep_spacing,
                                      rescale_betas_zero_snr=rescale_betas_zero_snr)
        betas = _betas(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self._acp = np.cumprod(1.0 - betas)
        self.betas = torch.from_numpy(betas)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.from_numpy(self._acp)
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else float(self._acp[0])
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self._ts = [int(t) for t in self.timesteps]

    def set_timesteps(self, num_inference_steps, device=None):
        c, N, n = self.config, self.config.num_train_timesteps, int(num_inference_steps)
        if not 0 < n <= N:
            raise ValueError(f"num_inference_steps = {num_inference_steps} must lie in [1, {N}]")
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, N - 1, n).round()[::-1].copy().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (N // n)).round()[::-1].copy().astype(np.int64) + c.steps_offset
        else:
            ts = np.round(np.arange(N, 0, -N / n)).astype(np.int64) - 1
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)
        self._ts = [int(t) for t in ts]
        self.num_inference_steps = n

    add_noise = DDPMScheduler.add_noise

    # ---- scalar part of one step (shared by `step` and the fused kernel) -------------------------
    def _coefficients_at(self, t: int, eta: float, use_clipped_model_output: bool):
        c, N = self.config, self.config.num_train_timesteps
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() before stepping")
        t_prev = t - N // self.num_inference_steps
        a_t = float(self._acp[t])
        a_prev = float(self._acp[t_prev]) if t_prev >= 0 else self.final_alpha_cumprod
        b_t = 1.0 - a_t
        sa, sb = math.sqrt(a_t), math.sqrt(b_t)
        if c.prediction_type == "epsilon":
            a_x, a_m, e_x, e_m = 1.0 / sa, -sb / sa, 0.0, 1.0
        elif c.prediction_type == "sample":
            a_x, a_m, e_x, e_m = 0.0, 1.0, 1.0 / sb, -sa / sb
        else:
            a_x, a_m, e_x, e_m = sa, -sb, sb, sa
        sigma = float(eta) * math.sqrt((1.0 - a_prev) / (1.0 - a_t) * (1.0 - a_t / a_prev))
        return dict(a_x=a_x, a_m=a_m, e_x=e_x, e_m=e_m, q_x=1.0 / sb, q_0=-sa / sb,
                    clip=float(c.clip_sample_range) if c.clip_sample else None, eps_from_x0=bool(use_clipped_model_output),
                    c_0=math.sqrt(a_prev), c_e=math.sqrt(1.0 - a_prev - sigma * sigma), c_n=sigma)

    def coefficients(self, step_index: int, eta: float = 0.0, use_clipped_model_output: bool = False):
        """x0 = a_x*x + a_m*m (clamped to +-clip unless clip is None);  eps = e_x*x + e_m*m, or q_x*x + q_0*x0 when eps_from_x0;
        x' = c_0*x0 + c_e*eps + c_n*noise.  Returns dict(a_x, a_m, e_x, e_m, q_x, q_0, clip, eps_from_x0, c_0, c_e, c_n)."""
        return self._coefficients_at(self._ts[step_index], eta, use_clipped_model_output)

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None,
             variance_noise=None, return_dict=True):
        """diffusers-compatible tensor update (torch ops, fp32 arithmetic)."""
        k = self._coefficients_at(int(timestep), eta, use_clipped_model_output)
        x, m = sample.float(), model_output.float()
        x0 = k["a_x"] * x + k["a_m"] * m
        if k["clip"] is not None:
            x0 = x0.clamp(-k["clip"], k["clip"])
        eps = k["q_x"] * x + k["q_0"] * x0 if k["eps_from_x0"] else k["e_x"] * x + k["e_m"] * m
        prev = k["c_0"] * x0 + k["c_e"] * eps
        if eta > 0:                                         # (diffusers draws whenever eta > 0, also where sigma_t comes out 0)
            if variance_noise is not None and generator is not None:
                raise ValueError("pass either `generator` or `variance_noise`, not both")
            if variance_noise is None:
                variance_noise = torch.randn(model_output.shape, generator=generator, device=model_output.device, dtype=torch.float32)
            prev = prev + k["c_n"] * variance_noise.float()
        prev, x0 = prev.to(sample.dtype), x0.to(sample.dtype)
        return SchedulerOutput(prev_sample=prev, pred_original_sample=x0) if return_dict else (prev,)


class UniPCMultistepScheduler(_Scheduler):
    """diffusers==0.24.0 UniPCMultistepScheduler (Zhao et al. 2023, "UniPC: a unified predictor-corrector framework"), restated
    like the rest of this file (diffusers is not a dependency): a multistep predictor of order `solver_order` in the
    data-prediction form plus a corrector that re-uses the model output of the NEXT step to raise the order by one - no
    extra UNet call.  With the corrector off, order 2 and bh2 it is DPM-Solver++(2M).

    Notation: s_j = sigmas[j] (sigma/alpha form), alpha_j = 1/sqrt(s_j^2+1), sigma_j = s_j*alpha_j, lambda_j = ln alpha_j -
    ln sigma_j; step i is at timesteps[i] and its target is index i+1.  Both updates are linear in their operands, so the
    schedule-dependent part is host float64 math (`scalars`, `coefficients`); the tensor update is either the torch
    expression of `step()` (fp32) or the fused HIP kernel `aa_cfg_unipc_step_tokens`.  Dynamic thresholding, Karras sigmas,
    the noise-prediction form (`predict_x0=False`) and `solver_p` are not implemented."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 solver_order=2, prediction_type="epsilon", thresholding=False, predict_x0=True, solver_type="bh2",
                 lower_order_final=True, disable_corrector=(), solver_p=None, use_karras_sigmas=False,
                 timestep_spacing="linspace", steps_offset=0, **_):
        if thresholding or use_karras_sigmas or not predict_x0 or solver_p is not None:
            raise NotImplementedError("UniPCMultistepScheduler: thresholding / use_karras_sigmas / predict_x0=False / solver_p "
                                      "are not implemented")
        if solver_order not in (1, 2, 3):
            raise ValueError(f"solver_order {solver_order!r}: 1, 2 or 3")
        if prediction_type not in ("epsilon", "sample", "v_prediction"):
            raise ValueError(f"prediction_type {prediction_type!r}: epsilon, sample or v_prediction")
        if solver_type in ("midpoint", "heun", "logrho"):      # (a DPM-Solver config: diffusers registers bh2 for these)
            solver_type = "bh2"
        if solver_type not in ("bh1", "bh2"):
            raise ValueError(f"solver_type {solver_type!r}: bh1 or bh2")
        if timestep_spacing not in ("leading", "trailing", "linspace"):
            raise ValueError(f"timestep_spacing {timestep_spacing!r}: leading, trailing or linspace")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, solver_order=solver_order, prediction_type=prediction_type,
                                      thresholding=thresholding, predict_x0=predict_x0, solver_type=solver_type,
                                      lower_order_final=lower_order_final, disable_corrector=tuple(disable_corrector),
                                      solver_p=solver_p, use_karras_sigmas=use_karras_sigmas,
                                      timestep_spacing=timestep_spacing, steps_offset=steps_offset)
        self._acp = _alphas_cumprod(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.alphas_cumprod = torch.from_numpy(self._acp)
        self.init_noise_sigma = 1.0
        self.disable_corrector = tuple(disable_corrector)
        self.timesteps = None
        self.sigmas = None

    def set_timesteps(self, num_inference_steps, device=None):
        c, N, n = self.config, self.config.num_train_timesteps, int(num_inference_steps)
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, N - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (N // (n + 1))).round()[::-1][:-1].copy().astype(np.int64)
            ts = ts + c.steps_offset
        else:
            ts = np.round(np.arange(N, 0, -N / n)).astype(np.int64) - 1
        if len(set(ts.tolist())) != len(ts):
            raise ValueError(f"{n} steps with {c.timestep_spacing!r} spacing repeat a timestep: the multistep history needs distinct ones")
        self._set_sigma_schedule(ts, device)
        self.num_inference_steps = n
        self.model_outputs = [None] * 3                     # m_{i-3}, m_{i-2}, m_{i-1}
        self.last_sample = None
        self.lower_order_nums = 0
        self._steps_done = 0
        self._step_index = None

    _alpha_sigma = staticmethod(DPMSolverMultistepScheduler._alpha_sigma)
    add_noise = DPMSolverMultistepScheduler.add_noise

    # ---- scalar part of one step (shared by `step` and the fused kernel) -------------------------
    @staticmethod
    def _b(h, count, solver_type):
        """(phi_1, B, [b_1 .. b_count]) of a step of log-SNR width h."""
        hh = -h
        phi1 = math.expm1(hh)
        B = phi1 if solver_type == "bh2" else hh
        g, f, b = phi1 / hh - 1.0, 1.0, []
        for j in range(1, count + 1):
            b.append(g * f / B)
            f *= j + 1
            g = g / hh - 1.0 / f
        return phi1, B, b

    @staticmethod
    def _rho(r, b):
        """Solves sum_k r_k^(j-1) rho_k = b_j, j = 1..len(r)."""
        R = np.array([[rk ** j for rk in r] for j in range(len(r))], dtype=np.float64)
        return [float(v) for v in np.linalg.solve(R, np.array(b[:len(r)], dtype=np.float64))]

    @staticmethod
    def scalars(sigmas, i, o_pred, o_corr, solver_type="bh2", prediction_type="epsilon"):
        """The scalars of step i over `sigmas` (float64 sequence, sigma/alpha form) with predictor order `o_pred` and corrector
        order `o_corr` (0: no corrector):
          m_i     = a_x*x + a_m*e                                              (x as handed in, before the correction)
          xhat_i  = q_l*xhat_{i-1} + q_1*m_{i-1} + q_2*m_{i-2} + q_3*m_{i-3} + q_n*m_i      (o_corr > 0; xhat_i = x otherwise)
          x_{i+1} = p_x*xhat_i + p_0*m_i + p_1*m_{i-1} + p_2*m_{i-2}
        Returns dict(q_l, q_1, q_2, q_3, q_n, p_x, p_0, p_1, p_2, a_x, a_m)."""
        U = UniPCMultistepScheduler
        al, sg, lam = {}, {}, {}
        for j in range(max(0, i - 3), i + 2):
            al[j], sg[j] = U._alpha_sigma(float(sigmas[j]))
            lam[j] = math.log(al[j]) - math.log(sg[j])
        k = dict(q_l=0.0, q_1=0.0, q_2=0.0, q_3=0.0, q_n=0.0, p_x=0.0, p_0=0.0, p_1=0.0, p_2=0.0)
        if prediction_type == "epsilon":
            k["a_x"], k["a_m"] = 1.0 / al[i], -sg[i] / al[i]
        elif prediction_type == "sample":
            k["a_x"], k["a_m"] = 0.0, 1.0
        elif prediction_type == "v_prediction":
            k["a_x"], k["a_m"] = al[i], -sg[i]
        else:
            raise ValueError(f"prediction_type {prediction_type!r}: epsilon, sample or v_prediction")
        if o_corr:
            o = int(o_corr)
            if not 1 <= o <= 3 or i - o < 0:
                raise ValueError(f"corrector order {o} at step {i}")
            h = lam[i] - lam[i - 1]
            phi1, B, b = U._b(h, o, solver_type)
            r = [(lam[i - 1 - j] - lam[i - 1]) / h for j in range(1, o)] + [1.0]
            rho = [0.5] if o == 1 else U._rho(r, b)
            k["q_l"] = sg[i] / sg[i - 1]
            k["q_1"] = -al[i] * phi1 + al[i] * B * sum(rho[j] / r[j] for j in range(o))
            for j in range(o - 1):                          # D_k = (m_{i-1-k} - m_{i-1}) / r_k
                k[f"q_{j + 2}"] = -al[i] * B * rho[j] / r[j]
            k["q_n"] = -al[i] * B * rho[o - 1]
        o = int(o_pred)
        if not 1 <= o <= 3 or i - (o - 1) < 0:
            raise ValueError(f"predictor order {o} at step {i}")
        h = lam[i + 1] - lam[i]
        phi1, B, b = U._b(h, max(o - 1, 1), solver_type)
        r = [(lam[i - j] - lam[i]) / h for j in range(1, o)]
        rho = [] if o == 1 else [0.5] if o == 2 else U._rho(r, b)
        k["p_x"] = sg[i + 1] / sg[i]
        k["p_0"] = -al[i + 1] * phi1 + al[i + 1] * B * sum(rho[j] / r[j] for j in range(o - 1))
        for j in range(o - 1):                              # D_k = (m_{i-k} - m_i) / r_k
            k[f"p_{j + 1}"] = -al[i + 1] * B * rho[j] / r[j]
        return k

    def orders(self, step_index: int, steps_done=None):
        """(predictor order, corrector order or 0) of step `step_index` when `steps_done` steps of this run came before it
        (default: the run began at index 0)."""
        c, n = self.config, len(self._ts)
        done = step_index if steps_done is None else int(steps_done)

        def pred(i, d):
            o = min(c.solver_order, n - i) if c.lower_order_final else c.solver_order
            return min(o, d + 1)                            # (lower_order_nums = min(d, solver_order))
        corr = pred(step_index - 1, done - 1) if done > 0 and (step_index - 1) not in self.disable_corrector else 0
        return pred(step_index, done), corr

    def coefficients(self, step_index: int, steps_done=None):
        """`scalars` of step `step_index` with this scheduler's order bookkeeping (see `orders`), plus `corr_on`."""
        o_pred, o_corr = self.orders(step_index, steps_done)
        k = self.scalars(self.sigmas, step_index, o_pred, o_corr, self.config.solver_type, self.config.prediction_type)
        k["corr_on"] = o_corr > 0
        return k

    def step(self, model_output, timestep, sample, return_dict=True):
        """diffusers-compatible tensor update (torch ops, fp32 arithmetic)."""
        if self._step_index is None:
            self._step_index = self.index_for_timestep(timestep)
        k = self.coefficients(self._step_index, self._steps_done)
        x = sample.float()
        m = k["a_x"] * x + k["a_m"] * model_output.float()
        m3, m2, m1 = self.model_outputs
        if k["corr_on"]:
            x = k["q_l"] * self.last_sample + k["q_1"] * m1 + k["q_n"] * m
            if k["q_2"] != 0.0:
                x = x + k["q_2"] * m2
            if k["q_3"] != 0.0:
                x = x + k["q_3"] * m3
        self.model_outputs = [m2, m1, m]
        self.last_sample = x
        prev = k["p_x"] * x + k["p_0"] * m
        if k["p_1"] != 0.0:
            prev = prev + k["p_1"] * m1
        if k["p_2"] != 0.0:
            prev = prev + k["p_2"] * m2
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self._steps_done += 1
        self._step_index += 1
        prev = prev.to(sample.dtype)
        return SchedulerOutput(prev_sample=prev, pred_original_sample=m.to(sample.dtype)) if return_dict else (prev,)


class EulerDiscreteScheduler(_Scheduler):
    """diffusers==0.24.0 EulerDiscreteScheduler in the configuration Stable Video Diffusion ships (the scheduler the
    reference's SVD pipelines drive: /root/reference/models/pipeline.py:399-401 set_timesteps, :419 scale_model_input,
    :440 step; /root/reference/train_svd.py:732-733): v-prediction, Karras sigmas between sigma_min and sigma_max,
    continuous timesteps t = 0.25 ln(sigma), leading spacing (init_noise_sigma = sqrt(sigma_max^2 + 1)).

    The schedule is host math (float64, sigmas rounded to float32 like diffusers); the tensor update is either the torch
    expression of `step()` or the fused HIP kernel `aa_cfg_euler_step_tokens` fed by `coefficients()`."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 prediction_type="v_prediction", interpolation_type="linear", use_karras_sigmas=True, sigma_min=0.002,
                 sigma_max=700.0, timestep_spacing="leading", timestep_type="continuous", steps_offset=1, **_):
        if prediction_type != "v_prediction" or not use_karras_sigmas or timestep_type != "continuous":
            raise NotImplementedError("only v_prediction / Karras sigmas / continuous timesteps (the SVD configuration)")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, prediction_type=prediction_type,
                                      interpolation_type=interpolation_type, use_karras_sigmas=use_karras_sigmas,
                                      sigma_min=sigma_min, sigma_max=sigma_max, timestep_spacing=timestep_spacing,
                                      timestep_type=timestep_type, steps_offset=steps_offset)
        acp = _alphas_cumprod(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self._train_sigmas = ((1 - acp) / acp) ** 0.5
        self.timesteps = None
        self.sigmas = None
        self._step_index = None

    def set_timesteps(self, num_inference_steps, device=None):
        c = self.config
        s_min = c.sigma_min if c.sigma_min is not None else float(self._train_sigmas[0])
        s_max = c.sigma_max if c.sigma_max is not None else float(self._train_sigmas[-1])
        rho = 7.0
        ramp = np.linspace(0, 1, num_inference_steps)
        lo, hi = s_min ** (1 / rho), s_max ** (1 / rho)
        sig = ((hi + ramp * (lo - hi)) ** rho).astype(np.float32)
        self._sig = np.concatenate([sig.astype(np.float64), [0.0]])
        self.sigmas = torch.from_numpy(np.concatenate([sig, np.zeros(1, np.float32)]))
        ts = torch.from_numpy((0.25 * np.log(sig.astype(np.float64))).astype(np.float32))
        self.timesteps = ts.to(device) if device is not None else ts
        self._ts = [float(t) for t in ts]
        self.num_inference_steps = num_inference_steps
        self._step_index = None

    @property
    def init_noise_sigma(self):
        m = float(self._sig.max())
        return m if self.config.timestep_spacing in ("linspace", "trailing") else (m * m + 1.0) ** 0.5

    def index_for_timestep(self, timestep):
        t = float(timestep)
        return min(range(len(self._ts)), key=lambda i: abs(self._ts[i] - t))

    def input_scale(self, step_index: int) -> float:
        s = self._sig[step_index]
        return 1.0 / math.sqrt(s * s + 1.0)

    def scale_model_input(self, sample, timestep):
        i = self._step_index if self._step_index is not None else self.index_for_timestep(timestep)
        return sample * self.input_scale(i)

    def coefficients(self, step_index: int):
        """x' = c_x * x + c_v * v for  x0 = v * (-s / sqrt(s^2+1)) + x / (s^2+1),  x' = x + (x - x0) / s * (s_next - s)."""
        s, sn = self._sig[step_index], self._sig[step_index + 1]
        r = (sn - s) / s
        return dict(c_x=1.0 + r * (1.0 - 1.0 / (s * s + 1.0)), c_v=r * s / math.sqrt(s * s + 1.0))

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        """diffusers-compatible tensor update (torch ops, fp32 arithmetic)."""
        if self._step_index is None:
            self._step_index = self.index_for_timestep(timestep)
        s, sn = self._sig[self._step_index], self._sig[self._step_index + 1]
        x = sample.float()
        x0 = model_output.float() * (-s / math.sqrt(s * s + 1.0)) + x / (s * s + 1.0)
        prev = (x + (x - x0) / s * (sn - s)).to(sample.dtype)
        self._step_index += 1
        return SchedulerOutput(prev_sample=prev, pred_original_sample=x0.to(sample.dtype)) if return_dict else (prev,)


# ------------------------------------------------------------------------------------- context windows
CONTEXT_WEIGHTS = ("flat", "pyramid")


def context_windows(num_frames, length, overlap, closed_loop=False, weights="pyramid"):
    """The window schedule of one denoising step over a clip of `num_frames` frames for a UNet that sees `length` frames at a time
    (MultiDiffusion over time, the context windows of the AnimateDiff ecosystem): a list of windows
    (frame_indices, normalised_weights, first_flags, last_flags), one entry per slot each.

    num_frames <= length: the single window range(num_frames) (callers treat it as "feature off").  Open clip, stride s = length -
    overlap: starts 0, s, 2s, ... while start + length < num_frames, then num_frames - length unless already present; window =
    range(start, start + length).  `closed_loop` (looping clips): starts 0, s, ... < num_frames, indices (start + j) % num_frames.
    Raw slot weights: "flat" 1, "pyramid" min(j + 1, length - j).  Normalisation per frame in float64: w_j over the sum of the raw
    weights of every (window, slot) that holds the frame - a frame held once gets exactly 1.0.  first[k][j] / last[k][j]: no earlier /
    no later window in list order holds the frame."""
    num_frames, length, overlap = int(num_frames), int(length), int(overlap)
    if length < 1 or not 0 <= overlap < length or num_frames < 1:
        raise ValueError(f"context_windows: need 1 <= length, 0 <= overlap < length and num_frames >= 1 (got num_frames {num_frames}, "
                         f"length {length}, overlap {overlap})")
    if weights not in CONTEXT_WEIGHTS:
        raise ValueError(f"context_windows: weights {weights!r} is not one of {CONTEXT_WEIGHTS}")
    if num_frames <= length:
        n = num_frames
        return [(list(range(n)), [1.0] * n, [True] * n, [True] * n)]
    stride = length - overlap
    if closed_loop:
        frames = [[(start + j) % num_frames for j in range(length)] for start in range(0, num_frames, stride)]
    else:
        starts = []
        start = 0
        while start + length < num_frames:
            starts.append(start)
            start += stride
        if num_frames - length not in starts:
            starts.append(num_frames - length)
        frames = [list(range(start, start + length)) for start in starts]
    raw = [1.0 if weights == "flat" else float(min(j + 1, length - j)) for j in range(length)]
    total = np.zeros(num_frames, dtype=np.float64)
    holders = [[] for _ in range(num_frames)]                   # windows that hold the frame, in list order
    for k, idx in enumerate(frames):
        for j, f in enumerate(idx):
            total[f] += raw[j]
            holders[f].append(k)
    return [(idx, [float(np.float64(raw[j]) / total[f]) for j, f in enumerate(idx)],
             [holders[f][0] == k for f in idx], [holders[f][-1] == k for f in idx]) for k, idx in enumerate(frames)]


# ------------------------------------------------------------------------------------- FreeInit
FREE_INIT_METHODS = ("butterworth", "gaussian", "ideal")
FREE_INIT_DEFAULTS = dict(num_iters=3, use_fast_sampling=False, method="butterworth", order=4, spatial_stop_frequency=0.25,
                          temporal_stop_frequency=0.25)


def check_free_init(free_init):
    """The `free_init` argument (FreeInit, diffusers `enable_free_init`): None (off), or a mapping with the keys of FREE_INIT_DEFAULTS -
    `num_iters` (an integer >= 1), `use_fast_sampling`, `method` ("butterworth" / "gaussian" / "ideal"), `order` (an integer >= 1; read
    by butterworth), `spatial_stop_frequency` and `temporal_stop_frequency` (numbers >= 0) - any of them left out taking its default;
    an unknown key or a value out of range raises ValueError.  Returns the completed dict, or None."""
    if free_init is None:
        return None
    if not hasattr(free_init, "keys"):
        raise ValueError(f"free_init {free_init!r}: a mapping with keys from {sorted(FREE_INIT_DEFAULTS)}")
    unknown = sorted(set(free_init.keys()) - set(FREE_INIT_DEFAULTS))
    if unknown:
        raise ValueError(f"free_init: unknown key(s) {unknown} (known: {sorted(FREE_INIT_DEFAULTS)})")
    c = dict(FREE_INIT_DEFAULTS)
    c.update({k: free_init[k] for k in free_init.keys()})
    for k in ("num_iters", "order"):
        if isinstance(c[k], bool) or not isinstance(c[k], int) or c[k] < 1:
            raise ValueError(f"free_init.{k} = {c[k]!r}: an integer >= 1")
    if not isinstance(c["use_fast_sampling"], bool):
        raise ValueError(f"free_init.use_fast_sampling = {c['use_fast_sampling']!r}: true or false")
    if c["method"] not in FREE_INIT_METHODS:
        raise ValueError(f"free_init.method = {c['method']!r}: one of {FREE_INIT_METHODS}")
    for k in ("spatial_stop_frequency", "temporal_stop_frequency"):
        v = c[k]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0.0 <= v < math.inf):       # (NaN fails the comparison)
            raise ValueError(f"free_init.{k} = {v!r}: a finite number >= 0")
        c[k] = float(v)
    return c


def free_init_filter(frames, h, w, method="butterworth", order=4, spatial_stop_frequency=0.25, temporal_stop_frequency=0.25):
    """The low-pass mask of FreeInit (diffusers `_get_free_init_freq_filter`) as float64 [frames, h, w] in SHIFTED index order (zero
    frequency at [frames // 2, h // 2, w // 2]).  With ss / ts the spatial / temporal stop frequency and
        d2 = ((ss / ts) (2 t / frames - 1))^2 + (2 y / h - 1)^2 + (2 x / w - 1)^2:
    butterworth 1 / (1 + (d2 / ss^2)^order), gaussian exp(-d2 / (2 ss^2)), ideal 1 where d2 <= 2 ss else 0 (diffusers compares the SQUARED
    distance with twice the stop frequency; restated as it is); all zeros when ss == 0 or ts == 0."""
    if method not in FREE_INIT_METHODS:
        raise ValueError(f"free_init_filter: method {method!r} is not one of {FREE_INIT_METHODS}")
    frames, h, w = int(frames), int(h), int(w)
    ss, ts = float(spatial_stop_frequency), float(temporal_stop_frequency)
    if ss == 0.0 or ts == 0.0:
        return torch.zeros((frames, h, w), dtype=torch.float64)
    t = (ss / ts) * (2.0 * torch.arange(frames, dtype=torch.float64) / frames - 1.0)
    y = 2.0 * torch.arange(h, dtype=torch.float64) / h - 1.0
    x = 2.0 * torch.arange(w, dtype=torch.float64) / w - 1.0
    d2 = (t * t)[:, None, None] + (y * y)[None, :, None] + (x * x)[None, None, :]
    if method == "butterworth":
        return 1.0 / (1.0 + (d2 / (ss * ss)) ** int(order))
    if method == "gaussian":
        return torch.exp(-d2 / (2.0 * ss * ss))
    return (d2 <= 2.0 * ss).to(torch.float64)


def free_init_symmetric_mask(mask):
    """The mask the kernel multiplies the UNSHIFTED spectrum with: Ms[k] = (Mu[k] + Mu[-k]) / 2, Mu = ifftshift(mask), -k modulo the
    size per axis (float64 in, float64 out).  Re IFFT3(Mu * FFT3 d) == IFFT3(Ms * FFT3 d) for real d: with an even axis Mu is symmetric
    already; with an odd one it is not, diffusers drops the imaginary part, and the symmetrised mask is that real part exactly."""
    dims = tuple(range(mask.dim()))
    mu = torch.roll(mask.to(torch.float64), [-(n // 2) for n in mask.shape], dims)            # ifftshift
    neg = torch.roll(torch.flip(mu, dims), [1] * mask.dim(), dims)                            # Mu[-k mod n]
    return 0.5 * (mu + neg)


def free_init_steps(num_inference_steps, num_iters, i, fast=False):
    """Denoising steps of FreeInit iteration `i` of `num_iters`: all of them, or under `use_fast_sampling` (diffusers)
    max(1, int(num_inference_steps / num_iters * (i + 1)))."""
    if not fast:
        return int(num_inference_steps)
    return max(1, int(num_inference_steps / num_iters * (i + 1)))
