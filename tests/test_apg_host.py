"""Adaptive Projected Guidance without a GPU: `pipeline.adaptive_projected_guidance` against the paper's pseudo-code written out here
(`project`, `normalized_guidance`, the momentum buffer), `check_apg` and the eval key, the keyword's way from `__call__` into `denoise`
and `_denoise_generic`, the refusal together with guidance_rescale, the generic loop's running update per window, and the fused loop of
the product TINY_UNET on the SIMT emulator - session run, aa_apg_tokens in place, the sampler's step kernel with guidance off - against
the oracle's UNet driven by a loop written here.

Fused loop against the oracle loop, three steps at guidance 9, max|fused - oracle| / max|oracle| of the final latents; APG with
{eta: 0, norm_threshold: half the first step's |t - u|, momentum: -0.5} is allowed twice what the same test measures with APG off (the
parent's path), the margin guidance_rescale, DDIM and UniPC were given.  Measured on the emulator (APG off, APG on; the first step
is clipped to s = 0.500, the later ones hardly or not at all):
  DPM-Solver++   1.813e-3  0.970e-3
  DDIM           2.255e-3  1.000e-3
  UniPC order 2  2.383e-3  1.269e-3"""
import pytest
import torch

import oracle
from animate_anything_amd import ops
from animate_anything_amd import pipeline as P
from animate_anything_amd.pipeline import APG_DEFAULTS, LatentToVideoPipeline, adaptive_projected_guidance, check_apg
from animate_anything_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler, context_windows
from animate_anything_amd.unet3d import UNet3DConditionModel
from test_ddim_host import _SessionStubUNet, _StubUNet
from util import TINY_UNET, rel_err, seeded_state


# ---- the paper's pseudo-code (Sadat et al. 2024, Algorithm 1), written out ----
class MomentumBuffer:
    def __init__(self, momentum):
        self.momentum, self.running_average = momentum, 0

    def update(self, update_value):
        new_average = self.momentum * self.running_average
        self.running_average = update_value + new_average


def normalize(v, dims):
    return v / v.norm(p=2, dim=dims, keepdim=True).clamp_min(1e-12)                  # torch.nn.functional.normalize


def project(v0, v1, dims):
    v1 = normalize(v1, dims)
    v0_parallel = (v0 * v1).sum(dim=dims, keepdim=True) * v1
    return v0_parallel, v0 - v0_parallel


def normalized_guidance(pred_cond, pred_uncond, guidance_scale, momentum_buffer=None, eta=1.0, norm_threshold=0.0):
    dims = list(range(1, pred_cond.dim()))
    diff = pred_cond - pred_uncond
    if momentum_buffer is not None:
        momentum_buffer.update(diff)
        diff = momentum_buffer.running_average
    if norm_threshold > 0:
        ones = torch.ones_like(diff)
        diff_norm = diff.norm(p=2, dim=dims, keepdim=True)
        diff = diff * torch.minimum(ones, norm_threshold / diff_norm)
    diff_parallel, diff_orthogonal = project(diff, pred_cond, dims)
    return pred_cond + (guidance_scale - 1) * (diff_orthogonal + eta * diff_parallel)


def test_the_closed_form_is_the_papers_pseudo_code():
    g = torch.Generator().manual_seed(3)
    scale = torch.tensor([1.0, 0.01, 3.0], dtype=torch.float64).reshape(3, 1, 1, 1, 1)
    for guidance in (1.5, 9.0):
        for eta in (0.0, 0.5, 1.0):
            for rho in (0.0, 5.0):
                for beta in (0.0, -0.5):
                    buf, running = (MomentumBuffer(beta) if beta != 0 else None), None
                    for _step in range(3):                                       # the momentum state carries over three calls
                        u = torch.randn(3, 4, 5, 6, 7, generator=g, dtype=torch.float64) * scale
                        t = 0.6 * u + 0.8 * torch.randn(3, 4, 5, 6, 7, generator=g, dtype=torch.float64) * scale
                        want = normalized_guidance(t, u, guidance, buf, eta, rho)
                        got, running = adaptive_projected_guidance(u, t, guidance, eta, rho, beta, running)
                        assert got.dtype == torch.float64 and (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
                        if beta != 0:
                            assert torch.equal(running, buf.running_average)
                        else:
                            assert running is None
                        if rho > 0:
                            norms = (t - u if buf is None else buf.running_average).reshape(3, -1).norm(dim=1)
                            assert (norms > rho).any() and (norms < rho).any()   # both branches of the clip
                        if eta == 1.0 and rho == 0.0 and beta == 0.0:
                            assert (got - (u + guidance * (t - u))).abs().max().item() <= 1e-12 * got.abs().max().item()   # plain guidance
    assert (got - (u + guidance * (t - u))).abs().max().item() > 1e-2              # and otherwise it does something


def test_sixteen_bit_operands_and_degenerate_clips():
    g = torch.Generator().manual_seed(4)
    u, t = torch.randn(2, 4, 3, 5, 5, generator=g), torch.randn(2, 4, 3, 5, 5, generator=g)
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        got, running = adaptive_projected_guidance(u.to(dt), t.to(dt), 9.0, 0.0, 3.0, -0.5, None)
        want = normalized_guidance(t.to(dt).double(), u.to(dt).double(), 9.0, MomentumBuffer(-0.5), 0.0, 3.0)
        assert got.dtype == torch.float32 and running.dtype == torch.float32
        assert (got.double() - want).abs().max().item() <= 2.0 ** -23 * want.abs().max().item()                  # float64 arithmetic, one rounding to fp32
    zero = torch.zeros_like(t)
    got, _ = adaptive_projected_guidance(u, zero, 9.0, 0.0, 0.0, 0.0)              # a text clip of zeros: no direction, the parallel part is 0
    assert torch.isfinite(got).all() and torch.allclose(got, 8.0 * (zero - u))
    assert torch.allclose(got, normalized_guidance(zero.double(), u.double(), 9.0, None, 0.0, 0.0).float())
    for rho in (0.0, 2.0):
        got, _ = adaptive_projected_guidance(t, t, 9.0, 0.5, rho, 0.0)             # u = t: a zero update, no division by its norm
        assert torch.equal(got, t)
    one = adaptive_projected_guidance(u[:, :1, :1, :1, :1], t[:, :1, :1, :1, :1], 9.0, 0.0, 0.0, 0.0)[0]          # one element: d is parallel to t
    assert torch.allclose(one, t[:, :1, :1, :1, :1], rtol=1e-6, atol=1e-6)


def test_check_apg():
    assert check_apg(None) is None
    assert check_apg({}) == APG_DEFAULTS == dict(eta=0.0, norm_threshold=0.0, momentum=0.0)
    assert check_apg({"eta": 1, "momentum": -0.5}) == dict(eta=1.0, norm_threshold=0.0, momentum=-0.5)
    assert check_apg(check_apg({"norm_threshold": 7.5})) == dict(eta=0.0, norm_threshold=7.5, momentum=0.0)       # a completed dict passes
    for bad in ({"beta": 0.5}, {"eta": 0.0, "rho": 1.0}, 0.5, "on", [0.0], True):
        with pytest.raises(ValueError, match="apg"):
            check_apg(bad)
    for bad in ({"eta": float("nan")}, {"eta": float("inf")}, {"eta": "0"}, {"eta": None}, {"eta": True}, {"norm_threshold": -1.0},
                {"norm_threshold": float("inf")}, {"momentum": 1.0}, {"momentum": -1.0}, {"momentum": 1.5}, {"momentum": float("nan")}):
        with pytest.raises(ValueError, match="apg"):
            check_apg(bad)
    assert "recommend" in check_apg.__doc__ and "tuned" in check_apg.__doc__


def test_eval_validates_the_key_before_any_model_is_loaded(tmp_path):
    from animate_anything_amd import eval as aa_eval
    missing = str(tmp_path / "no_such_checkpoint")
    for bad in ({"beta": 1}, {"momentum": 1.0}, {"norm_threshold": -2}, 0.5, "strong", True, [0.7]):
        with pytest.raises(ValueError, match="apg"):
            aa_eval.main_eval(missing, {"apg": bad})
        with pytest.raises(ValueError, match="apg"):
            aa_eval.batch_eval(None, None, None, None, {}, {"apg": bad}, str(tmp_path), False)
    with pytest.raises(ValueError, match="apg"):
        aa_eval.main_eval(missing, {"apg": {"eta": 0.0}, "guidance_rescale": 0.7})
    assert aa_eval._check_apg({}) is None and aa_eval._check_apg(None) is None     # absent: off
    assert aa_eval._check_apg({"apg": {}}) == APG_DEFAULTS and aa_eval._check_apg({"apg": {}, "guidance_rescale": 0}) == APG_DEFAULTS
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text("pretrained_model_path: x\nvalidation_data: {guidance_scale: 9}\n")
    assert aa_eval._check_apg(aa_eval.load_config(str(cfg_path))["validation_data"]) is None
    cfg = aa_eval.load_config(str(cfg_path), ["validation_data.apg.eta=0.25", "validation_data.apg.momentum=-0.5"])
    assert aa_eval._check_apg(cfg["validation_data"]) == dict(eta=0.25, norm_threshold=0.0, momentum=-0.5)
    cfg = aa_eval.load_config(str(cfg_path), ["validation_data.apg.momentum=2"])
    cfg["pretrained_model_path"] = missing
    with pytest.raises(ValueError, match="apg"):
        aa_eval.main_eval(**cfg)
    assert "apg" in aa_eval.__doc__


def _call_args(guidance, frames=3):
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g)
    lat, cond, mask = r(1, 4, frames, 4, 4), r(1, 4, 1, 4, 4), (r(1, 1, 1, 4, 4) > 0).float()
    return dict(latents=lat, prompt_embeds=r(1, 7, 16).half(), negative_prompt_embeds=r(1, 7, 16).half(), condition_latent=cond.half(),
                mask=mask.half(), motion=[3.0], num_inference_steps=3, guidance_scale=guidance, return_dict=False)


def test_the_keyword_reaches_denoise_and_the_generic_loop(monkeypatch):
    seen = []

    def fake_denoise(self, latents, *a, **k):
        seen.append(k.get("apg", "absent"))
        return latents.float()
    with monkeypatch.context() as m:
        m.setattr(LatentToVideoPipeline, "denoise", fake_denoise)
        pipe = LatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=DPMSolverMultistepScheduler())
        pipe(**_call_args(9.0))
        pipe(apg={"eta": 0.5}, **_call_args(9.0))
        assert seen == [None, dict(eta=0.5, norm_threshold=0.0, momentum=0.0)]
    del seen[:]
    with monkeypatch.context() as m:                                                 # no session: `denoise` hands over to the generic loop
        m.setattr(LatentToVideoPipeline, "_denoise_generic", lambda self, latents, *a, **k: (seen.append(k.get("apg", "absent")), latents.float())[1])
        pipe(apg={"momentum": -0.5}, **_call_args(9.0))
        pipe(apg={"momentum": -0.5}, **_call_args(1.0))                              # guidance <= 1: off
        assert seen == [dict(eta=0.0, norm_threshold=0.0, momentum=-0.5), None]


@pytest.mark.parametrize("unet", [_StubUNet, _SessionStubUNet], ids=["generic", "fused"])
def test_apg_with_guidance_rescale_is_refused_before_any_device_work(emu, monkeypatch, unet):
    for name in ("apg_tokens", "cfg_rescale_tokens", "cfg_dpm_step_tokens"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: pytest.fail(f"{_n} ran"))
    net = unet(torch.float16)
    monkeypatch.setattr(net, "session", lambda *a, **k: pytest.fail("a session was built"), raising=False)
    monkeypatch.setattr(_StubUNet, "__call__", lambda *a, **k: pytest.fail("the UNet ran"))
    pipe = LatentToVideoPipeline(vae=None, unet=net, scheduler=DPMSolverMultistepScheduler())
    with pytest.raises(ValueError, match="guidance_rescale"):
        pipe(apg={}, guidance_rescale=0.7, **_call_args(9.0))
    args = _call_args(9.0)
    pipe.scheduler.set_timesteps(3)
    for loop in (pipe.denoise, pipe._denoise_generic):
        with pytest.raises(ValueError, match="guidance_rescale"):
            loop(args["latents"], torch.cat([args["negative_prompt_embeds"], args["prompt_embeds"]]), args["condition_latent"], args["mask"], [3.0],
                 [int(t) for t in pipe.scheduler.timesteps], 9.0, guidance_rescale=0.7, apg={"eta": 0.0})
    with pytest.raises(ValueError, match="apg"):
        pipe(apg={"strength": 1.0}, **_call_args(9.0))


@pytest.mark.parametrize("scheduler", [DPMSolverMultistepScheduler, DDIMScheduler, UniPCMultistepScheduler])
def test_both_loops_apply_it_under_guidance_only(emu, monkeypatch, scheduler):
    """The fused loop (stub session on the emulator): one aa_apg_tokens per step, in place on the session's matrix, with one momentum
    buffer zeroed per `denoise`, and the step kernel with guidance off; the generic loop: adaptive_projected_guidance; apg=None and
    guidance_scale <= 1 launch nothing, allocate nothing and give the run without the keyword bit for bit."""
    calls, guided, torch_calls = [], [], []
    real, real_torch = ops.apg_tokens, P.adaptive_projected_guidance
    spy = lambda *a, **k: (calls.append((a[1:], k["momentum_buf"], None if k["momentum_buf"] is None else k["momentum_buf"].clone())), real(*a, **k))[1]
    for name, at in (("cfg_dpm_step_tokens", 4), ("cfg_ddim_step_tokens", 3), ("cfg_unipc_step_tokens", 3)):     # where `guidance` stands
        monkeypatch.setattr(ops, name, lambda *a, _s=getattr(ops, name), _at=at, **k: (guided.append(a[_at]), _s(*a, **k))[1])
    monkeypatch.setattr(P, "adaptive_projected_guidance", lambda *a: (torch_calls.append(a[2:]), real_torch(*a))[1])
    apg = dict(eta=0.0, norm_threshold=0.05, momentum=-0.5)
    outs = {}
    for guidance, on in ((9.0, None), (9.0, apg), (9.0, dict(apg, momentum=0.0)), (1.0, apg), (1.0, None)):
        del calls[:], guided[:], torch_calls[:]
        active = guidance > 1 and on is not None
        monkeypatch.setattr(ops, "apg_tokens", spy if active else lambda *a, **k: pytest.fail("aa_apg_tokens launched with APG off"))
        fused = LatentToVideoPipeline(vae=None, unet=_SessionStubUNet(torch.float16), scheduler=scheduler())
        monkeypatch.setattr(fused, "_denoise_generic", lambda *a, **k: pytest.fail("the fused loop was not selected"))
        got = fused(apg=on, **_call_args(guidance))[1]
        without = fused(**_call_args(guidance))[1] if not active else None
        assert len(calls) == (3 if active else 0)
        if active:
            assert all(c[0] == (1, 4, 3, 16, 9.0, 0.0, 0.05, on["momentum"]) for c in calls)                     # in place: no `out`
            if on["momentum"] != 0:
                assert len({c[1].data_ptr() for c in calls}) == 1 and calls[0][1].numel() == 4 * 3 * 16 and calls[0][1].dtype == torch.float32
                assert (calls[0][2] == 0).all() and (calls[1][2] != 0).any(), "zero before the first step, carried to the second"
            else:
                assert all(c[1] is None for c in calls)
        else:
            assert torch.equal(got, without), "APG off is the call without the keyword, bit for bit"
        assert guided == ([None] * 3 if guidance == 1.0 or active else [9.0] * 3) * (1 if active else 2)
        generic = LatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=scheduler())(apg=on, **_call_args(guidance))[1]
        assert [c[:4] for c in torch_calls] == ([(9.0, 0.0, 0.05, on["momentum"])] * 3 if active else [])
        if active and on["momentum"] != 0:
            assert torch_calls[0][4] is None and all(c[4] is not None for c in torch_calls[1:])
        assert rel_err(got, generic) < 2e-2
        outs[guidance, None if on is None else on["momentum"]] = got
    assert torch.equal(outs[1.0, -0.5], outs[1.0, None])
    assert not torch.equal(outs[9.0, -0.5], outs[9.0, None]) and not torch.equal(outs[9.0, -0.5], outs[9.0, 0.0])


def test_the_generic_loop_keeps_one_running_update_per_window(monkeypatch):
    seen = []
    real = P.adaptive_projected_guidance

    def spy(*a):
        out = real(*a)
        seen.append((a[6], out[1]))
        return out
    monkeypatch.setattr(P, "adaptive_projected_guidance", spy)
    context = {"frames": 4, "overlap": 2}
    windows = context_windows(10, 4, 2, False, "pyramid")
    n = len(windows)
    assert n == 4
    pipe = LatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float32), scheduler=DPMSolverMultistepScheduler())
    got = pipe(context=context, apg=dict(momentum=-0.5, norm_threshold=0.05), **_call_args(9.0, frames=10))[1]
    assert len(seen) == 3 * n and all(handed is None for handed, _ in seen[:n])
    for i in range(n, 3 * n):
        assert seen[i][0] is seen[i - n][1], "window j of a step is handed what window j of the previous step returned"
        assert seen[i][1].shape == (1, 4, 4, 4, 4)
    assert len({id(r) for _, r in seen}) == 3 * n
    del seen[:]
    other = pipe(context=context, apg=dict(momentum=0.0, norm_threshold=0.05), **_call_args(9.0, frames=10))[1]
    assert all(handed is None and r is None for handed, r in seen) and got.shape == (1, 4, 10, 4, 4) and not torch.equal(got, other)


@pytest.mark.parametrize("scheduler", [DPMSolverMultistepScheduler, DDIMScheduler])
def test_the_fused_loop_under_context_windows_guides_every_window_before_the_merge(emu, monkeypatch, scheduler):
    calls = []
    for name in ("window_gather_latents", "apg_tokens", "window_merge_tokens", "cfg_dpm_step_tokens", "cfg_ddim_step_tokens"):
        monkeypatch.setattr(ops, name, lambda *a, _s=getattr(ops, name), _n=name, **k: (calls.append((_n, a, k)), _s(*a, **k))[1])
    apg = dict(eta=0.0, norm_threshold=0.05, momentum=-0.5)
    case = _call_args(9.0, frames=10)
    fused = LatentToVideoPipeline(vae=None, unet=_SessionStubUNet(torch.float16), scheduler=scheduler())
    monkeypatch.setattr(fused, "_denoise_generic", lambda *a, **k: pytest.fail("the fused loop was not selected"))
    got = fused(context={"frames": 4, "overlap": 2}, apg=apg, **case)[1]
    names = [c[0] for c in calls]
    step = names[12]
    assert names == (["window_gather_latents", "apg_tokens", "window_merge_tokens"] * 4 + [step]) * 3 and step.endswith("_step_tokens")
    bufs = [c[2]["momentum_buf"].data_ptr() for c in calls if c[0] == "apg_tokens"]
    assert len(set(bufs)) == 4 and bufs == bufs[:4] * 3, "one momentum buffer per window of the schedule"
    for name, a, k in calls:
        if name == "apg_tokens":
            assert a[1:] == (1, 4, 4, 16, 9.0, 0.0, 0.05, -0.5) and k["momentum_buf"].numel() == 4 * 4 * 16      # the window's geometry
        elif name == "window_merge_tokens":
            assert a[2].shape == (11 * 16, 8) and a[4] is None                                                   # one half, guidance off
        elif name.endswith("_step_tokens"):
            assert a[0].shape == (11 * 16, 8) and a[4 if name == "cfg_dpm_step_tokens" else 3] is None
    generic = LatentToVideoPipeline(vae=None, unet=_StubUNet(torch.float16), scheduler=scheduler())(context={"frames": 4, "overlap": 2}, apg=apg, **case)[1]
    assert torch.isfinite(got).all() and rel_err(got, generic) < 2e-2


# ---- the product UNet's fused loop on the emulator against the oracle's UNet ----
STEPS, GUIDANCE = 3, 9.0
SAMPLERS = {"dpm": lambda: DPMSolverMultistepScheduler(), "ddim": lambda: DDIMScheduler(), "unipc": lambda: UniPCMultistepScheduler(solver_order=2)}


@pytest.fixture(scope="module")
def tiny_pair():
    torch.manual_seed(0)
    ref = oracle.UNet3DConditionModel(**TINY_UNET).eval()
    state = seeded_state(ref)
    ref.load_state_dict(state)
    net = UNet3DConditionModel(**TINY_UNET).eval()
    net.load_state_dict(state)
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g)
    case = dict(lat=r(1, 4, 2, 5, 6), cond=r(1, 4, 1, 5, 6), pos=r(1, 9, 64), neg=r(1, 9, 64), mask=torch.zeros(1, 1, 1, 5, 6))
    case["mask"][..., 1:4, 2:5] = 1
    return ref, net.half(), case


def oracle_loop(ref, case, scheduler, apg, norms=None):
    """The reference's sequence (batch the halves, guidance, the scheduler's step on [b*f, c, h, w]) around the oracle's UNet in fp32,
    with the paper's pseudo-code in the place of the guidance expression when `apg` is given.  `norms` collects |t - u| per step."""
    scheduler.set_timesteps(STEPS)
    x = case["lat"].clone()
    text, cond = torch.cat([case["neg"], case["pos"]]), torch.cat([case["cond"], case["cond"]])
    buf = MomentumBuffer(apg["momentum"]) if apg is not None and apg["momentum"] != 0 else None
    with torch.no_grad():
        for t in scheduler.timesteps:
            eps = ref(torch.cat([x, x]), int(t), text, cond, case["mask"], motion=torch.tensor([3.0])).sample
            e_u, e_t = eps[:1], eps[1:]
            if norms is not None:
                norms.append((e_t - e_u).double().norm().item())
            if apg is None:
                e = e_u + GUIDANCE * (e_t - e_u)
            else:
                e = normalized_guidance(e_t.double(), e_u.double(), GUIDANCE, buf, apg["eta"], apg["norm_threshold"]).float()
            b, c, f, h, w = x.shape
            flat = scheduler.step(e.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w), t, x.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)).prev_sample
            x = flat.reshape(b, f, c, h, w).permute(0, 2, 1, 3, 4).contiguous()
    return x


@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_fused_loop_of_the_tiny_unet_matches_the_oracle_loop(emu, monkeypatch, tiny_pair, sampler):
    ref, net, case = tiny_pair
    norms = []
    oracle_loop(ref, case, SAMPLERS[sampler](), None, norms)
    rho = float(torch.tensor(0.5 * norms[0], dtype=torch.float32))                 # about half the first step's |t - u|: the clip acts
    apg = dict(eta=0.0, norm_threshold=rho, momentum=-0.5)
    calls = []
    real = ops.apg_tokens
    stats = torch.zeros(1, 2)
    monkeypatch.setattr(ops, "apg_tokens", lambda *a, **k: (calls.append(a[1:]), real(*a, stats=stats, **k), calls.append(stats[0].tolist()))[1])
    dist, finals = {}, {}
    for on in (None, apg):
        want = oracle_loop(ref, case, SAMPLERS[sampler](), on)
        pipe = LatentToVideoPipeline(vae=None, unet=net, scheduler=SAMPLERS[sampler]())
        monkeypatch.setattr(pipe, "_denoise_generic", lambda *a, **k: pytest.fail("the fused loop was not selected"))
        pipe.scheduler.set_timesteps(STEPS)
        with torch.no_grad():
            got = pipe.denoise(case["lat"], torch.cat([case["neg"], case["pos"]]).half(), case["cond"].half(), case["mask"].half(), [3.0],
                               [int(t) for t in pipe.scheduler.timesteps], GUIDANCE, apg=on)
        assert torch.isfinite(got).all()
        dist[on is not None], finals[on is not None] = rel_err(got, want), (got, want)
    print(f"{sampler}: fused vs oracle, APG off {dist[False]:.4g}, APG {apg} {dist[True]:.4g} (bound {2 * dist[False]:.4g}); (s, p) per step {calls[1::2]}")
    assert calls[0::2] == [(1, 4, 2, 30, GUIDANCE, 0.0, rho, -0.5)] * STEPS
    assert calls[1][0] < 1.0, "the first step is clipped"
    assert rel_err(finals[True][1], finals[False][1]) > 0.05                       # APG moves the oracle's result: no no-op passes
    assert dist[False] > 0.0 and dist[True] <= 2 * dist[False]
