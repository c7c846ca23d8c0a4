"""aa_apg_tokens (Adaptive Projected Guidance, per clip on the UNet's token-layout output; two launches) against its definition in float64
evaluated from the same rounded inputs, on the emulator and on the GPU: the one-element clip, the hand-made two-element clip, odd sizes
with three clips, several workgroups per clip with a ragged tail, row pitches 4 / 8 / 16, the benchmark's shape; fp16 and bf16, guidance
1.5 and 9, eta 0 / 0.5 / 1, the norm threshold off and on (taken from the reference so that both branches are met), momentum 0 and -0.5
on a non-zero state, clips of deviation 1, 0.01 and 3, the text half correlated with the unconditional one; the exact-value probes that
catch a one-term error; `stats` and the rewritten momentum buffer; in place against out of place and a second call from the same state
bit for bit; sentinels around everything that must not be touched; every refusal of the entry point.

    d = t - u,  (r = d + beta r_prev, d = r,)  dd = <d,d>, dt = <d,t>, tt = <t,t>,  s = rho / sqrt(dd) if rho > 0 and dd > rho^2 else 1,
    p = s dt / tt if tt > 0 else 0,  a = 1 + (g - 1)(eta - 1) p,  c = (g - 1) s,  e = a t + c d

Bound (eps = 2^-24; from the arithmetic, no measurement behind it).  g, eta, rho, beta are chosen exact in fp32.
 * d: one subtraction, err_d = eps |d|.  With momentum r = d + beta r_prev: the rounding of d, of the product and of the sum (a fused
   multiply-add only drops one): err_d = eps (|t - u| + |beta r_prev| + |r|) (1 + 2^-20).  The rewritten momentum buffer is held to it.
 * the sums: a product of two fp32 values is exact in fp64; the accumulation of n <= 2^19 terms costs at most n 2^-53 <= acc = 2^-34
   of the sum of the magnitudes, which for dd and tt is the sum itself and for dt at most |d| |t| (norms over the clip).  With E the
   2-norm of err_d over the clip, the kernel's |d| lies within D_N = E + acc (N + E) of N = |d|, its dt within
   D_dt = (E + acc (N + E)) |t| of dt, its tt within acc tt of tt (a sum of squares: it vanishes only when every t is zero, and then
   exactly - no conditioning premise is needed for it).
 * s: not clipped, s = 1 exactly.  Clipped, rho / (N - D_N) - rho / N plus eps each for the fp64 square root and division, which
   -ffast-math may evaluate through refined estimates: D_s = rho / (N - D_N) - s + 2 eps s.  The test asserts D_N < N / 2 and
   |N / rho - 1| > 1e-3 > 10 D_N / N on the reference, so kernel and reference take the same branch.
 * p: D_p = (s + D_s)(|dt| + D_dt) / (tt (1 - acc)) - s |dt| / tt + 2 eps |p|   (a product and a division).
 * a, c: formed in fp64 and rounded once to fp32: D_a = |g - 1| |eta - 1| D_p + eps |a|,  D_c = |g - 1| D_s + eps |c|.
 * e: the operands' errors, D_a |t| + D_c |d| + (|c| + D_c) err_d =: x, then two products and one addition in fp32 (a fused multiply-add
   only drops a rounding), each at most eps of |a t| + |c d| + x: err32 = x + 2 eps (|a t| + |c d| + x) (1 + 2^-20) - an ABSOLUTE term
   in |a t| + |c d|, since with eta = 0 the two nearly cancel.  The store adds half an ulp of the storage type at |e| + err32.
 * stats: (s, p) rounded to fp32: D_s + eps s and D_p + eps |p|."""
import ctypes as C
import functools
import math

import pytest
import torch

import test_ddim_step
from animate_anything_amd import _lib, ops
from test_ddim_step import backend  # noqa: F401  (the emulator / GPU fixture; it sets test_ddim_step.DEV)

EPS = 2.0 ** -24
ACC = 2.0 ** -34
SENTINEL = 768.0                                       # (exact in fp16 and bf16)
GUARD = 2                                              # rows behind the last one / elements around the fp32 buffers: never written
SHAPES = [(1, 1, 1, 1, 8), (1, 1, 1, 2, 8), (2, 4, 3, 10, 8), (3, 4, 2, 37, 8), (2, 4, 5, 1031, 8),
          (2, 4, 3, 10, 4), (2, 4, 3, 10, 16), (2, 4, 5, 1031, 4), (2, 4, 5, 1031, 16)]
BENCH_SHAPE = (1, 4, 16, 4096, 8)
GUIDANCES = (1.5, 9.0)
ETAS = (0.0, 0.5, 1.0)
BETAS = (0.0, -0.5)
CLIP_SCALE = (1.0, 0.01, 3.0)
DTYPES = pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])


def dev():
    return test_ddim_step.DEV


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def half_ulp(v, dt):
    """Half an ulp of the storage type at magnitude v (float64 tensor)."""
    mant, emin = (10, -14) if dt == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(v.clamp_min(2.0 ** emin))).clamp_min(emin)
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def valid(m, shape, half=0):
    """The [clips, frames, hw, channels] view of what the step kernels consume of half `half` of a token matrix."""
    clips, ch, frames, hw, _ = shape
    return m[half * clips * (frames + 1) * hw:(half + 1) * clips * (frames + 1) * hw].reshape(clips, frames + 1, hw, m.shape[1])[:, 1:, :, :ch]


@functools.lru_cache(maxsize=None)
def tokens_of(shape, dt, kind="random"):
    """The rounded token matrix [2 * rows + GUARD, ld] (CPU): sentinels in frame 0, the padding columns and the guard rows.  "random":
    clip b of deviation CLIP_SCALE[b], u from one seed and t = 0.6 u' + 0.8 w with w from another (dt / tt is neither 0 nor 1);
    "scaled": u = t / 2 clip-wide; "hand": t = (1, 0), u = (1, -1); "zero_text": t = 0; "equal": u = t."""
    clips, ch, frames, hw, ld = shape
    rows = clips * (frames + 1) * hw
    tok = torch.full((2 * rows + GUARD, ld), SENTINEL, dtype=dt)
    salt = 13 * SHAPES.index(shape) if shape in SHAPES else 0
    scale = torch.tensor(CLIP_SCALE[:clips]).reshape(clips, 1, 1, 1)
    x1 = torch.randn(clips, frames, hw, ch, generator=torch.Generator().manual_seed(211 + salt))
    x2 = torch.randn(clips, frames, hw, ch, generator=torch.Generator().manual_seed(977 + salt))
    u, t = scale * x1, scale * (0.6 * x1 + 0.8 * x2)
    if kind == "scaled":
        t = t.to(dt).float().clamp_min(2.0 ** -10) if dt == torch.float16 else t.to(dt).float()   # (halving stays exact: no fp16 subnormals)
        u = 0.5 * t
    elif kind == "hand":
        assert (ch, frames, hw) == (1, 1, 2)
        t, u = torch.tensor([1.0, 0.0]).reshape(1, 1, 2, 1), torch.tensor([1.0, -1.0]).reshape(1, 1, 2, 1)
    elif kind == "zero_text":
        t = torch.zeros_like(t)
    elif kind == "equal":
        u = t
    else:
        assert kind == "random"
    valid(tok, shape, 0).copy_(u.to(dt))
    valid(tok, shape, 1).copy_(t.to(dt))
    return tok


@functools.lru_cache(maxsize=None)
def state_of(shape):
    """A non-zero running update r_prev, fp32 [clips, frames, hw, channels], of the clips' scale."""
    clips, ch, frames, hw, _ = shape
    g = torch.Generator().manual_seed(4001 + (SHAPES.index(shape) if shape in SHAPES else 0))
    return torch.randn(clips, frames, hw, ch, generator=g) * torch.tensor(CLIP_SCALE[:clips]).reshape(clips, 1, 1, 1)


def norms(shape, dt, kind, beta):
    """|d| per clip, in float64 from the rounded inputs (what rho is chosen from)."""
    tok = tokens_of(shape, dt, kind).double()
    d = valid(tok, shape, 1) - valid(tok, shape, 0)
    if beta != 0.0:
        d = d + beta * state_of(shape).double()
    return d.reshape(shape[0], -1).norm(dim=1)


def thresholds(shape, dt, kind, beta):
    """The norm thresholds to run (0: off): several clips - the geometric mean of the smallest and the largest |d|; one clip - |d| / 2
    and 2 |d|.  fp32 values."""
    n = norms(shape, dt, kind, beta)
    if shape[0] > 1:
        return (0.0, f32(math.sqrt(n.min().item() * n.max().item())))
    return (0.0, f32(0.5 * n[0].item()), f32(2.0 * n[0].item()))


@functools.lru_cache(maxsize=4)
def reference(shape, dt, kind, guidance, eta, rho, beta):
    """float64 from the rounded inputs: dict(e, err32 - the bound of e before the store -, r, err_r, s, d_s, p, d_p), e / err32 / r / err_r
    [clips, frames, hw, channels], the rest [clips]."""
    clips = shape[0]
    assert all(f32(v) == v for v in (guidance, eta, rho, beta))
    tok = tokens_of(shape, dt, kind).double()
    u, t = valid(tok, shape, 0), valid(tok, shape, 1)
    d = t - u
    err_d = EPS * d.abs()
    if beta != 0.0:
        prev = state_of(shape).double()
        r = d + beta * prev
        err_d = EPS * (d.abs() + (beta * prev).abs() + r.abs()) * (1 + 2.0 ** -20)
        d = r
    flat = lambda v: v.reshape(clips, -1)
    dd, dtt, tt = (flat(d) ** 2).sum(1), (flat(d) * flat(t)).sum(1), (flat(t) ** 2).sum(1)
    s, d_s, p, d_p = torch.ones(clips, dtype=torch.float64), torch.zeros(clips, dtype=torch.float64), torch.zeros(clips, dtype=torch.float64), torch.zeros(clips, dtype=torch.float64)
    for b in range(clips):
        N, E, nt = math.sqrt(dd[b].item()), flat(err_d)[b].norm().item(), math.sqrt(tt[b].item())
        d_n = E + ACC * (N + E)
        if rho > 0.0 and N > 0.0:
            assert abs(N / rho - 1.0) > 1e-3 and d_n < 1e-4 * N, "the clip test is not decided on this input"
            if N > rho:
                assert d_n < 0.5 * N
                s[b] = rho / N
                d_s[b] = rho / (N - d_n) - rho / N + 2 * EPS * s[b].item()
        if tt[b] > 0:
            p[b] = s[b] * dtt[b] / tt[b]
            d_dt = d_n * nt
            d_p[b] = ((s[b] + d_s[b]) * (dtt[b].abs() + d_dt) / (tt[b] * (1 - ACC)) - s[b] * dtt[b].abs() / tt[b]) + 2 * EPS * p[b].abs()
    g1 = guidance - 1.0
    a, c = 1.0 + g1 * (eta - 1.0) * p, g1 * s
    d_a, d_c = abs(g1) * abs(eta - 1.0) * d_p + EPS * a.abs(), abs(g1) * d_s + EPS * c.abs()
    col = lambda v: v.reshape(clips, 1, 1, 1)
    e = col(a) * t + col(c) * d
    x = col(d_a) * t.abs() + col(d_c) * d.abs() + (col(c).abs() + col(d_c)) * err_d
    err32 = x + 2 * EPS * ((col(a) * t).abs() + (col(c) * d).abs() + x) * (1 + 2.0 ** -20)
    return dict(e=e, err32=err32, r=d, err_r=err_d, s=s, d_s=d_s + EPS * s, p=p, d_p=d_p + EPS * p.abs())


def run(shape, dt, kind, guidance, eta, rho, beta, in_place, out_pad=4):
    """One call on the backend; checks everything that must stay untouched; returns (valid output, stats [clips, 2], momentum buffer
    or None), on the CPU."""
    clips, ch, frames, hw, ld = shape
    rows, n = clips * (frames + 1) * hw, clips * frames * hw * ch
    before = tokens_of(shape, dt, kind)
    buf = before.clone().to(dev())
    tok = buf[:2 * rows]
    sbuf = torch.full((2 * clips + 2 * GUARD,), -5.0, dtype=torch.float32).to(dev())
    mbuf = None
    if beta != 0.0:
        mbuf = torch.full((n + 2 * GUARD,), -5.0, dtype=torch.float32)
        mbuf[GUARD:GUARD + n] = state_of(shape).reshape(-1)
        mbuf = mbuf.to(dev())
    kw = dict(momentum_buf=None if mbuf is None else mbuf[GUARD:GUARD + n], stats=sbuf[GUARD:GUARD + 2 * clips])

    def fp32_buffers():
        s_host = sbuf.cpu()
        assert (s_host[:GUARD] == -5.0).all() and (s_host[GUARD + 2 * clips:] == -5.0).all(), "wrote around stats"
        if mbuf is None:
            return s_host[GUARD:GUARD + 2 * clips].reshape(clips, 2).clone(), None
        m_host = mbuf.cpu()
        assert (m_host[:GUARD] == -5.0).all() and (m_host[GUARD + n:] == -5.0).all(), "wrote around the momentum buffer"
        return s_host[GUARD:GUARD + 2 * clips].reshape(clips, 2).clone(), m_host[GUARD:GUARD + n].reshape(clips, frames, hw, ch).clone()

    if in_place:
        got = ops.apg_tokens(tok, clips, ch, frames, hw, guidance, eta, rho, beta, **kw)
        assert got.data_ptr() == tok.data_ptr() and got.shape[0] == rows and got.stride(0) == ld
        after = buf.cpu()
        keep = after.clone()
        valid(keep, shape, 0).copy_(valid(before, shape, 0))                      # everything but the valid region of the first half ...
        assert torch.equal(keep.view(torch.int16), before.view(torch.int16)), "wrote outside the unconditional clips' frames 1..T"
        return (valid(after, shape, 0).clone(),) + fp32_buffers()
    obuf = torch.full((rows + GUARD, ld + out_pad), SENTINEL, dtype=dt).to(dev())
    got = ops.apg_tokens(tok, clips, ch, frames, hw, guidance, eta, rho, beta, out=obuf[:rows], **kw)
    assert got.data_ptr() == obuf.data_ptr()
    assert torch.equal(buf.cpu().view(torch.int16), before.view(torch.int16)), "the input is only read"
    after = obuf.cpu()
    keep = after.clone()
    valid(keep, shape, 0).fill_(SENTINEL)
    assert (keep.float() == SENTINEL).all(), "wrote frame 0, a padding column or a guard row"
    return (valid(after, shape, 0).clone(),) + fp32_buffers()


def check(shape, dt, kind, guidance, eta, rho, beta, repeat=True):
    ref = reference(shape, dt, kind, guidance, eta, rho, beta)
    e, err32 = ref["e"], ref["err32"]
    bound = err32 + half_ulp(e.abs() + err32, dt)
    got, stats, mom = run(shape, dt, kind, guidance, eta, rho, beta, False)
    err = (got.double() - e).abs()
    s_err, p_err = (stats[:, 0].double() - ref["s"]).abs(), (stats[:, 1].double() - ref["p"]).abs()
    print(f"{shape} {dt} {kind} g {guidance} eta {eta} rho {rho:.4g} beta {beta}: s {[round(v, 4) for v in ref['s'].tolist()]} "
          f"p {[round(v, 4) for v in ref['p'].tolist()]} worst err/bound {(err / bound).max().item():.3f} (max err {err.max().item():.3g}), "
          f"s err {s_err.max().item():.3g} (D_s {ref['d_s'].max().item():.3g}), p err {p_err.max().item():.3g} (D_p {ref['d_p'].max().item():.3g})")
    assert (err <= bound).all()
    assert (s_err <= ref["d_s"]).all() and (p_err <= ref["d_p"]).all()
    assert (stats[:, 0][ref["s"] == 1.0] == 1.0).all(), "an unclipped clip has s = 1 exactly"
    if beta != 0.0:
        assert ((mom.double() - ref["r"]).abs() <= ref["err_r"]).all(), "the rewritten momentum buffer"
    else:
        assert mom is None
    if repeat:
        bits = lambda v: v.contiguous().view(torch.int16)
        same = lambda x, y: (x is None and y is None) or torch.equal(x, y)
        again, stats2, mom2 = run(shape, dt, kind, guidance, eta, rho, beta, False, out_pad=0)
        inplace, stats3, mom3 = run(shape, dt, kind, guidance, eta, rho, beta, True)
        assert torch.equal(bits(again), bits(got)) and torch.equal(stats2, stats) and same(mom2, mom), "a second call from the same state must repeat the bits"
        assert torch.equal(bits(inplace), bits(got)) and torch.equal(stats3, stats) and same(mom3, mom), "in place must equal out of place"
    return ref, got, stats


@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_float64_definition(backend, shape, dt):
    for beta in BETAS:
        rhos = thresholds(shape, dt, "random", beta)
        for rho in rhos:
            for guidance in GUIDANCES:
                for eta in ETAS:
                    ref, _, _ = check(shape, dt, "random", guidance, eta, rho, beta, repeat=eta == 0.5)
                    if rho > 0.0 and shape[0] > 1:
                        assert (ref["s"] < 1.0).any() and (ref["s"] == 1.0).any(), "one clip clipped, one not"
                    if shape[2] * shape[3] * shape[1] > 2:
                        assert ((ref["p"].abs() > 0.02) & ((ref["p"] / ref["s"]).abs() < 0.98)).all(), "dt / tt is neither 0 nor 1"
        if shape[0] == 1:
            clipped = [reference(shape, dt, "random", 9.0, 0.0, rho, beta)["s"][0].item() < 1.0 for rho in rhos[1:]]
            assert clipped == [True, False], "|d| / 2 clips, 2 |d| does not"


@pytest.mark.gpu
def test_the_benchmark_shape(monkeypatch):
    """16 x 64 x 64 x 4 elements per clip, 128 workgroups: on the GPU backend only."""
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    monkeypatch.setattr(test_ddim_step, "DEV", "cuda")
    for beta in BETAS:
        for rho in thresholds(BENCH_SHAPE, torch.float16, "random", beta):
            check(BENCH_SHAPE, torch.float16, "random", 9.0, 0.0, rho, beta)


@DTYPES
def test_the_one_element_clip_with_eta_zero_returns_the_text_prediction(backend, dt):
    """n = 1: d is parallel to t whatever the values, so with eta = 0 the whole update is projected away."""
    shape = SHAPES[0]
    for beta in BETAS:
        for rho in thresholds(shape, dt, "random", beta):
            for guidance in GUIDANCES:
                ref, got, _ = check(shape, dt, "random", guidance, 0.0, rho, beta)
                t = valid(tokens_of(shape, dt).double(), shape, 1)
                assert (ref["e"] - t).abs().max().item() <= 1e-12 * t.abs().max().item()
                assert ((got.double() - t).abs() <= ref["err32"] + half_ulp(t.abs() + ref["err32"], dt)).all()


@DTYPES
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4]], ids=lambda s: "x".join(map(str, s)))
def test_a_parallel_update_is_scaled_by_eta(backend, shape, dt):
    """u = t / 2 clip-wide: d = t / 2 lies along t, so the result is t + (g - 1) eta (t - u)."""
    tok = tokens_of(shape, dt, "scaled").double()
    u, t = valid(tok, shape, 0), valid(tok, shape, 1)
    assert torch.equal(u, 0.5 * t)
    for guidance in GUIDANCES:
        for eta in ETAS:
            ref, got, stats = check(shape, dt, "scaled", guidance, eta, 0.0, 0.0)
            want = t + (guidance - 1.0) * eta * (t - u)
            assert (ref["e"] - want).abs().max().item() <= 1e-12 * want.abs().max().item() and (ref["p"] - 0.5).abs().max().item() <= 1e-12
            assert ((got.double() - want).abs() <= ref["err32"] + half_ulp(want.abs() + ref["err32"], dt)).all()
            assert (stats[:, 0] == 1.0).all() and (stats[:, 1].double() - 0.5).abs().max().item() <= ref["d_p"].max().item()


@DTYPES
def test_an_orthogonal_update_passes_for_every_eta(backend, dt):
    """t = (1, 0), u = (1, -1): d = (0, 1) is orthogonal to t, p = 0 exactly and the result is t + (g - 1) d = (1, g - 1), exact in
    both storage types, for every eta."""
    shape = SHAPES[1]
    for guidance in GUIDANCES:
        for eta in ETAS:
            ref, got, stats = check(shape, dt, "hand", guidance, eta, 0.0, 0.0)
            assert got.reshape(-1).tolist() == [1.0, guidance - 1.0] and stats.reshape(-1).tolist() == [1.0, 0.0]
        _, got, stats = check(shape, dt, "hand", guidance, 0.0, 0.5, 0.0)              # |d| = 1 clipped to 1/2
        assert got.reshape(-1).tolist() == [1.0, 0.5 * (guidance - 1.0)] and stats[0, 1] == 0.0     # (s = 1/2 is held to D_s by check)


@DTYPES
@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[7]], ids=lambda s: "x".join(map(str, s)))
def test_eta_one_without_threshold_and_momentum_is_plain_guidance(backend, shape, dt):
    tok = tokens_of(shape, dt).double()
    u, t = valid(tok, shape, 0), valid(tok, shape, 1)
    for guidance in GUIDANCES:
        ref, got, stats = check(shape, dt, "random", guidance, 1.0, 0.0, 0.0)
        want = u + guidance * (t - u)
        assert (ref["e"] - want).abs().max().item() <= 1e-12 * want.abs().max().item()
        assert ((got.double() - want).abs() <= ref["err32"] + half_ulp(want.abs() + ref["err32"], dt)).all()
        assert (stats[:, 0] == 1.0).all()


@DTYPES
def test_a_text_clip_of_zeros_has_no_parallel_part(backend, dt):
    shape = SHAPES[3]
    for beta in BETAS:
        for rho in thresholds(shape, dt, "zero_text", beta):
            ref, got, stats = check(shape, dt, "zero_text", 9.0, 0.0, rho, beta)
            assert (stats[:, 1] == 0.0).all() and torch.isfinite(got.float()).all() and (ref["p"] == 0.0).all()


@DTYPES
def test_equal_halves_return_the_text_prediction(backend, dt):
    """u = t: d = 0, dd = 0 gives s = 1 (no division by the zero norm) and the output is t's bits."""
    shape = SHAPES[3]
    t = valid(tokens_of(shape, dt, "equal"), shape, 1)
    for rho in (0.0, 1.0):
        for eta in ETAS:
            _, got, stats = check(shape, dt, "equal", 9.0, eta, rho, 0.0)
            assert torch.equal(got.view(torch.int16), t.contiguous().view(torch.int16))
            assert (stats[:, 0] == 1.0).all() and (stats[:, 1] == 0.0).all()


def test_refusals_leave_the_output_untouched(backend):
    clips, ch, frames, hw, ld = 2, 4, 3, 10, 8
    rows, dt, n = clips * (frames + 1) * hw, torch.float16, clips * frames * hw * ch
    d_ = dev()
    g = torch.Generator().manual_seed(5)
    arena = torch.randn(8 * rows * ld, generator=g).to(dt).to(d_)                   # one allocation: views of it can overlap
    before = arena.clone()
    e = arena.element_size()
    tokens, out = arena[:2 * rows * ld], arena[3 * rows * ld:4 * rows * ld]
    stats = torch.zeros(2 * clips, dtype=torch.float32).to(d_)
    mom = torch.zeros(n, dtype=torch.float32).to(d_)
    lib = _lib.get()

    def call(workspace="own", workspace_bytes=None, **kw):
        d = _lib.AaApg()
        t = dict(tokens=tokens, out=out, momentum_buf=mom, stats=stats)
        t.update({k: v for k, v in kw.items() if k in t})
        for k, v in t.items():
            setattr(d, k, None if v is None else C.c_void_p(v if isinstance(v, int) else v.data_ptr()))
        f = dict(clips=clips, channels=ch, frames=frames, hw=hw, ld=ld, out_ld=ld, guidance=9.0, eta=0.0, norm_threshold=2.0, momentum=-0.5,
                 dtype=_lib.AA_F16)
        f.update({k: v for k, v in kw.items() if k in f})
        for k, v in f.items():
            setattr(d, k, v)
        ws = torch.zeros(64, dtype=torch.float64).to(d_) if isinstance(workspace, str) else workspace
        ptr = None if ws is None else C.c_void_p(ws if isinstance(ws, int) else ws.data_ptr())
        nbytes = 512 if workspace_bytes is None else workspace_bytes
        return lib.aa_apg_tokens(C.byref(d), ptr, nbytes, ops._stream(arena)), lib.aa_apg_workspace(C.byref(d))

    shape_, dtype_, align_, workspace_ = -1, -2, -3, -4                             # AA_E_SHAPE, AA_E_DTYPE, AA_E_ALIGN, AA_E_WORKSPACE
    assert call(tokens=None)[1] == clips * 1 * 3 * 8                                # (the size query: one part per clip, three fp64 sums)
    assert call(channels=1, frames=1, hw=1, tokens=None)[1] == clips * 3 * 8        # n = 1 is legal
    assert lib.aa_apg_tokens(None, None, 0, None) == shape_ and lib.aa_apg_workspace(None) == 0
    for name in ("tokens", "out"):
        assert call(**{name: None})[0] == shape_, name
    assert b"null" in lib.aa_last_error()
    assert call(workspace=None)[0] == workspace_
    assert call(workspace_bytes=clips * 3 * 8 - 8)[0] == workspace_ and b"workspace" in lib.aa_last_error()
    for bad in (dict(clips=0), dict(channels=0), dict(frames=0), dict(hw=0), dict(clips=-1), dict(hw=-3), dict(clips=70000),
                dict(clips=4, hw=2 ** 27, frames=1),                                 # 2^31 token rows
                dict(ld=ch - 1), dict(out_ld=ch - 1)):
        assert call(**bad)[0] == shape_, bad
    for name in ("guidance", "eta", "norm_threshold", "momentum"):
        for v in (math.nan, math.inf, -math.inf):
            assert call(**{name: v})[0] == shape_, (name, v)
    for bad in (dict(norm_threshold=-0.5), dict(momentum=1.0), dict(momentum=-1.0), dict(momentum=1.5),
                dict(momentum_buf=None), dict(momentum=0.0)):                       # momentum without a buffer, a buffer without momentum
        assert call(**bad)[0] == shape_, bad
    overlapping = [dict(out=tokens.data_ptr() + 2 * e),                             # out over tokens, shifted
                   dict(out=tokens, out_ld=ld + 4),                                 # same pointer, another pitch
                   dict(out=tokens.data_ptr() + rows * ld * e),                     # the text half
                   dict(out=tokens.data_ptr() + ((2 * rows - 1) * ld + ch - 2) * e),  # the last two valid elements
                   dict(stats=tokens.data_ptr() + 64), dict(stats=out.data_ptr() + 64),
                   dict(momentum_buf=tokens.data_ptr() + 64), dict(momentum_buf=out.data_ptr() + 64),
                   dict(stats=mom.data_ptr() + 16), dict(momentum_buf=stats.data_ptr() - 4 * (n - 1)),
                   dict(workspace=tokens.data_ptr() + 64), dict(workspace=out.data_ptr() + 128),
                   dict(workspace=stats.data_ptr()), dict(workspace=mom.data_ptr() + 8)]
    for bad in overlapping:
        assert call(**bad)[0] == shape_, bad
        assert b"overlap" in lib.aa_last_error()
    assert call(tokens=tokens.data_ptr() + 1)[0] == align_ and call(out=out.data_ptr() + 1)[0] == align_
    assert call(stats=stats.data_ptr() + 2)[0] == align_ and call(momentum_buf=mom.data_ptr() + 2)[0] == align_
    assert call(workspace=torch.zeros(64, dtype=torch.float64).to(d_)[1:].view(torch.int32)[1:], workspace_bytes=256)[0] == align_
    assert call(dtype=_lib.AA_F32)[0] == dtype_ and call(dtype=7)[0] == dtype_
    assert torch.equal(arena.cpu().view(torch.int16), before.cpu().view(torch.int16)) and (stats.cpu() == 0).all() and (mom.cpu() == 0).all()
    # the wrapper: dtype, shape, layout and the entry point's own refusals
    tok2, out2 = tokens.view(2 * rows, ld), out.view(rows, ld)
    args = (clips, ch, frames, hw, 9.0, 0.0, 2.0)
    with pytest.raises(RuntimeError, match="token matrix"):
        ops.apg_tokens(tok2.float(), *args, 0.0)
    with pytest.raises(RuntimeError, match="token matrix"):
        ops.apg_tokens(tok2, *args, 0.0, out=out2.to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="token matrix"):
        ops.apg_tokens(tok2.t(), *args, 0.0)
    with pytest.raises(RuntimeError, match="rows"):
        ops.apg_tokens(tok2[:-1], *args, 0.0)                                       # a short token matrix
    with pytest.raises(RuntimeError, match="rows"):
        ops.apg_tokens(tok2, *args, 0.0, out=out2[:-1])
    with pytest.raises(RuntimeError, match="rows"):
        ops.apg_tokens(tok2, clips, ld + 1, frames, hw, 9.0, 0.0, 2.0, 0.0)         # more channels than columns
    with pytest.raises(RuntimeError, match="stats"):
        ops.apg_tokens(tok2, *args, 0.0, out=out2, stats=torch.zeros(2 * clips + 1).to(d_))
    with pytest.raises(RuntimeError, match="stats"):
        ops.apg_tokens(tok2, *args, 0.0, out=out2, stats=torch.zeros(2 * clips, dtype=torch.float64).to(d_))
    with pytest.raises(RuntimeError, match="momentum_buf"):
        ops.apg_tokens(tok2, *args, -0.5, out=out2, momentum_buf=torch.zeros(n - 1).to(d_))
    with pytest.raises(RuntimeError, match="momentum_buf"):
        ops.apg_tokens(tok2, *args, -0.5, out=out2, momentum_buf=torch.zeros(n, dtype=torch.float64).to(d_))
    for bad in ((9.0, 0.0, -1.0, 0.0), (math.inf, 0.0, 2.0, 0.0), (9.0, math.nan, 2.0, 0.0), (9.0, 0.0, 2.0, -0.5), (9.0, 0.0, 2.0, 1.0)):
        with pytest.raises(RuntimeError, match="libaa_mi355"):
            ops.apg_tokens(tok2, clips, ch, frames, hw, *bad, out=out2)             # (momentum without its buffer among them)
    with pytest.raises(RuntimeError, match="libaa_mi355"):
        ops.apg_tokens(tok2, *args, 0.0, out=out2, momentum_buf=mom)                # a buffer without momentum
    with pytest.raises(RuntimeError, match="libaa_mi355"):
        ops.apg_tokens(tok2, 0, ch, frames, hw, 9.0, 0.0, 2.0, 0.0, out=out2)
    with pytest.raises(RuntimeError, match="libaa_mi355"):
        ops.apg_tokens(tok2, *args, 0.0, out=tok2[rows // 2:rows // 2 + rows])      # overlap, through the wrapper
    assert torch.equal(arena.cpu().view(torch.int16), before.cpu().view(torch.int16)) and (mom.cpu() == 0).all()
    # and the valid call on the same views works, on a longer token matrix too; the workspace is kept per geometry
    longer = arena[:(2 * rows + 3) * ld].view(2 * rows + 3, ld)
    got = ops.apg_tokens(longer, *args, -0.5, momentum_buf=mom, out=out2, stats=stats)
    assert got is out2 and not torch.equal(out2.cpu(), before[3 * rows * ld:4 * rows * ld].view(rows, ld).cpu())
    assert (stats.cpu() != 0).all() and (mom.cpu() != 0).any()
    key = (str(tok2.device), clips, ch, frames, hw)
    ws = ops._APG_WS[key]
    ops.apg_tokens(tok2, *args, 0.0, out=out2)
    assert ops._APG_WS[key] is ws and ws.dtype == torch.float64
