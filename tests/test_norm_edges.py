"""Normalisation kernels in the regimes the random inputs of the other tests never reach - ops.groupnorm (one kernel, the statistics +
apply pair, two sources), ops.groupnorm_coef, ops.layernorm, the LayerNorm inside ff_fused / linear_rows / seq_self_attention and the
LayerNorm folded into a contraction (pack_weight(ln=...)), fp16 and bf16, two backends as in test_kernels.py:

  eps        rows / groups of spread 2^-8 around zero (variance ~1.6e-5, every value in the normal range of fp16) with eps 1e-5 and 1e-6: the
             output scale is sqrt(var / (var + eps)) = 0.79 / 0.97 - a kernel that drops eps gives 1.0;
  constant   constant rows / channel groups (0, -0.75 and 50.0: far from zero, the pivot centring) next to live ones: the normalised value is
             exactly 0, the output beta - through the rows kernels its image W beta + b (+ residual) - and finite;
  small      GroupNorm over 6 / 8 / 24 elements (tokens_per_group 1 / 3 x 2 / 8 channels per group: n against n - 1 is a 9 % scale error),
             LayerNorm at C = 64;
  unit       rows of ordinary spread, as a yardstick for the same rule.

References are float64 torch on the stored values.  The tolerance is the rule of test_kernels_bf16.accept():
    max|got - ref64| <= 2 max|model - ref64| + 2^-12 max(1, max|ref64|)
with `model` the textbook arithmetic ((x - mean) rstd gamma + beta) in float32, rounded to the storage type where the kernel documents a
16-bit value: the output; for the rows kernels the normalised row x~, W diag(gamma), q / k / v, P and ff_fused's value * gelu(gate); for the
folded LayerNorm the packed W diag(gamma), and there the model follows the re-association pack_weight(ln=...) documents (the un-centred
product, statistics from fp32 row sums) - what that costs on a constant row at 50.0 is the fold's documented arithmetic, not an error.  Every case asserts that its own bound stays below 5e-3 max(1, max|ref64|): the one-line errors
these cases are after (eps dropped, n - 1 or C - 8 in a variance) move the outputs by 1 % to 30 %.

Worst kernel error / model error per family (every case prints its own: `pytest -s`, lines "edge-ratio"; cases the model hits exactly -
constant rows - are decided by the floor and left out of the ratio):

  family                                   emulator   MI355X
  groupnorm (one kernel / pair / 2 src)    1.00           1.00
  groupnorm_coef (fp32 coefficients)       exact        exact
  layernorm                                1.00           1.00
  linear_rows                              1.00           1.00
  ff_fused                                 1.00           1.00
  seq_self_attention                       1.19          1.19
  folded LayerNorm                         1.00         1.14
"""
import math

import pytest
import torch

from animate_anything_amd import _lib, ops
from test_kernels import _ln_fold_consume

DTYPES = [torch.float16, torch.bfloat16]
FACTOR = 2.0
DEV = "cpu"
BACKEND = "emu"


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    global DEV, BACKEND
    BACKEND = request.param
    if request.param == "emu":
        DEV = "cpu"
        request.getfixturevalue("emu")
    else:
        assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
        DEV = "cuda"
    yield request.param
    DEV, BACKEND = "cpu", "emu"


def judge(got, ref, model, family, note=""):
    """The acceptance rule of the module docstring."""
    got, ref, model = got.detach().double().cpu(), ref.double(), model.double()
    assert got.shape == ref.shape == model.shape, (got.shape, ref.shape, model.shape)
    assert torch.isfinite(got).all(), f"{family} {note}: not finite"
    top = max(1.0, ref.abs().max().item())
    e_got, e_model = (got - ref).abs().max().item(), (model - ref).abs().max().item()
    bound = FACTOR * e_model + 2.0 ** -12 * top
    ratio = "exact model" if e_model < 2.0 ** -14 * top else f"{e_got / e_model:.3f}"
    print(f"edge-ratio | {family} | {BACKEND} | {ratio} | kernel {e_got:.4g} model {e_model:.4g} bound {bound:.4g} ref max {top:.4g} {note}")
    assert bound < 5e-3 * top, f"degenerate model: bound {bound} (ref max {top})"
    assert e_got <= bound, f"{family} {note}: kernel error {e_got} > {bound} = {FACTOR} x model error {e_model} + floor (ref max {top})"


def both(fn, dtype, out_16=True):
    """fn(dtype, round) -> the operation: ref64 = fn(float64, identity), model = fn(float32, rounding to `dtype`) (+ the output rounding)."""
    rd = lambda t: t.to(dtype).to(t.dtype)
    ref, model = fn(torch.float64, lambda t: t), fn(torch.float32, rd)
    return ref, (rd(model) if out_16 else model)


def gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc


def affine(r, C, dtype):
    """gamma ~ 0.1, beta ~ 0.1, clamped: |n| gamma + |beta| stays below 1 for |n| <= 4.6, so max(1, max|ref|) = 1 and bf16's own output rounding
    (2^-9 below 1, 2^-8 from 1 on) leaves the bound of the rule below 5e-3."""
    return (0.1 * (1.0 + 0.3 * r(C)).clamp(0.4, 1.6)).to(dtype), (0.1 * r(C)).clamp(-0.25, 0.25).to(dtype)


def tiny_spread(r, *shape):
    """Spread 2^-8 around zero, every magnitude in [2^-9, 3 * 2^-9] (normal fp16 numbers): variance ~1.6e-5."""
    u = r(*shape)
    return u.sign() * (0.5 + u.abs().fmod(1.0)) * 2.0 ** -8


# ===================================================================================================== GroupNorm
def gn_input(regime, n_img, tokens, C, groups, dtype, seed):
    """[n_img * tokens, C] stored values.  constant: every third channel group of an image group is constant (50.0 / -0.75 / 0.0 by image
    group), its neighbours live."""
    r = gen(seed)
    cg = C // groups
    if regime == "eps":
        x = tiny_spread(r, n_img, tokens, C)
    else:
        x = r(n_img, tokens, C) * 1.5 + 0.3
        if regime == "constant":
            for i in range(n_img):
                for gi in range(1, groups, 3):
                    x[i, :, gi * cg:(gi + 1) * cg] = (50.0, -0.75, 0.0)[i % 3]
    return x.reshape(n_img * tokens, C).to(dtype)


def gn_stats(x, n_img, tokens, groups, dt, eps):
    """x [n_img * tokens, C] -> per-element mean and rstd, textbook two-pass arithmetic in `dt`."""
    C = x.shape[1]
    xg = x.detach().cpu().to(dt).reshape(n_img, tokens, groups, C // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    expand = lambda t: t.expand_as(xg).reshape(n_img * tokens, C)
    return expand(mean), expand(1.0 / torch.sqrt(var + eps))


GN_SHAPES = [   # (n_img, tokens, C, groups, c1)
    (3, 37, 64, 8, 0), (3, 37, 64, 32, 0), (3, 37, 64, 32, 24), (2, 300, 320, 32, 0),
]
GN_SMALL = [(5, 1, 64, 32, 0), (5, 3, 64, 32, 0), (5, 1, 64, 8, 0), (5, 3, 64, 8, 0), (4, 3, 64, 32, 24)]


def run_groupnorm(x, gamma, beta, n_img, tokens, groups, eps, c1, two_pass):
    C = x.shape[1]
    xd = x.to(DEV)
    x0, x1 = (xd, None) if c1 == 0 else (xd[:, :C - c1].contiguous(), xd[:, C - c1:].contiguous())
    lib = _lib.get()
    ops.GN_PLANS = []
    tune, ops.AUTOTUNE = ops.AUTOTUNE, False
    lib.aa_set_groupnorm_two_pass(int(two_pass))
    try:
        y = ops.groupnorm(x0, gamma.to(DEV), beta.to(DEV), n_img, tokens, groups, eps=eps, silu=False, x1=x1)
    finally:
        lib.aa_set_groupnorm_two_pass(0)
        ops.AUTOTUNE = tune
        plans, ops.GN_PLANS = ops.GN_PLANS, None
    assert (plans[0] is None) == two_pass, plans              # the form the case is about did run
    return y


def gn_case(regime, shape, eps, dtype, two_pass, seed):
    n_img, tokens, C, groups, c1 = shape
    x = gn_input(regime, n_img, tokens, C, groups, dtype, seed)
    r = gen(seed + 1)
    gamma, beta = affine(r, C, dtype)

    def fn(dt, rd):
        mean, rstd = gn_stats(x, n_img, tokens, groups, dt, eps)
        return (x.to(dt) - mean) * rstd * gamma.to(dt) + beta.to(dt)

    ref, model = both(fn, dtype)
    y = run_groupnorm(x, gamma, beta, n_img, tokens, groups, eps, c1, two_pass)
    note = f"{regime} {shape} eps {eps} {dtype} {'pair' if two_pass else 'one kernel'}"
    judge(y, ref, model, "groupnorm", note)
    if regime == "eps":                                        # the regime is the one meant: eps carries 3 % .. 21 % of the scale
        mean, rstd = gn_stats(x, n_img, tokens, groups, torch.float64, 0.0)
        mean, rstd_eps = gn_stats(x, n_img, tokens, groups, torch.float64, eps)
        assert (rstd_eps / rstd).max().item() < (0.98 if eps < 5e-6 else 0.82)
    if regime == "constant":                                   # var = 0: exactly beta (to the floor of the rule), on its own
        cg = C // groups
        yy = y.double().cpu().reshape(n_img, tokens, C)
        for gi in range(1, groups, 3):
            sl = slice(gi * cg, (gi + 1) * cg)
            want = beta.double()[sl].expand(n_img, tokens, cg)
            judge(yy[:, :, sl], want, want, "groupnorm", note + f" constant group {gi}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("two_pass", [False, True])
@pytest.mark.parametrize("shape", GN_SHAPES)
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_groupnorm_eps_matters(backend, eps, shape, two_pass, dtype):
    gn_case("eps", shape, eps, dtype, two_pass, 301)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("two_pass", [False, True])
@pytest.mark.parametrize("shape", GN_SHAPES)
def test_groupnorm_constant_groups(backend, shape, two_pass, dtype):
    gn_case("constant", shape, 1e-5, dtype, two_pass, 311)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("two_pass", [False, True])
@pytest.mark.parametrize("shape", GN_SMALL)
def test_groupnorm_small_counts(backend, shape, two_pass, dtype):
    gn_case("unit", shape, 1e-5, dtype, two_pass, 321)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("regime,shape,eps", [("eps", GN_SHAPES[1], 1e-5), ("eps", GN_SHAPES[3], 1e-6), ("constant", GN_SHAPES[0], 1e-5),
                                              ("unit", GN_SMALL[1], 1e-5), ("unit", GN_SMALL[2], 1e-5)])
def test_groupnorm_coef_edges(backend, regime, shape, eps, dtype):
    """The fp32 (scale, shift) per channel that linear_rows(affine=...) applies: scale = gamma rstd, shift = beta - mean scale."""
    n_img, tokens, C, groups, _ = shape
    x = gn_input(regime, n_img, tokens, C, groups, dtype, 331)
    r = gen(332)
    gamma, beta = (1.0 + 0.3 * r(C)).to(dtype), r(C).to(dtype)

    def fn(dt, rd):
        mean, rstd = gn_stats(x, n_img, tokens, groups, dt, eps)
        mean, rstd = mean.reshape(n_img, tokens, C)[:, 0], rstd.reshape(n_img, tokens, C)[:, 0]
        sc = rstd * gamma.to(dt)
        return torch.stack([sc, beta.to(dt) - mean * sc], dim=1)

    ref, model = both(fn, dtype, out_16=False)
    coef = ops.groupnorm_coef(x.to(DEV), gamma.to(DEV), beta.to(DEV), n_img, tokens, groups, eps)
    judge(coef[:, 0], ref[:, 0], model[:, 0], "groupnorm_coef", f"scale {regime} {shape} eps {eps} {dtype}")
    judge(coef[:, 1], ref[:, 1], model[:, 1], "groupnorm_coef", f"shift {regime} {shape} eps {eps} {dtype}")


# ===================================================================================================== LayerNorm rows
def ln_rows(regime, rows, C, dtype, seed, live=(1.5, 0.3), far=50.0):
    """[rows, C] stored values.  constant: rows 1, 5, 9, .. hold `far`, rows 2, 6, .. -0.75, rows 3, 7, .. 0.0; the others are live
    (`live` = their spread and mean: a LayerNorm does not care, a kernel that adds x to its output does)."""
    r = gen(seed)
    if regime == "eps":
        return tiny_spread(r, rows, C).to(dtype)
    x = r(rows, C) * live[0] + live[1]
    if regime == "constant":
        x[1::4], x[2::4], x[3::4] = far, -0.75, 0.0
    return x.to(dtype)


def ln_norm(x, dt, eps):
    """(x - mean) rstd per row, two-pass arithmetic in `dt`."""
    xf = x.detach().cpu().to(dt)
    mean = xf.mean(dim=1, keepdim=True)
    var = ((xf - mean) ** 2).mean(dim=1, keepdim=True)
    return (xf - mean) / torch.sqrt(var + eps)


def constant_rows(regime, rows):
    return [i for i in range(rows) if i % 4] if regime == "constant" else []


REGIMES = [("eps", 1e-5), ("eps", 1e-6), ("constant", 1e-5), ("unit", 1e-5)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [64, 320])
@pytest.mark.parametrize("regime,eps", REGIMES)
def test_layernorm_edges(backend, regime, eps, C, dtype):
    rows = 11
    x = ln_rows(regime, rows, C, dtype, 341)
    r = gen(342)
    gamma, beta = affine(r, C, dtype)
    ref, model = both(lambda dt, rd: ln_norm(x, dt, eps) * gamma.to(dt) + beta.to(dt), dtype)
    y = ops.layernorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), eps)
    note = f"{regime} C {C} eps {eps} {dtype}"
    judge(y, ref, model, "layernorm", note)
    for i in constant_rows(regime, rows):
        judge(y[i], beta.double(), beta.double(), "layernorm", note + f" constant row {i}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,n_out", [(130, 320), (37, 64)])
@pytest.mark.parametrize("regime,eps", REGIMES)
def test_linear_rows_layernorm_edges(backend, regime, eps, rows, n_out, dtype):
    """LayerNorm(x) W^T + b + residual; a constant row gives exactly the image of beta, W beta + b, rounded, + residual, rounded."""
    C = 320
    x = ln_rows(regime, rows, C, dtype, 351)
    r = gen(352)
    w, b, res = r(n_out, C, sc=0.06 * C ** -0.5).to(dtype), r(n_out, sc=0.02).to(dtype), r(rows, n_out, sc=0.02).to(dtype)      # (|output| < 0.5: two 16-bit roundings, see affine())
    gamma, beta = (1.0 + 0.3 * r(C)).to(dtype), (0.2 * r(C)).to(dtype)

    def fn(dt, rd):        # (linear_rows.h: the residual is added to the ROUNDED product)
        xn = rd(ln_norm(x, dt, eps))
        wg = rd(w.to(dt) * gamma.to(dt)[None, :])
        return rd(xn @ wg.t() + (w.to(dt) @ beta.to(dt) + b.to(dt))) + res.to(dt)

    ref, model = both(fn, dtype)
    to = lambda t: t.to(DEV)
    pk = ops.pack_linear_rows(to(w), to(b), ln=(to(gamma), to(beta), eps))
    assert ops.linear_rows_ok(C, n_out, rows, dtype)
    y = ops.linear_rows(to(x), pk, to(res))
    note = f"{regime} rows {rows} n_out {n_out} eps {eps} {dtype}"
    judge(y, ref, model, "linear_rows", note)
    image = w.double() @ beta.double() + b.double()
    for i in constant_rows(regime, rows)[:12]:
        want = image + res[i].double()
        judge(y[i], want, (image.to(dtype).double() + res[i].double()).to(dtype).double(), "linear_rows", note + f" constant row {i}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("regime,eps", REGIMES)
def test_ff_fused_layernorm_edges(backend, regime, eps, dtype):
    """GEGLU(LayerNorm(x) W1^T + b1) W2^T + b2 + x (no proj_out: the second product's weights are W2 itself)."""
    C, rows = 320, 45
    # x is part of the output: live rows of spread 0.05 (still 250 x eps in variance) keep it below 0.5 (two 16-bit roundings: see affine()); the far constant is 60.0 here,
    # in the upper half of its binade - at 50.0 bf16's own rounding of the output (2^-3 at 50) would put the bound of the rule past 5e-3
    x = ln_rows(regime, rows, C, dtype, 361, live=(0.05, 0.01), far=60.0)
    r = gen(362)
    w1, b1 = r(8 * C, C, sc=C ** -0.5).to(dtype), r(8 * C, sc=0.2).to(dtype)
    w2, b2 = r(C, 4 * C, sc=0.15 * (4 * C) ** -0.5).to(dtype), r(C, sc=0.02).to(dtype)
    gamma, beta = (1.0 + 0.3 * r(C)).to(dtype), (0.2 * r(C)).to(dtype)

    def fn(dt, rd):
        xn = rd(ln_norm(x, dt, eps))
        wg = rd(w1.to(dt) * gamma.to(dt)[None, :])
        y = xn @ wg.t() + (w1.to(dt) @ beta.to(dt) + b1.to(dt))
        val, gate = y.chunk(2, dim=-1)
        h = rd(val * gate * 0.5 * (1.0 + torch.erf(gate / math.sqrt(2.0))))
        return h @ w2.to(dt).t() + b2.to(dt) + x.to(dt)

    ref, model = both(fn, dtype)
    to = lambda t: t.to(DEV)
    pk = ops.pack_ff_fused(to(w1), to(b1), to(w2), to(b2), ln=(to(gamma), to(beta), eps))
    assert ops.ff_fused_ok(C, rows, dtype)
    y = ops.ff_fused(to(x), pk)
    note = f"{regime} eps {eps} {dtype}"
    judge(y, ref, model, "ff_fused", note)
    for i in constant_rows(regime, rows)[:6]:
        judge(y[i], ref[i], model[i], "ff_fused", note + f" constant row {i}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("regime,eps", REGIMES)
def test_seq_self_attention_layernorm_edges(backend, regime, eps, dtype):
    """softmax(q k^T / 8) v with [q | k | v] = LayerNorm(x) W^T over 17 frames x 9 pixels (a tile with idle waves, sequences that straddle the
    32-row blocks).  Constant rows all normalise to 0: their q / k / v are W beta."""
    C, clips, frames, hw = 320, 1, 17, 9
    heads, rows = C // 64, clips * frames * hw
    x = ln_rows(regime, rows, C, dtype, 371)
    r = gen(372)
    wq, wk, wv = r(C, C, sc=C ** -0.5).to(dtype), r(C, C, sc=C ** -0.5).to(dtype), r(C, C, sc=0.08 * C ** -0.5).to(dtype)      # (|v| < 0.5: see affine())
    gamma, beta = (1.0 + 0.3 * r(C)).to(dtype), (0.2 * r(C)).to(dtype)

    def fn(dt, rd):
        xn = rd(ln_norm(x, dt, eps))

        def proj(w):
            wg = rd(w.to(dt) * gamma.to(dt)[None, :])
            return rd(xn @ wg.t() + w.to(dt) @ beta.to(dt)).reshape(clips, frames, hw, heads, 64).permute(0, 2, 3, 1, 4)

        q, k, v = proj(wq), proj(wk), proj(wv)
        s = rd(q * (0.125 * math.log2(math.e))) @ k.transpose(-1, -2)
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        o = (rd(p) @ v) / p.sum(-1, keepdim=True)
        return o.permute(0, 3, 1, 2, 4).reshape(rows, C)

    ref, model = both(fn, dtype)
    to = lambda t: t.to(DEV)
    pk = ops.pack_seq_qkv(to(wq), to(wk), to(wv), ln=(to(gamma), to(beta), eps))
    assert ops.seq_self_attention_ok(C, frames, rows, dtype)
    y = ops.seq_self_attention(to(x), pk, clips, hw, frames, (frames * hw, 1, hw))
    judge(y, ref, model, "seq_self_attention", f"{regime} eps {eps} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("regime,eps", [("eps", 1e-5), ("constant", 1e-5)])
def test_folded_layernorm_edges(backend, regime, eps, raw, dtype):
    """pack_weight(ln=...): the producing contraction (tile 49: its tile spans the 320-channel row) leaves the row sums of what it stores, the
    consumer (tile 39) folds the LayerNorm - from the raw sums (`raw`) or from aa_ln_finalize's coefficients.  The rows are produced as
    x = 0 W0^T + residual, so the stored rows are the regime's rows exactly."""
    M, C, N = 130, 320, 320
    x = ln_rows(regime, M, C, dtype, 381)
    r = gen(382)
    w1, b1 = r(N, C, sc=0.008).to(dtype), r(N, sc=0.1).to(dtype)                  # (|output| < 1: see affine())
    gamma, beta = (1.0 + 0.3 * r(C)).to(dtype), (0.2 * r(C)).to(dtype)
    to = lambda t: t.to(DEV)
    ops.FORCE_TILE = 49
    try:
        y, st = ops.conv_gemm(torch.zeros(M, 64, dtype=dtype, device=DEV), ops.pack_weight(torch.zeros(C, 64, dtype=dtype, device=DEV)), ops.linear_geom(M),
                              residual=to(x), row_stats=True)
    finally:
        ops.FORCE_TILE = -1
    assert st is not None and st.data is not None and torch.equal(y.cpu(), x)
    z = _ln_fold_consume(y, st, ops.pack_weight(to(w1), to(b1), ln=(to(gamma), to(beta), eps)), 39, raw)

    def fn(dt, rd):
        """ref64: the LayerNorm, then the product.  model: the arithmetic pack_weight(ln=...) documents, in float32 - the UN-centred product
        x W'^T, row sums and E[x^2] - E[x]^2 in fp32, rstd (x W'^T - mean colsum(W')) + (b + W beta) - on the packed (rounded) W'."""
        wg = rd(w1.to(dt) * gamma.to(dt)[None, :])
        if dt == torch.float64:
            return ln_norm(x, dt, eps) @ wg.t() + (w1.to(dt) @ beta.to(dt) + b1.to(dt))
        xf = x.to(dt)
        mean = xf.sum(1, keepdim=True) / C
        var = ((xf * xf).sum(1, keepdim=True) / C - mean * mean).clamp_min(0.0)
        return (xf @ wg.t() - mean * wg.sum(1)[None, :]) / torch.sqrt(var + eps) + (w1.to(dt) @ beta.to(dt) + b1.to(dt))

    ref, model = both(fn, dtype)
    judge(z, ref, model, "folded LayerNorm", f"{regime} eps {eps} raw {raw} {dtype}")
