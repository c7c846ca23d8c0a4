"""The transfer curve of every fused activation, point by point: a sweep of ~4000 stored values over [-12, 12] (dense in [-4, 4], plus
+-0 and the clamp points +-8 of the GELU fit) goes through each place an activation lives, and every output element is compared with
float64  x Phi(x) (erf GELU),  x sigma(x) (SiLU),  x sigma(1.702 x) (quick GELU)  of the stored input.  Two backends as in test_kernels.py.

Per-element bound (nothing measured goes into it):
    half an ulp of the storage type at the result (the one store rounding; ff_fused documents two: h = value * gelu(gate), then the sum)
  + 2^-21 |result|                                   (__expf / exp2 / rcp and the handful of fp32 operations around them)
  + 2.6e-5 max(1, |x|)                               GELU only: the bound csrc/kernels/conv_gemm.h claims for its sigmoid-of-a-quintic fit
                                                     (in float64 the fit's own error is 2.52e-5, at x = -2.07),
    times |value| where the GELU is a gate (GEGLU, ff_fused: value = gate = x)
  + 1.1 * 4e-6 max(1, |n|)                           GroupNorm only: the normalised value n is formed in fp32 from fp32 statistics
                                                     (|d silu / dn| <= 1.1).
A slope that is 3 % off or a fit coefficient moved in its third digit miss this by two to three orders of magnitude.

Worst error / bound over every element, in brackets the largest share of the allowance - the bound without the store rounding - that an
element used (each case prints its own: `pytest -s`, lines "act-curve"):

  place                                   emulator   MI355X
  blend SiLU / GELU / quick GELU          1.000 (0.94)    1.000 (0.94)
  conv_gemm SiLU epilogue                 1.000 (0.00)     1.000 (0.20)
  GEGLU epilogue (gelu_erf_f, _2)         0.997 (0.89)    0.997 (0.89)
  groupnorm(silu=True), both forms        0.993 (-0.00)      0.993 (-0.00)
  ff_fused (the GELU in three parts)      0.995 (0.91)       0.995 (0.91)
"""
import math

import pytest
import torch

from animate_anything_amd import _lib, ops
from animate_anything_amd._lib import AA_ACT_GELU, AA_ACT_QUICK_GELU, AA_ACT_SILU

DTYPES = [torch.float16, torch.bfloat16]
GELU_FIT = 2.6e-5          # conv_gemm.h: "|error| <= 2.6e-5 absolute over the whole real line"


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    if request.param == "emu":
        request.getfixturevalue("emu")
        yield "cpu"
    else:
        assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
        yield "cuda"


def sweep(dtype, n):
    """`n` stored values: 3/4 of them evenly over [-4, 4], the rest evenly over [-12, 12], then +-0, +-8 and the largest normal steps around
    them; shuffled (seeded), so that no tile, lane or group sees a monotone ramp."""
    special = torch.tensor([0.0, -0.0, 8.0, -8.0, 7.99, -7.99, 8.01, -8.01, 12.0, -12.0, 2.0 ** -14, -2.0 ** -14], dtype=torch.float64)
    m = n - special.numel()
    dense = torch.linspace(-4.0, 4.0, 3 * m // 4, dtype=torch.float64)
    wide = torch.linspace(-12.0, 12.0, m - dense.numel(), dtype=torch.float64)
    x = torch.cat([dense, wide, special])
    return x[torch.randperm(n, generator=torch.Generator().manual_seed(7))].to(dtype)


def half_ulp(ref, dtype):
    """Half the spacing of `dtype` at |ref| (float64 tensor), subnormal range included."""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return 0.5 * torch.exp2(e - mant)


CURVES = {
    AA_ACT_SILU: lambda x: x * torch.sigmoid(x),
    AA_ACT_GELU: lambda x: x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))),
    AA_ACT_QUICK_GELU: lambda x: x * torch.sigmoid(1.702 * x),
}


def check(got, ref, rounding, allowance, what, dev):
    """|got - ref| <= rounding + allowance per element; prints the worst error / bound, and the worst share of the allowance (the part of
    the bound that is not the store rounding) that an element used: (error - rounding) / allowance."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err = (got - ref).abs()
    ratio = err / (rounding + allowance)
    used = ((err - rounding) / allowance.clamp_min(1e-300)).max().item()
    worst = ratio.argmax().item()
    print(f"act-curve | {what} | {'emu' if dev == 'cpu' else 'gpu'} | worst error/bound {ratio.reshape(-1)[worst].item():.4f} "
          f"(error {err.reshape(-1)[worst].item():.3g}, expected {ref.reshape(-1)[worst].item():.6g}) | allowance used {used:.3f}")
    assert (ratio <= 1.0).all(), (f"{what}: {int((ratio > 1.0).sum())} elements beyond the bound, worst {ratio.max().item():.6g}x at expected "
                                  f"{ref.reshape(-1)[worst].item()!r}; allowance used {used:.3g}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", [AA_ACT_SILU, AA_ACT_GELU, AA_ACT_QUICK_GELU])
def test_blend_activation_curve(backend, act, dtype):
    x = sweep(dtype, 63 * 64).reshape(63, 64)
    xd = x.double()
    ref = CURVES[act](xd)
    allow = 2.0 ** -21 * ref.abs() + (GELU_FIT * xd.abs().clamp_min(1.0) if act == AA_ACT_GELU else 0.0)
    check(ops.blend(x.to(backend), act=act), ref, half_ulp(ref, dtype), allow, f"blend act {act} {dtype}", backend)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_gemm_silu_curve(backend, dtype):
    """Identity weights, K = N = 64: the accumulator is the stored x exactly."""
    x = sweep(dtype, 63 * 64).reshape(63, 64)
    y = ops.conv_gemm(x.to(backend), ops.pack_weight(torch.eye(64, dtype=dtype, device=backend)), ops.linear_geom(63), act=AA_ACT_SILU)
    ref = CURVES[AA_ACT_SILU](x.double())
    check(y, ref, half_ulp(ref, dtype), 2.0 ** -21 * ref.abs(), f"conv_gemm silu {dtype}", backend)


def geglu_tiles(D, rows, dtype):
    """One tile id per kernel family that takes a [rows, D] x [2 D, D] GEGLU call: {family name: tile}.  Families by aa_conv_gemm_tile_flags:
    compiled tiles (general epilogue: gelu_erf_f), the DMA schedules with the branch-free epilogue (gelu_erf_2), the hand-scheduled stream."""
    x = torch.zeros(rows, D, dtype=dtype)
    pw = ops.pack_weight(torch.zeros(2 * D, D, dtype=dtype), geglu=True)
    d = ops._conv_gemm_desc(x, pw, ops.linear_geom(rows))[0]
    fam = {}
    for tile, _ in ops._tile_candidates(d, rows):
        fam.setdefault(ops.TILE_TABLE.flags(tile), tile)
    return fam


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 192])
def test_geglu_curve(backend, D, dtype):
    """W = [I; I]: value = gate = x, the output is x * gelu(x) rounded once - at the automatic tile and at one tile of every kernel family
    that offers itself for the shape (D = 192: the wide value / gate pairing)."""
    n = 63 * 64 if D == 64 else 21 * 192
    x = sweep(dtype, n).reshape(-1, D)
    rows = x.shape[0]
    eye = torch.eye(D, dtype=dtype, device=backend)
    pw = ops.pack_weight(torch.cat([eye, eye]), geglu=True)
    xd = x.double()
    ref = xd * CURVES[AA_ACT_GELU](xd)
    allow = 2.0 ** -21 * ref.abs() + xd.abs() * GELU_FIT * xd.abs().clamp_min(1.0)
    fam = geglu_tiles(D, rows, dtype)
    assert len(fam) >= 2, fam                                 # compiled and hand-scheduled tiles at the least
    for flags, tile in [(None, -1)] + sorted(fam.items()):
        ops.FORCE_TILE = tile
        try:
            y = ops.conv_gemm(x.to(backend), pw, ops.linear_geom(rows))
        finally:
            ops.FORCE_TILE = -1
        check(y, ref, half_ulp(ref, dtype), allow, f"geglu D {D} tile {tile} (family flags {flags}) {dtype}", backend)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("two_pass", [False, True])
def test_groupnorm_silu_curve(backend, two_pass, dtype):
    """gamma = 1, beta = 0, one group of 64 channels; the sweep is padded with zeros and standardised in float64 so that the group has mean 0
    and variance 1 (to storage rounding) - the normalised values cover the sweep's range.  The reference takes the statistics of the STORED
    group in float64."""
    C, eps = 64, 1e-6
    s = sweep(dtype, 63 * 64).double()
    tokens = int(math.ceil((s * s).sum().item() / C)) + 1
    assert tokens <= 1024
    g = torch.zeros(tokens * C, dtype=torch.float64)
    g[torch.randperm(tokens * C, generator=torch.Generator().manual_seed(8))[:s.numel()]] = s
    g = (g - g.mean()) / g.var(unbiased=False).sqrt()
    x = g.to(dtype).reshape(tokens, C)
    xd = x.double()
    n = (xd - xd.mean()) / (xd.var(unbiased=False) + eps).sqrt()
    assert n.min().item() < -11.0 and n.max().item() > 11.0 and abs(xd.var(unbiased=False).item() - 1.0) < 1e-2
    ref = CURVES[AA_ACT_SILU](n)
    allow = 2.0 ** -21 * ref.abs() + 1.1 * 4e-6 * n.abs().clamp_min(1.0)
    ones, zeros = torch.ones(C, dtype=dtype, device=backend), torch.zeros(C, dtype=dtype, device=backend)
    lib = _lib.get()
    tune, ops.AUTOTUNE = ops.AUTOTUNE, False
    ops.GN_PLANS = []
    lib.aa_set_groupnorm_two_pass(int(two_pass))
    try:
        y = ops.groupnorm(x.to(backend), ones, zeros, 1, tokens, 1, eps=eps, silu=True)
    finally:
        lib.aa_set_groupnorm_two_pass(0)
        ops.AUTOTUNE = tune
        plans, ops.GN_PLANS = ops.GN_PLANS, None
    assert (plans[0] is None) == two_pass, plans               # the form the case is about did run
    check(y, ref, half_ulp(ref, dtype), allow, f"groupnorm silu two_pass {two_pass} {dtype}", backend)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ff_fused_gelu_curve(backend, dtype):
    """No LayerNorm, no proj_out, no biases; W1's value and gate rows select channel j mod C, W2 the first C hidden units:
    out = round(round(x * gelu(x)) + x) - the GELU of ff_fused.h, evaluated in three parts between the matrix passes."""
    C, rows = 320, 13
    x = sweep(dtype, rows * C).reshape(rows, C)
    sel = torch.eye(C, dtype=dtype).repeat(4, 1)                                    # [4 C, C]: hidden unit j reads channel j mod C
    w1 = torch.cat([sel, sel])
    w2 = torch.zeros(C, 4 * C, dtype=dtype)
    w2[:, :C] = torch.eye(C, dtype=dtype)
    to = lambda t: t.to(backend)
    pk = ops.pack_ff_fused(to(w1), None, to(w2), None)
    assert ops.ff_fused_ok(C, rows, dtype)
    y = ops.ff_fused(to(x), pk)
    xd = x.double()
    h = xd * CURVES[AA_ACT_GELU](xd)
    ref = h + xd
    allow = 2.0 ** -21 * h.abs() + xd.abs() * GELU_FIT * xd.abs().clamp_min(1.0)
    check(y, ref, half_ulp(h, dtype) + half_ulp(ref, dtype), allow, f"ff_fused gelu {dtype}", backend)
