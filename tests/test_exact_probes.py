"""Probes whose correct output is exactly representable, so that a one-term error shows (two backends as in test_kernels.py):

contractions   integer activations in {-2 .. 2}, weights in {-1, 0, 1}, small integer bias / residual / row vector, out_scale 1 or 0.5: every
               product and every fp32 partial sum is an integer far below 2^24 and the result fits the storage type - asserted first, on the
               CPU in float64 (|output| and every prefix sum along K <= 2048 in fp16, <= 256 in bf16; the result survives the cast) - so the kernel
               must return the float64 result BIT FOR BIT (torch.equal).  ops.conv_gemm in every form and at every tile the library offers for the
               shape, ops.linear_rows, and the `pre` projection of ops.seq_self_attention.
selector       attention whose keys are distinct +-1 codes, q_i = c * code(pi(i)), V integer in [-8, 8]: the matching key leads every other by
               >= 30 bits (asserted on float64 scores), the output is row v[pi(i)] to 2 ulp of the storage type (2^-9 |v| fp16, 2^-6 |v| bf16: one
               rounding of P while the lazy maximum lags, and the output rounding) plus what the other keys can weigh at the asserted lead
               (keys * 2^-(lead - 1) * 8: 1e-7).  Exact addressing: column offsets, row strides, heads, kv_outer_div, kv_seq_mod, temporal
               strides, causal masks, ragged query and key tails - every launch form of test_kernels_bf16.attn_form, and seq_self_attention.
counting       q = 0: every p is exactly 1; v_j[d] = (j % D == d), so the output is count_d / L (causal: L = i + 1) to 1 ulp.  A key dropped or
               counted twice moves a count by one; for seq_self_attention (Wq = 0) so does a row leaking in from the neighbouring sequence.
softmax_rows   a row whose last column carries half the mass, against float64, per element.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from animate_anything_amd import ops
from test_kernels import X_TILES, nhwc
from test_kernels_bf16 import attn_form, flagged

DTYPES = [torch.float16, torch.bfloat16]
DEV = "cpu"
LOG2E = 1.4426950408889634


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


def limit(dtype):
    return 2048.0 if dtype == torch.float16 else 256.0


class Ints:
    """Seeded integer-valued tensors (float64 on the CPU; .to(dtype) is exact)."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def act(self, *shape):                                   # {-2 .. 2}
        return torch.randint(-2, 3, shape, generator=self.g).double()

    def weight(self, *shape, density=2.0 / 3.0):             # {-1, 0, 1}
        return torch.randint(-1, 2, shape, generator=self.g).double() * (torch.rand(shape, generator=self.g) < density * 1.5).double()

    def small(self, *shape, top=3):                          # {-top .. top}
        return torch.randint(-top, top + 1, shape, generator=self.g).double()


def density(K, dtype):
    """Share of non-zero weights: bf16 holds integers to 256 only, so long K loops get sparser weights (still in {-1, 0, 1})."""
    return 2.0 / 3.0 if dtype == torch.float16 or K <= 320 else 0.25


def exact_precondition(ref, dtype, a=None, w=None):
    """|ref| within the integer range of the storage type and unchanged by the cast; with the im2col matrix `a` [M, K] and `w` [N, K]: every
    prefix sum along K within it too (a partial sum of any K split is the difference of two of them: below 2^24 in fp32 by a wide margin)."""
    assert ref.abs().max().item() <= limit(dtype), ref.abs().max().item()
    assert torch.equal(ref.to(dtype).double(), ref), "the expected result is not representable"
    if a is not None:
        step = 64
        acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float64)
        for k in range(0, a.shape[1], step):
            acc += a[:, k:k + step] @ w[:, k:k + step].t()
            assert acc.abs().max().item() <= limit(dtype), (k, acc.abs().max().item())


def tiles_for(x0, pw, g, **kw):
    """Every (tile, K splits) pair ops._tile_candidates offers for this call, after the automatic choice (-1, 0)."""
    d = ops._conv_gemm_desc(x0, pw, g, **kw)[0]
    return [(-1, 0)] + list(ops._tile_candidates(d, g.rows))


def run_tiles(x0, pw, g, ref, dtype, what, **kw):
    """The call at every offered tile: bit-equal to `ref` (float64) cast to the output type."""
    want = ref.to(kw.get("out_dtype") or dtype)
    ran = 0
    for tile, splits in tiles_for(x0, pw, g, **{k: v for k, v in kw.items() if k != "out"}):
        ops.FORCE_TILE, ops.K_SPLITS = tile, splits
        try:
            y = ops.conv_gemm(x0, pw, g, **kw)
        finally:
            ops.FORCE_TILE, ops.K_SPLITS = -1, 0
        bad = (y.cpu() != want).nonzero()
        assert bad.numel() == 0, f"{what} tile {tile} splits {splits}: {bad.shape[0]} elements differ, first {bad[0].tolist()}: got {y.cpu()[tuple(bad[0])].item()} want {want[tuple(bad[0])].item()}"
        ran += 1
    return ran


def dev(t, dtype):
    return None if t is None else t.to(dtype).to(DEV)


# ===================================================================================================== contractions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,N", [(300, 320, 320), (130, 64, 192), (70, 448, 256), (300, 192, 128)])
def test_exact_linear(backend, M, K, N, dtype):
    """Bias + residual at out_scale 0.5 and the plain product, at every tile offered (N = 320 / 192 / 256 / 128: every column width)."""
    r = Ints(1000 + M + K)
    x, w, b = r.act(M, K), r.weight(N, K, density=density(K, dtype)), r.small(N)
    res = 2.0 * r.small(M, N) + (x @ w.t() + b).remainder(2.0)                    # makes (acc + bias + residual) even: exact after * 0.5
    ref = (x @ w.t() + b + res) * 0.5
    exact_precondition(ref, dtype, x, w)
    exact_precondition(x @ w.t() + b, dtype)
    xd, pw = dev(x, dtype), ops.pack_weight(dev(w, dtype), dev(b, dtype))
    n = run_tiles(xd, pw, ops.linear_geom(M), ref, dtype, f"linear {M}x{K}x{N} {dtype}", residual=dev(res, dtype), out_scale=0.5)
    n += run_tiles(xd, pw, ops.linear_geom(M), x @ w.t() + b, dtype, f"linear plain {M}x{K}x{N} {dtype}")
    assert n >= 4, n


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,N", X_TILES)
def test_exact_x_tiles_every_loop_shape(backend, cfg, N, dtype):
    """The hand-scheduled tiles over K loops of 1, 3, 5 and 7 steps (prologue, peeled first / last steps, steady state), M tail."""
    M = 300
    for K in (64, 192, 320, 448):
        r = Ints(1100 + K)
        x, w, b, res = r.act(M, K), r.weight(N, K, density=density(K, dtype)), r.small(N), r.small(M, N)
        ref = x @ w.t() + b + res
        exact_precondition(ref, dtype, x, w)
        ops.FORCE_TILE = cfg
        try:
            y = ops.conv_gemm(dev(x, dtype), ops.pack_weight(dev(w, dtype), dev(b, dtype)), ops.linear_geom(M), residual=dev(res, dtype))
        finally:
            ops.FORCE_TILE = -1
        assert torch.equal(y.cpu(), ref.to(dtype)), f"tile {cfg} K {K}: {(y.cpu() != ref.to(dtype)).sum().item()} elements differ"


def conv_ref(x, wt, b, stride=1, pad=1, up_to=None):
    xr = x if up_to is None else F.interpolate(x, size=up_to, mode="nearest")
    if pad == 0:
        xr = F.pad(xr, (0, 1, 0, 1))
    return F.conv2d(xr, wt, b, stride=stride, padding=pad)


def im2col(x, stride=1, pad=1, up_to=None):
    xr = x if up_to is None else F.interpolate(x, size=up_to, mode="nearest")
    if pad == 0:
        xr = F.pad(xr, (0, 1, 0, 1))
    cols = F.unfold(xr, 3, padding=pad, stride=stride)                              # [n, C * 9, L]
    return cols.permute(0, 2, 1).reshape(-1, cols.shape[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin", [16, 64])
@pytest.mark.parametrize("stride,pad,up_to", [(1, 1, None), (2, 1, None), (2, 0, None), (1, 1, (9, 13))])
def test_exact_conv3x3(backend, stride, pad, up_to, cin, dtype):
    """3x3 at stride 1 / 2, Downsample2D's asymmetric padding, the nearest resize in front; 16 input channels run the gather kernel,
    64 the LDS-DMA kernels (every offered tile); 72 output channels leave a column tail."""
    n, h, w, cout = 2, 5, 7, 72
    r = Ints(1200 + 10 * stride + pad + cin)
    x, wt, b = r.act(n, cin, h, w), r.weight(cout, cin, 3, 3), r.small(cout)
    ref = nhwc(conv_ref(x, wt, b, stride, pad, up_to))
    exact_precondition(ref, dtype, im2col(x, stride, pad, up_to), wt.reshape(cout, -1))
    g = ops.conv3x3_geom(n, h, w, stride=stride, pad=pad, up_to=up_to)
    run_tiles(dev(nhwc(x), dtype), ops.pack_weight(dev(wt, dtype), dev(b, dtype)), g, ref, dtype, f"conv3x3 s{stride} p{pad} up {up_to} cin {cin} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_temporal_conv_two_sources_rowvec(backend, dtype):
    """(3, 1, 1) temporal convolution + residual; a 3x3 convolution over two sources (x1) with a row vector per image (rowvec_div) and a
    residual, 3 x 9 x 11 pixels (M = 297: row tails at every tile height)."""
    clips, frames, hw, c = 2, 5, 6, 64
    r = Ints(1300)
    x5, wt, b = r.act(clips, c, frames, hw, 1), r.weight(c, c, 3, 1, 1), r.small(c)
    tok = x5.permute(0, 2, 3, 4, 1).reshape(-1, c).contiguous()
    res = r.small(tok.shape[0], c)
    ref = F.conv3d(x5, wt, b, padding=(1, 0, 0)).permute(0, 2, 3, 4, 1).reshape(-1, c) + res
    exact_precondition(ref, dtype)
    run_tiles(dev(tok, dtype), ops.pack_weight(dev(wt, dtype), dev(b, dtype)), ops.tconv_geom(clips, frames, hw), ref, dtype, f"tconv {dtype}",
              residual=dev(res, dtype))
    n, h, w, c0, c1, N = 3, 9, 11, 64, 64, 320
    xa, xb = r.act(n, c0, h, w), r.act(n, c1, h, w)
    w2, b2, rv, res2 = r.weight(N, c0 + c1, 3, 3, density=density(1152, dtype)), r.small(N), r.small(n, N), r.small(n * h * w, N)
    xcat = torch.cat([xa, xb], 1)
    ref2 = nhwc(conv_ref(xcat, w2, b2) + rv[:, :, None, None]) + res2
    exact_precondition(ref2, dtype, im2col(xcat), w2.reshape(N, -1))
    run_tiles(dev(nhwc(xa), dtype), ops.pack_weight(dev(w2, dtype), dev(b2, dtype)), ops.conv3x3_geom(n, h, w), ref2, dtype, f"two sources {dtype}",
              x1=dev(nhwc(xb), dtype), rowvec=dev(rv, dtype), rowvec_div=h * w, residual=dev(res2, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_row_bias_and_fp32_output(backend, dtype):
    """bias_per_row (general epilogue of every tile) and the fp32 output of the compiled kernel, out_scale 0.5 (halves are exact in fp32)."""
    M, K, N = 130, 64, 192
    r = Ints(1400)
    x, w, brow = r.act(M, K), r.weight(N, K), r.small(M)
    ref = x @ w.t() + brow[:, None]
    exact_precondition(ref, dtype, x, w)
    xd, pw = dev(x, dtype), ops.pack_weight(dev(w, dtype))
    run_tiles(xd, pw, ops.linear_geom(M), ref, dtype, f"row bias {dtype}", bias=dev(brow, dtype), bias_per_row=True)
    y = ops.conv_gemm(xd, pw, ops.linear_geom(M), bias=dev(brow, dtype), bias_per_row=True, out_dtype=torch.float32, out_scale=0.5)
    assert y.dtype == torch.float32 and torch.equal(y.cpu().double(), ref * 0.5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,splits", [(1, 3), (3, 5), (16, 2), (36, 5), (39, 3), (40, 2), (41, 7), (42, 3), (43, 4), (44, 5), (45, 4), (46, 3), (47, 4), (48, 5), (49, 3)])
def test_exact_explicit_k_splits(backend, cfg, splits, dtype):
    """fp32 partials over uneven K ranges + the reduce launch; tiles 46 / 47 / 48 also finish inside the kernel (tickets): the partial sums are
    integers, so every split, in any order, gives the same bits."""
    n, h, w, cin = 2, 9, 11, 128
    N = 320 if ops.TILE_TABLE[cfg][1] == 320 else 256
    r = Ints(1500)
    x, wt, b, res = r.act(n, cin, h, w), r.weight(N, cin, 3, 3, density=density(1152, dtype)), r.small(N), r.small(n * h * w, N)
    ref = nhwc(conv_ref(x, wt, b)) + res
    exact_precondition(ref, dtype, im2col(x), wt.reshape(N, -1))
    pw = ops.pack_weight(dev(wt, dtype), dev(b, dtype))
    for tickets in ((False, True) if cfg in (46, 47, 48) else (False,)):
        keep = ops.USE_TICKETS
        ops.FORCE_TILE, ops.K_SPLITS, ops.USE_TICKETS = cfg, splits, tickets
        try:
            y = ops.conv_gemm(dev(nhwc(x), dtype), pw, ops.conv3x3_geom(n, h, w), residual=dev(res, dtype))
        finally:
            ops.FORCE_TILE, ops.K_SPLITS, ops.USE_TICKETS = -1, 0, keep
        assert torch.equal(y.cpu(), ref.to(dtype)), f"tile {cfg} splits {splits} tickets {tickets}: {(y.cpu() != ref.to(dtype)).sum().item()} elements differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 5, 7, 64, 72), (3, 9, 11, 128, 320)])
def test_exact_four_parity_upsample(backend, n, h, w, cin, cout, dtype):
    """Upsample2D as four 2x2 convolutions (the summed taps are integers in {-4 .. 4}: the packing's one rounding is exact), every pixel
    written exactly once, at every tile offered for a class."""
    r = Ints(1600 + cin)
    x, wt, b = r.act(n, cin, h, w), r.weight(cout, cin, 3, 3, density=density(9 * cin, dtype)), r.small(cout)
    ref = nhwc(conv_ref(x, wt, b, up_to=(2 * h, 2 * w)))
    exact_precondition(ref, dtype, im2col(x, up_to=(2 * h, 2 * w)), wt.reshape(cout, -1))
    tok = dev(nhwc(x), dtype)
    packed = ops.pack_upsample2x_weights(dev(wt, dtype), dev(b, dtype))
    g00 = ops.Geom(n, h, w, h, w, 1, 1, 1)
    for tile, splits in tiles_for(tok, packed[(0, 0)], g00):
        out = torch.full((n * 4 * h * w, cout), float("nan"), dtype=dtype, device=DEV)
        ops.FORCE_TILE, ops.K_SPLITS = tile, splits
        try:
            for (a, bb), pw in packed.items():
                ops.conv_gemm(tok, pw, ops.Geom(n, h, w, h, w, 1, 1 - a, 1 - bb), out=out, out_map=(2, 2, a, bb))
        finally:
            ops.FORCE_TILE, ops.K_SPLITS = -1, 0
        assert torch.equal(out.cpu(), ref.to(dtype)), f"tile {tile} splits {splits}: {(out.cpu() != ref.to(dtype)).sum().item()} elements differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,n_out,debug", [(128, 320, 0), (300, 320, 0), (37, 960, 0), (130, 32, 0), (680, 320, 1)])
def test_exact_linear_rows(backend, rows, n_out, debug, dtype, monkeypatch):
    """x W^T (+ b) (+ residual) with the rows in registers, no LayerNorm; (680, 320) under the plan for a 2-CU chip: the last round split
    over stages."""
    monkeypatch.setattr(ops, "LINEAR_ROWS_DEBUG", debug)
    r = Ints(1700 + rows)
    x, w, b, res = r.act(rows, 320), r.weight(n_out, 320), r.small(n_out), r.small(rows, n_out)
    exact_precondition(x @ w.t() + b + res, dtype, x, w)
    assert ops.linear_rows_ok(320, n_out, rows, dtype)
    for with_b, with_res in ((True, True), (False, False)):
        ref = x @ w.t() + (b if with_b else 0.0) + (res if with_res else 0.0)
        exact_precondition(ref, dtype)
        pk = ops.pack_linear_rows(dev(w, dtype), dev(b, dtype) if with_b else None)
        y = ops.linear_rows(dev(x, dtype), pk, dev(res, dtype) if with_res else None)
        assert torch.equal(y.cpu(), ref.to(dtype)), f"bias {with_b} residual {with_res}: {(y.cpu() != ref.to(dtype)).sum().item()} elements differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,frames,hw", [(320, 17, 9), (512, 17, 5), (640, 9, 7)])
def test_exact_seq_attention_pre_projection(backend, C, frames, hw, dtype):
    """x' = x W_pre^T + b_pre + residual inside seq_self_attention: exact; the attention behind it (over LayerNorm(x')) only has to be finite."""
    rows = frames * hw
    r = Ints(1800 + C)
    x, wp, bp, res = r.act(rows, C), r.weight(C, C, density=density(C, dtype)), r.small(C), r.small(rows, C)
    ref = x @ wp.t() + bp + res
    exact_precondition(ref, dtype, x, wp)
    g = torch.Generator().manual_seed(5)
    wq, wk, wv = ((torch.randn(C, C, generator=g) * C ** -0.5).to(dtype).to(DEV) for _ in range(3))
    pk = ops.pack_seq_qkv(wq, wk, wv, ln=(torch.ones(C, dtype=dtype, device=DEV), torch.zeros(C, dtype=dtype, device=DEV), 1e-5))
    assert ops.seq_self_attention_ok(C, frames, rows, dtype)
    o, x_pre = ops.seq_self_attention(dev(x, dtype), pk, 1, hw, frames, (frames * hw, 1, hw), pre=ops.pack_seq_pre(dev(wp, dtype), dev(bp, dtype)),
                                      residual=dev(res, dtype))
    assert torch.equal(x_pre.cpu(), ref.to(dtype)), f"{(x_pre.cpu() != ref.to(dtype)).sum().item()} elements differ"
    assert torch.isfinite(o.float()).all()


# ===================================================================================================== attention probes
def ulp(ref, dtype):
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.exp2(e - mant)


def codes(S, H, L, D, seed):
    """Distinct +-1 codes per (sequence, head): [S, H, L, D].  D = 8: the first L of a seeded shuffle of all 256 sign patterns."""
    g = torch.Generator().manual_seed(seed)
    if D == 8:
        assert L <= 256
        allc = ((torch.arange(256)[:, None] >> torch.arange(8)[None, :]) & 1).double() * 2.0 - 1.0
        return torch.stack([torch.stack([allc[torch.randperm(256, generator=g)[:L]] for _ in range(H)]) for _ in range(S)])
    return torch.randint(0, 2, (S, H, L, D), generator=g).double() * 2.0 - 1.0


def selector_inputs(S, Sk, H, Lq, Lkv, D, c, causal, seed, kv_of):
    """q [S, H, Lq, D] = c * code(pi(i)) of the key sequence kv_of(s); k [Sk, H, Lkv, D] codes; v [Sk, H, Lkv, D] integers in [-8, 8];
    pi [S, H, Lq] (causal: pi(i) <= i).  Asserts the lead of the matching key on float64 scores; returns it in bits."""
    g = torch.Generator().manual_seed(seed + 1)
    k = codes(Sk, H, Lkv, D, seed)
    v = torch.randint(-8, 9, (Sk, H, Lkv, D), generator=g).double()
    pi = torch.randint(0, Lkv, (S, H, Lq), generator=g)
    if causal:
        pi = torch.minimum(pi, torch.arange(Lq)[None, None, :].expand(S, H, Lq))
    ks = torch.tensor([kv_of(s) for s in range(S)])
    q = c * torch.gather(k[ks], 2, pi[..., None].expand(S, H, Lq, D))
    s = q @ k[ks].transpose(-1, -2) * (D ** -0.5) * LOG2E
    match = torch.gather(s, 3, pi[..., None])
    lead = (match - s.scatter(3, pi[..., None], -math.inf).amax(-1, keepdim=True)).min().item() if Lkv > 1 else math.inf
    assert lead >= 30.0, lead
    want = torch.gather(v[ks], 2, pi[..., None].expand(S, H, Lq, D))
    return q, k, v, want, lead


def counting_inputs(S, Sk, H, Lq, Lkv, D, causal, seed):
    """q = 0, k codes (irrelevant), v_j[d] = (j % D == d): the output is count_d / L, L = keys in sight."""
    k = torch.randint(0, 2, (Sk, H, Lkv, D), generator=torch.Generator().manual_seed(seed)).double() * 2.0 - 1.0
    v = (torch.arange(Lkv)[:, None] % D == torch.arange(D)[None, :]).double().expand(Sk, H, Lkv, D).contiguous()
    q = torch.zeros(S, H, Lq, D, dtype=torch.float64)
    if causal:
        seen = torch.arange(1, Lq + 1).double()
        want = v[0, 0].cumsum(0)[:Lq] / seen[:, None]
    else:
        want = (v[0, 0].sum(0) / Lkv)[None, :].expand(Lq, D)
    return q, k, v, want[None, None].expand(S, H, Lq, D)


# ---- layouts: logical [S, H, L, D] tensors <-> the token matrices ops.attention addresses
def lay_rows(t):          # [S, H, L, D] -> [S * L, H * D]
    S, H, L, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(S * L, H * D)


def lay_temporal(t, clips, hw):          # sequence s = clip * hw + pixel, position = frame: row (clip * frames + frame) * hw + pixel
    S, H, L, D = t.shape
    return t.reshape(clips, hw, H, L, D).permute(0, 3, 1, 2, 4).reshape(clips * L * hw, H * D)


def unlay_rows(o, S, H, L, D):
    return o.reshape(S, L, H, D).permute(0, 2, 1, 3)


def unlay_temporal(o, clips, hw, H, L, D):
    return o.reshape(clips, L, hw, H, D).permute(0, 2, 3, 1, 4).reshape(clips * hw, H, L, D)


# (name, form, layout, S, Sk, H, Lq, Lkv, D, c, causal, flags, extra)
ATTN_CASES = [
    ("self-17", "one-wave-32", "self", 3, 3, 2, 17, 17, 64, 8, False, 0, {}),
    ("causal-17", "one-wave-32", "self", 2, 2, 2, 17, 17, 64, 8, True, 0, {}),
    ("cross-33x77", "one-wave-64", "cross", 2, 2, 1, 33, 77, 64, 8, False, 0, {}),
    ("cross-130x200", "four-wave", "cross", 2, 2, 2, 130, 200, 64, 8, False, 0, {}),
    ("self-300", "four-wave", "self", 2, 2, 1, 300, 300, 64, 8, False, 0, {}),
    ("causal-300", "four-wave", "self", 1, 1, 2, 300, 300, 64, 8, True, 0, {}),
    ("text-129x77", "short-key", "cross", 4, 2, 2, 129, 77, 64, 8, False, 0, {"div": 2}),
    ("text-256x96", "short-key", "cross", 2, 2, 1, 256, 96, 64, 8, False, 0, {"div": 1}),
    ("text-129x77-general", "four-wave", "cross", 4, 2, 2, 129, 77, 64, 8, False, 4, {"div": 2}),
    ("temporal-2x129x17", "four-seq", "temporal", 258, 258, 1, 17, 17, 64, 8, False, 0, {"clips": 2, "hw": 129}),
    ("temporal-2x6x5", "one-wave-32", "temporal", 12, 12, 2, 5, 5, 64, 8, False, 0, {"clips": 2, "hw": 6}),
    ("table-2x5", "one-wave-32", "table", 10, 2, 2, 3, 4, 64, 8, False, 0, {"clips": 2, "hw": 5}),
    ("two-blocks-600x712", "two-blocks", "cross", 1, 1, 1, 600, 712, 64, 8, False, 8, {}),
    ("vector-8", "vector", "self", 2, 2, 4, 100, 100, 8, 32, False, 0, {}),
    ("vector-80", "vector", "self", 2, 2, 2, 289, 289, 80, 8, False, 0, {}),
]


def run_attention(layout, q, k, v, dtype, causal, flags, extra, dev_=None):
    """Pack the logical tensors into the layout's token matrices, run ops.attention, unpack the output to [S, H, Lq, D]."""
    S, H, Lq, D = q.shape
    Sk, _, Lkv, _ = k.shape
    C = H * D
    to = lambda t: t.to(dtype).to(DEV if dev_ is None else dev_)
    if layout == "self":                 # one [S * L, 3 C] matrix: column offsets 0 / C / 2 C, row pitch 3 C
        qkv = to(torch.cat([lay_rows(q), lay_rows(k), lay_rows(v)], dim=1))
        o = flagged(flags, lambda: ops.attention(qkv, 0, qkv, C, qkv, 2 * C, H, S, 1, Lq, Lkv, (Lq, 0, 1), (Lkv, 0, 1), causal=causal, head_dim=D))
        return unlay_rows(o.double().cpu(), S, H, Lq, D)
    if layout == "cross":                # q [S * Lq, C], [k | v] [Sk * Lkv, 2 C]; sequence s reads key sequence s // div
        qm, kv = to(lay_rows(q)), to(torch.cat([lay_rows(k), lay_rows(v)], dim=1))
        o = flagged(flags, lambda: ops.attention(qm, 0, kv, 0, kv, C, H, S, 1, Lq, Lkv, (Lq, 0, 1), (Lkv, 0, 1), kv_outer_div=extra.get("div", 1),
                                                causal=causal, head_dim=D))
        return unlay_rows(o.double().cpu(), S, H, Lq, D)
    clips, hw = extra["clips"], extra["hw"]
    if layout == "temporal":             # one [clips * frames * hw, 3 C] matrix, a sequence = one pixel over the frames
        qkv = to(torch.cat([lay_temporal(q, clips, hw), lay_temporal(k, clips, hw), lay_temporal(v, clips, hw)], dim=1))
        st = (Lq * hw, 1, hw)
        o = flagged(flags, lambda: ops.attention(qkv, 0, qkv, C, qkv, 2 * C, H, clips, hw, Lq, Lkv, st, st, causal=causal, head_dim=D))
        return unlay_temporal(o.double().cpu(), clips, hw, H, Lq, D)
    assert layout == "table"             # temporal queries, sequence number n reads K / V table entry n % clips
    qm, kv = to(lay_temporal(q, clips, hw)), to(torch.cat([lay_rows(k), lay_rows(v)], dim=1))
    o = flagged(flags, lambda: ops.attention(qm, 0, kv, 0, kv, C, H, clips, hw, Lq, Lkv, (Lq * hw, 1, hw), (Lkv, 0, 1), kv_seq_mod=clips, head_dim=D))
    return unlay_temporal(o.double().cpu(), clips, hw, H, Lq, D)


def kv_of(layout, extra, S, Sk):
    if layout == "cross":
        return lambda s: s // extra.get("div", 1)
    if layout == "table":
        return lambda s: s % extra["clips"]
    return lambda s: s


def selector_check(o, want, lead, Lkv, dtype, what):
    """2 ulp of the storage type (2^-9 |v| / 2^-6 |v|) + the weight of the other keys at the asserted lead."""
    rel = 2.0 ** -9 if dtype == torch.float16 else 2.0 ** -6
    bound = rel * want.abs() + Lkv * 2.0 ** -(lead - 1.0) * 8.0
    err = (o - want).abs()
    assert torch.isfinite(o).all() and (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements off, worst {err.max().item()} at {(err - bound).argmax().item()}"


def counting_check(o, want, dtype, what):
    err = (o - want.to(dtype).double()).abs()
    assert torch.isfinite(o).all() and (err <= ulp(want, dtype)).all(), f"{what}: {int((err > ulp(want, dtype)).sum())} elements off by more than 1 ulp, worst {err.max().item()}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_attention_selector(backend, case, dtype):
    name, form, layout, S, Sk, H, Lq, Lkv, D, c, causal, flags, extra = case
    nseq = S
    assert attn_form(Lq, Lkv, nseq, causal=causal, flags=flags, head_dim=D) == form
    q, k, v, want, lead = selector_inputs(S, Sk, H, Lq, Lkv, D, c, causal, 2000 + Lq + Lkv, kv_of(layout, extra, S, Sk))
    o = run_attention(layout, q, k, v, dtype, causal, flags, extra)
    selector_check(o, want, lead, Lkv, dtype, f"selector {name} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_attention_counting(backend, case, dtype):
    name, form, layout, S, Sk, H, Lq, Lkv, D, c, causal, flags, extra = case
    q, k, v, want = counting_inputs(S, Sk, H, Lq, Lkv, D, causal, 2100 + Lq)
    o = run_attention(layout, q, k, v, dtype, causal, flags, extra)
    counting_check(o, want, dtype, f"counting {name} {dtype}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_probes_eight_sequences_per_workgroup(dtype):
    """2 x 2053 temporal sequences of 17 (not a multiple of 8), eight per workgroup - too slow for the emulator, as in test_kernels.py."""
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    clips, hw, H, L, D = 2, 2053, 2, 17, 64
    S = clips * hw
    assert attn_form(L, L, S) == "eight-seq"
    extra = {"clips": clips, "hw": hw}
    q, k, v, want, lead = selector_inputs(S, S, H, L, L, D, 8, False, 2200, lambda s: s)
    selector_check(run_attention("temporal", q, k, v, dtype, False, 0, extra, dev_="cuda"), want, lead, L, dtype, f"selector eight-seq {dtype}")
    q, k, v, want = counting_inputs(S, S, H, L, L, D, False, 2201)
    counting_check(run_attention("temporal", q, k, v, dtype, False, 0, extra, dev_="cuda"), want, dtype, f"counting eight-seq {dtype}")


# ---- seq_self_attention: q / k / v are channels of x, picked out by 0 / +-1 weights (no LayerNorm)
def seq_probe_weights(C, dtype, zero_q=False):
    """Head h: k = channels [0, 64) in the order (d (2 h + 1)) % 64, q = channels [64, 128) in the same order (the inner products are those of
    the codes), v = (-1)^h * channels 128 + (d + 13 h) % 64."""
    heads = C // 64
    wq, wk, wv = torch.zeros(C, C), torch.zeros(C, C), torch.zeros(C, C)
    d = torch.arange(64)
    for h in range(heads):
        src = (d * (2 * h + 1)) % 64
        wk[h * 64 + d, src] = 1.0
        if not zero_q:
            wq[h * 64 + d, 64 + src] = 1.0
        wv[h * 64 + d, 128 + (d + 13 * h) % 64] = -1.0 if h % 2 else 1.0
    return ops.pack_seq_qkv(wq.to(dtype).to(DEV), wk.to(dtype).to(DEV), wv.to(dtype).to(DEV))


def seq_expected_v(vch, heads):
    """vch [..., 64] (channels 128 .. 191 of a row) -> that row's v over all heads [..., heads * 64]."""
    d = torch.arange(64)
    return torch.cat([vch[..., (d + 13 * h) % 64] * (-1.0 if h % 2 else 1.0) for h in range(heads)], dim=-1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,clips,frames,hw", [(320, 2, 17, 15), (320, 1, 17, 37), (320, 1, 32, 3), (512, 1, 17, 16), (640, 1, 9, 11)])
def test_seq_self_attention_selector_and_counting(backend, C, clips, frames, hw, dtype):
    """The selector and the counting probe through the fused kernel: one tile, tail tiles with idle waves, sequences that straddle the 32-row
    blocks, every channel width."""
    heads, S = C // 64, clips * hw
    rows = S * frames
    g = torch.Generator().manual_seed(2300 + C + hw)
    code = codes(S, 1, frames, 64, 2301 + hw)[:, 0]                                   # [S, frames, 64]
    pi = torch.randint(0, frames, (S, frames), generator=g)
    vch = torch.randint(-8, 9, (S, frames, 64), generator=g).double()
    qch = 8.0 * torch.gather(code, 1, pi[..., None].expand(S, frames, 64))
    s = qch @ code.transpose(-1, -2) * 0.125 * LOG2E
    lead = (torch.gather(s, 2, pi[..., None]) - s.scatter(2, pi[..., None], -math.inf).amax(-1, keepdim=True)).min().item()
    assert lead >= 30.0, lead
    x = torch.zeros(S, frames, C, dtype=torch.float64)
    x[..., 0:64], x[..., 64:128], x[..., 128:192] = code, qch, vch
    x[..., 192:] = torch.randint(-2, 3, (S, frames, C - 192), generator=g).double()   # channels no weight reads
    tok = lambda t: t.reshape(clips, hw, frames, -1).permute(0, 2, 1, 3).reshape(rows, -1)   # token order clip, frame, pixel
    assert ops.seq_self_attention_ok(C, frames, rows, dtype)
    o = ops.seq_self_attention(tok(x).to(dtype).to(DEV), seq_probe_weights(C, dtype), clips, hw, frames, (frames * hw, 1, hw)).double().cpu()
    want = seq_expected_v(torch.gather(vch, 1, pi[..., None].expand(S, frames, 64)), heads)
    selector_check(o, tok(want), lead, frames, dtype, f"seq selector C {C} {dtype}")
    # counting: Wq = 0, v_j[d] = (j % 64 == d) in channels 128 .. 191 (the other channels as before: the codes still feed k)
    onehot = (torch.arange(frames)[:, None] % 64 == torch.arange(64)[None, :]).double()
    x[..., 128:192] = onehot[None]
    o = ops.seq_self_attention(tok(x).to(dtype).to(DEV), seq_probe_weights(C, dtype, zero_q=True), clips, hw, frames, (frames * hw, 1, hw)).double().cpu()
    want = seq_expected_v((onehot.sum(0) / frames)[None, None, :].expand(S, frames, 64), heads)
    counting_check(o, tok(want), dtype, f"seq counting C {C} {dtype}")


# ===================================================================================================== softmax_rows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [1, 255, 256, 257, 300])
def test_softmax_rows_last_column_carries_half_the_mass(backend, cols, dtype):
    """Scores in [-2, 2] with the LAST column lifted to ln(sum of the others): its probability is 1/2 (cols = 1: 1).  Per element against
    float64: half an ulp of the storage type + 2^-20 relative (the exponent x - max reaches -10 here and is itself rounded to fp32: 10 * 2^-24
    relative in exp, plus __expf, the fp32 sum and the reciprocal: below 16 * 2^-24 together)."""
    g = torch.Generator().manual_seed(2400 + cols)
    s = (torch.rand(5, cols, generator=g) * 4.0 - 2.0).float()
    if cols > 1:
        s[:, -1] = torch.log(torch.exp(s[:, :-1].double()).sum(1)).float()
    ref = s.double().softmax(-1)
    assert cols == 1 or (ref[:, -1] - 0.5).abs().max().item() < 1e-6
    y = ops.softmax_rows(s.to(DEV), dtype).double().cpu()
    bound = 0.5 * ulp(ref, dtype) + 2.0 ** -20 * ref
    assert ((y - ref).abs() <= bound).all(), ((y - ref).abs() / bound).max().item()
