"""aa_quant_rows_fp8 / aa_linear_fp8 (the opt-in OCP e4m3 FeedForward path) on the SIMT emulator: the scale rule, the rounding, the tail masking
and the two epilogues against torch restatements with bounds derived from the number formats.  tests/test_gpu_fp8.py repeats the kernel checks on
the MI355X at the real shapes (the arbiter of the matrix instruction's operand layout)."""
import pytest
import torch
import torch.nn.functional as F

from animate_anything_amd import ops

FP8_MAX, TINY = 448.0, 1e-12


def dequant(q):
    return q.view(torch.float8_e4m3fn).float()


def e4m3_step(v):
    """Spacing of the e4m3 grid at magnitude |v| (3 mantissa bits; below the smallest normal number 2^-6 the grid is 2^-9)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -6)))
    return torch.exp2(e - 3)


def check_quant(x, q, s, y):
    """`y` = the fp32 rows that were quantised (x itself, or LayerNorm(x) restated in float64).
    Bound per element: half an e4m3 step at the element's magnitude, times the scale, plus the rounding of the kernel's own fp32 arithmetic:
    the kernel multiplies by fl(448 / amax) instead of dividing by s (two roundings, 2^-23 relative together with the product's), which can move
    an element that sits within 2^-22 of a rounding boundary to the other neighbour - so the half step is widened by |y| 2^-21; with a LayerNorm in
    front the normalised value itself carries the fp32 error of the statistics (mean / variance sums over K <= 5120 terms, rsqrt to 1 ulp at
    -ffast-math precision 2^-22, three more operations): |y| 2^-18 + amax 2^-20 covers it with room."""
    assert q.dtype == torch.uint8 and s.dtype == torch.float32
    assert not ((q & 0x7F) == 0x7F).any(), "NaN byte"
    amax = y.abs().amax(dim=1).clamp_min(TINY)
    want_s = (amax.double() / FP8_MAX).float()
    ln = y is not x
    tol_s = 2.0 ** -17 if ln else 2.0 ** -22
    assert ((s.double() - want_s.double()).abs() <= tol_s * want_s.double()).all(), "scale rule"
    d = dequant(q).double() * s.double()[:, None]
    step = e4m3_step(y.double() / s.double()[:, None]) * s.double()[:, None]
    slack = y.abs().double() * (2.0 ** -18 if ln else 2.0 ** -21) + (amax.double()[:, None] * 2.0 ** -20 if ln else 0.0)
    err = (d - y.double()).abs()
    assert (err <= 0.5 * step + slack).all(), (err - 0.5 * step - slack).max().item()
    assert (dequant(q).abs() <= FP8_MAX).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows,K", [(1, 640), (7, 1280), (9, 2560), (6, 5120)])
def test_quant_rows_plain(emu, dtype, rows, K):
    """rows not a multiple of the four rows of a workgroup; every piece count of the kernel (K <= 1024, 2048, 3072, 5120)."""
    g = torch.Generator().manual_seed(rows + K)
    x = (torch.randn(rows, K, generator=g) * 3.0).to(dtype)
    q, s = ops.quant_rows_fp8(x)
    check_quant(x.float(), q, s, x.float())


def test_quant_rows_special_rows(emu):
    """An all-zero row (zero bytes, the finite scale tiny / 448), a row whose maximum is exactly 448 s (the byte 0x7E, never 0x7F), a row with one huge
    outlier (everything else lands in the subnormal range or at zero), tiny values next to it."""
    K = 640
    x = torch.zeros(5, K)
    x[1] = torch.linspace(-1.0, 1.0, K)
    x[1, 17] = 7.0                                            # the maximum: 448 s exactly
    x[2] = torch.randn(K, generator=torch.Generator().manual_seed(1)) * 1e-3
    x[2, 5] = -60000.0
    x[3] = torch.randn(K, generator=torch.Generator().manual_seed(2)) * 1e-4
    x[4] = 448.0
    x = x.half()
    q, s = ops.quant_rows_fp8(x)
    check_quant(x.float(), q, s, x.float())
    assert (q[0] == 0).all() and torch.isfinite(s).all() and s[0].item() == pytest.approx(TINY / FP8_MAX, rel=1e-6)
    assert q[1, 17].item() == 0x7E and q[2, 5].item() == 0xFE and (q[4] == 0x7E).all()
    assert (s > 0).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows,K", [(5, 640), (3, 1280)])
def test_quant_rows_layernorm(emu, dtype, rows, K):
    g = torch.Generator().manual_seed(K)
    x = (torch.randn(rows, K, generator=g) * 2.0 + 0.5).to(dtype)
    gamma, beta = (1.0 + 0.3 * torch.randn(K, generator=g)).to(dtype), (0.2 * torch.randn(K, generator=g)).to(dtype)
    q, s = ops.quant_rows_fp8(x, ln=(gamma, beta, 1e-5))
    y = F.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-5).float()
    check_quant(x.float(), q, s, y)


def unpack_rows(w, n):
    """Undo the kernel's row order (ops._fp8_row_perm): channel order again."""
    out = torch.empty_like(w)
    out[ops._fp8_row_perm(n, w.device)] = w
    return out


@pytest.mark.parametrize("geglu", [False, True])
def test_pack_weight_fp8_round_trip(geglu):
    g = torch.Generator().manual_seed(3)
    n, k = 256, 128
    w, b = (torch.randn(n, k, generator=g) * 0.05).half(), torch.randn(n, generator=g).half()
    w[3] = 0                                                   # a dead channel: zeros and a finite scale
    pk = ops.pack_weight_fp8(w, b, geglu=geglu)
    src = torch.arange(n)
    if geglu:
        d = n // 2
        val = torch.arange(d).reshape(d // 32, 1, 32)
        src = torch.cat([val, val + d], dim=1).reshape(-1)
    wf = w.float()[src]
    scale = wf.abs().amax(dim=1).clamp_min(TINY) / FP8_MAX
    assert torch.equal(pk.scale, scale) and torch.equal(pk.bias, b.float()[src])
    want = (wf / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(unpack_rows(pk.w, n), want)
    assert not ((pk.w & 0x7F) == 0x7F).any()
    # the dequantised weights are within half an e4m3 step of the originals
    err = (dequant(want).double() * scale.double()[:, None] - wf.double()).abs()
    assert (err <= 0.5 * e4m3_step(wf.double() / scale.double()[:, None]) * scale.double()[:, None] * (1 + 2.0 ** -20)).all()


def linear_case(dev, M, N, K, dtype, geglu, residual, seed=0):
    """Quantised operands in, the float64 product of the DEQUANTISED operands as the reference: both sides see exactly the same numbers, what is
    left is the fp32 accumulation order and the final rounding.  Returns (err, bound) per element, and for geglu the library's erf-GELU term."""
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(M, K, generator=g) * 2.0).half()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    b = (torch.randn(N, generator=g) * 0.2).half()
    res = torch.randn(M, N // 2 if geglu else N, generator=g).to(dtype) if residual else None
    pk = ops.pack_weight_fp8(w, b, geglu=geglu)
    to = lambda t: None if t is None else t.to(dev)
    pk_dev = ops.PackedWeightFp8(to(pk.w), to(pk.scale), to(pk.bias), pk.n, pk.k, pk.geglu)
    q, s = ops.quant_rows_fp8(to(a))
    got = ops.linear_fp8(q, s, pk_dev, residual=to(res), dtype=dtype).cpu()
    q, s = q.cpu(), s.cpu()
    assert got.dtype == dtype and torch.isfinite(got.float()).all()
    aq, wq = dequant(q).double(), dequant(unpack_rows(pk.w, N)).double()
    sa, sw = s.double()[:, None], pk.scale.double()[None, :]
    y = (aq @ wq.T) * sa * sw + pk.bias.double()[None, :]
    mag = (aq.abs() @ wq.abs().T) * sa * sw                   # sum |a| |w| sa sw
    acc_bound = K * 2.0 ** -24 * mag
    if geglu:
        # y is in pack order: blocks of 32 value / 32 gate channels
        yb, ab = y.reshape(M, N // 64, 2, 32), acc_bound.reshape(M, N // 64, 2, 32)
        val, gate = yb[:, :, 0].reshape(M, -1), yb[:, :, 1].reshape(M, -1)
        want = val * F.gelu(gate)
        # d(val gelu(gate)) <= |gelu(gate)| d val + |val| 1.13 d gate   (|gelu'| <= 1.13)
        acc_bound = F.gelu(gate).abs() * ab[:, :, 0].reshape(M, -1) + val.abs() * 1.13 * ab[:, :, 1].reshape(M, -1)
    else:
        want = y if res is None else y + res.double()
    ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -14))) - (10 if dtype == torch.float16 else 7))
    err = (got.double() - want).abs()
    bound = 0.5 * ulp + acc_bound
    if geglu:                                                  # tests/test_ff_fused.py: the fast-math erf-GELU against torch's, relative to the output's range
        bound = bound + 1e-2 * max(1.0, want.abs().max().item())
    return err, bound


SHAPES = [(1, 640, 2560), (127, 1280, 640), (129, 640, 2560), (300, 1280, 5120)]       # (M, N, K): ff-out of both widths; 300 = two tiles + a straddling tail


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_fp8_plain(emu, M, N, K, dtype, residual):
    err, bound = linear_case("cpu", M, N, K, dtype, False, residual, seed=M)
    assert (err <= bound).all(), (err - bound).max().item()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(1, 5120, 640), (129, 5120, 640), (37, 10240, 1280), (200, 192, 128)])
def test_linear_fp8_geglu(emu, M, N, K, dtype):
    """GEGLU.proj of both widths (N = 8 C); N = 192: a column tile whose second half is padding."""
    err, bound = linear_case("cpu", M, N, K, dtype, True, False, seed=M)
    assert (err <= bound).all(), (err - bound).max().item()


def test_linear_fp8_exact_integers(emu):
    """Operands that are small integers (exact in e4m3, exact sums in fp32), unit scales, an ASYMMETRIC weight matrix: any mix-up of rows, columns
    or k halves in the fragment bookkeeping changes the result, which must be exact."""
    M, N, K = 130, 192, 256
    g = torch.Generator().manual_seed(9)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    w = torch.randint(-2, 3, (N, K), generator=g).float() + (torch.arange(N)[:, None] % 3 == 0).float()
    q = a.to(torch.float8_e4m3fn).view(torch.uint8)
    wq = w.to(torch.float8_e4m3fn).view(torch.uint8)
    pk = ops.PackedWeightFp8(wq[ops._fp8_row_perm(N, "cpu")].contiguous(), torch.ones(N), None, N, K, False)
    got = ops.linear_fp8(q, torch.ones(M), pk, dtype=torch.float16)
    assert torch.equal(got.float(), (a @ w.T))


def test_linear_fp8_rejects_bad_shapes(emu):
    q, s = torch.zeros(4, 192, dtype=torch.uint8), torch.ones(4)
    pk = ops.PackedWeightFp8(torch.zeros(64, 192, dtype=torch.uint8), torch.ones(64), None, 64, 192, False)
    with pytest.raises(RuntimeError, match="linear_fp8"):
        ops.linear_fp8(q, s, pk, dtype=torch.float16)
