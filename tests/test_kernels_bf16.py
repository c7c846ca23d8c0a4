"""Per-kernel parity in bf16 storage (AA_BF16: its own matrix instruction, its own packed dot product) for attention, the contractions,
the folded LayerNorm, the norms and the step glue - the shapes of the fp16 tests in test_kernels.py / test_svd.py, on the same two
backends (the SIMT emulator, and the MI355X under `-m gpu`: only that one runs the hardware forms of the bf16 intrinsics).

No fixed tolerance.  Every case computes, from the same stored bf16 inputs,
  ref64   the operation in float64 torch,
  model   the operation in float32 torch, rounded to bf16 exactly where the kernel documents a 16-bit value: attention - Q * (scale log2 e),
          P and the output (the vector kernels of head_dim 8 / 80: the output only); contractions - the output, and the activated value in
          front of a residual add where the fp16 tests write `.half().float()`; the four-parity upsample - the summed taps
          (ops.pack_upsample2x_weights: "one rounding"); folded LayerNorm - the packed W diag(gamma); norms and glue - the output,
  got     the kernel,
and asserts  max|got - ref64| <= FACTOR * max|model - ref64| + 2^-12 * max(1, max|ref64|)  (accept()).  FACTOR = 2 covers the order of
summation; the floor is an eighth of a bf16 half-ulp at the reference scale (a case the model hits exactly must not demand bit equality).
The bound itself is asserted to stay within 8x (the ulp ratio of bf16 / fp16) the tolerance of the corresponding fp16 test.  Outputs of
>= 10 000 elements also pass a signed check: the mean of (|got| - |ref64|) / |ref64| over the elements above 2^-6 of the maximum is
within 2^-11 (round-to-nearest: ~0; a store that truncates towards zero: ~ -1.4e-3) - `model` is held to the same check in the test.

Worst kernel error / model error per family (every case prints its own: `pytest -s`, lines "bf16-ratio"):

  family                                          emulator   MI355X
  attention, head_dim 64 (matrix cores)           1.55       not measured
  attention, head_dim 8 / 80 (vector ALUs)        1.00       not measured
  contractions (aa_conv_gemm), 16-bit output      1.22       not measured
  folded LayerNorm                                1.00       not measured
  norms                                           1.00       not measured
  glue                                            1.00       not measured
  fp32 outputs (row-bias linear, groupnorm_coef)  2.89 (*)   not measured

(*) kernel 7.2e-7 against model 2.5e-7 on coefficients of size 2: both are fp32 summation noise 300x below the floor of the rule, which
is what decides these cases - the ratio says nothing there and no factor other than 2 is used anywhere.  The attention figure is one 64-element row
of test_attention_lazy_maximum (row 25, kernel 7.7e-4 against model 5.0e-4 at a reference maximum of 0.15: the maximum over so few elements
is itself noisy); whole-tensor attention cases stay at or below 1.09.  Worst signed error: 2.1e-4 for kernel and
model alike (limit 4.9e-4).
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from animate_anything_amd import _lib, ops
from animate_anything_amd._lib import AA_ACT_SILU
from test_kernels import _ln_fold_consume, nhwc

BF = torch.bfloat16
FACTOR = 2.0
DEV = "cpu"
BACKEND = "emu"
LOG2E = 1.4426950408889634


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


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


def rb(t):
    """Round to nearest-even bf16, back in the dtype it came in."""
    return t.to(BF).to(t.dtype)


def cv(t, dt):
    return t.detach().cpu().to(dt)


def both(fn, out_bf16=True):
    """fn(dtype, round) -> the operation; ref64 = fn(float64, identity), model = fn(float32, bf16 rounding) (+ the output rounding)."""
    ref = fn(torch.float64, lambda t: t)
    model = fn(torch.float32, rb)
    return ref, (rb(model) if out_bf16 else model)


def signed_error(x, ref):
    keep = ref.abs() > 2.0 ** -6 * ref.abs().max()
    return ((x.abs()[keep] - ref.abs()[keep]) / ref.abs()[keep]).mean().item()


def accept(got, ref, model, fp16_tol, family, rel=False, note=""):
    """The acceptance rule of the module docstring.  `fp16_tol`: the tolerance of the fp16 test of the same operation (`rel`: that test
    scales it by max|ref| (util.rel_err), otherwise by max(1, max|ref|) (test_kernels.close))."""
    got, ref, model = got.detach().double().cpu(), ref.double(), model.double()
    assert got.shape == ref.shape == model.shape, (got.shape, ref.shape, model.shape)
    assert torch.isfinite(got).all()
    top = ref.abs().max().item()
    e_got, e_model = (got - ref).abs().max().item(), (model - ref).abs().max().item()
    bound = FACTOR * e_model + 2.0 ** -12 * max(1.0, top)
    print(f"bf16-ratio | {family} | {BACKEND} | {e_got / max(e_model, 1e-30):.3f} | kernel {e_got:.4g} model {e_model:.4g} bound {bound:.4g} ref max {top:.4g} {note}")
    assert bound <= 8.0 * fp16_tol * (top if rel else max(1.0, top)), f"degenerate model: bound {bound} (ref max {top})"
    assert e_got <= bound, f"kernel error {e_got} > {bound} = {FACTOR} x model error {e_model} + floor (ref max {top})"
    if ref.numel() >= 10000:
        s_model, s_got = signed_error(model, ref), signed_error(got, ref)
        print(f"bf16-signed | {family} | {BACKEND} | kernel {s_got:.3g} model {s_model:.3g}")
        assert abs(s_model) <= 2.0 ** -11, f"the model's own signed error {s_model}"
        assert abs(s_got) <= 2.0 ** -11, f"signed relative error {s_got}: a biased store conversion?"


# ===================================================================================================== attention
def attn_pair(q, k, v, scale=None, causal=False, mfma=True):
    """q [..., Lq, D], k / v [..., Lk, D] (stored bf16) -> (ref64, model, the fp64 scores in bits).  The model of the matrix-core kernels
    (attention.h): Q * (scale log2 e) rounded when it is loaded, fp32 scores, p = exp2(s - max) summed in fp32 and rounded for the P operand,
    fp32 O / l rounded on the store; the vector kernels (`mfma` False) keep everything but the output in fp32."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    q, k, v = q.detach().cpu(), k.detach().cpu(), v.detach().cpu()
    mask = torch.ones(q.shape[-2], k.shape[-2], dtype=torch.bool).tril() if causal else None
    s = q.double() @ k.double().transpose(-1, -2) * scale
    if causal:
        s = s.masked_fill(~mask, -math.inf)
    ref = s.softmax(-1) @ v.double()
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    qc = q.float() * c
    sm = (rb(qc) if mfma else qc) @ k.float().transpose(-1, -2)
    if causal:
        sm = sm.masked_fill(~mask, -math.inf)
    p = torch.exp2(sm - sm.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    model = rb(((rb(p) if mfma else p) @ v.float()) / l)
    return ref, model, s * LOG2E


def attn_form(q_len, kv_len, nseq, causal=False, flags=0, head_dim=64):
    """The launch attention_t (aa_api_impl.h) picks - restated here so that a case says which kernel form it is about."""
    if head_dim in (8, 80):
        return "vector"
    if q_len >= 128 and 64 < kv_len <= 96 and not causal and not flags & 4:
        return "short-key"
    if q_len >= 512 and kv_len >= 512 and flags & 8:
        return "two-blocks"
    if q_len > 64:
        return "four-wave"
    if kv_len <= 32 and q_len <= 32:
        return "eight-seq" if nseq >= 4096 else "four-seq" if nseq >= 256 else "one-wave-32"
    return "one-wave-32" if kv_len <= 32 else "one-wave-64"


def flagged(flags, fn):
    keep, ops.ATTN_FLAGS = ops.ATTN_FLAGS, flags
    try:
        return fn()
    finally:
        ops.ATTN_FLAGS = keep


def plain_attention(q, kv, n, heads, Lq, Lkv, causal=False, scale=None):
    """q [n*Lq, heads*64], kv [n*Lkv, 2*heads*64] (K | V) -> kernel output, (ref64, model, scores) in the same token layout."""
    o = ops.attention(q, 0, kv, 0, kv, heads * 64, heads, n, 1, Lq, Lkv, (Lq, 0, 1), (Lkv, 0, 1), causal=causal, scale=scale)
    qq = q.reshape(n, Lq, heads, 64).transpose(1, 2)
    kk = kv.reshape(n, Lkv, 2, heads, 64)
    ref, model, s = attn_pair(qq, kk[:, :, 0].transpose(1, 2), kk[:, :, 1].transpose(1, 2), scale=scale, causal=causal)
    lay = lambda t: t.transpose(1, 2).reshape(n * Lq, heads * 64)
    return o, lay(ref), lay(model), s


@pytest.mark.parametrize("Lq,Lkv,n,heads,form", [(300, 300, 2, 1, "four-wave"), (1100, 1100, 1, 2, "four-wave"), (1024, 200, 1, 2, "four-wave"),
                                                  (50, 200, 2, 1, "one-wave-64"), (33, 77, 2, 1, "one-wave-64"), (17, 17, 3, 2, "one-wave-32")])
def test_attention_ring_and_single_tile(backend, Lq, Lkv, n, heads, form):
    """The four-wave ring (ragged last workgroup / wave / key tile, cross lengths), the one-wave 64-key ring and tile, the one-wave 32-key tile."""
    assert attn_form(Lq, Lkv, n) == form
    q, kv = rnd(n * Lq, heads * 64, seed=41), rnd(n * Lkv, 2 * heads * 64, seed=42)
    o, ref, model, _ = plain_attention(q, kv, n, heads, Lq, Lkv)
    assert o.dtype == BF
    accept(o, ref, model, 1e-2, "attention")


def test_attention_large_scale(backend):
    """33 x 77 at three times the usual score scale (widely spread scores: the rounding of Q * c and of P shows)."""
    n, Lq, Lkv = 2, 33, 77
    q, kv = rnd(n * Lq, 64, scale=3.0, seed=141), rnd(n * Lkv, 128, scale=2.0, seed=142)
    o, ref, model, _ = plain_attention(q, kv, n, 1, Lq, Lkv)
    accept(o, ref, model, 1e-2, "attention")


@pytest.mark.parametrize("L", [20, 77, 300, 1030])
def test_attention_causal(backend, L):
    n, heads = (2, 2) if L < 1000 else (1, 2)
    C_ = heads * 64
    assert attn_form(L, L, n, causal=True) == ("one-wave-32" if L == 20 else "four-wave")
    qkv = rnd(n * L, 3 * C_, seed=33)
    o = ops.attention(qkv, 0, qkv, C_, qkv, 2 * C_, heads, n, 1, L, L, (L, 0, 1), (L, 0, 1), causal=True)
    x = qkv.reshape(n, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    ref, model, _ = attn_pair(x[0], x[1], x[2], causal=True)
    lay = lambda t: t.permute(0, 2, 1, 3).reshape(n * L, C_)
    accept(o, lay(ref), lay(model), 1e-2, "attention")


def temporal_case(clips, frames, hw, heads, seed, dev=None):
    C_ = heads * 64
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(clips * frames * hw, 3 * C_, generator=g).to(BF).to(DEV if dev is None else dev)
    st = (frames * hw, 1, hw)
    o = ops.attention(qkv, 0, qkv, C_, qkv, 2 * C_, heads, clips, hw, frames, frames, st, st)
    x = qkv.reshape(clips, frames, hw, 3, heads, 64).permute(3, 0, 2, 4, 1, 5)       # [3,b,hw,h,T,d]
    ref, model, _ = attn_pair(x[0], x[1], x[2])
    lay = lambda t: t.permute(0, 3, 1, 2, 4).reshape(-1, C_)                          # -> [b,T,hw,h,d]
    accept(o, lay(ref), lay(model), 1e-2, "attention")


@pytest.mark.parametrize("clips,frames,hw,heads,form", [(2, 5, 6, 2, "one-wave-32"), (2, 17, 129, 1, "four-seq")])
def test_attention_temporal(backend, clips, frames, hw, heads, form):
    """Temporal strides (a sequence = one pixel over the frames); 258 sequences run four per workgroup, the last workgroup with idle waves."""
    assert attn_form(frames, frames, clips * hw) == form and (form != "four-seq" or (clips * hw) % 4 != 0)
    temporal_case(clips, frames, hw, heads, 38)


@pytest.mark.gpu
def test_attention_temporal_eight_sequences_per_workgroup():
    """>= 4096 short sequences, eight per workgroup (2 x 2053: not a multiple of 8) - too slow for the emulator, as in test_kernels.py."""
    global BACKEND
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    assert attn_form(17, 17, 2 * 2053) == "eight-seq"
    BACKEND = "gpu"
    try:
        temporal_case(2, 17, 2053, 2, 39, dev="cuda")
    finally:
        BACKEND = "emu"


@pytest.mark.parametrize("L,Lt,heads,frames", [(300, 77, 2, 2), (129, 96, 1, 1), (1000, 65, 1, 3), (256, 77, 5, 1)])
def test_attention_short_key_sequences(backend, L, Lt, heads, frames):
    """attention_shortkv_kernel<bf16_t> (K / V^T fragments resident in registers) and the general kernel on the same call, per-clip text
    layout (kv_outer_div = frames), ragged query tails, every key count edge."""
    clips = 2
    C_ = heads * 64
    assert attn_form(L, Lt, clips * frames) == "short-key" and attn_form(L, Lt, clips * frames, flags=4) == "four-wave"
    q, kv = rnd(clips * frames * L, C_, seed=161), rnd(clips * Lt, 2 * C_, scale=1.5, seed=162)
    run = lambda: ops.attention(q, 0, kv, 0, kv, C_, heads, clips * frames, 1, L, Lt, (L, 0, 1), (Lt, 0, 1), kv_outer_div=frames)
    o = run()
    o_general = flagged(ops.ATTN_FLAGS | 4, run)
    qq = q.reshape(clips, frames, L, heads, 64).permute(0, 1, 3, 2, 4)
    kk = kv.reshape(clips, 1, Lt, 2, heads, 64).permute(3, 0, 1, 4, 2, 5)
    ref, model, _ = attn_pair(qq, kk[0], kk[1])
    lay = lambda t: t.permute(0, 1, 3, 2, 4).reshape(-1, C_)
    accept(o, lay(ref), lay(model), 1e-2, "attention", note="short-key")
    accept(o_general, lay(ref), lay(model), 1e-2, "attention", note="general")


def test_attention_cross_text_and_table_addressing(backend):
    """kv_outer_div (one text per clip, shared by its frames) and kv_seq_mod (sequence n reads K / V table entry n % clips)."""
    clips, frames, heads, L, Lt = 2, 2, 1, 40, 77
    C_ = heads * 64
    q, kv = rnd(clips * frames * L, C_, seed=32), rnd(clips * Lt, 2 * C_, seed=33)
    o = ops.attention(q, 0, kv, 0, kv, C_, heads, clips * frames, 1, L, Lt, (L, 0, 1), (Lt, 0, 1), kv_outer_div=frames)
    qq = q.reshape(clips, frames, L, heads, 64).permute(0, 1, 3, 2, 4)
    kk = kv.reshape(clips, 1, Lt, 2, heads, 64).permute(3, 0, 1, 4, 2, 5)
    ref, model, _ = attn_pair(qq, kk[0], kk[1])
    lay = lambda t: t.permute(0, 1, 3, 2, 4).reshape(-1, C_)
    accept(o, lay(ref), lay(model), 1e-2, "attention")
    clips, frames, hw, heads, L = 2, 3, 5, 2, 4
    q, kv = rnd(clips * frames * hw, heads * 64, seed=4), rnd(clips * L, 2 * heads * 64, seed=5)
    o = ops.attention(q, 0, kv, 0, kv, heads * 64, heads, clips, hw, frames, L, (frames * hw, 1, hw), (L, 0, 1), kv_seq_mod=clips)
    qf = q.reshape(clips, frames, hw, heads, 64).permute(0, 2, 3, 1, 4)                      # [b, p, h, T, d]
    table = (torch.arange(clips * hw) % clips).reshape(clips, hw)
    kf = kv.reshape(clips, L, 2, heads, 64).cpu()[table]                                      # [b, p, L, 2, h, d]
    ref, model, _ = attn_pair(qf, kf[:, :, :, 0].permute(0, 1, 3, 2, 4), kf[:, :, :, 1].permute(0, 1, 3, 2, 4))
    lay = lambda t: t.permute(0, 3, 1, 2, 4).reshape(-1, heads * 64)
    accept(o, lay(ref), lay(model), 3e-3, "attention", rel=True)


@pytest.mark.parametrize("Lq,Lkv,qs", [(70, 300, 2.0), (40, 200, 0.3), (33, 77, 3.0)])
def test_attention_deferred_max(backend, Lq, Lkv, qs):
    """test_kernels.test_attention_deferred_max in bf16: widely spread scores, a key that spikes against one query deep in the sequence,
    a row whose first tile holds only very negative scores, and a quiet case."""
    n = 2
    q, kv = rnd(n * Lq, 64, scale=qs, seed=141), rnd(n * Lkv, 128, scale=2.0, seed=142)
    kk, qq = kv.reshape(n, Lkv, 2, 64), q.reshape(n, Lq, 64)
    kk[0, Lkv - 70, 0] = (qq[0, 5].float() * 4.0).to(BF)
    kk[1, :64, 0] = (-qq[1, 7].float().sign() * 3.0).to(BF)
    o, ref, model, s = plain_attention(q, kv, n, 1, Lq, Lkv)
    if qs >= 2.0:     # the constructed rows, on the stored values: the spike leads its row; row 7's first tile lies > 6 bits below the rest
        assert s[0, 0, 5].argmax().item() == Lkv - 70
        assert s[1, 0, 7, :64].max().item() < s[1, 0, 7, 64:].max().item() - 6.0
    accept(o, ref, model, 1e-2, "attention")


@pytest.mark.parametrize("Lq,Lkv,qo", [(70, 520, 0), (130, 330, 0), (600, 712, 0), (600, 712, 32)])
def test_attention_lazy_maximum(backend, Lq, Lkv, qo):
    """test_kernels.test_attention_lazy_maximum in bf16 (8 mantissa bits, the range of fp32): the staircase, the overflowing spike, the flat
    row and the row whose every later key sits ~2 bits up; (600, 712) also through the two-blocks-per-wave kernel (ATTN_FLAGS 8), the special
    rows in a wave's first (qo 0) or second (qo 32) block.  That the constructed keys still put the scores where the branches need them
    after rounding to bf16 is asserted on ref64's scores."""
    n = 1
    q, kv = rnd(n * Lq, 64, seed=151), rnd(n * Lkv, 128, seed=152)
    kk = kv.reshape(n, Lkv, 2, 64)
    qq = q.reshape(n, Lq, 64).float()
    s = 8.0 / math.log2(math.e)
    unit = lambda r: qq[0, r] / (qq[0, r] ** 2).sum()
    for t in range(1, Lkv // 64):
        kk[0, 64 * t + 9, 0] = (unit(qo + 3) * s * (6.0 + 3.5 * t)).to(BF)
    kk[0, Lkv - 40, 0] = (unit(qo + 11) * s * 300.0).to(BF)
    q[qo + 17] = 0
    kk[0, 64:, 0] += (unit(qo + 25) * s * 2.0).to(BF)
    qh, kh, vh = q.reshape(n, 1, Lq, 64), kk[:, :, 0].reshape(n, 1, Lkv, 64), kk[:, :, 1].reshape(n, 1, Lkv, 64)
    ref, model, bits = attn_pair(qh, kh, vh)
    ref, model, bits = ref.reshape(n * Lq, 64), model.reshape(n * Lq, 64), bits.reshape(Lq, Lkv)
    # the branches are walked: (staircase) from the second stair on every full tile's maximum beats everything before it by 2..6 bits - below
    # the 6-bit threshold one tile at a time; (spike) > 100 bits over the rest of its row: exp2 overflows against any earlier maximum;
    # (flat) all scores equal; (row 25) the later keys lift the row by about 2 bits
    stair = bits[qo + 3].clone()
    stair[Lkv - 40] = -math.inf                       # (query 11's spike key scores at random against query 3: not part of the staircase)
    tops = [stair[64 * t:64 * t + 64].max().item() for t in range(Lkv // 64)]
    steps = [tops[t] - max(tops[:t]) for t in range(2, len(tops))]
    assert tops[1] > tops[0] and all(2.0 < d < 6.0 for d in steps), (tops, steps)
    spike = bits[qo + 11]
    assert spike.argmax().item() == Lkv - 40 and spike.max().item() - spike[torch.arange(Lkv) != Lkv - 40].max().item() > 100.0
    assert bits[qo + 17].abs().max().item() == 0.0
    lift = q.reshape(Lq, 64)[qo + 25].double().cpu() @ (unit(qo + 25) * s * 2.0).to(BF).double().cpu() / 8.0 * LOG2E
    assert 1.9 < lift.item() < 2.1, lift
    for flags in ((0, 8) if Lq >= 512 and Lkv >= 512 else (0,)):
        assert attn_form(Lq, Lkv, n, flags=flags) == ("two-blocks" if flags else "four-wave")
        o = flagged(flags, lambda: ops.attention(q, 0, kv, 0, kv, 64, 1, n, 1, Lq, Lkv, (Lq, 0, 1), (Lkv, 0, 1)))
        accept(o, ref, model, 1e-2, "attention", note=f"flags {flags}")
        for r in (3, 11, 17, 25):
            accept(o[qo + r], ref[qo + r], model[qo + r], 1e-2, "attention", note=f"flags {flags} row {r}")


@pytest.mark.parametrize("D,L,heads", [(8, 100, 4), (8, 300, 4), (80, 289, 2)])
def test_attention_vector_kernels(backend, D, L, heads):
    """attention_small_kernel<bf16_t, 8 / 80>: one and several 256-key tiles, a ragged tail above 256 keys for head_dim 80."""
    n = 2
    C_ = heads * D
    assert attn_form(L, L, n, head_dim=D) == "vector"
    qkv = rnd(n * L, 3 * C_, scale=1.5 if D == 8 else 1.0, seed=171)
    o = ops.attention(qkv, 0, qkv, C_, qkv, 2 * C_, heads, n, 1, L, L, (L, 0, 1), (L, 0, 1), head_dim=D)
    x = qkv.reshape(n, L, 3, heads, D).permute(2, 0, 3, 1, 4)
    ref, model, _ = attn_pair(x[0], x[1], x[2], mfma=False)
    lay = lambda t: t.permute(0, 2, 1, 3).reshape(n * L, C_)
    accept(o, lay(ref), lay(model), 1e-2, "attention-vector")


# ===================================================================================================== contractions
def forced(fn, tile=-1, splits=0, ablate=0, tickets=None):
    keep = ops.USE_TICKETS
    ops.FORCE_TILE, ops.K_SPLITS, ops.DEBUG_ABLATE = tile, splits, ablate
    if tickets is not None:
        ops.USE_TICKETS = tickets
    try:
        return fn()
    finally:
        ops.FORCE_TILE, ops.K_SPLITS, ops.DEBUG_ABLATE, ops.USE_TICKETS = -1, 0, 0, keep


def conv_ref(x, wt, b, dt, stride=1, pad=1, up_to=None):
    xr = cv(x, dt)
    if up_to is not None:
        xr = F.interpolate(xr, size=up_to, mode="nearest")
    if pad == 0:
        xr = F.pad(xr, (0, 1, 0, 1))
    return F.conv2d(xr, cv(wt, dt), None if b is None else cv(b, dt), stride=stride, padding=pad)


ALL_TILES = [(0, 320), (1, 640), (2, 256), (3, 256), (4, 640), (5, 320), (6, 320), (7, 512), (8, 128), (9, 64), (10, 640), (11, 320), (12, 256), (13, 512),
             (14, 320), (15, 256), (16, 128), (17, 64), (18, 128), (19, 64), (20, 256), (21, 320), (22, 256), (23, 256), (24, 256), (25, 256), (26, 320),
             (27, 256), (28, 256), (29, 640), (30, 320), (31, 128), (32, 320), (33, 256), (36, 256), (37, 640), (38, 512), (39, 320), (40, 256), (41, 256),
             (42, 640), (43, 512), (44, 256), (45, 128), (46, 256), (47, 128), (48, 128), (49, 320)]


@pytest.mark.parametrize("cfg,N", ALL_TILES)
def test_dma_tile_shapes(backend, cfg, N):
    """Every tile of the LDS-DMA kernel (forced) in bf16: 3x3 convolution with halo, M tail, row vector, residual."""
    n, h, w, cin = 3, 9, 11, 64
    x, wt, b = rnd(n, cin, h, w, seed=61), rnd(N, cin, 3, 3, scale=0.05, seed=62), rnd(N, seed=63)
    g = ops.conv3x3_geom(n, h, w)
    res, temb = rnd(g.rows, N, seed=64), rnd(n, N, seed=65)
    y = forced(lambda: ops.conv_gemm(nhwc(x), ops.pack_weight(wt, b), g, residual=res, rowvec=temb, rowvec_div=h * w), tile=cfg)
    assert y.dtype == BF
    ref, model = both(lambda dt, r: r(nhwc(conv_ref(x, wt, b, dt) + cv(temb, dt)[:, :, None, None])) + cv(res, dt))
    accept(y, ref, model, 2e-2, "contraction")


@pytest.mark.parametrize("stride,pad,up_to", [(1, 1, None), (2, 1, None), (2, 0, None), (1, 1, (10, 14)), (1, 1, (9, 13))])
def test_conv3x3_general_path(backend, stride, pad, up_to):
    """16 input channels: the gather (non-DMA) path - strides, Downsample2D's asymmetric padding, nearest resize in front."""
    n, h, w, cin, cout = 2, 5, 7, 16, 72
    x, wt, b = rnd(n, cin, h, w, seed=11), rnd(cout, cin, 3, 3, scale=0.1, seed=12), rnd(cout, seed=13)
    g = ops.conv3x3_geom(n, h, w, stride=stride, pad=pad, up_to=up_to)
    y = ops.conv_gemm(nhwc(x), ops.pack_weight(wt, b), g)
    ref, model = both(lambda dt, r: nhwc(conv_ref(x, wt, b, dt, stride, pad, up_to)))
    accept(y, ref, model, 2e-2, "contraction")


def test_conv3x3_concat_rowvec_cin5(backend):
    n, h, w, cout = 3, 4, 6, 64
    a, bsrc = rnd(n, 8, h, w, seed=14), rnd(n, 16, h, w, seed=15)
    wt, b, temb = rnd(cout, 24, 3, 3, scale=0.1, seed=16), rnd(cout, seed=17), rnd(n, cout, seed=18)
    y = ops.conv_gemm(nhwc(a), ops.pack_weight(wt, b), ops.conv3x3_geom(n, h, w), x1=nhwc(bsrc), rowvec=temb, rowvec_div=h * w)
    ref, model = both(lambda dt, r: nhwc(conv_ref(torch.cat([a, bsrc], 1), wt, b, dt) + cv(temb, dt)[:, :, None, None]))
    accept(y, ref, model, 2e-2, "contraction")
    x5, w5 = rnd(n, 5, h, w, seed=19), rnd(cout, 5, 3, 3, scale=0.2, seed=20)          # 5 input channels zero-padded to 8
    pw = ops.pack_weight(w5, b)
    assert pw.cin == 8 and pw.k_pad == 128
    y5 = ops.conv_gemm(nhwc(F.pad(x5, (0, 0, 0, 0, 0, 3))), pw, ops.conv3x3_geom(n, h, w))
    ref, model = both(lambda dt, r: nhwc(conv_ref(x5, w5, b, dt)))
    accept(y5, ref, model, 2e-2, "contraction")


def test_temporal_conv(backend):
    clips, frames, hh, ww, c = 2, 5, 2, 3, 16
    x = rnd(clips, c, frames, hh, ww, seed=21)
    wt, b = rnd(c, c, 3, 1, 1, scale=0.2, seed=22), rnd(c, seed=23)
    tok = x.permute(0, 2, 3, 4, 1).reshape(-1, c).contiguous()
    res = rnd(tok.shape[0], c, seed=24)
    y = ops.conv_gemm(tok, ops.pack_weight(wt, b), ops.tconv_geom(clips, frames, hh * ww), residual=res)
    ref, model = both(lambda dt, r: F.conv3d(cv(x, dt), cv(wt, dt), cv(b, dt), padding=(1, 0, 0)).permute(0, 2, 3, 4, 1).reshape(-1, c) + cv(res, dt))
    accept(y, ref, model, 2e-2, "contraction")


@pytest.mark.parametrize("cfg,N", [(34, 320), (35, 256)])
@pytest.mark.parametrize("h,w,c0,c1", [(16, 16, 128, 0), (8, 32, 64, 64), (4, 64, 192, 0), (32, 16, 64, 0)])
def test_conv3x3_halo_slab_kernel(backend, cfg, N, h, w, c0, c1):
    n = 2
    cin = c0 + c1
    x, wt, b = rnd(n, cin, h, w, seed=181), rnd(N, cin, 3, 3, scale=0.04, seed=182), rnd(N, seed=183)
    g = ops.conv3x3_geom(n, h, w)
    res, temb = rnd(g.rows, N, seed=184), rnd(n, N, seed=185)
    tok = nhwc(x)
    x0, x1 = (tok, None) if c1 == 0 else (tok[:, :c0].contiguous(), tok[:, c0:].contiguous())
    pw = ops.pack_weight(wt, b)
    assert pw.k_order == 1
    y = forced(lambda: ops.conv_gemm(x0, pw, g, x1=x1, residual=res, rowvec=temb, rowvec_div=h * w, act=AA_ACT_SILU), tile=cfg)
    ref, model = both(lambda dt, r: r(nhwc(F.silu(conv_ref(x, wt, b, dt) + cv(temb, dt)[:, :, None, None]))) + cv(res, dt))
    accept(y, ref, model, 2e-2, "contraction")


@pytest.mark.parametrize("n,h,w,cin,cout,tile", [(3, 9, 11, 128, 320, -1), (2, 5, 7, 64, 72, 47), (2, 8, 8, 64, 256, 36), (2, 8, 8, 64, 256, 1)])
def test_upsample2x_as_four_parity_convs(backend, n, h, w, cin, cout, tile):
    """Four 2x2 convolutions scattering into the parity classes of the x2 grid: NaN-prefilled output (every pixel written exactly once);
    the model sums the taps of a class in fp32 and rounds them once, as ops.pack_upsample2x_weights does."""
    x, wt, b = rnd(n, cin, h, w, seed=141), rnd(cout, cin, 3, 3, scale=0.05, seed=142), rnd(cout, seed=143)
    tok = nhwc(x)
    out = torch.full((n * 4 * h * w, cout), float("nan"), dtype=BF, device=DEV)

    def run():
        for (a, bb), pw in ops.pack_upsample2x_weights(wt, b).items():
            assert (pw.kh, pw.kw) == (2, 2)
            ops.conv_gemm(tok, pw, ops.Geom(n, h, w, h, w, 1, 1 - a, 1 - bb), out=out, out_map=(2, 2, a, bb))
    forced(run, tile=tile)
    assert torch.isfinite(out.float()).all()
    groups = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}

    def classes(dt, r):
        y = torch.zeros(n, cout, 2 * h, 2 * w, dtype=dt)
        for a in (0, 1):
            for bb in (0, 1):
                f = torch.stack([torch.stack([sum(cv(wt, torch.float32)[:, :, dy, dx] for dy in groups[a][p] for dx in groups[bb][q_]) for q_ in (0, 1)], -1)
                                 for p in (0, 1)], -2)
                y[:, :, a::2, bb::2] = F.conv2d(F.pad(cv(x, dt), (1 - bb, bb, 1 - a, a)), r(f).to(dt), cv(b, dt))
        return nhwc(y)
    ref = nhwc(conv_ref(x, wt, b, torch.float64, up_to=(2 * h, 2 * w)))
    model = rb(classes(torch.float32, rb))
    assert (classes(torch.float64, lambda t: t.double()) - ref).abs().max().item() < 1e-5      # (the class decomposition itself; taps summed in fp32)
    accept(out, ref, model, 2e-2, "contraction")


def test_upsample2x_parity_convs_split_k(backend):
    n, h, w, cin, cout = 1, 4, 4, 256, 128
    x, wt, b = rnd(n, cin, h, w, seed=151), rnd(cout, cin, 3, 3, scale=0.03, seed=152), rnd(cout, seed=153)
    out = torch.full((n * 4 * h * w, cout), float("nan"), dtype=BF, device=DEV)

    def run():
        for (a, bb), pw in ops.pack_upsample2x_weights(wt, b).items():
            ops.conv_gemm(nhwc(x), pw, ops.Geom(n, h, w, h, w, 1, 1 - a, 1 - bb), out=out, out_map=(2, 2, a, bb))
    forced(run, splits=3)
    assert torch.isfinite(out.float()).all()
    ref = nhwc(conv_ref(x, wt, b, torch.float64, up_to=(2 * h, 2 * w)))
    # (model: the 3x3 form with the output rounding only; the summed-tap rounding of the classes makes the kernel's error larger than this
    #  model's by up to 2^-9 |w| sqrt(K) |x| - inside the factor, measured in the ratio)
    accept(out, ref, rb(nhwc(conv_ref(x, wt, b, torch.float32, up_to=(2 * h, 2 * w)))), 2e-2, "contraction")


@pytest.mark.parametrize("cfg,splits", [(1, 3), (36, 3), (39, 3), (46, 3), (49, 3), (41, 7)])
def test_split_k_through_the_reduce_launch(backend, cfg, splits):
    """fp32 partials + reduce launch with the fused epilogue (SiLU, rounding, residual) in bf16."""
    n, h, w, cin = 2, 9, 11, 128
    N = 320 if ops.TILE_TABLE[cfg][1] == 320 else 256
    x, wt, b = rnd(n, cin, h, w, seed=91), rnd(N, cin, 3, 3, scale=0.05, seed=92), rnd(N, seed=93)
    g = ops.conv3x3_geom(n, h, w)
    res = rnd(g.rows, N, seed=94)
    ops.TRACE = []
    try:
        y = forced(lambda: ops.conv_gemm(nhwc(x), ops.pack_weight(wt, b), g, residual=res, act=AA_ACT_SILU), tile=cfg, splits=splits, tickets=False)
        assert _lib.get().aa_conv_gemm_reduce_launches(C.byref(ops.TRACE[0][0])) == 1
    finally:
        ops.TRACE = None
    ref, model = both(lambda dt, r: r(nhwc(F.silu(conv_ref(x, wt, b, dt)))) + cv(res, dt))
    accept(y, ref, model, 2e-2, "contraction")


@pytest.mark.parametrize("cfg,N", [(41, 256), (42, 320), (43, 256), (36, 256), (44, 256), (45, 128), (46, 256), (48, 128)])
@pytest.mark.parametrize("K,splits", [(128, 4), (192, 2), (320, 2), (448, 2)])
def test_split_k_with_tickets_short_and_odd_k_ranges(backend, cfg, N, K, splits):
    """K ranges of 1, 3, 5 and 7 stages with ops.USE_TICKETS: tiles 46 / 48 finish inside the kernel (asserted), the others through the
    reduce launch; two calls give the same bits."""
    M = 270
    x, w, b = rnd(M, K, seed=231), rnd(N, K, scale=0.1, seed=232), rnd(N, seed=233)
    pw = ops.pack_weight(w, b)
    ops.TRACE = []
    try:
        y = forced(lambda: ops.conv_gemm(x, pw, ops.linear_geom(M)), tile=cfg, splits=splits, tickets=True)
        tickets = _lib.get().aa_conv_gemm_tickets(C.byref(ops.TRACE[0][0]))
    finally:
        ops.TRACE = None
    assert (tickets > 0) == (cfg in (46, 47, 48)), tickets
    y2 = forced(lambda: ops.conv_gemm(x, pw, ops.linear_geom(M)), tile=cfg, splits=splits, tickets=True)
    assert torch.equal(y, y2)
    ref, model = both(lambda dt, r: cv(x, dt) @ cv(w, dt).t() + cv(b, dt))
    accept(y, ref, model, 2e-2, "contraction")


@pytest.mark.parametrize("M,K,D,with_res", [(70, 64, 64, False), (150, 64, 128, True), (200, 128, 192, False), (200, 128, 384, False)])
def test_geglu(backend, M, K, D, with_res):
    x, w, b = rnd(M, K, seed=8), rnd(2 * D, K, scale=0.2 if K == 64 else 0.1, seed=9), rnd(2 * D, seed=10)
    r_ = rnd(M, D, seed=59) if with_res else None
    y = ops.conv_gemm(x, ops.pack_weight(w, b, geglu=True), ops.linear_geom(M), residual=r_)

    def fn(dt, r):
        h = cv(x, dt) @ cv(w, dt).t() + cv(b, dt)
        z = h[:, :D] * F.gelu(h[:, D:])
        return r(z) + cv(r_, dt) if with_res else z
    ref, model = both(fn)
    accept(y, ref, model, 2e-2, "contraction")


def test_linear_fp32_out_scale_rowbias(backend):
    M, K, N = 130, 64, 192
    x, w, b = rnd(M, K, seed=5), rnd(N, K, scale=0.1, seed=6), rnd(M, seed=7)
    y = ops.conv_gemm(x, ops.pack_weight(w), ops.linear_geom(M), bias=b, bias_per_row=True, out_dtype=torch.float32, out_scale=0.5)
    assert y.dtype == torch.float32
    ref, model = both(lambda dt, r: 0.5 * (cv(x, dt) @ cv(w, dt).t() + cv(b, dt)[:, None]), out_bf16=False)
    accept(y, ref, model, 2e-2, "fp32-output")


@pytest.mark.parametrize("shape", ["dma", "generic", "splitk"])
def test_conv_gemm_acc_scale(backend, shape):
    """out = acc_scale * (x W^T + b) + residual (test_svd.test_conv_gemm_acc_scale)."""
    m, k, n = (300, 64, 64) if shape != "splitk" else (40, 2048, 64)
    if shape == "generic":
        k = 24
    x, wt, bias, res = rnd(m, k, seed=3), rnd(n, k, scale=k ** -0.5, seed=4), rnd(n, seed=5), rnd(m, n, seed=6)
    got = forced(lambda: ops.conv_gemm(x, ops.pack_weight(wt, bias), ops.linear_geom(m), residual=res, acc_scale=0.375), splits=4 if shape == "splitk" else 0)
    ref, model = both(lambda dt, r: 0.375 * (cv(x, dt) @ cv(wt, dt).t() + cv(bias, dt)) + cv(res, dt))
    accept(got, ref, model, 3e-3, "contraction", rel=True)


@pytest.mark.parametrize("big", [4, 30, 37, 39, 42])
def test_sparse_last_round_is_split_to_small_tiles(backend, big):
    """DEBUG_ABLATE 4 (a 2-CU chip): two full rounds of a big tile + a tail handed to a small-tile launch; the tail rows on their own."""
    n, h, w, cin, N = 3, 15, 16, 64, 320
    x, wt, b = rnd(n, cin, h, w, seed=71), rnd(N, cin, 3, 3, scale=0.05, seed=72), rnd(N, seed=73)
    g = ops.conv3x3_geom(n, h, w)
    res = rnd(g.rows, N, seed=74)
    y = forced(lambda: ops.conv_gemm(nhwc(x), ops.pack_weight(wt, b), g, residual=res), tile=big, ablate=4)
    ref, model = both(lambda dt, r: r(nhwc(conv_ref(x, wt, b, dt))) + cv(res, dt))
    accept(y[:512], ref[:512], model[:512], 2e-2, "contraction")
    accept(y[512:], ref[512:], model[512:], 2e-2, "contraction", note="tail")


# ===================================================================================================== folded LayerNorm
def ln_fold_pair(y, w1, b1, gamma, beta, N, geglu):
    """LayerNorm -> projection (-> GEGLU) on the stored rows `y`; the model rounds W diag(gamma) (ops.pack_weight(ln=...)) and the output."""
    def fn(dt, r):
        yf = cv(y, dt)
        xn = F.layer_norm(yf, (yf.shape[1],), None, None, 1e-5)
        h = xn @ r(cv(w1, dt) * cv(gamma, dt)[None, :]).t() + (cv(w1, dt) @ cv(beta, dt) + cv(b1, dt))
        return h[:, :N] * F.gelu(h[:, N:]) if geglu else h
    return both(fn)


def check_row_sums(st, y):
    """The fp16 tests' bounds, unchanged: fp32 sums over the stored values, bf16 products are exact in fp32."""
    yf = y.float().cpu()
    tot = st.data.float().sum(dim=1).cpu()
    for got, want in ((tot[:, 0], yf.sum(dim=1)), (tot[:, 1], (yf * yf).sum(dim=1))):
        assert (got - want).abs().max().item() <= 2e-3 * max(1.0, want.abs().max().item()), (got - want).abs().max().item()


@pytest.mark.parametrize("M,C_,ptile,ctile,geglu", [(300, 320, 49, 39, False), (300, 320, 39, 36, True), (520, 256, 36, 38, True), (300, 256, 38, 1, False),
                                                   (200, 640, 49, 49, False), (300, 128, 47, 0, False), (300, 256, 46, 3, True),
                                                   (300, 640, 47, 36, True), (200, 1280, 46, 39, False)])
def test_layernorm_folded_into_the_consuming_contraction(backend, M, C_, ptile, ctile, geglu):
    """row_stats through dot2_f32(bf16_t) / ones_pair(bf16_t) on what the producer stores; the consumer on the un-normalised rows."""
    a, w0, b0, r_ = rnd(M, 128, seed=201), rnd(C_, 128, scale=0.2, seed=202), rnd(C_, seed=203), rnd(M, C_, seed=204) + 3.0
    N = 640 if ops.TILE_TABLE[ctile][1] == 320 else 384
    w1, b1 = rnd(2 * N if geglu else N, C_, scale=0.08, seed=205), rnd(2 * N if geglu else N, seed=206)
    gamma, beta = rnd(C_, seed=207) * 0.3 + 1.0, rnd(C_, seed=208) * 0.2
    y, st = forced(lambda: ops.conv_gemm(a, ops.pack_weight(w0, b0), ops.linear_geom(M), residual=r_, row_stats=True), tile=ptile)
    assert st is not None and st.rows == M and st.data.shape == (M, st.parts, 2) and y.dtype == BF
    check_row_sums(st, y)
    ref, model = both(lambda dt, r: cv(a, dt) @ cv(w0, dt).t() + cv(b0, dt) + cv(r_, dt))
    accept(y, ref, model, 2e-2, "ln-fold", note="producer")
    pw = ops.pack_weight(w1, b1, geglu=geglu, ln=(gamma, beta, 1e-5))
    assert pw.bias is None and pw.ln_cols.shape == (2, pw.n_pad)
    z = _ln_fold_consume(y, st, pw, ctile, raw=True)
    z4 = _ln_fold_consume(y, st, pw, ctile, raw=False)
    ref, model = ln_fold_pair(y, w1, b1, gamma, beta, N, geglu)
    accept(z, ref, model, 2e-2, "ln-fold", note="raw sums")
    accept(z4, ref, model, 2e-2, "ln-fold", note="aa_ln_finalize")


@pytest.mark.parametrize("M,C_,ptile,ctile,geglu", [(300, 320, 49, 39, False), (500, 320, 39, 36, True), (520, 256, 36, 38, True), (300, 256, 46, 1, False),
                                                   (200, 128, 47, 0, False), (300, 256, 40, 3, True), (700, 320, 37, 49, False)])
def test_layernorm_coefficients_from_the_producer(backend, M, C_, ptile, ctile, geglu):
    """row_coef: the producer writes (-mean, sqrt(var + eps), rstd, 0) itself - bit-equal to aa_ln_finalize on the partial sums."""
    a, w0, b0, r_ = rnd(M, 128, seed=261), rnd(C_, 128, scale=0.2, seed=262), rnd(C_, seed=263), rnd(M, C_, seed=264) + 2.0
    N = 640 if ops.TILE_TABLE[ctile][1] == 320 else 384
    w1, b1 = rnd(2 * N if geglu else N, C_, scale=0.08, seed=265), rnd(2 * N if geglu else N, seed=266)
    gamma, beta = rnd(C_, seed=267) * 0.3 + 1.0, rnd(C_, seed=268) * 0.2
    pw0 = ops.pack_weight(w0, b0)
    y, st = forced(lambda: ops.conv_gemm(a, pw0, ops.linear_geom(M), residual=r_, row_stats=True, coef_eps=1e-5), tile=ptile)
    y2, st2 = forced(lambda: ops.conv_gemm(a, pw0, ops.linear_geom(M), residual=r_, row_stats=True), tile=ptile)
    assert st is not None and st.data is None and st._coef.shape == (M, 4), "the tile spans the row: coefficients expected"
    assert torch.equal(y, y2) and st2.data is not None
    assert torch.equal(st._coef.cpu(), st2.coef(C_, 1e-5).cpu())
    check_row_sums(st2, y)
    yd = y.double().cpu()
    mean, rstd = yd.mean(1), 1.0 / torch.sqrt(yd.var(1, unbiased=False) + 1e-5)
    coef = st._coef.double().cpu()
    assert (-coef[:, 0] - mean).abs().max().item() <= 2e-3 * max(1.0, mean.abs().max().item())
    assert (coef[:, 2] - rstd).abs().max().item() <= 2e-3 * max(1.0, rstd.abs().max().item())
    z = forced(lambda: ops.conv_gemm(y, ops.pack_weight(w1, b1, geglu=geglu, ln=(gamma, beta, 1e-5)), ops.linear_geom(M), ln_stats=st), tile=ctile)
    ref, model = ln_fold_pair(y, w1, b1, gamma, beta, N, geglu)
    accept(z, ref, model, 2e-2, "ln-fold")


@pytest.mark.parametrize("ctile,geglu", [(36, False), (36, True), (38, True), (39, False), (14, False), (3, True), (49, False)])
def test_layernorm_fold_with_a_split_off_last_round(backend, ctile, geglu):
    M, C_ = 720, 320
    N = 320 if ops.TILE_TABLE[ctile][1] == 320 else (384 if geglu else 256)
    y = rnd(M, C_, seed=231) * 2.0 + 1.5
    w1, b1 = rnd(2 * N if geglu else N, C_, scale=0.06, seed=232), rnd(2 * N if geglu else N, seed=233)
    gamma, beta = rnd(C_, seed=234) * 0.3 + 1.0, rnd(C_, seed=235) * 0.2
    yf = y.float()
    st = ops.RowStats(torch.stack([yf.sum(1), (yf * yf).sum(1)], dim=1).reshape(M, 1, 2).contiguous().to(DEV), M, 1)
    z = _ln_fold_consume(y, st, ops.pack_weight(w1, b1, geglu=geglu, ln=(gamma, beta, 1e-5)), ctile, raw=False, ablate=4)
    ref, model = ln_fold_pair(y, w1, b1, gamma, beta, N, geglu)
    accept(z[:512], ref[:512], model[:512], 2e-2, "ln-fold")
    accept(z[512:], ref[512:], model[512:], 2e-2, "ln-fold", note="tail")


@pytest.mark.parametrize("C_,ptile,ctile,geglu,raw,splits", [
    (320, 49, 39, False, False, 0), (320, 49, 36, True, False, 0), (320, 49, 39, False, True, 0), (320, 49, 1, False, False, 0), (320, 49, 3, True, False, 0),
    (320, 49, 36, False, False, 3), (640, 47, 36, True, True, 0), (1280, 46, 39, False, False, 0)])
def test_layernorm_fold_cancellation(backend, C_, ptile, ctile, geglu, raw, splits):
    """Rows with mean 50 / std ~1 (bf16 ulp at 50: 0.25 - the rows are coarsely quantised, which the stored-tensor sanity ranges below allow
    for) and rows with one 200x outlier channel, through every consumer form; statistics bounds as in the fp16 test."""
    M = 300
    a, w0, b0 = rnd(M, 128, seed=241), rnd(C_, 128, scale=0.05, seed=242), rnd(C_, scale=0.5, seed=243)
    r_ = rnd(M, C_, scale=0.5, seed=244) + 50.0
    r_[5::16] -= 50.0
    r_[5::16, 13] += 200.0
    bn = ops.TILE_TABLE[ctile][1]
    N = 640 if bn == 320 else (384 if geglu or bn < 256 else 512)
    w1, b1 = rnd(2 * N if geglu else N, C_, scale=0.08, seed=245), rnd(2 * N if geglu else N, seed=246)
    gamma, beta = rnd(C_, seed=247) * 0.3 + 1.0, rnd(C_, seed=248) * 0.2
    y, st = forced(lambda: ops.conv_gemm(a, ops.pack_weight(w0, b0), ops.linear_geom(M), residual=r_, row_stats=True), tile=ptile)
    assert st is not None
    yf = y.float().cpu()
    assert 45.0 < yf[0].mean().item() < 55.0 and 0.5 < yf[0].std().item() < 2.0 and yf[5].abs().max().item() > 150.0
    z = _ln_fold_consume(y, st, ops.pack_weight(w1, b1, geglu=geglu, ln=(gamma, beta, 1e-5)), ctile, raw, splits)
    ref, model = ln_fold_pair(y, w1, b1, gamma, beta, N, geglu)
    accept(z, ref, model, 2e-2, "ln-fold")
    tot = st.data.float().sum(dim=1).cpu()
    mean = tot[:, 0] / C_
    var = tot[:, 1] / C_ - mean * mean
    assert ((mean - yf.mean(1)).abs() <= 1e-4 * yf.mean(1).abs().clamp_min(1.0)).all()
    assert ((var - yf.var(1, unbiased=False)).abs() <= 1e-2 * yf.var(1, unbiased=False)).all()


# ===================================================================================================== norms
@pytest.mark.parametrize("C_", [64, 320, 640, 1280])
def test_layernorm(backend, C_):
    x, g, b = rnd(11, C_, seed=28) * 3 + 1, rnd(C_, seed=29), rnd(C_, seed=30)
    ref, model = both(lambda dt, r: F.layer_norm(cv(x, dt), (C_,), cv(g, dt), cv(b, dt), 1e-5))
    accept(ops.layernorm(x, g, b, 1e-5), ref, model, 2e-2, "norms")


def gn_pair(x, gamma, beta, n, frames, C_, hw, groups, silu):
    def fn(dt, r):
        x5 = cv(x, dt).reshape(n // frames, frames, C_, hw).permute(0, 2, 1, 3)          # [B,C,T,HW]
        y = F.group_norm(x5, groups, cv(gamma, dt), cv(beta, dt), 1e-5)
        return (F.silu(y) if silu else y).permute(0, 2, 3, 1).reshape(-1, C_)
    return both(fn)


def gn_forms(x0, x1, gamma, beta, n_img, per, groups, silu):
    """ops.groupnorm without the autotuner: the library's own choice, then the statistics + apply pair; the plans of both calls."""
    lib = _lib.get()
    ops.GN_PLANS = []
    tune, ops.AUTOTUNE = ops.AUTOTUNE, False
    try:
        y1 = ops.groupnorm(x0, gamma, beta, n_img, per, groups, eps=1e-5, silu=silu, x1=x1)
        lib.aa_set_groupnorm_two_pass(1)
        y2 = ops.groupnorm(x0, gamma, beta, n_img, per, groups, eps=1e-5, silu=silu, x1=x1)
    finally:
        lib.aa_set_groupnorm_two_pass(0)
        ops.AUTOTUNE = tune
        plans, ops.GN_PLANS = ops.GN_PLANS, None
    return y1, y2, plans


@pytest.mark.parametrize("C_,hw,frames,c1,groups,one_pass", [(64, 37, 1, 0, 32, None), (64, 37, 1, 24, 32, None), (80, 37, 3, 0, 8, None), (2560, 3, 1, 0, 32, None),
                                                            (320, 64, 1, 0, 32, True), (640, 100, 1, 320, 32, True), (1280, 64, 3, 0, 32, True),
                                                            (96, 50, 2, 0, 32, True), (2560, 256, 1, 1280, 32, True)])
def test_groupnorm(backend, C_, hw, frames, c1, groups, one_pass):
    """One-pass and two-pass forms, two concatenated sources, per-frame and clip-wide (frames > 1) statistics, 2560 channels."""
    n = (3 if one_pass is None else 2) * frames
    c0 = C_ - c1
    x = rnd(n, C_, hw, 1, seed=141) * 1.5 - 0.7
    gamma, beta = rnd(C_, seed=142), rnd(C_, seed=143)
    tok = nhwc(x)
    x0, x1 = (tok, None) if c1 == 0 else (tok[:, :c0].contiguous(), tok[:, c0:].contiguous())
    y1, y2, plans = gn_forms(x0, x1, gamma, beta, n // frames, frames * hw, groups, True)
    assert plans[1] is None and (one_pass is None or plans[0] is not None), plans
    ref, model = gn_pair(x, gamma, beta, n, frames, C_, hw, groups, True)
    accept(y1, ref, model, 2e-2, "norms", note="one kernel" if plans[0] is not None else "two kernels")
    accept(y2, ref, model, 2e-2, "norms", note="two kernels")


def test_groupnorm_large_mean(backend):
    """mean 50 / -70, std 1 in bf16 storage (ulp 0.25 .. 0.5): pivot-centred statistics, both forms."""
    n, C_, hw, groups = 2, 64, 300, 8
    g = torch.Generator().manual_seed(131)
    x = torch.randn(n, C_, hw, 1, generator=g) + 50.0
    x[:, 32:] -= 120.0
    x = x.to(BF).to(DEV)
    gamma, beta = torch.ones(C_, dtype=BF, device=DEV), torch.zeros(C_, dtype=BF, device=DEV)
    y1, y2, _ = gn_forms(nhwc(x), None, gamma, beta, n, hw, groups, False)
    ref, model = gn_pair(x, gamma, beta, n, 1, C_, hw, groups, False)
    accept(y1, ref, model, 5e-3, "norms")
    accept(y2, ref, model, 5e-3, "norms", note="two kernels")


@pytest.mark.parametrize("groups_img,per,x_mean", [(3, 64, 0.0), (2, 160, 50.0), (5, 32, 3.0)])
def test_groupnorm_coef(backend, groups_img, per, x_mean):
    """The statistics pass alone, fp32 (scale, shift) per image group and channel, against fp64.  (No fp16 test looks at the coefficients
    themselves; the cap uses 2e-3, the tightest tolerance any fp16 kernel test applies to a 16-bit result.)"""
    C_, rows = 320, groups_img * per
    g = torch.Generator().manual_seed(21)
    r = lambda *s: torch.randn(*s, generator=g)
    x = (r(rows, C_) * (1.0 + r(1, C_).abs()) + x_mean + r(groups_img, 1, 1).repeat(1, per, 1).reshape(rows, 1)).to(BF).to(DEV)
    gamma, beta = (1.0 + 0.3 * r(C_)).to(BF).to(DEV), (0.2 * r(C_)).to(BF).to(DEV)
    coef = ops.groupnorm_coef(x, gamma, beta, groups_img, per, 32, 1e-6)
    assert coef.dtype == torch.float32 and coef.shape == (groups_img, 2, C_)

    def fn(dt, _):
        xg = cv(x, dt).reshape(groups_img, per, 32, C_ // 32)
        mean = xg.mean(dim=(1, 3), keepdim=True)
        rstd = 1.0 / torch.sqrt(xg.var(dim=(1, 3), unbiased=False, keepdim=True) + 1e-6)
        scale = (rstd.expand(groups_img, 1, 32, C_ // 32).reshape(groups_img, C_)) * cv(gamma, dt)
        shift = cv(beta, dt) - mean.expand(groups_img, 1, 32, C_ // 32).reshape(groups_img, C_) * scale
        return torch.stack([scale, shift], dim=1)
    ref, model = both(fn, out_bf16=False)
    accept(coef, ref, model, 2e-3, "fp32-output")


# ===================================================================================================== glue
def test_softmax_rows_and_timestep_embedding(backend):
    g = torch.Generator().manual_seed(35)
    s = (torch.randn(5, 300, generator=g) * 4).to(DEV)
    ref, model = both(lambda dt, r: cv(s, dt).softmax(-1))
    y = ops.softmax_rows(s, BF)
    assert y.dtype == BF
    accept(y, ref, model, 2e-3, "glue")
    t = torch.tensor([951.0, 3.0, 0.0, 501.5], dtype=torch.float32, device=DEV)

    def emb(dt, r):
        freq = torch.exp(-math.log(10000.0) * torch.arange(160, dtype=dt) / 160)
        arg = cv(t, dt)[:, None] * freq[None, :]
        return torch.cat([arg.cos(), arg.sin()], dim=-1)
    ref, model = both(emb)
    accept(ops.timestep_embedding(t, 320, BF), ref, model, 2e-3, "glue")


@pytest.mark.parametrize("with_mask,sample_f32", [(True, True), (False, False)])
def test_pack_latents(backend, with_mask, sample_f32):
    bs, b, c, frames, h, w = 1, 2, 4, 3, 3, 5
    g = torch.Generator().manual_seed(151)
    sample = torch.randn(bs, c, frames, h, w, generator=g).to(torch.float32 if sample_f32 else BF).to(DEV)
    cond = rnd(bs, c, 1, h, w, seed=152)
    mask = (torch.rand(1, 1, 1, h, w, generator=g) > 0.5).to(BF).to(DEV) if with_mask else None
    y = ops.pack_latents(sample, cond, mask, b, BF)
    full = torch.cat([cond.float().cpu(), sample.float().cpu()], dim=2).repeat(b // bs, 1, 1, 1, 1)
    if with_mask:
        full = torch.cat([mask.float().cpu().repeat(b, 1, frames + 1, 1, 1), full], dim=1)
    ref = torch.zeros(b, frames + 1, h, w, 8)
    ref[..., :full.shape[1]] = full.permute(0, 2, 3, 4, 1)
    assert y.dtype == BF and torch.equal(y.cpu(), ref.reshape(-1, 8).to(BF))


def state_close(got, want):
    """The fp32 state, to the fp16 tests' 1e-5."""
    got, want = got.float().cpu(), want.float().cpu()
    assert (got - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())


def test_cfg_dpm_step(backend):
    """The bf16 copy of the latents is the round-to-nearest of the fp32 state, exactly."""
    n = 1000
    g = torch.Generator().manual_seed(35)
    eu, et = rnd(n, seed=36), rnd(n, seed=37)
    x, x0p = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    lp = torch.empty(n, dtype=BF, device=DEV)
    xr, x0r = x.clone(), x0p.clone()
    ops.cfg_dpm_step(eu, et, x, x0p, lp, 9.0, 0.7, 0.71, 0.9, -0.2, -0.05)
    eps = eu.float() + 9.0 * (et.float() - eu.float())
    x0 = (xr - 0.7 * eps) / 0.71
    state_close(x, 0.9 * xr + 0.2 * x0 + 0.05 * (x0 - x0r))
    state_close(x0p, x0)
    assert torch.equal(lp.cpu(), x.cpu().to(BF))


@pytest.mark.parametrize("cfg", [True, False])
def test_cfg_dpm_step_tokens(backend, cfg):
    clips, c, frames, h, w, ld = 2, 4, 3, 2, 5, 4
    b = 2 * clips if cfg else clips
    g = torch.Generator().manual_seed(161)
    eps_tok = rnd(b * (frames + 1) * h * w, ld, seed=162)
    x = torch.randn(clips, c, frames, h, w, generator=g).to(DEV)
    x0p = torch.randn(clips, c, frames, h, w, generator=g).to(DEV)
    lp = torch.empty(clips, c, frames, h, w, dtype=BF, device=DEV)
    nt = torch.zeros(b, dtype=torch.float32, device=DEV)
    xr, x0r = x.clone().cpu(), x0p.clone().cpu()
    k = dict(sigma_s=0.7, alpha_s=0.71, c_x=0.9, c_d0=-0.2, c_d1=-0.05)
    ops.cfg_dpm_step_tokens(eps_tok, x, x0p, lp, 9.0 if cfg else None, k, next_t=nt, next_t_value=913.0)
    e = eps_tok.float().cpu().reshape(b, frames + 1, h, w, ld).permute(0, 4, 1, 2, 3)[:, :c, 1:]
    eps = e[:clips] + 9.0 * (e[clips:] - e[:clips]) if cfg else e
    x0 = (xr - 0.7 * eps) / 0.71
    state_close(x, 0.9 * xr + 0.2 * x0 + 0.05 * (x0 - x0r))
    state_close(x0p, x0)
    assert torch.equal(lp.cpu(), x.cpu().to(BF))
    assert torch.equal(nt.cpu(), torch.full((b,), 913.0))


@pytest.mark.parametrize("guided", [True, False])
def test_cfg_euler_step_tokens(backend, guided):
    """bf16 v-prediction tokens into the fp32 Euler state (this step keeps no 16-bit copy of the latents: the state alone is checked)."""
    g = torch.Generator().manual_seed(2)
    clips, f, c, h, w = 2, 3, 4, 3, 5
    v = rnd((2 if guided else 1) * clips * f * h * w, 4, seed=7)
    x = torch.randn(clips, f, c, h, w, generator=g)
    scale_f = torch.linspace(1.0, 3.0, f)
    v5 = v.float().cpu().reshape(-1, clips, f, h, w, c).permute(0, 1, 2, 5, 3, 4)
    vv = v5[0] + scale_f.reshape(1, f, 1, 1, 1) * (v5[1] - v5[0]) if guided else v5[0]
    want = 0.9 * x + (-0.2) * vv
    xd, nt, ns = x.to(DEV), torch.zeros(4, device=DEV), torch.zeros(1, device=DEV)
    ops.cfg_euler_step_tokens(v, xd, scale_f.to(DEV) if guided else None, 0.9, -0.2, next_t=nt, next_t_value=1.25, next_scale=ns, next_scale_value=0.5)
    state_close(xd, want)
    assert torch.all(nt.cpu() == 1.25) and ns.item() == 0.5


def test_blend(backend):
    """The four uses of aa_blend in test_svd.test_blend_kernel."""
    x, y = rnd(60, 24, seed=1), rnd(60, 24, seed=2)
    rv = rnd(5, 40, seed=3)[:, 8:32]                                    # a column slice of a wider matrix
    ref, model = both(lambda dt, r: 0.3 * cv(x, dt) + 0.7 * cv(y, dt))
    accept(ops.blend(x, y, 0.3, 0.7), ref, model, 2e-3, "glue", rel=True)
    idx = (torch.arange(60) // 4) % 5
    ref, model = both(lambda dt, r: cv(x, dt) + cv(rv, dt)[idx])
    accept(ops.blend(x, rowvec=rv, rowvec_div=4, rowvec_mod=5), ref, model, 2e-3, "glue", rel=True)
    ref, model = both(lambda dt, r: F.silu(cv(x, dt) + cv(y, dt)))
    accept(ops.blend(x, y, act=AA_ACT_SILU), ref, model, 2e-3, "glue", rel=True)
    ref, model = both(lambda dt, r: cv(x, dt) + cv(rv, dt)[torch.arange(60) % 5])
    accept(ops.blend(x, rowvec=rv, rowvec_div=1, rowvec_mod=5, out=x.clone()), ref, model, 2e-3, "glue", rel=True)
