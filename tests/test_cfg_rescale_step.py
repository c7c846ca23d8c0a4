"""aa_cfg_rescale_tokens (guidance_rescale, diffusers `rescale_noise_cfg`, per clip on the UNet's token-layout output; two launches) against
the formula in float64 evaluated from the same rounded inputs, on the emulator and on the GPU: the smallest legal clip (n = 2), the
hand-made step of test_ddim_step.py, odd sizes with three clips, several workgroups per clip with a ragged tail, row pitches 4 / 8 / 16,
the benchmark's shape; fp16 and bf16, guidance 1.5 and 9, rescale 0 / 0.7 / 1, inputs of mean 0 and mean 50, clips of different scale
(deviation 1 and 0.01), the two halves from different seeds, a constant clip (std(c) == 0: k = 1), in place against out of place and
a second call bit for bit, sentinels around everything that must not be touched, and every refusal of the entry point.

    c = u + g (t - u),   k = 1 + phi (sd_t / sd_c - 1),   e = k c          (sd: unbiased, over the clip's n elements)

Bound (eps = 2^-24; from the arithmetic, no measurement behind it).
 * c: g handed over in fp32, one subtraction, one product (together 3 eps on |g (t - u)|) and one addition (eps on |c|):
       err_c = eps (3 |g (t - u)| + |c|) (1 + 2^-20)          per element (a fused multiply-add only drops a rounding)
 * sd_c: the deviation is Lipschitz in the sup norm, |sd(a) - sd(b)| <= sqrt(n / (n - 1)) max|a - b|, so the kernel's deviation of its
   fp32 c lies within D_c = sqrt(n / (n - 1)) max err_c + acc sd_c of sd_c.  sd_t is exact up to the accumulation: D_t = acc sd_t.
   acc = 2^-30: fp64 sums of n <= 2^19 terms (n 2^-53 <= 2^-34 relative to the sum of the magnitudes), taken about the clip's first
   element x_0, which costs a factor 1 + z^2 with z = (x_0 - mean) / sd in the difference sum d^2 - (sum d)^2 / n; the test asserts
   z^2 <= 31 on its inputs, and the square root halves the relative error.  (2^-34 * 2^5 / 2 = 2^-30.)
 * the factor: r = sd_t / sd_c lies below (sd_t + D_t) / (sd_c - D_c) (the test asserts D_c < sd_c / 2 on the reference); one
   division and one square root per deviation (3 eps r), phi handed over in fp32 and the product with r - 1 (2 eps phi |r - 1|), the
   final addition (eps |k|):
       D_k = phi (D_r + 3 eps r) + 2 eps phi |r - 1| + eps |k|
   (the kernel forms the factor in fp64 and rounds it once to fp32, inside this model).  `factor` is held to D_k.
   rescale = 0 and a constant clip give k = 1 exactly: D_k = 0.
 * e: |k| err_c + D_k (|c| + err_c) and the rounding of the product, eps (|k c| + that); the store adds half an ulp of the storage
   type at |e| (2^-11 relative in fp16 above 2^-14, 2^-8 in bf16)."""
import ctypes as C
import functools
import math

import pytest
import torch

import test_ddim_step
from animate_anything_amd import _lib, ops
from test_ddim_step import backend  # noqa: F401  (the emulator / GPU fixture; it sets test_ddim_step.DEV)

EPS = 2.0 ** -24
ACC = 2.0 ** -30
SENTINEL = 768.0                                       # (exact in fp16 and bf16)
GUARD = 2                                              # rows behind the last one: never read into the result, never written
SHAPES = [(1, 1, 1, 2, 8), (2, 4, 3, 10, 8), (3, 4, 2, 37, 8), (2, 4, 5, 1031, 8),
          (2, 4, 3, 10, 4), (2, 4, 3, 10, 16), (2, 4, 5, 1031, 4), (2, 4, 5, 1031, 16)]
BENCH_SHAPE = (1, 4, 16, 4096, 8)
GUIDANCES = (1.5, 9.0)
RESCALES = (0.0, 0.7, 1.0)
CLIP_SCALE = (1.0, 0.01, 1.0)


def dev():
    return test_ddim_step.DEV


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
def tokens_of(shape, dt, mean, constant_clip=-1):
    """The rounded token matrix [2 * rows + GUARD, ld] (CPU): sentinels in frame 0, the padding columns and the guard rows; clip b of
    deviation CLIP_SCALE[b] about `mean`; the unconditional and the text half from different seeds."""
    clips, ch, frames, hw, ld = shape
    rows = clips * (frames + 1) * hw
    tok = torch.full((2 * rows + GUARD, ld), SENTINEL, dtype=dt)
    for half, seed in ((0, 211), (1, 977)):
        g = torch.Generator().manual_seed(seed + 13 * SHAPES.index(shape) if shape in SHAPES else seed)
        x = torch.randn(clips, frames, hw, ch, generator=g) * torch.tensor(CLIP_SCALE[:clips]).reshape(clips, 1, 1, 1) + mean
        if constant_clip >= 0:
            x[constant_clip] = mean + 0.25 + half                                 # u and t constant (and different): c is constant
        valid(tok, shape, half).copy_(x.to(dt))
    return tok


@functools.lru_cache(maxsize=None)
def reference(shape, dt, mean, guidance, rescale, constant_clip=-1):
    """float64 from the rounded inputs: (e, bound of e before the store, k, D_k), the first two [clips, frames, hw, channels]."""
    clips, ch, frames, hw, _ = shape
    n = ch * frames * hw
    tok = tokens_of(shape, dt, mean, constant_clip).double()
    u, t = valid(tok, shape, 0), valid(tok, shape, 1)
    g32, phi32 = float(torch.tensor(guidance, dtype=torch.float32)), float(torch.tensor(rescale, dtype=torch.float32))
    c = u + guidance * (t - u)
    err_c = EPS * (3 * abs(guidance) * (t - u).abs() + c.abs()) * (1 + 2.0 ** -20) + abs(g32 - guidance) * (t - u).abs()
    flat = lambda v: v.reshape(clips, -1)
    sd_t, sd_c = flat(t).std(dim=1), flat(c).std(dim=1)
    k, d_k = torch.ones(clips, dtype=torch.float64), torch.zeros(clips, dtype=torch.float64)
    for b in range(clips):
        if rescale == 0.0 or flat(c)[b].max() == flat(c)[b].min():
            continue                                                              # k = 1 exactly
        for v in (flat(t)[b], flat(c)[b]):                                        # the premise of `acc`
            z2 = ((v[0] - v.mean()) ** 2 / v.var(unbiased=False)).item()
            assert z2 <= 31.0, f"first element {z2 ** 0.5:.1f} deviations off the mean: the accumulation model does not cover this input"
        st, sc = sd_t[b].item(), sd_c[b].item()
        dc = math.sqrt(n / (n - 1)) * flat(err_c)[b].max().item() + ACC * sc
        assert dc < 0.5 * sc, "std(c) is not resolved by fp32 on this input"
        r = st / sc
        d_r = (st + ACC * st) / (sc - dc) - r
        k[b] = 1.0 + rescale * (r - 1.0)
        d_k[b] = rescale * (d_r + 3 * EPS * r) + 2 * EPS * rescale * abs(r - 1.0) + EPS * abs(k[b].item()) + abs(phi32 - rescale) * abs(r - 1.0)
    kk, dk = k.reshape(clips, 1, 1, 1), d_k.reshape(clips, 1, 1, 1)
    e = kk * c
    err32 = kk.abs() * err_c + dk * (c.abs() + err_c)
    err32 = err32 + EPS * (e.abs() + err32)
    return e, err32, k, d_k


def run(shape, dt, mean, guidance, rescale, in_place, constant_clip=-1, out_pad=4):
    """One call on the backend; checks everything that must stay untouched; returns (valid output on the CPU, factor on the CPU)."""
    clips, ch, frames, hw, ld = shape
    rows = clips * (frames + 1) * hw
    before = tokens_of(shape, dt, mean, constant_clip)
    buf = before.clone().to(dev())
    tok = buf[:2 * rows]
    factor = torch.full((clips,), -5.0, dtype=torch.float32).to(dev())
    if in_place:
        got = ops.cfg_rescale_tokens(tok, clips, ch, frames, hw, guidance, rescale, factor=factor)
        assert got.data_ptr() == tok.data_ptr() and got.shape[0] == rows and got.stride(0) == ld
        after = buf.cpu()
        keep = after.clone()
        valid(keep, shape, 0).copy_(valid(before, shape, 0))                      # everything but the valid region of the first half ...
        assert torch.equal(keep.view(torch.int16), before.view(torch.int16)), "wrote outside the unconditional clips' frames 1..T"
        return valid(after, shape, 0).clone(), factor.cpu()
    obuf = torch.full((rows + GUARD, ld + out_pad), SENTINEL, dtype=dt).to(dev())
    got = ops.cfg_rescale_tokens(tok, clips, ch, frames, hw, guidance, rescale, out=obuf[:rows], factor=factor)
    assert got.data_ptr() == obuf.data_ptr()
    assert torch.equal(buf.cpu().view(torch.int16), before.view(torch.int16)), "the input is only read"
    after = obuf.cpu()
    keep = after.clone()
    valid(keep, shape, 0).fill_(SENTINEL)
    assert (keep.float() == SENTINEL).all(), "wrote frame 0, a padding column or a guard row"
    return valid(after, shape, 0).clone(), factor.cpu()


def check(shape, dt, mean, guidance, rescale, constant_clip=-1):
    e, err32, k, d_k = reference(shape, dt, mean, guidance, rescale, constant_clip)
    bound = err32 + half_ulp(e.abs() + err32, dt)
    got, factor = run(shape, dt, mean, guidance, rescale, False, constant_clip)
    err, f_err = (got.double() - e).abs(), (factor.double() - k).abs()
    print(f"{shape} {dt} mean {mean} g {guidance} phi {rescale}: k {[round(v, 5) for v in k.tolist()]} worst err/bound "
          f"{(err / bound).max().item():.3f} (max err {err.max().item():.3g}), factor err {f_err.max().item():.3g} (D_k {d_k.max().item():.3g})")
    assert (err <= bound).all()
    assert (f_err <= d_k).all()
    if rescale == 0.0:
        assert (factor == 1.0).all(), "rescale 0 must give k = 1 exactly"
    again, factor2 = run(shape, dt, mean, guidance, rescale, False, constant_clip, out_pad=0)
    inplace, factor3 = run(shape, dt, mean, guidance, rescale, True, constant_clip)
    bits = lambda v: v.contiguous().view(torch.int16)
    assert torch.equal(bits(again), bits(got)) and torch.equal(factor2, factor), "a second call must repeat the bits"
    assert torch.equal(bits(inplace), bits(got)) and torch.equal(factor3, factor), "in place must equal out of place"
    return k


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_float64_formula(backend, shape, dt):
    for mean in (0.0, 50.0):
        for guidance in GUIDANCES:
            for rescale in RESCALES:
                k = check(shape, dt, mean, guidance, rescale)
                if rescale > 0 and shape[0] > 1 and mean == 0.0:
                    assert k[0] != k[1], "clips of different scale have different factors"


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_a_constant_clip_is_left_unscaled(backend, dt):
    """std(c) == 0 on clip 1 (diffusers: NaN): k = 1 there, the other clips are rescaled as ever."""
    shape = SHAPES[2]
    for mean in (0.0, 50.0):
        k = check(shape, dt, mean, 9.0, 0.7, constant_clip=1)
        assert k[1] == 1.0 and k[0] != 1.0 and k[2] != 1.0
        _, factor = run(shape, dt, mean, 9.0, 0.7, False, constant_clip=1)
        assert factor[1] == 1.0 and torch.isfinite(factor).all()


def test_the_benchmark_shape(backend):
    check(BENCH_SHAPE, torch.float16, 0.0, 9.0, 0.7)


def test_refusals_leave_the_output_untouched(backend):
    clips, ch, frames, hw, ld = 2, 4, 3, 10, 8
    rows, dt = clips * (frames + 1) * hw, torch.float16
    d_ = dev()
    g = torch.Generator().manual_seed(5)
    arena = torch.randn(8 * rows * ld, generator=g).to(dt).to(d_)                   # one allocation: views of it can overlap
    before = arena.clone()
    e = arena.element_size()
    tokens, out = arena[:2 * rows * ld], arena[3 * rows * ld:4 * rows * ld]
    factor = torch.zeros(clips, dtype=torch.float32).to(d_)
    lib = _lib.get()

    def call(workspace="own", workspace_bytes=None, **kw):
        d = _lib.AaCfgRescale()
        t = dict(tokens=tokens, out=out, factor=factor)
        t.update({k: v for k, v in kw.items() if k in t})
        for k, v in t.items():
            setattr(d, k, None if v is None else C.c_void_p(v if isinstance(v, int) else v.data_ptr()))
        f = dict(clips=clips, channels=ch, frames=frames, hw=hw, ld=ld, out_ld=ld, guidance=9.0, rescale=0.7, dtype=_lib.AA_F16)
        f.update({k: v for k, v in kw.items() if k in f})
        for k, v in f.items():
            setattr(d, k, v)
        ws = torch.zeros(64, dtype=torch.float64).to(d_) if isinstance(workspace, str) else workspace
        ptr = None if ws is None else C.c_void_p(ws if isinstance(ws, int) else ws.data_ptr())
        nbytes = 512 if workspace_bytes is None else workspace_bytes
        return lib.aa_cfg_rescale_tokens(C.byref(d), ptr, nbytes, ops._stream(arena)), lib.aa_cfg_rescale_workspace(C.byref(d))

    shape_, dtype_, align_, workspace_ = -1, -2, -3, -4                             # AA_E_SHAPE, AA_E_DTYPE, AA_E_ALIGN, AA_E_WORKSPACE
    assert call(tokens=None)[1] == clips * 1 * 4 * 8                                # (the size query: one part per clip, four fp64 sums)
    assert lib.aa_cfg_rescale_tokens(None, None, 0, None) == shape_ and lib.aa_cfg_rescale_workspace(None) == 0
    for name in ("tokens", "out"):
        assert call(**{name: None})[0] == shape_, name
    assert b"null" in lib.aa_last_error()
    assert call(workspace=None)[0] == workspace_
    assert call(workspace_bytes=clips * 4 * 8 - 8)[0] == workspace_ and b"workspace" in lib.aa_last_error()
    for bad in (dict(clips=0), dict(channels=0), dict(frames=0), dict(hw=0), dict(clips=-1), dict(hw=-3), dict(clips=70000),
                dict(channels=1, frames=1, hw=1),                                   # n = 1: no deviation
                dict(ld=ch - 1), dict(out_ld=ch - 1)):
        assert call(**bad)[0] == shape_, bad
    for bad in (dict(rescale=-0.1), dict(rescale=1.5), dict(rescale=math.nan), dict(rescale=math.inf),
                dict(guidance=math.nan), dict(guidance=math.inf), dict(guidance=-math.inf)):
        assert call(**bad)[0] == shape_, bad
    overlapping = [dict(out=tokens.data_ptr() + 2 * e),                             # out over tokens, shifted
                   dict(out=tokens, out_ld=ld + 4),                                 # same pointer, another pitch
                   dict(out=tokens.data_ptr() + rows * ld * e),                     # the text half
                   dict(out=tokens.data_ptr() + ((2 * rows - 1) * ld + ch - 2) * e),  # the last two valid elements
                   dict(factor=tokens.data_ptr() + 64), dict(factor=out.data_ptr() + 64),
                   dict(workspace=tokens.data_ptr() + 64), dict(workspace=out.data_ptr() + 128),
                   dict(workspace=factor.data_ptr())]
    for bad in overlapping:
        assert call(**bad)[0] == shape_, bad
        assert b"overlap" in lib.aa_last_error()
    assert call(tokens=tokens.data_ptr() + 1)[0] == align_ and call(out=out.data_ptr() + 1)[0] == align_
    assert call(factor=factor.data_ptr() + 2)[0] == align_
    assert call(workspace=torch.zeros(64, dtype=torch.float64).to(d_)[1:].view(torch.int32)[1:], workspace_bytes=256)[0] == align_
    assert call(dtype=_lib.AA_F32)[0] == dtype_ and call(dtype=7)[0] == dtype_
    assert torch.equal(arena.cpu().view(torch.int16), before.cpu().view(torch.int16)) and (factor.cpu() == 0).all()
    # the wrapper: dtype, shape, layout and the entry point's own refusals
    tok2, out2 = tokens.view(2 * rows, ld), out.view(rows, ld)
    with pytest.raises(RuntimeError, match="token matrix"):
        ops.cfg_rescale_tokens(tok2.float(), clips, ch, frames, hw, 9.0, 0.7)
    with pytest.raises(RuntimeError, match="token matrix"):
        ops.cfg_rescale_tokens(tok2, clips, ch, frames, hw, 9.0, 0.7, out=out2.to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="token matrix"):
        ops.cfg_rescale_tokens(tok2.t(), clips, ch, frames, hw, 9.0, 0.7)
    with pytest.raises(RuntimeError, match="rows"):
        ops.cfg_rescale_tokens(tok2[:-1], clips, ch, frames, hw, 9.0, 0.7)           # a short token matrix
    with pytest.raises(RuntimeError, match="rows"):
        ops.cfg_rescale_tokens(tok2, clips, ch, frames, hw, 9.0, 0.7, out=out2[:-1])
    with pytest.raises(RuntimeError, match="rows"):
        ops.cfg_rescale_tokens(tok2, clips, ld + 1, frames, hw, 9.0, 0.7)            # more channels than columns
    with pytest.raises(RuntimeError, match="factor"):
        ops.cfg_rescale_tokens(tok2, clips, ch, frames, hw, 9.0, 0.7, out=out2, factor=torch.zeros(clips + 1).to(d_))
    with pytest.raises(RuntimeError, match="factor"):
        ops.cfg_rescale_tokens(tok2, clips, ch, frames, hw, 9.0, 0.7, out=out2, factor=torch.zeros(clips, dtype=torch.float64).to(d_))
    for bad in (dict(rescale=1.01), dict(rescale=-1.0), dict(guidance=math.inf)):
        with pytest.raises(RuntimeError, match="libaa_mi355"):
            ops.cfg_rescale_tokens(tok2, clips, ch, frames, hw, bad.get("guidance", 9.0), bad.get("rescale", 0.7), out=out2)
    with pytest.raises(RuntimeError, match="libaa_mi355"):
        ops.cfg_rescale_tokens(tok2, 0, ch, frames, hw, 9.0, 0.7, out=out2)
    with pytest.raises(RuntimeError, match="libaa_mi355"):
        ops.cfg_rescale_tokens(tok2, clips, ch, frames, hw, 9.0, 0.7, out=tok2[rows // 2:rows // 2 + rows])      # overlap, through the wrapper
    assert torch.equal(arena.cpu().view(torch.int16), before.cpu().view(torch.int16))
    # and the valid call on the same views works, on a longer token matrix too; the workspace is kept per geometry
    longer = arena[:(2 * rows + 3) * ld].view(2 * rows + 3, ld)
    got = ops.cfg_rescale_tokens(longer, clips, ch, frames, hw, 9.0, 0.7, out=out2, factor=factor)
    assert got is out2 and not torch.equal(out2.cpu(), before[3 * rows * ld:4 * rows * ld].view(rows, ld).cpu()) and (factor.cpu() != 0).all()
    key = (str(tok2.device), clips, ch, frames, hw)
    ws = ops._CFG_RESCALE_WS[key]
    ops.cfg_rescale_tokens(tok2, clips, ch, frames, hw, 9.0, 0.7, out=out2)
    assert ops._CFG_RESCALE_WS[key] is ws and ws.dtype == torch.float64
