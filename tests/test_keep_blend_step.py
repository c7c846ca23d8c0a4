"""aa_keep_blend (the known-region blend of inpainting samplers on fp32 planes x[clips, C, T, hw]; one launch) against the formula in
float64 evaluated from the same rounded inputs and the fp32-rounded a and s, on the emulator and on the GPU:

    kn  = a * known + s * noise                     (no noise operand: s = 0, kn = a * known)
    out = x where m >= 1,   kn where m <= 0,   m * x + (1 - m) * kn otherwise

Shapes: the smallest, a basic multi-clip / multi-frame one, odd sizes (element-by-element form), a 16-byte form, the same on views
shifted by one element (element by element on a vector-sized shape), several workgroups with a ragged tail, three channels (decoded
video), the benchmark's latents once.  Per shape a list of configurations covers all four broadcast forms of `known` and of `mask`,
both in fp32 / fp16 / bf16, with and without noise, abar in {0.9991, 0.5041, 0.0047} and (a, s) = (1, 0), masks all 0 / all 1 /
binary / soft / mixed (with values above 1 and below 0), inputs of mean 0 and mean 50: the two small shapes run every (broadcast,
dtype) pair and every (scalars, mask, mean, noise) tuple, the larger ones a thinned list that still holds every value of every
parameter (asserted below).

Bound for 0 < m < 1 (eps = 2^-24; from the arithmetic, not from a run):  |err| <= 8 eps (|x| + |a known| + |s noise|).  It covers
each association -ffast-math may choose for the blend - m x + (1 - m) kn, kn + m (x - kn), x + (1 - m) (kn - x) - with at most one
rounding per operation: kn costs at most 2 eps on |a known| + |s noise| (two products, one sum; fused forms drop roundings), 1 - m
one eps on a factor below 1, each product and the final sum one eps on magnitudes below |x| + |kn|; summed generously below 8 eps of
|x| + |a known| + |s noise|.  m <= 0: kn alone, the same bound without the |x| term.
Exact bits: m >= 1 gives x; m <= 0 with (a, s) = (1, 0) and no noise gives `known` widened to fp32; in place equals out of place; a
second call repeats the first.  NaN planted in x where m <= 0, and in known / noise where every element that reads them has m >= 1,
never reaches the output.  Sentinel guards in front of and behind every buffer stay untouched, the inputs are only read, and every
refusal of the entry point and of the wrapper leaves the output untouched."""
import ctypes as C
import itertools
import math

import pytest
import torch

import test_ddim_step
from animate_anything_amd import _lib, ops
from test_ddim_step import backend  # noqa: F401  (the emulator / GPU fixture; it sets test_ddim_step.DEV)

EPS = 2.0 ** -24
SENTINEL = 768.0                                       # (exact in fp16 and bf16)
GUARD = 8                                              # elements in front of and behind every buffer: 16 bytes of the 16-bit types, 32 of fp32
SMALL = [(1, 1, 1, 1), (2, 4, 3, 10), (3, 4, 2, 37)]
LARGE = [(2, 4, 3, 1024), (2, 4, 5, 1031), (1, 3, 2, 4100)]
BENCH_SHAPE = (1, 4, 16, 4096)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BROADCASTS = tuple(itertools.product((False, True), repeat=4))          # known over clips, known over frames, mask over clips, mask over frames
SCALARS = tuple((math.sqrt(ab), math.sqrt(1.0 - ab)) for ab in (0.9991, 0.5041, 0.0047)) + ((1.0, 0.0),)
KINDS = ("zeros", "ones", "binary", "soft", "mixed")
MEANS = (0.0, 50.0)


def _configs():
    """(broadcast, known dtype, mask dtype, noisy, scalars, mask kind, mean): every (broadcast, dtype pair) with the rest cycling, then
    every (scalars, kind, mean, noisy) with broadcast and dtypes cycling."""
    out = []
    for j, (bc, (kdt, mdt)) in enumerate(itertools.product(BROADCASTS, itertools.product(DTYPES, DTYPES))):
        out.append((bc, kdt, mdt, j % 2 == 0, SCALARS[(j // 2) % 4], KINDS[j % 5], MEANS[(j // 7) % 2]))
    for j, (sc, kind, mean, noisy) in enumerate(itertools.product(SCALARS, KINDS, MEANS, (True, False))):
        out.append((BROADCASTS[(5 * j + 3) % 16], DTYPES[j % 3], DTYPES[(j // 3) % 3], noisy, sc, kind, mean))
    return out


FULL = _configs()
THIN = FULL[:144:7] + FULL[144::9]
for _i, _values in enumerate((BROADCASTS, DTYPES, DTYPES, (True, False), SCALARS, KINDS, MEANS)):
    assert {c[_i] for c in THIN} == set(_values), f"the thinned list misses a value of parameter {_i}"


def dev():
    return test_ddim_step.DEV


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def guarded(data, shift):
    """[GUARD + shift sentinels | data | GUARD sentinels] as one flat buffer on the CPU."""
    buf = torch.full((2 * GUARD + shift + data.numel(),), SENTINEL, dtype=data.dtype)
    buf[GUARD + shift:GUARD + shift + data.numel()] = data.reshape(-1)
    return buf


def inside(buf, shape, shift):
    n = math.prod(shape)
    return buf[GUARD + shift:GUARD + shift + n].view(shape)


def guards_intact(buf, shape, shift):
    n = math.prod(shape)
    b = buf.cpu().float()
    return bool((b[:GUARD + shift] == SENTINEL).all() and (b[GUARD + shift + n:] == SENTINEL).all())


def make_inputs(shape, cfg, seed):
    """The rounded operands on the CPU (clean: nothing planted) and the mask expanded to x's shape."""
    clips, ch, frames, hw = shape
    (k_all_clips, k_all_frames, m_all_clips, m_all_frames), kdt, mdt, noisy, _sc, kind, mean = cfg
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) + mean
    kshape = (clips if k_all_clips else 1, ch, frames if k_all_frames else 1, hw)
    mshape = (clips if m_all_clips else 1, frames if m_all_frames else 1, hw)
    known = (torch.randn(kshape, generator=g) + mean).to(kdt)
    noise = (torch.randn(shape, generator=g) + mean) if noisy else None
    u = torch.rand(mshape, generator=g)
    soft = 0.05 + 0.9 * torch.rand(mshape, generator=g)
    if kind == "zeros":
        m = torch.zeros(mshape)
    elif kind == "ones":
        m = torch.ones(mshape)
    elif kind == "binary":
        m = (u < 0.5).float()
    elif kind == "soft":
        m = soft
    else:
        m = torch.where(u < 0.2, torch.zeros(()), torch.where(u < 0.4, torch.ones(()), torch.where(u < 0.8, soft, torch.where(u < 0.9, torch.tensor(1.5), torch.tensor(-0.25)))))
    m = m.to(mdt)
    return x, known, m, noise


def reference(x, known, m, noise, a, s):
    """float64 from the rounded inputs and the fp32-rounded scalars: (out, bound, m expanded to x's shape)."""
    a32, s32 = float(torch.tensor(a, dtype=torch.float32)), float(torch.tensor(s, dtype=torch.float32))
    xd, kd, md = x.double(), known.double().expand(x.shape), m.double()[:, None].expand(x.shape)
    nd = noise.double() if noise is not None else torch.zeros_like(xd)
    kn = a32 * kd + s32 * nd
    out = torch.where(md >= 1, xd, torch.where(md <= 0, kn, md * xd + (1 - md) * kn))
    mag = (a32 * kd).abs() + (s32 * nd).abs()
    bound = torch.where(md >= 1, torch.zeros_like(xd), 8 * EPS * torch.where(md <= 0, mag, xd.abs() + mag))
    return out, bound, md


def check(shape, cfg, seed, shift=0):
    clips, ch, frames, hw = shape
    _bc, _kdt, _mdt, noisy, (a, s), kind, mean = cfg
    if not noisy:
        s = 0.0
    x, known, m, noise = make_inputs(shape, cfg, seed)
    want, bound, md = reference(x, known, m, noise, a, s)
    # NaN where it must not matter: x under m <= 0; known / noise where every element that reads them has m >= 1
    px, pk, pn = x.clone(), known.clone(), None if noise is None else noise.clone()
    held, free = md <= 0, md >= 1
    if held.any():
        px.view(-1)[held.reshape(-1).nonzero()[0]] = math.nan
    free_k = free
    if known.shape[0] == 1:
        free_k = free_k.all(dim=0, keepdim=True)
    if known.shape[2] == 1:
        free_k = free_k.all(dim=2, keepdim=True)
    if free_k.any():
        pk.view(-1)[free_k.reshape(-1).nonzero()[0]] = math.nan
    if pn is not None and free.any():
        pn.view(-1)[free.reshape(-1).nonzero()[-1]] = math.inf
    d_ = dev()
    cpu = dict(x=guarded(px, shift), known=guarded(pk, shift), mask=guarded(m, shift), noise=None if pn is None else guarded(pn, shift))
    shapes = dict(x=shape, known=tuple(known.shape), mask=tuple(m.shape), noise=shape)

    def run(in_place):
        bufs = {k: None if v is None else v.clone().to(d_) for k, v in cpu.items()}
        view = {k: None if v is None else inside(v, shapes[k], shift) for k, v in bufs.items()}
        obuf = None if in_place else torch.full((2 * GUARD + shift + x.numel(),), SENTINEL).to(d_)
        out = None if in_place else inside(obuf, shape, shift)
        got = ops.keep_blend(view["x"], view["known"], view["mask"], a, s, noise=view["noise"], out=out)
        assert got.data_ptr() == (view["x"] if in_place else out).data_ptr() and tuple(got.shape) == shape
        for k, v in bufs.items():
            if v is None:
                continue
            assert guards_intact(v, shapes[k], shift), f"wrote around {k}"
            if not (in_place and k == "x"):
                assert torch.equal(bits(v.cpu()), bits(cpu[k])), f"{k} is only read"
        if not in_place:
            assert guards_intact(obuf, shape, shift), "wrote around out"
        return got.cpu().clone()

    got = run(False)
    assert torch.isfinite(got).all(), "a planted NaN / Inf reached the output"
    err = (got.double() - want).abs()
    assert (err <= bound).all(), f"{shape} {cfg}: worst err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}"
    assert torch.equal(bits(got)[free], bits(x)[free]), "m >= 1 hands x through bit for bit"
    if (a, s) == (1.0, 0.0) and not noisy:
        assert torch.equal(bits(got)[held], bits(known.float().expand(shape))[held]), "m <= 0 with (1, 0) gives known widened to fp32"
    assert torch.equal(bits(run(False)), bits(got)), "a second call must repeat the bits"
    assert torch.equal(bits(run(True)), bits(got)), "in place must equal out of place"
    soft = ~(held | free)
    return (err[soft] / bound[soft]).max().item() if soft.any() else 0.0


def sweep(shape, configs, shift=0):
    worst = 0.0
    for j, cfg in enumerate(configs):
        worst = max(worst, check(shape, cfg, 1000 * (SMALL + LARGE + [BENCH_SHAPE]).index(shape) + j, shift))
    print(f"{shape} shift {shift}: {len(configs)} configurations, worst err / bound where 0 < m < 1: {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_every_configuration_on_the_small_shapes(backend, shape):
    sweep(shape, FULL)


@pytest.mark.parametrize("shape", LARGE, ids=lambda s: "x".join(map(str, s)))
def test_the_larger_shapes(backend, shape):
    sweep(shape, THIN)


def test_shifted_views_take_the_element_form(backend):
    """(2, 4, 3, 1024) on views one element behind a 16-byte boundary: hw % 4 == 0, but no 16-byte access is legal."""
    sweep(LARGE[0], THIN, shift=1)


def test_the_benchmark_shape(backend):
    sweep(BENCH_SHAPE, [((False, False, False, False), torch.float16, torch.float16, True, SCALARS[1], "mixed", 0.0)])


def test_the_motion_masks_layout_and_five_dimensions(backend):
    """x as [clips, C, T, h, w] with the mask as [1, 1, 1, h, w] (the motion mask) equals the 4-d call with [1, 1, hw]."""
    shape, cfg = (2, 4, 3, 4, 6), ((False, False, False, False), torch.float16, torch.float16, True, SCALARS[1], "mixed", 0.0)
    x, known, m, noise = make_inputs((2, 4, 3, 24), cfg, 77)
    d_ = dev()
    flat = ops.keep_blend(x.to(d_), known.to(d_), m.to(d_), 0.7, 0.3, noise=noise.to(d_), out=torch.empty(x.shape).to(d_))
    five = ops.keep_blend(x.view(shape).to(d_), known.view(1, 4, 1, 4, 6).to(d_), m.view(1, 1, 1, 4, 6).to(d_), 0.7, 0.3,
                          noise=noise.view(shape).to(d_), out=torch.empty(shape).to(d_))
    assert torch.equal(bits(five.cpu().view(x.shape)), bits(flat.cpu()))


def test_refusals_leave_the_output_untouched(backend):
    clips, ch, frames, hw = 2, 4, 3, 12
    n = clips * ch * frames * hw
    d_ = dev()
    g = torch.Generator().manual_seed(5)
    arena = torch.randn(8 * n, generator=g).to(d_)                                  # one allocation: views of it can overlap
    before = arena.clone()
    x, out, known, mask, noise = arena[:n], arena[n:2 * n], arena[2 * n:3 * n], arena[3 * n:3 * n + clips * frames * hw], arena[4 * n:5 * n]
    lib = _lib.get()

    def call(**kw):
        d = _lib.AaKeepBlend()
        t = dict(x=x, out=out, known=known, mask=mask, noise=noise)
        t.update({k: v for k, v in kw.items() if k in t})
        for k, v in t.items():
            setattr(d, k, None if v is None else C.c_void_p(v if isinstance(v, int) else v.data_ptr()))
        f = dict(clips=clips, channels=ch, frames=frames, hw=hw, known_clips=clips, known_frames=frames, mask_clips=clips, mask_frames=frames,
                 known_dtype=_lib.AA_F32, mask_dtype=_lib.AA_F32, a=0.7, s=0.3)
        f.update({k: v for k, v in kw.items() if k in f})
        for k, v in f.items():
            setattr(d, k, v)
        return lib.aa_keep_blend(C.byref(d), ops._stream(arena))

    shape_, dtype_, align_ = -1, -2, -3                                             # AA_E_SHAPE, AA_E_DTYPE, AA_E_ALIGN
    assert lib.aa_keep_blend(None, None) == shape_
    for name in ("x", "out", "known", "mask"):
        assert call(**{name: None}) == shape_, name
        assert b"null" in lib.aa_last_error()
    for bad in (dict(clips=0), dict(channels=0), dict(frames=0), dict(hw=0), dict(clips=-1), dict(hw=-3), dict(frames=70000),
                dict(clips=20000), dict(clips=60000, channels=1, frames=60000, hw=4)):
        assert call(**bad) == shape_, bad
        assert b"geometry" in lib.aa_last_error()
    for bad in (dict(known_clips=0), dict(known_clips=3), dict(known_frames=2), dict(known_frames=0), dict(mask_clips=3), dict(mask_clips=-1),
                dict(mask_frames=2), dict(mask_frames=4)):
        assert call(**bad) == shape_, bad
    for bad in (dict(a=math.nan), dict(a=math.inf), dict(s=math.nan), dict(s=-math.inf)):
        assert call(**bad) == shape_, bad
        assert b"finite" in lib.aa_last_error()
    assert call(noise=None) == shape_ and b"noise" in lib.aa_last_error()           # s != 0 without noise
    for bad in (dict(known_dtype=7), dict(mask_dtype=-1), dict(known_dtype=3)):
        assert call(**bad) == dtype_, bad
    for bad in (dict(x=x.data_ptr() + 2), dict(out=out.data_ptr() + 1), dict(noise=noise.data_ptr() + 2), dict(known=known.data_ptr() + 2),
                dict(mask=mask.data_ptr() + 1), dict(known=known.data_ptr() + 1, known_dtype=_lib.AA_F16), dict(mask=mask.data_ptr() + 1, mask_dtype=_lib.AA_BF16)):
        assert call(**bad) == align_, bad
    e = 4
    overlapping = [dict(out=x.data_ptr() + e), dict(out=x.data_ptr() + (n - 1) * e), dict(out=x.data_ptr() - e),
                   dict(out=known), dict(out=known.data_ptr() + (n - 1) * e), dict(out=mask), dict(out=mask.data_ptr() - (n - 1) * e),
                   dict(out=noise), dict(out=noise.data_ptr() + 8 * e), dict(known=out), dict(mask=out.data_ptr() + 4 * e), dict(noise=out)]
    for bad in overlapping:
        assert call(**bad) == shape_, bad
        assert b"overlap" in lib.aa_last_error()
    assert torch.equal(bits(arena.cpu()), bits(before.cpu()))
    # the wrapper: dtype, shape, contiguity, device, and the entry point's own refusals
    x4, o4, k4, n4 = (t.view(clips, ch, frames, hw) for t in (x, out, known, noise))
    m3 = mask.view(clips, frames, hw)
    with pytest.raises(RuntimeError, match="x must be fp32"):
        ops.keep_blend(x4.half(), k4, m3, 0.7, 0.3, noise=n4, out=o4)
    with pytest.raises(RuntimeError, match="x must be fp32"):
        ops.keep_blend(x, k4, m3, 0.7, 0.3, noise=n4, out=o4)
    with pytest.raises(RuntimeError, match="noise must be fp32"):
        ops.keep_blend(x4, k4, m3, 0.7, 0.3, noise=n4.half(), out=o4)
    with pytest.raises(RuntimeError, match="noise must be fp32"):
        ops.keep_blend(x4, k4, m3, 0.7, 0.3, noise=n4[:1], out=o4)
    with pytest.raises(RuntimeError, match="out must be fp32"):
        ops.keep_blend(x4, k4, m3, 0.7, 0.3, noise=n4, out=o4[:1])
    with pytest.raises(RuntimeError, match="known must be"):
        ops.keep_blend(x4, k4.double(), m3, 0.7, 0.3, noise=n4, out=o4)
    with pytest.raises(RuntimeError, match="mask must be"):
        ops.keep_blend(x4, k4, m3 > 0, 0.7, 0.3, noise=n4, out=o4)
    with pytest.raises(RuntimeError, match="known .* is not"):
        ops.keep_blend(x4, k4[:, :2].contiguous(), m3, 0.7, 0.3, noise=n4, out=o4)
    with pytest.raises(RuntimeError, match="known .* is not"):
        ops.keep_blend(x4, k4[:, :, :2].contiguous(), m3, 0.7, 0.3, noise=n4, out=o4)
    with pytest.raises(RuntimeError, match="mask .* is not"):
        ops.keep_blend(x4, k4, m3[:, :2].contiguous(), 0.7, 0.3, noise=n4, out=o4)
    with pytest.raises(RuntimeError, match="mask .* is not"):
        ops.keep_blend(x4, k4, mask.view(clips, frames, hw, 1), 0.7, 0.3, noise=n4, out=o4)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.keep_blend(x4, k4, m3, 0.7, 0.3, noise=n4.transpose(0, 1).contiguous().transpose(0, 1), out=o4)
    with pytest.raises(RuntimeError, match="noise operand"):
        ops.keep_blend(x4, k4, m3, 0.7, 0.3, out=o4)
    if d_ == "cuda":
        with pytest.raises(RuntimeError, match="device|GPU only"):
            ops.keep_blend(x4, k4.cpu(), m3, 0.7, 0.3, noise=n4, out=o4)
    for bad in (dict(a=math.nan), dict(s=math.inf)):
        with pytest.raises(RuntimeError, match="libaa_mi355"):
            ops.keep_blend(x4, k4, m3, bad.get("a", 0.7), bad.get("s", 0.3), noise=n4, out=o4)
    with pytest.raises(RuntimeError, match="libaa_mi355"):
        ops.keep_blend(x4, k4, m3, 0.7, 0.3, noise=n4, out=arena[n // 2:n // 2 + n].view(clips, ch, frames, hw))       # overlap, through the wrapper
    assert torch.equal(bits(arena.cpu()), bits(before.cpu()))
    # and the valid call on the same views works: out of place, then in place (returns x)
    got = ops.keep_blend(x4, k4, m3, 0.7, 0.3, noise=n4, out=o4)
    assert got is o4 and not torch.equal(out.cpu(), before[n:2 * n].cpu())
    assert torch.equal(bits(arena[:n].cpu()), bits(before[:n].cpu()))
    assert ops.keep_blend(x4, k4, m3, 0.7, 0.3, noise=n4) is x4 and torch.equal(bits(x.cpu()), bits(out.cpu()))
