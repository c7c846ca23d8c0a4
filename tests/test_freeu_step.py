"""aa_freeu_tokens (FreeU on the two operands of an up-block resnet, token layout, one launch) against the float64 seven-basis formula
evaluated from the same rounded inputs, on the emulator and on the GPU: odd planes, 1-pixel axes, aliasing modes, the half-channel
boundary inside a 16-byte vector, several images, the real 16x16-level shape, a 4096-pixel plane; fp16 and bf16, dense and padded rows,
in place and out of place, inputs of mean 0 and mean 50, the identity (b = s = 1) bit for bit, and every refusal of the entry point.

Bound (eps = 2^-24, no measurement behind it).  The skip half is y = x + sum_k t_k with t_k = (s - 1) / hw * S_k * phi_k(pixel),
S_k = sum_pixels x * phi_k, |phi_k| <= 1, so |t_k| <= A := |s - 1| * mean_plane |x|.
 * S_k: one product and one addition per pixel on a chain of at most L = ceil(hw / 32) + 6 additions (a thread's pixels one after
   another, three exchanges inside the wave, three additions over the waves): relative to sum |x| at most (L + 1) eps.
 * phi_k: table entries rounded to fp32 (eps / 2 each), phi_5 / phi_6 from two products and a sum of them: within 4 eps of the exact
   value, in S_k and again in the apply: 8 eps.
 * the factor (s - 1) / hw: s is handed over in fp32 (relative eps, which s - 1 magnifies by |s| / |s - 1|), a division and a product: 3 eps;
   the product with phi_k and the accumulation into y: 2 eps.
   Together |t_k error| <= A * K * eps with K = L + 14 + |s| / |s - 1|.
 * the seven additions onto x round partial sums bounded by |x| + 7 A: 7 (|x| + 7 A) eps.
 * one rounding to the storage type: half an ulp (2^-11 relative in fp16 above 2^-14, 2^-8 in bf16) at |y| plus the fp32 error.
The hidden half is one fp32 product (b rounded to fp32: 2 eps |x b|) and the rounding to the storage type."""
import ctypes as C
import functools
import math

import pytest
import torch

import test_ddim_step
from animate_anything_amd import _lib, ops
from freeu_util import fourier_filter_basis
from test_ddim_step import backend  # noqa: F401  (the emulator / GPU fixture; it sets test_ddim_step.DEV)

EPS = 2.0 ** -24
CASES = [(3, 7, 10, 72, 40), (2, 2, 2, 16, 8), (2, 1, 1, 1280, 1280), (2, 1, 5, 16, 16), (2, 16, 16, 1280, 1280), (1, 64, 64, 8, 8)]
SCALARS = [(1.2, 0.9), (1.4, 0.2), (1.0, 1.0)]
SENTINEL = 768.0                                       # (exact in fp16 and bf16)
GUARD = 2                                              # rows behind the last one: never read into the result, never written


def dev():
    return test_ddim_step.DEV


def half_ulp(v, dt):
    """Half an ulp of the storage type at magnitude v (float64 tensor)."""
    mant, emin = (10, -14) if dt == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(v.clamp_min(2.0 ** emin))).clamp_min(emin)
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


@functools.lru_cache(maxsize=None)
def operands(case, dt, mean):
    """Rounded inputs (dense, CPU) and the float64 references that do not depend on the scalars: Re(P skip) and mean_plane |skip|."""
    images, h, w, ch, cs = case
    g = torch.Generator().manual_seed(191 + 7 * CASES.index(case) + int(mean))
    hidden = (torch.randn(images * h * w, ch, generator=g) + mean).to(dt)
    skip = (torch.randn(images * h * w, cs, generator=g) + mean).to(dt)
    planes = skip.double().reshape(images, h, w, cs).permute(0, 3, 1, 2)                      # [images, C, h, w]
    proj = fourier_filter_basis(planes, 2.0) - planes                                        # Re(P x): the filter is x + (s - 1) Re(P x)
    amean = planes.abs().mean(dim=(-2, -1), keepdim=True).expand_as(planes)
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(images * h * w, cs)
    return hidden, skip, tok(proj), tok(amean)


def bounds(case, dt, mean, b, s):
    images, h, w, ch, cs = case
    hidden, skip, proj, amean = operands(case, dt, mean)
    want_h = hidden.double().clone()
    want_h[:, :ch // 2] *= b
    err_h = 2 * EPS * want_h.abs()
    bound_h = err_h + half_ulp(want_h.abs() + err_h, dt)
    bound_h[:, ch // 2:] = 0.0                                                               # copied columns: exact
    x = skip.double()
    want_s = x + (s - 1.0) * proj
    if s == 1.0:
        return want_h, bound_h, want_s, torch.zeros_like(want_s)
    a = abs(s - 1.0) * amean
    k = math.ceil(h * w / 32) + 6 + 14 + abs(s) / abs(s - 1.0)
    err32 = EPS * (7 * a * k + 7 * (x.abs() + 7 * a))
    return want_h, bound_h, want_s, err32 + half_ulp(want_s.abs() + err32, dt)


def pitched(t, ld):
    """A [rows, C] view with row pitch `ld` (and GUARD rows behind it) of a sentinel-filled buffer on the backend, holding t."""
    rows, c = t.shape
    buf = torch.full((rows + GUARD, ld), SENTINEL, dtype=t.dtype).to(dev())
    view = buf[:rows, :c]
    view.copy_(t.to(dev()))
    return buf, view


def check_untouched(buf, rows, c):
    assert (buf[:rows, c:].float() == SENTINEL).all() and (buf[rows:].float() == SENTINEL).all(), "wrote outside the tensor"


@pytest.mark.parametrize("in_place", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("pad", [8, 0], ids=["padded", "dense"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_against_the_float64_formula(backend, case, dt, pad, in_place):
    images, h, w, ch, cs = case
    rows = images * h * w
    for mean in (0.0, 50.0):
        hidden, skip, _, _ = operands(case, dt, mean)
        for b, s in SCALARS:
            hbuf, hv = pitched(hidden, ch + pad)
            sbuf, sv = pitched(skip, cs + pad)
            if in_place:
                (hobuf, ho), (sobuf, so) = (hbuf, hv), (sbuf, sv)
            else:
                hobuf, ho = pitched(torch.full_like(hidden, SENTINEL), ch + pad)
                sobuf, so = pitched(torch.full_like(skip, SENTINEL), cs + pad)
            got_h, got_s = ops.freeu(hv, sv, images, h, w, b, s, hidden_out=ho, skip_out=so)
            assert got_h.data_ptr() == ho.data_ptr() and got_s.data_ptr() == so.data_ptr()
            for buf, c in ((hbuf, ch), (sbuf, cs), (hobuf, ch), (sobuf, cs)):
                check_untouched(buf.cpu(), rows, c)
            if not in_place:                                                                 # the inputs are only read
                assert torch.equal(hv.cpu(), hidden) and torch.equal(sv.cpu(), skip)
            got_h, got_s = got_h.cpu(), got_s.cpu()
            if (b, s) == (1.0, 1.0):
                assert torch.equal(got_h.view(torch.int16), hidden.view(torch.int16)), "b = 1 must return the bits of hidden"
                assert torch.equal(got_s.view(torch.int16), skip.view(torch.int16)), "s = 1 must return the bits of skip"
                continue
            want_h, bound_h, want_s, bound_s = bounds(case, dt, mean, b, s)
            err_h, err_s = (got_h.double() - want_h).abs(), (got_s.double() - want_s).abs()
            print(f"mean {mean} b {b} s {s}: hidden worst err/bound {(err_h / bound_h.clamp_min(1e-300)).max().item():.3f}, "
                  f"skip worst err/bound {(err_s / bound_s).max().item():.3f} (max err {err_s.max().item():.3g})")
            assert (err_h <= bound_h).all(), ("hidden", mean, b, s)
            assert (err_s <= bound_s).all(), ("skip", mean, b, s)
            assert torch.equal(got_h[:, ch // 2:].view(torch.int16), hidden[:, ch // 2:].view(torch.int16))


def test_one_half_may_be_in_place_and_a_second_call_repeats_the_bits(backend):
    """hidden in place with skip out of place (and the reverse); no atomics, fixed summation order: the same call gives the same bits."""
    case, dt = CASES[0], torch.float16
    images, h, w, ch, cs = case
    hidden, skip, _, _ = operands(case, dt, 0.0)
    b, s = SCALARS[0]
    want_h, bound_h, want_s, bound_s = bounds(case, dt, 0.0, b, s)
    outs = []
    for hidden_in_place in (True, False, True):
        hv, sv = hidden.clone().to(dev()), skip.clone().to(dev())
        ho, so = ops.freeu(hv, sv, images, h, w, b, s, hidden_out=hv if hidden_in_place else None, skip_out=None if hidden_in_place else sv)
        assert (ho.data_ptr() == hv.data_ptr()) == hidden_in_place and (so.data_ptr() == sv.data_ptr()) == (not hidden_in_place)
        assert ((ho.double().cpu() - want_h).abs() <= bound_h).all() and ((so.double().cpu() - want_s).abs() <= bound_s).all()
        outs.append((ho.cpu(), so.cpu()))
    for ho, so in outs[1:]:
        assert torch.equal(ho, outs[0][0]) and torch.equal(so, outs[0][1])


def test_the_table_is_built_once_per_plane_and_has_zeros_along_a_one_pixel_axis(backend):
    t = ops.freeu_trig_table(1, 5, dev())
    assert t is ops.freeu_trig_table(1, 5, dev()) and t.dtype == torch.float32 and tuple(t.shape) == (5, 4)
    assert (t[:, :2] == 0).all() and t[0, 2] == 1 and t[0, 3] == 0
    t = ops.freeu_trig_table(4, 1, dev()).cpu()
    assert (t[:, 2:] == 0).all() and torch.allclose(t[:, 0], torch.tensor([1.0, 0.0, -1.0, 0.0]), atol=1e-7)


def test_refusals_leave_the_outputs_untouched(backend):
    images, h, w, ch, cs = 2, 3, 5, 24, 16
    rows, dt = images * h * w, torch.float16
    d_ = dev()
    g = torch.Generator().manual_seed(5)
    arena = torch.randn(8 * rows * 32, generator=g).to(dt).to(d_)                            # one allocation: views of it can overlap
    before = arena.clone()
    at = lambda off, c: arena[off:off + rows * c].view(rows, c)
    hidden, hidden_out, skip, skip_out = at(0, ch), at(rows * 32, ch), at(2 * rows * 32, cs), at(3 * rows * 32, cs)
    trig = ops.freeu_trig_table(h, w, d_)
    lib = _lib.get()

    def call(**kw):
        d = _lib.AaFreeU()
        t = dict(hidden=hidden, hidden_out=hidden_out, skip=skip, skip_out=skip_out, trig=trig)
        t.update({k: v for k, v in kw.items() if k in t})
        for k, v in t.items():
            setattr(d, k, None if v is None else C.c_void_p(v if isinstance(v, int) else v.data_ptr()))
        f = dict(images=images, h=h, w=w, c_hidden=ch, c_skip=cs, hidden_ld=ch, hidden_out_ld=ch, skip_ld=cs, skip_out_ld=cs,
                 b=1.2, s=0.9, dtype=_lib.AA_F16)
        f.update({k: v for k, v in kw.items() if k in f})
        for k, v in f.items():
            setattr(d, k, v)
        return lib.aa_freeu_tokens(C.byref(d), ops._stream(arena))

    shape = -1                                                                               # AA_E_SHAPE
    assert lib.aa_freeu_tokens(None, None) == shape
    for name in ("hidden", "hidden_out", "skip", "skip_out", "trig"):
        assert call(**{name: None}) == shape, name
    assert b"null" in lib.aa_last_error()
    for bad in (dict(c_hidden=12), dict(c_skip=12), dict(c_hidden=9), dict(c_hidden=23), dict(c_skip=0),
                dict(hidden_ld=ch - 8), dict(hidden_out_ld=ch - 8), dict(skip_ld=cs - 8), dict(skip_out_ld=cs - 8),
                dict(h=0), dict(w=0), dict(h=-1), dict(images=0)):
        assert call(**bad) == shape, bad
    e = arena.element_size()
    overlapping = [dict(hidden_out=hidden.data_ptr() + 16),                                  # output over its input, shifted
                   dict(hidden_out=hidden, hidden_out_ld=ch + 8),                            # same pointer, another pitch
                   dict(skip_out=skip.data_ptr() + 16 * e * cs),
                   dict(skip_out=skip, skip_ld=cs + 8),
                   dict(skip_out=hidden), dict(skip=hidden), dict(skip=hidden_out), dict(hidden_out=skip_out), dict(hidden_out=skip),
                   dict(skip=hidden.data_ptr() + (rows * ch - 8) * e),                       # two tensors that share 16 bytes
                   dict(trig=arena.data_ptr() + 4 * rows * 32 * e, skip_out=arena.data_ptr() + 4 * rows * 32 * e + 32)]
    for bad in overlapping:
        assert call(**bad) == shape, bad
        assert b"overlap" in lib.aa_last_error()
    assert call(hidden=hidden.data_ptr() + 2, hidden_out=hidden.data_ptr() + 2) == -3        # AA_E_ALIGN
    assert call(dtype=_lib.AA_F32) == -2                                                     # AA_E_DTYPE
    assert torch.equal(arena.cpu().view(torch.int16), before.cpu().view(torch.int16))
    # the wrapper: dtype, shape and layout
    with pytest.raises(RuntimeError, match="token matrix"):
        ops.freeu(hidden.float(), skip, images, h, w, 1.2, 0.9)
    with pytest.raises(RuntimeError, match="token matrix"):
        ops.freeu(hidden, skip.to(torch.bfloat16), images, h, w, 1.2, 0.9)
    with pytest.raises(RuntimeError, match="token matrix"):
        ops.freeu(hidden.t(), skip, images, h, w, 1.2, 0.9)
    with pytest.raises(RuntimeError, match="rows"):
        ops.freeu(hidden, skip[:-1], images, h, w, 1.2, 0.9)
    with pytest.raises(RuntimeError, match="shape"):
        ops.freeu(hidden, skip, images, h, w, 1.2, 0.9, skip_out=hidden_out)
    with pytest.raises(RuntimeError, match="libaa_mi355"):
        ops.freeu(hidden, skip, images, h, w, 1.2, 0.9, hidden_out=hidden, skip_out=hidden[:, :cs])      # the entry point, through the wrapper
    assert torch.equal(arena.cpu().view(torch.int16), before.cpu().view(torch.int16))
    # and the valid call on the same views works
    ho, so = ops.freeu(hidden, skip, images, h, w, 1.2, 0.9, hidden_out=hidden_out, skip_out=skip_out)
    assert not torch.equal(so.cpu(), before[3 * rows * 32:3 * rows * 32 + rows * cs].view(rows, cs).cpu())
