"""aa_freeinit_mix (FreeInit's re-initialisation out = z + LP(a x + s n0 - z), LP a 3-d low-pass over (frames, h, w) as direct DFTs per
axis; five launches) against float64 torch.fft on the CPU evaluated from the same rounded fp32 inputs and the same fp32 mask table,
on the emulator and on the GPU: the smallest volume, odd axes (where the symmetrised mask matters), axes that are no power of two,
ragged tiles, a single frame, every filter method - and, on the GPU, the real shape 8 x 16 x 64 x 64 with the default filter.  The stop
frequencies of the small cases are wide on purpose: the defaults leave a mask of ~0 at these sizes, which a kernel returning z would pass;
every case asserts on its reference that the mask spans >= 0.3 and that max|LP(d)| >= 0.1.

Bound.  The test computes the same direct-DFT passes in float32 torch on the CPU (matrix products with the fp32 tables); the max error of
that against float64 is the yardstick Y of the case.  The kernel may show 8 Y - both are fp32 sums of the same lengths that differ only
in order and FMA contraction - plus one fp32 ulp of the result for the final `z +`.

Exact: a zero mask returns z, out = x repeats the out-of-place bits, a second call repeats them, guard elements behind `out` and the
workspace keep their sentinel, and every refusal leaves a sentinel-filled `out` as it was."""
import ctypes as C
import functools
import math

import pytest
import torch

import test_ddim_step
from animate_anything_amd import _lib, ops
from animate_anything_amd.schedulers import free_init_filter
from test_ddim_step import backend  # noqa: F401  (the emulator / GPU fixture; it sets test_ddim_step.DEV)

A, S = 0.068, 0.998
SENTINEL = 768.0
GUARD = 64
#        volumes, T, h, w, method, order, spatial stop, temporal stop
CASES = [(1, 2, 1, 1, "ideal", 4, 1.0, 1.0),
         (8, 3, 2, 5, "butterworth", 4, 0.6, 0.6),
         (8, 4, 6, 8, "butterworth", 4, 0.5, 0.25),
         (3, 5, 7, 3, "gaussian", 4, 0.6, 0.4),
         (8, 16, 8, 8, "ideal", 4, 0.5, 0.5),
         (4, 7, 12, 20, "butterworth", 2, 0.5, 0.5),
         (2, 24, 6, 10, "butterworth", 4, 0.4, 0.6),
         (4, 1, 4, 4, "gaussian", 4, 0.7, 0.7)]
REAL_CASE = (8, 16, 64, 64, "butterworth", 4, 0.25, 0.25)


def case_id(c):
    return "x".join(map(str, c[:4])) + "-" + c[4]


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def tables_of(case, dev):
    _, T, h, w, method, order, ss, ts = case
    return ops.free_init_tables(T, h, w, free_init_filter(T, h, w, method, order, ss, ts), dev)


@functools.lru_cache(maxsize=None)
def inputs(case):
    vols, T, h, w = case[:4]
    g = torch.Generator().manual_seed(1009 + 31 * (CASES.index(case) if case in CASES else 99))
    return tuple(torch.randn(vols, T, h, w, generator=g) for _ in range(3))          # x, n0, z (fp32)


def dft_f32(re, im, table, axis, inverse):
    """One direct-DFT pass in float32 along `axis` of (re, im): matrix products with the (cos, sin) table indexed by j * k mod n."""
    n = table.shape[0]
    idx = (torch.arange(n)[:, None] * torch.arange(n)[None, :]) % n
    c, s = table[:, 0][idx], table[:, 1][idx]                                         # [j, k]
    mm = lambda v, m: torch.movedim(torch.matmul(torch.movedim(v, axis, -1), m), -1, axis)
    if inverse:
        return mm(re, c) - mm(im, s), mm(re, s) + mm(im, c)
    return mm(re, c) + mm(im, s), mm(im, c) - mm(re, s)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(float64 reference, yardstick Y): torch.fft in float64 from the fp32 inputs and the fp32 mask table; Y = max error of the
    float32 direct-DFT passes (the kernel's arithmetic as torch matrix products) against it."""
    vols, T, h, w = case[:4]
    x, n0, z = inputs(case)
    tab = tables_of(case, "cpu")
    ms = tab.mask.double()
    a, s = f32(A), f32(S)
    d = a * x.double() + s * n0.double() - z.double()
    lp = torch.fft.ifftn(ms * torch.fft.fftn(d, dim=(-3, -2, -1)), dim=(-3, -2, -1)).real
    assert (ms.max() - ms.min()).item() >= 0.3, "the mask is (nearly) constant at this size: the case does not test the filter"
    assert lp.abs().max().item() >= 0.1, "LP(d) is (nearly) zero: a kernel that returns z would pass"
    ref = z.double() + lp
    tw = tab.twiddle
    t_t, t_h, t_w = tw[:T], tw[T:T + h], tw[T + h:]
    re = (torch.tensor(a) * x + torch.tensor(s) * n0) - z
    im = torch.zeros_like(re)
    for table, axis in ((t_w, -1), (t_h, -2), (t_t, -3)):
        re, im = dft_f32(re, im, table, axis, False)
    m = tab.mask * (torch.tensor(1.0) / (torch.tensor(float(T)) * torch.tensor(float(h * w))))
    re, im = re * m, im * m
    for table, axis in ((t_t, -3), (t_h, -2), (t_w, -1)):
        re, im = dft_f32(re, im, table, axis, True)
    yard = ((z + re).double() - ref).abs().max().item()
    return ref, yard


def ulp32(v):
    """One fp32 ulp at magnitude v (float64 tensor)."""
    e = torch.floor(torch.log2(v.clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 23)


def run(case, dev, tables=None, alias=False):
    """One call on the backend with guards behind `out` and the workspace; returns the result on the CPU."""
    x, n0, z = (t.to(dev) for t in inputs(case))
    n = x.numel()
    tables = tables if tables is not None else tables_of(case, dev)
    ws = torch.full((2 * n + GUARD,), SENTINEL, dtype=torch.float32).to(dev)
    if alias:
        buf = torch.cat([x.reshape(-1).cpu(), torch.full((GUARD,), SENTINEL)]).to(dev)
        x = buf[:n].view(x.shape)
        out = x
    else:
        buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32).to(dev)
        out = buf[:n].view(x.shape)
    got = ops.freeinit_mix(x, n0, z, A, S, tables, out=out, workspace=ws[:2 * n])
    assert got is out
    assert (buf[n:].cpu() == SENTINEL).all(), "wrote behind out"
    assert (ws[2 * n:].cpu() == SENTINEL).all(), "wrote behind the workspace"
    for t, src in zip((n0, z) if alias else (x, n0, z), inputs(case)[1:] if alias else inputs(case)):
        assert torch.equal(t.cpu(), src), "an input is only read"
    return out.cpu().clone()


def check(case, dev):
    ref, yard = reference(case)
    got = run(case, dev)
    err = (got.double() - ref).abs()
    bound = 8.0 * yard + ulp32(ref.abs())
    print(f"{case_id(case)} on {dev}: max err {err.max().item():.3g}, yardstick {yard:.3g}, ratio {err.max().item() / max(yard, 1e-30):.2f}, "
          f"worst err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    bits = lambda v: v.contiguous().view(torch.int32)
    assert torch.equal(bits(run(case, dev)), bits(got)), "a second call must repeat the bits"
    assert torch.equal(bits(run(case, dev, alias=True)), bits(got)), "out = x must equal out of place"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_against_float64_fft(backend, case):
    check(case, test_ddim_step.DEV)


@pytest.mark.gpu
def test_the_real_shape_with_the_default_filter():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    check(REAL_CASE, "cuda")


@pytest.mark.parametrize("case", [CASES[1], CASES[5]], ids=case_id)
def test_a_zero_mask_returns_the_fresh_noise(backend, case):
    dev = test_ddim_step.DEV
    _, T, h, w = case[:4]
    zero = ops.free_init_tables(T, h, w, free_init_filter(T, h, w, "butterworth", 4, 0.0, 0.25), dev)
    assert not zero.mask.cpu().any()
    assert torch.equal(run(case, dev, tables=zero), inputs(case)[2])


def test_refusals_leave_the_output_untouched(backend):
    dev = test_ddim_step.DEV
    case = CASES[1]
    vols, T, h, w = case[:4]
    n = vols * T * h * w
    tab = tables_of(case, dev)
    g = torch.Generator().manual_seed(7)
    arena = torch.randn(8 * n, generator=g).to(dev)                                   # one allocation: views of it can overlap
    arena[3 * n:4 * n] = SENTINEL
    before = arena.clone()
    x, n0, z, out, ws = arena[:n], arena[n:2 * n], arena[2 * n:3 * n], arena[3 * n:4 * n], arena[4 * n:6 * n]
    lib = _lib.get()

    def call(workspace="own", workspace_bytes=None, **kw):
        d = _lib.AaFreeInit()
        t = dict(x=x, n0=n0, z=z, out=out, mask=tab.mask, twiddle=tab.twiddle)
        t.update({k: v for k, v in kw.items() if k in t})
        for k, v in t.items():
            setattr(d, k, None if v is None else C.c_void_p(v if isinstance(v, int) else v.data_ptr()))
        f = dict(volumes=vols, frames=T, h=h, w=w, a=A, s=S)
        f.update({k: v for k, v in kw.items() if k in f})
        for k, v in f.items():
            setattr(d, k, v)
        wsp = ws if isinstance(workspace, str) else workspace
        ptr = None if wsp is None else C.c_void_p(wsp if isinstance(wsp, int) else wsp.data_ptr())
        nbytes = 8 * n if workspace_bytes is None else workspace_bytes
        return lib.aa_freeinit_mix(C.byref(d), ptr, nbytes, ops._stream(arena)), lib.aa_freeinit_workspace(C.byref(d))

    shape_, align_, workspace_ = -1, -3, -4                                           # AA_E_SHAPE, AA_E_ALIGN, AA_E_WORKSPACE
    assert call(x=None)[1] == 8 * n                                                   # (the size query: one complex fp32 per element)
    assert lib.aa_freeinit_mix(None, None, 0, None) == shape_ and lib.aa_freeinit_workspace(None) == 0
    for name in ("x", "n0", "z", "out", "mask", "twiddle"):
        assert call(**{name: None})[0] == shape_, name
        assert b"null" in lib.aa_last_error()
    for bad in (dict(volumes=0), dict(frames=0), dict(h=0), dict(w=0), dict(volumes=-1), dict(w=-3),
                dict(frames=129), dict(h=129), dict(w=129), dict(volumes=1 << 30)):
        assert call(**bad)[0] == shape_, bad
        assert call(**bad)[1] == 0, bad
    for bad in (dict(a=math.nan), dict(a=math.inf), dict(s=math.nan), dict(s=-math.inf)):
        assert call(**bad)[0] == shape_, bad
    assert call(workspace=None)[0] == workspace_
    assert call(workspace_bytes=8 * n - 4)[0] == workspace_ and b"workspace" in lib.aa_last_error()
    e = 4
    overlapping = [dict(out=n0), dict(out=z), dict(out=n0.data_ptr() + 4 * e), dict(out=z.data_ptr() - 4 * e),      # out on n0 / z
                   dict(out=x.data_ptr() + 2 * e),                                    # out over x, shifted
                   dict(out=tab.mask), dict(out=tab.twiddle),
                   dict(workspace=out.data_ptr() + 8), dict(workspace=x.data_ptr() + 8), dict(workspace=z.data_ptr() + 8)]
    for bad in overlapping:
        assert call(**bad)[0] == shape_, bad
        assert b"overlap" in lib.aa_last_error()
    for name in ("x", "n0", "z", "out"):
        assert call(**{name: arena.data_ptr() + 7 * n * e + 2})[0] == align_, name
    assert call(workspace=ws.data_ptr() + 4, workspace_bytes=8 * n)[0] == align_
    assert torch.equal(arena.cpu().view(torch.int32), before.cpu().view(torch.int32)), "a refusal wrote something"
    assert (out.cpu() == SENTINEL).all()
    # the wrapper: dtype, shape, device and the entry point's own refusals
    shp = (vols, T, h, w)
    xv, nv, zv, ov = (t.view(shp) for t in (x, n0, z, out))
    with pytest.raises(RuntimeError, match="fp32"):
        ops.freeinit_mix(xv, nv.double(), zv, A, S, tab, out=ov)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.freeinit_mix(xv, nv, zv[:-1], A, S, tab, out=ov)
    with pytest.raises(RuntimeError, match="tables"):
        ops.freeinit_mix(xv.view(vols, T, w, h), nv.view(vols, T, w, h), zv.view(vols, T, w, h), A, S, tab, out=ov.view(vols, T, w, h))
    with pytest.raises(RuntimeError, match="libaa_mi355"):
        ops.freeinit_mix(xv, nv, zv, A, S, tab, out=nv)                               # out on n0, through the wrapper
    with pytest.raises(RuntimeError, match="libaa_mi355"):
        ops.freeinit_mix(xv, nv, zv, math.nan, S, tab, out=ov)
    with pytest.raises(RuntimeError, match="libaa_mi355"):
        ops.freeinit_mix(xv, nv, zv, A, S, tab, out=ov, workspace=ws[:2 * n - 2])
    assert torch.equal(arena.cpu().view(torch.int32), before.cpu().view(torch.int32))
    # and the valid call on the same views works; the workspace is kept per geometry
    got = ops.freeinit_mix(xv, nv, zv, A, S, tab, out=ov)
    assert got is ov and not (ov.cpu() == SENTINEL).any()
    key = (str(xv.device), vols, T, h, w)
    kept = ops._FREE_INIT_WS[key]
    ops.freeinit_mix(xv, nv, zv, A, S, tab, out=ov)
    assert ops._FREE_INIT_WS[key] is kept and kept.numel() >= 2 * n


def test_the_tables_are_cached_per_shape_and_mask():
    m = free_init_filter(3, 2, 5, "butterworth", 4, 0.6, 0.6)
    t1 = ops.free_init_tables(3, 2, 5, m, "cpu")
    assert ops.free_init_tables(3, 2, 5, m.clone(), "cpu") is t1
    t2 = ops.free_init_tables(3, 2, 5, free_init_filter(3, 2, 5, "gaussian", 4, 0.6, 0.6), "cpu")
    assert t2 is not t1 and not torch.equal(t1.mask, t2.mask) and torch.equal(t1.twiddle, t2.twiddle)
    assert t1.mask.dtype == torch.float32 and tuple(t1.twiddle.shape) == (10, 2)
    ang = 2.0 * math.pi * torch.arange(5, dtype=torch.float64) / 5
    assert torch.equal(t1.twiddle[5:], torch.stack([torch.cos(ang), torch.sin(ang)], dim=1).float())
    with pytest.raises(RuntimeError, match="mask"):
        ops.free_init_tables(3, 2, 4, m, "cpu")
