"""aa_window_gather_latents and aa_window_merge_tokens (context windows: the UNet on overlapping windows of a long clip, the per-window
predictions blended per frame, one solver update) on the emulator and on the GPU.  The gather is a copy and must be bit-exact.  The
merge is run over whole schedules of schedulers.context_windows - one launch per window, in order - and what the step kernel will
read from the merged token matrix, m_u + g (m_t - m_u) of its two halves under guidance and m_u without, is held against the formula in
float64 evaluated from the same rounded inputs (tokens, the fp32 weights):

    merged[b, f] = sum over the (window k, slot j) that hold frame f of  w_kj * c_kj,    c = u + g (t - u)   (guidance off: c = u)

A frame held by several windows must hold ONE value in both halves (guidance then leaves it as it is).

Bound (eps = 2^-24; from the arithmetic, no measurement behind it), per element of a frame held by K windows:
 * per contribution: c costs one subtraction, the product with g and one addition, w * c one product:
       w eps (3 |g (t - u)| + |c|) + eps |w c|
 * each of the K - 1 additions: eps * sum |w c|
 * the store: half an ulp of the storage type at the result (2^-11 relative in fp16 above 2^-14, 2^-8 in bf16).
A frame held by one window has weight 1.0 exactly and is never multiplied: the stored bits are the input's, in both halves.

Also: sentinels in the merged matrix's frame-0 rows, padding columns and guard rows, and in the accumulator rows of every frame outside
the launched window; a second run over the used accumulator repeats the bits (a frame's first window writes, it does not add); every
refusal of both entry points leaves the outputs untouched."""
import ctypes as C
import functools
import math

import pytest
import torch

import test_ddim_step
from animate_anything_amd import _lib, ops
from animate_anything_amd.schedulers import context_windows
from test_cfg_rescale_step import half_ulp
from test_ddim_step import backend  # noqa: F401  (the emulator / GPU fixture; it sets test_ddim_step.DEV)

EPS = 2.0 ** -24
SENTINEL = 768.0                                       # (exact in fp16 and bf16)
GUARD = 2                                              # rows behind the last one: never read into the result, never written
# (clips, channels, window, total, hw, ld): the smallest legal case; the vector form (4 channels) with K up to 2; the element-wise form at
# an odd channel count with three clips; several workgroups per frame with a ragged tail and a frame held by three windows; pitches 4 / 16
SHAPES = [(1, 1, 1, 2, 1, 8), (2, 4, 3, 7, 10, 8), (3, 3, 2, 5, 37, 8), (2, 4, 5, 12, 1031, 8),
          (2, 4, 3, 7, 10, 4), (2, 4, 3, 7, 10, 16), (2, 4, 5, 12, 1031, 4), (2, 4, 5, 12, 1031, 16)]
BENCH_SHAPE = (1, 4, 16, 32, 4096, 8)
OVERLAP = {1: 0, 2: 1, 3: 1, 5: 2, 16: 4}              # by window length
GUIDANCES = (None, 1.5, 9.0)


def dev():
    return test_ddim_step.DEV


def schedule(shape, closed_loop, weights):
    _, _, window, total, _, _ = shape
    return context_windows(total, window, OVERLAP[window], closed_loop=closed_loop, weights=weights)


def valid(m, clips, frames, hw, ch, half=0):
    """The [clips, frames, hw, channels] view of frames 1..frames of half `half` of a token matrix of `frames` + 1 frames."""
    rows = clips * (frames + 1) * hw
    return m[half * rows:(half + 1) * rows].reshape(clips, frames + 1, hw, m.shape[1])[:, 1:, :, :ch]


@functools.lru_cache(maxsize=None)
def window_tokens(shape, dt, guided, k):
    """The rounded token matrix window k's UNet run leaves (CPU): [(2 if guided else 1) * rows + GUARD, ld], sentinels in frame 0, the
    padding columns and the guard rows; the unconditional and the text half from different seeds."""
    clips, ch, window, _, hw, ld = shape
    halves = 2 if guided else 1
    rows = clips * (window + 1) * hw
    tok = torch.full((halves * rows + GUARD, ld), SENTINEL, dtype=dt)
    for half in range(halves):
        g = torch.Generator().manual_seed(1000 * k + 17 * half + hw)
        valid(tok, clips, window, hw, ch, half).copy_(torch.randn(clips, window, hw, ch, generator=g).to(dt))
    return tok


def reference(shape, dt, guidance, windows):
    """float64 from the rounded inputs: (merged [clips, total, hw, channels], its bound before the store, windows per frame)."""
    clips, ch, window, total, hw, _ = shape
    ref = torch.zeros(clips, total, hw, ch, dtype=torch.float64)
    err, mag = torch.zeros_like(ref), torch.zeros_like(ref)
    count = torch.zeros(total, dtype=torch.int64)
    for k, (idx, wn, _, _) in enumerate(windows):
        tok = window_tokens(shape, dt, guidance is not None, k).double()
        u = valid(tok, clips, window, hw, ch, 0)
        if guidance is None:
            c, gd = u, torch.zeros_like(u)
        else:
            gd = guidance * (valid(tok, clips, window, hw, ch, 1) - u)
            c = u + gd
        w = torch.tensor(wn, dtype=torch.float64).float().double().reshape(1, window, 1, 1)        # the fp32 weights the kernel is handed
        ref[:, idx] += w * c
        err[:, idx] += w * EPS * (3 * gd.abs() + c.abs()) + EPS * (w * c).abs()
        mag[:, idx] += (w * c).abs()
        count[idx] += 1
    assert (count >= 1).all()
    err += (count - 1).reshape(1, total, 1, 1) * EPS * mag
    return ref, err, count


def run_schedule(shape, dt, guidance, windows, state=None, check_acc=True):
    """One launch per window on the backend, in order; checks what must stay untouched after every launch.  `state`: (acc, merged) of
    an earlier run to run over again.  Returns (merged buffer on the CPU, acc, merged) - the latter two on the backend."""
    clips, ch, window, total, hw, ld = shape
    halves = 2 if guidance is not None else 1
    out_rows = halves * clips * (total + 1) * hw
    if state is None:
        acc = torch.full((clips, total, hw, ch), -SENTINEL, dtype=torch.float32).to(dev())
        buf = torch.full((out_rows + GUARD, ld), SENTINEL, dtype=dt).to(dev())
    else:
        acc, buf = state
    for k, win in enumerate(windows):
        before_tok = window_tokens(shape, dt, guidance is not None, k)
        tok = before_tok.to(dev())
        acc_before = acc.cpu() if check_acc else None
        got = ops.window_merge_tokens(tok[:tok.shape[0] - GUARD], acc, buf[:out_rows], win, guidance)
        assert got.data_ptr() == buf.data_ptr()
        assert torch.equal(tok.cpu().view(torch.int16), before_tok.view(torch.int16)), "the tokens are only read"
        if check_acc:
            outside = [f for f in range(total) if f not in win[0]]
            assert torch.equal(acc.cpu()[:, outside], acc_before[:, outside]), "wrote accumulator rows of a frame outside the window"
            once = [f for f, first, last in zip(win[0], win[2], win[3]) if first and last]
            assert torch.equal(acc.cpu()[:, once], acc_before[:, once]), "touched the accumulator of a frame held by one window"
    after = buf.cpu()
    keep = after.clone()
    for half in range(halves):
        valid(keep, clips, total, hw, ch, half).fill_(SENTINEL)
    assert (keep.float() == SENTINEL).all(), "wrote a frame-0 row, a padding column or a guard row"
    return after, acc, buf


def check(shape, dt, guidance, closed_loop, weights, check_acc=True):
    clips, ch, window, total, hw, _ = shape
    windows = schedule(shape, closed_loop, weights)
    ref, err32, count = reference(shape, dt, guidance, windows)
    bound = err32 + half_ulp(ref.abs() + err32, dt)
    after, acc, buf = run_schedule(shape, dt, guidance, windows, check_acc=check_acc)
    halves = 2 if guidance is not None else 1
    m = [valid(after, clips, total, hw, ch, half) for half in range(halves)]
    got = m[0].double() if guidance is None else m[0].double() + guidance * (m[1].double() - m[0].double())      # what the step kernel reads
    err = (got - ref).abs()
    print(f"{shape} {dt} g {guidance} {'closed' if closed_loop else 'open'} {weights}: {len(windows)} windows, up to {int(count.max())} per frame, "
          f"worst err/bound {(err / bound).max().item():.3f} (max err {err.max().item():.3g})")
    assert torch.isfinite(got).all() and (err <= bound).all()
    bits = lambda v: v.contiguous().view(torch.int16)
    for k, (idx, _, first, last) in enumerate(windows):
        for half in range(halves):
            src = valid(window_tokens(shape, dt, guidance is not None, k), clips, window, hw, ch, half)
            for j, f in enumerate(idx):
                if first[j] and last[j]:                                          # a frame held by one window: the input's bits
                    assert torch.equal(bits(m[half][:, f]), bits(src[:, j])), (k, j, f, half)
    if halves == 2:
        several = [f for f in range(total) if count[f] > 1]
        assert torch.equal(bits(m[0][:, several]), bits(m[1][:, several])), "a blended frame holds one value in both halves"
    again, _, _ = run_schedule(shape, dt, guidance, windows, state=(acc, buf), check_acc=check_acc)      # over the used accumulator
    assert torch.equal(again.view(torch.int16), after.view(torch.int16)), "a second run must repeat the bits"
    return count


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_merge_against_the_float64_formula(backend, shape, dt):
    most = 0
    for guidance in GUIDANCES:
        for closed_loop in (False, True):
            for weights in ("flat", "pyramid"):
                most = max(most, int(check(shape, dt, guidance, closed_loop, weights).max()))
    assert most >= (3 if shape[2] == 5 else 2 if shape[2] > 1 else 1)             # the schedules really overlap


def test_merge_at_the_benchmark_shape(backend):
    """32 frames of 64 x 64 latents in windows of 16 with overlap 4: the three launches of one step."""
    check(BENCH_SHAPE, torch.float16, 9.0, False, "pyramid", check_acc=False)


@pytest.mark.parametrize("shape", [(1, 1, 2, 1, 1), (2, 4, 7, 3, 10), (3, 3, 5, 2, 37), (2, 4, 12, 5, 1031), (1, 4, 9, 4, 1028), (1, 4, 32, 16, 4096)],
                         ids=lambda s: "x".join(map(str, s)))
def test_gather_is_a_bit_exact_copy(backend, shape):
    """(clips, channels, total, window, hw): odd sizes take the element-wise form, hw % 4 == 0 the 16-byte form; random BITS (NaN and
    infinity patterns among them) prove a copy; the guard floats around `dst` stay."""
    clips, ch, total, window, hw = shape
    g = torch.Generator().manual_seed(hw)
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (clips, ch, total, hw, 1), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    for closed_loop in (False, True):
        for win in context_windows(total, window, OVERLAP.get(window, 1), closed_loop=closed_loop):
            n = clips * ch * window * hw
            buf = torch.full((n + 8,), SENTINEL, dtype=torch.float32).to(dev())
            dst = buf[4:4 + n].view(clips, ch, window, hw, 1)
            srcd = src.to(dev())
            got = ops.window_gather_latents(srcd, win, out=dst)
            assert got.data_ptr() == dst.data_ptr()
            assert torch.equal(srcd.cpu().view(torch.int32), src.view(torch.int32)), "the source is only read"
            after = buf.cpu()
            assert (after[:4] == SENTINEL).all() and (after[4 + n:] == SENTINEL).all()
            want = src[:, :, torch.tensor(win[0])]
            assert torch.equal(after[4:4 + n].view(torch.int32), want.reshape(-1).view(torch.int32))
    fresh = ops.window_gather_latents(src.to(dev()), win)                           # `out` left to the wrapper
    assert fresh.shape == (clips, ch, window, hw, 1) and torch.equal(fresh.cpu().view(torch.int32), want.view(torch.int32))


def _window(frames, weights=None, first=None, last=None):
    n = len(frames)
    return (list(frames), weights or [0.5] * n, first or [True] * n, last or [False] * n)


def test_merge_refusals_leave_the_outputs_untouched(backend):
    clips, ch, window, total, hw, ld = 2, 4, 3, 7, 10, 8
    rows, out_rows, dt = 2 * clips * (window + 1) * hw, 2 * clips * (total + 1) * hw, torch.float16     # both halves: guidance is on
    d_ = dev()
    g = torch.Generator().manual_seed(5)
    arena = torch.randn((rows + 2 * out_rows) * ld, generator=g).to(dt).to(d_)        # one allocation: views of it can overlap
    before = arena.clone()
    e = arena.element_size()
    tokens, merged = arena[:rows * ld], arena[rows * ld:(rows + out_rows) * ld]
    acc = torch.full((clips, total, hw, ch), 3.0, dtype=torch.float32).to(d_)
    lib = _lib.get()

    def call(win=_window([2, 3, 4]), window_frames=None, **kw):
        d = _lib.AaWindowMerge()
        t = dict(tokens=tokens, acc=acc, merged=merged)
        t.update({k: v for k, v in kw.items() if k in t})
        for k, v in t.items():
            setattr(d, k, None if v is None else C.c_void_p(v if isinstance(v, int) else v.data_ptr()))
        f = dict(clips=clips, channels=ch, total_frames=total, hw=hw, ld=ld, out_ld=ld, guidance_on=1, guidance=9.0, dtype=_lib.AA_F16)
        f.update({k: v for k, v in kw.items() if k in f})
        for k, v in f.items():
            setattr(d, k, v)
        d.window = ops.window_desc(win)
        if window_frames is not None:
            d.window.window_frames = window_frames
        return lib.aa_window_merge_tokens(C.byref(d), ops._stream(arena))

    shape_, dtype_, align_ = -1, -2, -3                                             # AA_E_SHAPE, AA_E_DTYPE, AA_E_ALIGN
    assert lib.aa_window_merge_tokens(None, None) == shape_
    for name in ("tokens", "acc", "merged"):
        assert call(**{name: None}) == shape_, name
    assert b"null" in lib.aa_last_error()
    for bad in (dict(clips=0), dict(channels=0), dict(total_frames=0), dict(hw=0), dict(clips=-1), dict(hw=-3), dict(clips=70000),
                dict(channels=9), dict(ld=ch - 1), dict(out_ld=ch - 1), dict(window_frames=0), dict(window_frames=-2),
                dict(window_frames=_lib.AA_WINDOW_MAX + 1), dict(total_frames=2),            # the window is longer than the clip
                dict(win=_window([2, 3, 7])), dict(win=_window([-1, 3, 4])),                 # a frame outside [0, total)
                dict(win=_window([2, 3, 2])),                                                # a repeated frame: two slots would race
                dict(win=_window([2, 3, 4], [0.5, math.nan, 0.5])), dict(win=_window([2, 3, 4], [math.inf, 0.5, 0.5])),
                dict(guidance=math.nan), dict(guidance=math.inf), dict(guidance=-math.inf)):
        assert call(**bad) == shape_, bad
    overlapping = [dict(merged=tokens.data_ptr() + 2 * e), dict(merged=tokens.data_ptr() + ((rows - 1) * ld + ch - 2) * e),
                   dict(tokens=merged.data_ptr() + 64), dict(acc=tokens.data_ptr() + 64), dict(acc=merged.data_ptr() + 128),
                   dict(tokens=acc.data_ptr()), dict(merged=acc.data_ptr() + acc.numel() * 4 - 4)]
    for bad in overlapping:
        assert call(**bad) == shape_, bad
        assert b"overlap" in lib.aa_last_error()
    assert call(tokens=tokens.data_ptr() + 1) == align_ and call(merged=merged.data_ptr() + 1) == align_
    assert call(acc=acc.data_ptr() + 2) == align_
    assert call(dtype=_lib.AA_F32) == dtype_ and call(dtype=7) == dtype_
    assert torch.equal(arena.cpu().view(torch.int16), before.cpu().view(torch.int16)) and (acc.cpu() == 3.0).all()
    # the wrapper: dtype, shape, layout and the entry point's own refusals
    tok2, out2 = tokens.view(rows, ld), merged.view(out_rows, ld)
    win = _window([2, 3, 4])
    with pytest.raises(RuntimeError, match="token matrix"):
        ops.window_merge_tokens(tok2.float(), acc, out2, win, 9.0)
    with pytest.raises(RuntimeError, match="token matrix"):
        ops.window_merge_tokens(tok2, acc, out2.to(torch.bfloat16), win, 9.0)
    with pytest.raises(RuntimeError, match="token matrix"):
        ops.window_merge_tokens(tok2.t(), acc, out2, win, 9.0)
    with pytest.raises(RuntimeError, match="rows"):
        ops.window_merge_tokens(tok2[:-1], acc, out2, win, 9.0)                      # guidance needs both halves
    with pytest.raises(RuntimeError, match="rows"):
        ops.window_merge_tokens(tok2, acc, out2[:-1], win, 9.0)
    with pytest.raises(RuntimeError, match="acc"):
        ops.window_merge_tokens(tok2, acc.double(), out2, win, 9.0)
    with pytest.raises(RuntimeError, match="acc"):
        ops.window_merge_tokens(tok2, acc[0], out2, win, 9.0)
    with pytest.raises(RuntimeError, match="length"):
        ops.window_merge_tokens(tok2, acc, out2, ([2, 3, 4], [0.5, 0.5], [True] * 3, [False] * 3), 9.0)
    for bad in (_window([2, 3, 2]), _window([2, 3, 7]), _window([2, 3, 4], [0.5, math.inf, 0.5])):
        with pytest.raises(RuntimeError, match="libaa_mi355"):
            ops.window_merge_tokens(tok2, acc, out2, bad, 9.0)
    with pytest.raises(RuntimeError, match="libaa_mi355"):
        ops.window_merge_tokens(tok2, acc, out2, win, math.inf)
    assert torch.equal(arena.cpu().view(torch.int16), before.cpu().view(torch.int16)) and (acc.cpu() == 3.0).all()
    # and the valid call on the same views works: frames 2..4 of the accumulator, nothing of the merged matrix (no slot is a last one)
    ops.window_merge_tokens(tok2, acc, out2, win, 9.0)
    a = acc.cpu()
    assert (a[:, [0, 1, 5, 6]] == 3.0).all() and not (a[:, 2:5] == 3.0).any()
    assert torch.equal(arena.cpu().view(torch.int16), before.cpu().view(torch.int16))


def test_gather_refusals_leave_the_output_untouched(backend):
    clips, ch, total, window, hw = 2, 4, 7, 3, 12
    d_ = dev()
    g = torch.Generator().manual_seed(6)
    n_src, n_dst = clips * ch * total * hw, clips * ch * window * hw
    arena = torch.randn(n_src + n_dst, generator=g).to(d_)
    before = arena.clone()
    src, dst = arena[:n_src], arena[n_src:]
    lib = _lib.get()

    def call(win=_window([2, 3, 4]), window_frames=None, **kw):
        d = _lib.AaWindowGather()
        t = dict(src=src, dst=dst)
        t.update({k: v for k, v in kw.items() if k in t})
        for k, v in t.items():
            setattr(d, k, None if v is None else C.c_void_p(v if isinstance(v, int) else v.data_ptr()))
        f = dict(clips=clips, channels=ch, total_frames=total, hw=hw)
        f.update({k: v for k, v in kw.items() if k in f})
        for k, v in f.items():
            setattr(d, k, v)
        d.window = ops.window_desc(win)
        if window_frames is not None:
            d.window.window_frames = window_frames
        return lib.aa_window_gather_latents(C.byref(d), ops._stream(arena))

    shape_, align_ = -1, -3
    assert lib.aa_window_gather_latents(None, None) == shape_
    for bad in (dict(src=None), dict(dst=None), dict(clips=0), dict(channels=0), dict(total_frames=0), dict(hw=0), dict(hw=-3),
                dict(clips=40000), dict(window_frames=0), dict(window_frames=_lib.AA_WINDOW_MAX + 1), dict(total_frames=2),
                dict(win=_window([2, 3, 7])), dict(win=_window([-1, 3, 4])), dict(win=_window([2, 3, 2])),
                dict(dst=src.data_ptr() + 16), dict(dst=src.data_ptr() + (n_src - 1) * 4), dict(src=dst.data_ptr() + 4)):
        assert call(**bad) == shape_, bad
    assert b"overlap" in lib.aa_last_error()
    assert call(src=src.data_ptr() + 2) == align_ and call(dst=dst.data_ptr() + 1) == align_
    assert call(win=_window([2, 3, 4], [math.nan] * 3)) == 0                       # the weights are not the gather's business
    arena[n_src:] = before[n_src:]
    src5 = src.view(clips, ch, total, hw, 1)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.window_gather_latents(src5.half(), _window([2, 3, 4]))
    with pytest.raises(RuntimeError, match="fp32"):
        ops.window_gather_latents(src, _window([2, 3, 4]))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.window_gather_latents(src5, _window([2, 3, 4]), out=dst[:clips * ch * 2 * hw].view(clips, ch, 2, hw, 1))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.window_gather_latents(src5.transpose(0, 1), _window([2, 3, 4]))
    for bad in (_window([2, 3, 2]), _window([2, 3, 7])):
        with pytest.raises(RuntimeError, match="libaa_mi355"):
            ops.window_gather_latents(src5, bad, out=dst.view(clips, ch, window, hw, 1))
    assert torch.equal(arena.cpu().view(torch.int32), before.cpu().view(torch.int32))
