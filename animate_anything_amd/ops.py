"""Torch-tensor front end of the C ABI (include/aa_mi355.h).

Tensors only carry device memory here: every function checks its operands, fills the C descriptor
and enqueues the HIP kernels on torch's current stream.  Activations are channels-last token
matrices `[tokens, C]` (see DESIGN.md "Data layout").  There is no fallback: operands that are not
on the GPU raise, as does a missing library.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import (AA_ACT_GELU, AA_ACT_NONE, AA_ACT_QUICK_GELU, AA_ACT_SILU, AA_BF16, AA_F16, AA_F32, AaAttention, AaAttnOperand,
                   AaBlend, AaConvGemm, AaFFFused, AaLinearRows, AaLinearFp8, AaQuantRowsFp8, AaDdimStepTok, AaDpmStep, AaDpmStepTok, AaEulerStepTok, AaGroupNorm, AaPackFrames, AaPackLatents, AaSeqSelfAttn, AaUnipcStepTok, AaFreeU, AaCfgRescale, AaApg, AaWindow, AaWindowGather, AaWindowMerge, AaFreeInit, AaKeepBlend)

_DT = {torch.float16: AA_F16, torch.bfloat16: AA_BF16, torch.float32: AA_F32}

# bench.py sets this to a list to record every contraction launch of one step (descriptor + the
# tensors that keep its pointers alive) so the dominant kernel can be re-timed in isolation.
TRACE = None

# Tile-shape autotuning of aa_conv_gemm: the first time a contraction signature is seen on the GPU
# (outside hipGraph capture) every tile shape of the library's table that fits is timed on the real
# operands and the fastest index is remembered for that signature (descriptor field `tile`).
AUTOTUNE = True
LAST_STAMPS = None
GN_PLANS = None            # a list: groupnorm() appends (groups per workgroup, pieces per thread, parts, grid) or None per call
MAX_OPERAND_BYTES = 1 << 31      # the contraction kernel's 32-bit operand offsets
FORCE_TILE = -1       # tests / sweeps: >= 0 puts this tile-table index into AaConvGemm.tile of every conv_gemm call (strict: ineligible = error)
# experiments: AaAttention._pad.  bit 0 (1): s_setprio 1 around the matrix clusters of the head_dim-64 kernel; bit 2 (4): short key sequences take the
# general kernel instead of attention_shortkv_kernel (A/B); bit 3 (8): long sequences take the two-query-blocks-per-wave kernel (round 6 experiment: slower, profiles/r06g_*).  (The eager row maximum of rounds 2-4 is a COMPILE-time variant: build.build(variant=
# ("eager", ["-DAA_ATTN_EAGER_MAX=1"])) loaded through AA_LIBRARY - there is no run-time bit for it.)  Unknown bits are rejected.
ATTN_FLAGS = int(os.environ.get("AA_ATTN_FLAGS", "0"))
if ATTN_FLAGS & ~13:
    raise RuntimeError(f"AA_ATTN_FLAGS={ATTN_FLAGS}: only bits 0 (value 1), 2 (value 4) and 3 (value 8) exist")
# A folded LayerNorm's row statistics reach the consumer as aa_ln_finalize's per-row coefficients (one 4.7 us launch per consumer, 99 per
# step) or raw (ABI 106 `ln_parts`: the consumer finalises 2 / 10 partial sums per row itself with independent loads).  Measured (r04h/i):
# the raw form removes 80 launches (-0.37 ms) and costs the K = 320 ... 1280 consumers 4-7 % (+0.7 ms: square root, reciprocal and the
# sums sit in every tile's prologue) - the launch stays the default.
LN_FINALIZE_LAUNCH = os.environ.get("AA_LN_RAW", "0") != "1"
TILE_PICKER = None    # tests / scripts/debug: callable(signature key, [(tile, K splits), ...]) -> the pair a conv_gemm call runs with (GPU or emulator)
PRODUCER_COEF = os.environ.get("AA_PRODUCER_COEF", "1") == "1"   # ABI 107: a producer whose tile spans the row writes the LayerNorm coefficients itself (no aa_ln_finalize launch)
LN_RAW_ANY_PARTS = False     # tests: let the consumer finalise any number of partial sums per row (a chain of dependent loads: +12-23 %)
K_SPLITS = 0          # tests: explicit K split count for calls that are not autotuned (0 = library decides)
# K-split launches of the hand-scheduled tiles can finish inside the kernel (AaConvGemm.tickets, ABI 106).  Measured on the step (r04g):
# not faster than partials + reduce launch (the autotuner moved the 8x8-level shapes to the compiled tile + reduce launch; step 62.5 ms
# with, 61.9 ms without) - the release / acquire fences around the ticket write back and invalidate the XCD's L2.  Off unless asked for.
USE_TICKETS = os.environ.get("AA_TICKETS", "0") == "1"
DEBUG_ABLATE = int(os.environ.get("AA_DEBUG_ABLATE", "0"))      # profiling only: forwarded to AaConvGemm.debug (16: row-major tile order, A/B of the grouped order)
class _TileTable:
    """The library's tile table (aa_conv_gemm_tile_info), read on first use: entries (rows, columns, K step, stages)."""

    def __init__(self):
        self._rows = None

    def _load(self):
        if self._rows is None:
            lib, rows, info = _lib.get(), [], (C.c_int32 * 7)()
            while lib.aa_conv_gemm_tile_info(len(rows), info) == 0:
                rows.append(tuple(info) + (int(lib.aa_conv_gemm_tile_flags(len(rows))),))
            self._rows = rows
        return self._rows

    def __iter__(self):
        return iter([(r[0], r[1], r[4], r[5]) for r in self._load()])

    def __len__(self):
        return len(self._load())

    def __getitem__(self, i):
        r = self._load()[i]
        return (r[0], r[1], r[4], r[5])

    def wave_cols(self, i):
        return self._load()[i][3]

    def per_cu(self, i):
        return self._load()[i][6]

    def flags(self, i):
        """aa_conv_gemm_tile_flags: bit 0 halo-slab kernel, bit 1 hand-scheduled stream, higher bits the DMA schedule."""
        return self._load()[i][7]


TILE_TABLE = _TileTable()
_tile_cache = {}


def _tile_table_id():
    """What a saved tile choice is valid for: the library version and the exact tile table it indexes."""
    lib = _lib.get()
    return {"aa_version": int(lib.aa_version()), "arch": "gfx950",
            "tiles": [list(TILE_TABLE._load()[i]) for i in range(len(TILE_TABLE))]}


def save_tile_cache(path):
    """Persist the autotuned (tile, K splits) choices (json) so a later process can skip the tuning launches."""
    import json
    with open(path, "w") as f:
        order = lambda kv: [(0, x, "") if isinstance(x, int) else (1, 0, str(x)) for x in kv[0]]      # (group signatures mix words and numbers)
        json.dump({"id": _tile_table_id(), "choices": [[list(k), list(v)] for k, v in sorted(_tile_cache.items(), key=order)]}, f)


def load_tile_cache(path):
    """Load choices saved by `save_tile_cache`; a file written against another library version / tile table is ignored
    (returns False): its indices would select arbitrary tiles."""
    import json
    with open(path) as f:
        blob = json.load(f)
    if not isinstance(blob, dict) or blob.get("id") != _tile_table_id():
        return False
    for k, v in blob["choices"]:
        _tile_cache[tuple(k)] = tuple(v)
    return True


if os.environ.get("AA_DUMP_TILE_CACHE"):                  # debugging aid: what did this process's autotuner choose
    import atexit
    atexit.register(lambda: save_tile_cache(os.environ["AA_DUMP_TILE_CACHE"]))

DEFAULT_TILE_CACHE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tile_cache_gfx950.json")
_default_cache_tried = False


def _load_default_tile_cache():
    """The committed tile choices for the benchmarked shapes (written by `bench.py --tile-cache`): fresh boxes then skip
    the tuning launches - and their box-to-box jitter - for every signature the file knows."""
    global _default_cache_tried
    if not _default_cache_tried:
        _default_cache_tried = True
        if os.path.exists(DEFAULT_TILE_CACHE) and os.environ.get("AA_NO_TILE_CACHE", "0") != "1":
            try:
                load_tile_cache(DEFAULT_TILE_CACHE)
            except Exception:
                pass


TICKET_COUNTERS = 1 << 16
_tickets = {}


def _ticket_array(t: torch.Tensor):
    """The zero-initialised counter array of AaConvGemm.tickets for the stream `t`'s calls run on: one per (device, stream) -
    K-split launches in flight on different streams must not share counters; the kernels hand every counter back as zero.
    Launches recorded into a hipGraph use a separate array per device (a capture stream is short-lived; the replays of the
    graphs of one device run one at a time in this package).  Never allocated inside a capture: a call captured before any eager
    call on that device gets None (partials + reduce launch)."""
    if not t.is_cuda:
        if not _addressable(t):
            return None
        a = _tickets.get("host")
        if a is None:
            a = _tickets["host"] = torch.zeros(TICKET_COUNTERS, dtype=torch.int32)
        return a
    capturing = torch.cuda.is_current_stream_capturing()
    key = (str(t.device), "graph" if capturing else torch.cuda.current_stream(t.device).cuda_stream)
    a = _tickets.get(key)
    if a is None and not capturing:
        a = _tickets[key] = torch.zeros(TICKET_COUNTERS, dtype=torch.int32, device=t.device)
        gkey = (str(t.device), "graph")
        if gkey not in _tickets:
            _tickets[gkey] = torch.zeros(TICKET_COUNTERS, dtype=torch.int32, device=t.device)
    return a


def _tile_candidates(d, rows):
    """(tile, k_splits) pairs worth timing: every tile shape that divides the packed width with the library's own split
    decision (0), plus explicit K splits where they turn an under-filled single round of workgroups into (nearly)
    full ones - the 16x16 / 8x8 levels, where 170 tiles of 256x256 would leave a third of the CUs idle."""
    dma = (d.c0 + d.c1) % 64 == 0 and d.c0 % 64 == 0 and d.out_dtype == d.dtype
    if not dma:
        return []
    out = []
    lib = _lib.get()
    for i, (bm, bn, bk, _st) in enumerate(TILE_TABLE):
        if not lib.aa_conv_gemm_tile_ok(C.byref(d), i):                 # width, GEGLU pairing, slab-kernel geometry
            continue
        out.append((i, 0))
        if TILE_TABLE.flags(i) & 1:                                     # halo-slab kernel: no K split
            continue
        if d.geglu or bm < 128:
            continue
        tiles = -(-rows // bm) * (d.n_pad // bn)
        slots = 256 * TILE_TABLE.per_cu(i)
        nk = d.k_pad // bk
        if tiles >= slots:
            continue
        fill1 = tiles / slots
        for sp in (2, 3, 4, 5, 6, 8):
            if nk // sp < 8:
                break
            wgs = tiles * sp
            fill = wgs / (-(-wgs // slots) * slots)
            if wgs <= 3 * slots and fill >= 0.8 and fill > fill1 + 0.1:
                out.append((i, sp))
    return out


AUTOTUNE_EVENTS = 0      # signatures tuned by timing launches in this process (0 when the committed tile cache covers the workload)


def _autotune(lib, d, stream, key, rows, dev):
    global AUTOTUNE_EVENTS
    AUTOTUNE_EVENTS += 1
    cands = _tile_candidates(d, rows)
    if "stats" in key:                                   # the caller wants the row statistics: only ways of carrying the call out that emit them
        def emits(c, sp):
            d.tile, d.k_splits = c, sp
            need = lib.aa_conv_gemm_workspace(C.byref(d))
            keep = (d.workspace, d.workspace_bytes)
            d.workspace, d.workspace_bytes = (C.c_void_p(1), need) if need else (None, 0)      # (only its presence is looked at)
            n = lib.aa_conv_gemm_row_stats_parts(C.byref(d))
            d.workspace, d.workspace_bytes = keep
            return n > 0
        cands = [c for c in cands if emits(*c)] or cands
    best = (-1, 0)
    if len(cands) == 1:                                  # (one way left - e.g. the only tile that emits the row statistics: take it, do not
        best = cands[0]                                  #  fall back to the library's own choice, which may be another: ADVICE r04)
    if len(cands) > 1:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ws_keep = (d.workspace, d.workspace_bytes)

        def timed(c, sp, reps, raw=False):
            d.tile, d.k_splits = c, sp
            need = lib.aa_conv_gemm_workspace(C.byref(d))
            ws = torch.empty(max(need // 4, 1), dtype=torch.float32, device=dev)
            d.workspace, d.workspace_bytes = C.c_void_p(ws.data_ptr()), need
            if lib.aa_conv_gemm(C.byref(d), stream) != 0:
                return None
            # one launch per measurement, synchronised in between: back-to-back launches of one kernel overlap
            # their tails, which hides exactly the last-round under-fill that a dependent chain of kernels pays
            ts = []
            for _ in range(reps):
                e0.record()
                lib.aa_conv_gemm(C.byref(d), stream)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            if raw:
                return ts
            ts.sort()
            return ts[len(ts) // 2] if reps > 5 else ts[1]

        # screening pass over every candidate, then a run-off between the four fastest: three interleaved passes of seven launches
        # each, median of the 21 (r04: with one 11-launch pass per finalist the choice flipped between runs on close calls - clock /
        # power drift during a pass favours whoever runs at the right moment - and a flipped 3x3 choice costs 0.1 ms of the step)
        first = sorted((t, c) for c in cands for t in [timed(c[0], c[1], 5)] if t is not None)
        finalists = [c for _, c in first[:4]]
        samples = {c: [] for c in finalists}
        for _ in range(3):
            for c in finalists:
                ts = timed(c[0], c[1], 7, raw=True)
                if ts is not None:
                    samples[c] += ts
        final = sorted((sorted(v)[len(v) // 2], c) for c, v in samples.items() if v)
        if final:
            best = final[0][1]
        d.workspace, d.workspace_bytes = ws_keep
    _tile_cache[key] = best
    return best


def _autotune_groupnorm(lib, d, ws, nbytes, stream, key):
    """(1, 0) if the statistics + apply pair beats the single kernel for this signature, else (0, 0)."""
    global AUTOTUNE_EVENTS
    info = (C.c_int32 * 4)()
    best = (0, 0)
    if lib.aa_groupnorm_plan(C.byref(d), info):
        AUTOTUNE_EVENTS += 1
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(two):
            lib.aa_set_groupnorm_two_pass(two)
            try:
                ts = []
                for i in range(9):
                    e0.record()
                    lib.aa_groupnorm(C.byref(d), C.c_void_p(ws.data_ptr()), nbytes, stream)
                    e1.record()
                    e1.synchronize()
                    if i >= 2:
                        ts.append(e0.elapsed_time(e1))
            finally:
                lib.aa_set_groupnorm_two_pass(0)
            ts.sort()
            return ts[len(ts) // 2]

        t1, t2 = timed(0), timed(1)
        best = (1, 0) if t2 < t1 else (0, 0)
    _tile_cache[key] = best
    return best


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _addressable(t: torch.Tensor) -> bool:      # on the GPU - or anywhere, while the library in use takes host pointers (the tests' emulator build)
    return t.is_cuda or _lib.host_pointers_ok()


def _check(*tensors, contiguous=True):
    for t in tensors:
        if t is None:
            continue
        if not _addressable(t):
            raise RuntimeError("animate_anything_amd ops run on the GPU only (tensor is on %s)" % t.device)
        if contiguous and not t.is_contiguous():
            raise RuntimeError("animate_anything_amd ops need contiguous tensors")


def _check_token_matrix(op, name, t, ref, how_many, device_of=None, rows=None, channels=0):
    """One token-matrix operand `name` of `op`: 2-d, rows contiguous (they may be pitched), fp16 / bf16 and of `ref`'s dtype (`how_many`: "all" /
    "both", as the message counts the operands); device_of = (name, tensor): on that tensor's device; rows: holds `rows` rows of `channels` channels."""
    _check(t, contiguous=False)
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or t.dtype != ref.dtype or t.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError(f"{op}: {name} must be a 2-d fp16 / bf16 token matrix with contiguous rows, {how_many} of one dtype")
    if device_of is not None and t.device != device_of[1].device:
        raise RuntimeError(f"{op}: {name} is on {t.device}, {device_of[0]} on {device_of[1].device}")
    if rows is not None and (t.shape[0] < rows or t.shape[1] < channels):
        raise RuntimeError(f"{op}: {name} {tuple(t.shape)} does not hold {rows} rows of {channels} channels")


def _stream(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def _run(fn, *args):
    rc = fn(*args)
    if rc != 0:
        raise RuntimeError("libaa_mi355: " + _lib.get().aa_last_error().decode())


def _round_up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------- weights
@dataclass
class PackedWeight:
    """Weights laid out for aa_conv_gemm: [n_pad, k_pad], k ordered (tap, channel)."""
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    n_out: int
    kh: int
    kw: int
    cin: int          # channels per tap as stored (after padding to a multiple of 8)
    geglu: int = 0    # 0, or the value/gate interleave granularity of a GEGLU projection
    k_order: int = 0  # 0: K = (tap, channel); 1: K = (64-channel chunk, tap, channel)
    ln_cols: Optional[torch.Tensor] = None   # LayerNorm folded into these weights: fp32 [2, n_pad] = colsum(W'), b + beta W^T
    ln_eps: float = 0.0

    @property
    def n_pad(self):
        return self.w.shape[0]

    @property
    def k_pad(self):
        return self.w.shape[1]


def pack_weight(weight: torch.Tensor, bias: Optional[torch.Tensor] = None, geglu: bool = False, ln=None) -> PackedWeight:
    """Pack an nn.Linear [n,k], nn.Conv2d [n,c,kh,kw] or nn.Conv3d [n,c,kt,1,1] weight.

    GEGLU (diffusers `GEGLU.proj`, rows [0,d) = value, [d,2d) = gate) is re-ordered into alternating
    blocks of 32 value rows / 32 gate rows: a value block and its gate block are then neighbouring accumulator
    blocks of the same wavefront and the gating happens in registers.

    `ln` = (gamma, beta, eps) folds the LayerNorm in front of an nn.Linear into it (AaConvGemm.ln_stats):
    LN(x) W^T + b = rstd (x W'^T) - rstd mean colsum(W') + (b + beta W^T) with W' = W diag(gamma) rounded to the storage type;
    colsum is taken over the ROUNDED W', so the mean term cancels exactly what the matrix cores accumulate."""
    w = weight.detach()
    b_ln = None
    if ln is not None:
        gamma, beta, eps = ln
        assert w.dim() == 2, "the LayerNorm fold is for nn.Linear weights"
        wf = w.float()
        b_ln = wf @ beta.detach().float() + (0.0 if bias is None else bias.detach().float())      # fp32 [n]
        w = (wf * gamma.detach().float()[None, :]).to(w.dtype)
        bias = None
    if w.dim() == 2:
        n, kh, kw, cin = w.shape[0], 1, 1, w.shape[1]
        w4 = w.reshape(n, 1, 1, cin)
    elif w.dim() == 4:
        n, cin, kh, kw = w.shape
        w4 = w.permute(0, 2, 3, 1)
    elif w.dim() == 5:
        n, cin, kh, kw = w.shape[0], w.shape[1], w.shape[2], 1
        assert w.shape[3] == 1 and w.shape[4] == 1
        w4 = w.reshape(n, cin, kh).permute(0, 2, 1).reshape(n, kh, 1, cin)
    else:
        raise ValueError("unsupported weight rank %d" % w.dim())
    cpad = _round_up(cin, 8)
    if cpad != cin:
        w4 = torch.nn.functional.pad(w4, (0, cpad - cin))
    k = kh * kw * cpad
    k_order = 0
    if kh * kw > 1 and cpad % 64 == 0 and n % 8 == 0:      # (only shapes that take the LDS-DMA path)
        # multi-tap filter: chunk-major K so the 9 (3) taps of one 64-channel slab are consecutive K steps
        w4 = w4.reshape(n, kh * kw, cpad // 64, 64).permute(0, 2, 1, 3)
        k_order = 1
    w2 = w4.reshape(n, k)
    b = None if bias is None else bias.detach()
    if geglu:
        d = n // 2
        gran = 32                                          # one 32-column accumulator block of value, the next one of gate
        assert d % gran == 0, "GEGLU inner width must be a multiple of 32"
        val = torch.arange(d, device=w.device).reshape(d // gran, 1, gran)
        src = torch.cat([val, val + d], dim=1).reshape(-1)
        w2 = w2[src]
        b = None if b is None else b[src]
        b_ln = None if b_ln is None else b_ln[src]
    n_pad, k_pad = _round_up(n, 64), _round_up(k, 64)
    out = torch.zeros(n_pad, k_pad, dtype=w.dtype, device=w.device)
    out[:n, :k] = w2
    if b is not None and geglu and n_pad != n:
        b = torch.nn.functional.pad(b, (0, n_pad - n))
    ln_cols, ln_eps = None, 0.0
    if ln is not None:
        ln_cols = torch.zeros(2, n_pad, dtype=torch.float32, device=w.device)
        ln_cols[0] = out.float().sum(dim=1)
        ln_cols[1, :n] = b_ln
        ln_eps = float(ln[2])
    return PackedWeight(out.contiguous(), None if b is None else b.contiguous(), n, kh, kw, cpad, gran if geglu else 0, k_order,
                        ln_cols, ln_eps)


def pack_upsample2x_weights(weight: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """Nearest x2 upsample + 3x3 / pad 1 convolution (diffusers Upsample2D) == four 2x2 convolutions on the STORED grid, one per
    output parity class (a, b) = (Y & 1, X & 1): virtual rows Y-1, Y, Y+1 of output row Y = 2y + a read stored rows
    (y-1, y, y) for a = 0 and (y, y, y+1) for a = 1 - the taps that read the same stored pixel are summed here (fp32, one
    rounding).  Returns {(a, b): PackedWeight of the [N, C, 2, 2] filter}; class (a, b) runs with padding (1 - a, 1 - b) and
    out_map (2, 2, a, b).  4/9 of the multiply-adds of the 3x3 form; zero padding of the virtual grid == zero padding of the
    stored grid for every class (the summed taps of a class fall inside or outside together)."""
    n, c, kh, kw = weight.shape
    assert kh == 3 and kw == 3
    w = weight.detach().float()
    groups = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}          # parity -> taps of the two stored rows / columns
    out = {}
    for a in (0, 1):
        for b in (0, 1):
            f = torch.zeros(n, c, 2, 2, dtype=torch.float32, device=w.device)
            for r, dys in enumerate(groups[a]):
                for q, dxs in enumerate(groups[b]):
                    for dy in dys:
                        for dx in dxs:
                            f[:, :, r, q] += w[:, :, dy, dx]
            out[(a, b)] = pack_weight(f.to(weight.dtype), bias)
    return out


@dataclass
class RowStats:
    """Partial (sum, sum of squares) per row of a token matrix, [rows, parts, 2] fp32, left by the contraction that wrote it
    (AaConvGemm.row_stats); `coef(channels, eps)` turns them (aa_ln_finalize, once) into the per-row (-mean, sqrt(var + eps),
    rstd, 0) that the contraction folding the LayerNorm of that matrix takes (AaConvGemm.ln_stats)."""
    data: Optional[torch.Tensor]      # None: the producer wrote the finished coefficients itself (AaConvGemm.row_coef, ABI 107)
    rows: int
    parts: int
    _coef: Optional[torch.Tensor] = None
    _coef_key: tuple = ()

    def coef(self, channels, eps):
        if self._coef is None or self._coef_key != (channels, eps):
            if self.data is None:
                raise RuntimeError("RowStats: finished coefficients for (channels, eps) = %r were asked for %r" % (self._coef_key, (channels, eps)))
            out = torch.empty(self.rows, 4, dtype=torch.float32, device=self.data.device)
            _run(_lib.get().aa_ln_finalize, _ptr(self.data), self.parts, _ptr(out), self.rows, channels, float(eps), _stream(self.data))
            self._coef, self._coef_key = out, (channels, eps)
        return self._coef

    def repeat(self, n):
        if self.data is None:
            return RowStats(None, self.rows * n, 0, torch.cat([self._coef] * n), self._coef_key)
        return RowStats(torch.cat([self.data] * n), self.rows * n, self.parts)


# ------------------------------------------------------------------------------------- contraction
@dataclass
class Geom:
    """Output grid and source mapping of one aa_conv_gemm call (all in pixels / tokens)."""
    n_img: int
    h_in: int
    w_in: int
    h_out: int
    w_out: int
    stride: int = 1
    pad_h: int = 0
    pad_w: int = 0
    h_virt: int = 0
    w_virt: int = 0

    @property
    def rows(self):
        return self.n_img * self.h_out * self.w_out


def linear_geom(rows: int) -> Geom:
    return Geom(1, 1, rows, 1, rows)


def conv3x3_geom(n, h, w, stride=1, pad=1, up_to=None) -> Geom:
    """3x3 conv over [n,h,w]; `up_to`=(H,W) inserts a nearest resize in front (Upsample2D);
    stride 2 / pad 1 is the UNet Downsample2D, stride 2 / pad 0 with a one-pixel bottom/right halo
    the VAE one (F.pad (0,1,0,1))."""
    hv, wv = (h, w) if up_to is None else up_to
    if stride == 1:
        ho, wo = hv, wv
    elif pad == 1:
        ho, wo = (hv + 2 - 3) // stride + 1, (wv + 2 - 3) // stride + 1
    else:
        ho, wo = (hv + 1 - 3) // stride + 1, (wv + 1 - 3) // stride + 1
    return Geom(n, h, w, ho, wo, stride, pad, pad, hv, wv)


def tconv_geom(clips, frames, hw) -> Geom:
    """Conv3d (3,1,1), padding (1,0,0): a 3x1 conv over a [clips, frames, hw] grid."""
    return Geom(clips, frames, hw, frames, hw, 1, 1, 0)


def conv_gemm(x0: torch.Tensor, pw: PackedWeight, g: Geom, x1: Optional[torch.Tensor] = None,
              rowvec: Optional[torch.Tensor] = None, rowvec_div: int = 1,
              residual: Optional[torch.Tensor] = None, act: int = AA_ACT_NONE, out_dtype=None,
              out_scale: float = 1.0, bias_per_row: bool = False, out: Optional[torch.Tensor] = None,
              bias: Optional[torch.Tensor] = "packed", acc_scale: float = 1.0, out_map=None, ln_stats=None, row_stats: bool = False,
              coef_eps: Optional[float] = None):
    """`out_map` = (sy, sx, oy, ox): GEMM row (img, y, x) goes to pixel (y * sy + oy, x * sx + ox) of the [n_img, h_out * sy,
    w_out * sx] grid that `out` (required then) holds - AaConvGemm.out_sy .. out_ox.
    `ln_stats` = RowStats of x0's rows (from the call that produced x0): `pw` must carry a folded LayerNorm (pack_weight(ln=...)).
    `row_stats=True`: returns (out, RowStats or None) - the partial row statistics of `out` when this call can emit them; with
    `coef_eps` (the epsilon of the LayerNorm that will consume them) a call whose tile spans the output row writes the finished
    per-row coefficients itself (ABI 107: no aa_ln_finalize launch in front of the consumer)."""
    lib = _lib.get()
    osc = 1 if out_map is None else out_map[0] * out_map[1]
    if out_map is not None and (out is None or out.shape[0] != g.rows * osc):
        raise RuntimeError("conv_gemm: out_map needs `out` = the whole [n_img * h_out * sy * w_out * sx, N] grid")
    b = pw.bias if isinstance(bias, str) else bias
    _check(x0, x1, pw.w, b, residual, out)
    if rowvec is not None:                                 # may be a column slice of a wider matrix (row pitch = stride(0))
        if not _addressable(rowvec) or rowvec.stride(-1) != 1:
            raise RuntimeError("conv_gemm: rowvec must be a GPU tensor with contiguous rows")
    c0 = x0.shape[-1]
    c1 = 0 if x1 is None else x1.shape[-1]
    # The LDS-DMA kernel addresses every operand with 32-bit byte offsets (< 2 GiB).  Bigger activations (the VAE above
    # 512x512 x 16 frames) are cut along the image axis - images are independent rows of the implicit GEMM.
    n_cols_ = pw.n_out // 2 if pw.geglu else pw.n_out
    in_rows = g.n_img * g.h_in * g.w_in
    biggest = 2 * max(in_rows * max(c0, c1), g.rows * max(osc * (n_cols_ if out is None else out.stride(0)),
                                                          0 if residual is None else residual.stride(0)))
    if biggest >= MAX_OPERAND_BYTES and g.n_img > 1 and not bias_per_row:
        if out is None:
            out = torch.empty(g.rows, n_cols_, dtype=x0.dtype if out_dtype is None else out_dtype, device=x0.device)
        parts = min(g.n_img, -(-biggest // (MAX_OPERAND_BYTES // 2)))
        per = -(-g.n_img // parts)
        ri, ro = g.h_in * g.w_in, g.h_out * g.w_out
        for i0 in range(0, g.n_img, per):
            n = min(per, g.n_img - i0)
            gi = Geom(n, g.h_in, g.w_in, g.h_out, g.w_out, g.stride, g.pad_h, g.pad_w, g.h_virt, g.w_virt)
            rv = rowvec
            if rowvec is not None:                         # row-vector groups are whole images (or whole clips of them)
                assert (i0 * ro) % rowvec_div == 0 and ((i0 + n) * ro) % rowvec_div == 0 or i0 + n == g.n_img
                rv = rowvec[(i0 * ro) // rowvec_div:]
            ls = None
            if ln_stats is not None:                       # the statistics of a chunk's rows (the folded call is linear: ri == ro)
                if ln_stats.data is None:                  # finished coefficients from the producer (ABI 107): slice those
                    ls = RowStats(None, n * ri, 0, ln_stats._coef[i0 * ri:(i0 + n) * ri], ln_stats._coef_key)
                else:
                    ls = RowStats(ln_stats.data[i0 * ri:(i0 + n) * ri], n * ri, ln_stats.parts)
            conv_gemm(x0[i0 * ri:(i0 + n) * ri], pw, gi, None if x1 is None else x1[i0 * ri:(i0 + n) * ri], rv, rowvec_div,
                      None if residual is None else residual[i0 * ro:(i0 + n) * ro], act, out_dtype, out_scale, False,
                      out[i0 * ro * osc:(i0 + n) * ro * osc], bias, acc_scale, out_map, ls)
        return (out, None) if row_stats else out           # (chunks may run different tiles: no common statistics layout - the caller keeps its LayerNorm)
    d, key, out, b = _conv_gemm_desc(x0, pw, g, x1, rowvec, rowvec_div, residual, act, out_dtype, out_scale, bias_per_row, out, bias,
                                     acc_scale, out_map, ln_stats, row_stats)
    _choose_tile(lib, d, key, g.rows, x0, (x0, x1, residual, rowvec), out)
    ws = None
    need = lib.aa_conv_gemm_workspace(C.byref(d))        # split-K scratch for few-tile / long-K calls
    if DEBUG_ABLATE & 8:                                  # phase probe: [workgroup][8] shader-clock stamps
        global LAST_STAMPS
        ws = LAST_STAMPS = torch.zeros(2, 1 << 16, 8, dtype=torch.int64, device=x0.device)
        d.workspace, d.workspace_bytes = _ptr(ws), ws.numel() * 8
    elif need:
        ws = torch.empty(need // 4, dtype=torch.float32, device=x0.device)
        d.workspace, d.workspace_bytes = _ptr(ws), need
    stats = None
    if row_stats:                                         # after tile / workspace are settled: the plan decides whether it can emit them
        parts = lib.aa_conv_gemm_row_stats_parts(C.byref(d))
        if parts > 0 and coef_eps is not None and PRODUCER_COEF and lib.aa_conv_gemm_row_coef_ok(C.byref(d)):
            coef = torch.empty(g.rows, 4, dtype=torch.float32, device=x0.device)       # the tile spans the row: finished coefficients
            stats = RowStats(None, g.rows, 0, coef, (pw.n_out, float(coef_eps)))
            d.row_coef, d.row_coef_eps = _ptr(coef), float(coef_eps)
        elif parts > 0:
            stats = RowStats(torch.empty(g.rows, parts, 2, dtype=torch.float32, device=x0.device), g.rows, parts)
            d.row_stats, d.row_stats_parts = _ptr(stats.data), parts
    _run(lib.aa_conv_gemm, C.byref(d), _stream(x0))
    if TRACE is not None:
        TRACE.append((d, (x0, x1, pw, b, rowvec, residual, out, ws, stats, ln_stats)))
    return (out, stats) if row_stats else out


def _conv_gemm_desc(x0, pw, g, x1=None, rowvec=None, rowvec_div=1, residual=None, act=AA_ACT_NONE, out_dtype=None, out_scale=1.0,
                    bias_per_row=False, out=None, bias="packed", acc_scale=1.0, out_map=None, ln_stats=None, row_stats=False):
    """The descriptor of one contraction (conv_gemm's arguments) with everything but the way it is carried out (tile, K split,
    workspace, statistics outputs): -> (descriptor, tile-choice signature, out, bias).  Shared by conv_gemm and conv_gemm_group."""
    b = pw.bias if isinstance(bias, str) else bias
    c0 = x0.shape[-1]
    c1 = 0 if x1 is None else x1.shape[-1]
    if c0 + c1 != pw.cin:
        raise RuntimeError(f"conv_gemm: activation has {c0}+{c1} channels, weight expects {pw.cin}")
    n_cols = pw.n_out // 2 if pw.geglu else pw.n_out
    odt = x0.dtype if out_dtype is None else out_dtype
    if out is None:
        out = torch.empty(g.rows, n_cols, dtype=odt, device=x0.device)
    d = AaConvGemm()
    d.a0, d.a1, d.w, d.bias = _ptr(x0), _ptr(x1), _ptr(pw.w), _ptr(b)
    d.rowvec, d.residual, d.out = _ptr(rowvec), _ptr(residual), _ptr(out)
    d.c0, d.c1 = c0, c1
    d.n_img, d.h_in, d.w_in = g.n_img, g.h_in, g.w_in
    d.h_virt, d.w_virt = g.h_virt or g.h_in, g.w_virt or g.w_in
    d.h_out, d.w_out = g.h_out, g.w_out
    d.kh, d.kw, d.stride, d.pad_h, d.pad_w = pw.kh, pw.kw, g.stride, g.pad_h, g.pad_w
    d.n_out, d.n_pad, d.k_pad = pw.n_out, pw.n_pad, pw.k_pad
    d.rowvec_div = rowvec_div
    d.rowvec_ld = 0 if rowvec is None or rowvec.dim() < 2 else rowvec.stride(0)
    d.ldo = out.stride(0)
    d.ldr = 0 if residual is None else residual.stride(0)
    d.act, d.geglu, d.bias_per_row = act, int(pw.geglu), int(bias_per_row)
    d.dtype, d.out_dtype, d.out_scale = _DT[x0.dtype], _DT[odt], out_scale
    d.acc_scale = 0.0 if acc_scale == 1.0 else float(acc_scale)
    if out_map is not None:
        d.out_sy, d.out_sx, d.out_oy, d.out_ox = (int(v) for v in out_map)
    if ln_stats is not None:
        if pw.ln_cols is None or ln_stats.rows != g.rows:
            raise RuntimeError("conv_gemm: ln_stats needs weights packed with a folded LayerNorm and statistics of every row of x0")
        if ln_stats.data is None or LN_FINALIZE_LAUNCH or (ln_stats.parts not in (2, 10) and not LN_RAW_ANY_PARTS):      # aa_ln_finalize in between (r04h: finalising the pieces of a row one dependent load
                                                                                      # after the other costs the consumer 12-23 %: unrolled forms for 2 / 10 parts only)
            d.ln_stats, d.ln_cols = _ptr(ln_stats.coef(c0, pw.ln_eps)), _ptr(pw.ln_cols)
        else:                                             # the kernel finalises the producer's partial sums itself
            d.ln_stats, d.ln_cols = _ptr(ln_stats.data), _ptr(pw.ln_cols)
            d.ln_parts, d.ln_eps = ln_stats.parts, float(pw.ln_eps)
    elif pw.ln_cols is not None:
        raise RuntimeError("conv_gemm: these weights carry a folded LayerNorm: pass the row statistics of x0 (ln_stats)")
    if acc_scale == 0.0:
        raise ValueError("conv_gemm: acc_scale == 0 is not representable (0 means 1 in the C ABI)")
    d.k_order = pw.k_order
    d.debug = DEBUG_ABLATE
    tk = _ticket_array(x0) if USE_TICKETS else None
    if tk is not None:
        d.tickets, d.tickets_len = _ptr(tk), tk.numel()
    d.tile, d.k_splits = -1, K_SPLITS
    key = (d.dtype, g.n_img, g.h_in, g.w_in, d.h_virt, d.w_virt, g.h_out, g.w_out, g.stride, pw.kh, pw.kw, c0, c1,
           pw.n_out, d.geglu, residual is not None) + (("ln",) if ln_stats is not None else ()) + (("stats",) if row_stats else ())
    if odt != x0.dtype:                                   # another output type runs the gather kernel: never the tile tuned for the 16-bit call of the same shape
        key += (("out", d.out_dtype),)
    return d, key, out, b


def _aliases(inputs, outs):
    """Does an input share storage with an output (tuning launches write the outputs repeatedly: only safe when none does)."""
    ptrs = {o.untyped_storage().data_ptr() for o in outs}
    return any(t is not None and t.untyped_storage().data_ptr() in ptrs for t in inputs)


def _choose_tile(lib, d, key, rows, x0, inputs, out):
    """Settle (d.tile, d.k_splits) of one contraction: TILE_PICKER, else the tile cache / autotuner, else the library's own choice."""
    d.tile, d.k_splits = -1, K_SPLITS
    if TILE_PICKER is not None and FORCE_TILE < 0 and K_SPLITS == 0:      # tile fuzzing (tests, scripts/debug): any eligible pair must be right
        cands = _tile_candidates(d, rows)
        d.tile, d.k_splits = TILE_PICKER(key, cands) if cands else (-1, 0)
    elif AUTOTUNE and x0.is_cuda and FORCE_TILE < 0 and K_SPLITS == 0:    # (explicit tile / split requests of tests and sweeps are not re-tuned)
        _load_default_tile_cache()
        choice = _tile_cache.get(key)
        if choice is None and not _aliases(inputs, (out,)) and not torch.cuda.is_current_stream_capturing():
            choice = _autotune(lib, d, _stream(x0), key, rows, x0.device)
        d.tile, d.k_splits = (-1, 0) if choice is None else choice
    if FORCE_TILE >= 0:                                   # tests / sweeps: THIS tile or an error (aa_conv_gemm rejects a tile that
        d.tile = FORCE_TILE                               # cannot carry out the call; the thread-local override merely prefers)


# Independent contractions issued back to back each pay a kernel boundary (ramp, partial last round: ~13 us per extra half-size kernel,
# profiles/design_history_r05.md).  aa_conv_gemm_group runs 2..4 of them as ONE launch of one hand-scheduled tile.
#   bit 0 (1): the four parity classes of Upsample2D - on: -0.30 ms of the step (12 launches + 4 leftover launches + 4 reduce launches -> 3);
#   bit 1 (2): ResnetBlock2D's conv_shortcut next to conv1 - OFF: measured +0.13 ms on the step (the single conv1 keeps its split-off last
#              round on a small tile, the group runs every row on the big one; profiles/r16_group_ab_same_box.txt).
# AA_GROUP=0 restores the separate launches everywhere, AA_GROUP=3 groups at both sites.
GROUP = int(os.environ.get("AA_GROUP", "1"))
if GROUP & ~3:
    raise RuntimeError(f"AA_GROUP={GROUP}: only bits 0 (value 1, Upsample2D classes) and 1 (value 2, conv_shortcut + conv1) exist")
GROUP_MAX = 4


def _group_key(keys):
    """The tile-choice signature of a group: its members' signatures in call order, flat (the tile cache stores flat keys)."""
    out = ("group", len(keys))
    for k in keys:
        out += ("|",) + tuple(k)
    return out


def _autotune_group(lib, arr, n, ds, cands, stream, key):
    """The fastest of `cands` (tiles every member accepts) for this group, timed like _autotune: one launch per measurement."""
    global AUTOTUNE_EVENTS
    AUTOTUNE_EVENTS += 1
    best = cands[0]
    if len(cands) > 1:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(c, reps):
            for d in ds:
                d.tile = c[0]
            if lib.aa_conv_gemm_group(arr, n, stream) != 0:
                return []
            ts = []
            for _ in range(reps):
                e0.record()
                lib.aa_conv_gemm_group(arr, n, stream)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            return ts

        samples = {c: [] for c in cands}
        for _ in range(3):                                # interleaved passes (clock / power drift must not favour one candidate)
            for c in cands:
                samples[c] += timed(c, 7)
        final = sorted((sorted(v)[len(v) // 2], c) for c, v in samples.items() if v)
        if final:
            best = final[0][1]
    _tile_cache[key] = best
    return best


def conv_gemm_group(calls, unsplit_only=False):
    """2..4 independent contractions as ONE kernel launch (aa_conv_gemm_group): `calls` = dicts of conv_gemm's arguments (x0, pw, g and
    keywords; no ln_stats / row_stats / out_dtype).  No member may read another member's output.  Every member runs on one tile, chosen
    per group signature (TILE_PICKER, tile cache, autotuner) among the tiles the library offers for this group, with one K range.
    Returns the list of outputs - or None, with nothing launched, when the library offers no tile for the group (the caller then
    issues the calls one by one).  `unsplit_only`: also None when a member on its own would run with a K split (a long-K member
    that needs the split to fill the chip loses more inside a group than the launch saves)."""
    lib = _lib.get()
    n = len(calls)
    if not 2 <= n <= GROUP_MAX:
        raise RuntimeError(f"conv_gemm_group: {n} calls (2..{GROUP_MAX})")
    ms = []
    for kw in calls:
        kw = dict(kw)
        x0, pw, g = kw.pop("x0"), kw.pop("pw"), kw.pop("g")
        if kw.get("ln_stats") is not None or kw.get("row_stats") or kw.get("out_dtype") is not None:
            raise RuntimeError("conv_gemm_group: members carry no folded LayerNorm, row statistics or output dtype of their own")
        osc = 1 if kw.get("out_map") is None else kw["out_map"][0] * kw["out_map"][1]
        if kw.get("out_map") is not None and (kw.get("out") is None or kw["out"].shape[0] != g.rows * osc):
            raise RuntimeError("conv_gemm_group: out_map needs `out` = the whole [n_img * h_out * sy * w_out * sx, N] grid")
        _check(x0, kw.get("x1"), pw.w, kw.get("residual"), kw.get("out"))
        d, key, out, b = _conv_gemm_desc(x0, pw, g, **kw)
        ms.append((d, key, out, (x0, kw.get("x1"), pw, b, kw.get("rowvec"), kw.get("residual"), out, None, None, None), g.rows))
    ds = [m[0] for m in ms]
    x0 = calls[0]["x0"]
    if unsplit_only:
        for (d, key, out, keep, rows) in ms:
            _choose_tile(lib, d, key, rows, x0, (keep[0], keep[1], keep[5], keep[4]), out)
            if d.k_splits > 1 or lib.aa_conv_gemm_workspace(C.byref(d)):
                return None
    for d in ds:
        d.tile, d.k_splits, d.tickets, d.tickets_len = -1, 1, None, 0
    arr = (C.POINTER(AaConvGemm) * n)(*[C.pointer(d) for d in ds])
    cands = [(i, 0) for i in range(len(TILE_TABLE)) if lib.aa_conv_gemm_group_ok(arr, n, i)]
    if FORCE_TILE >= 0:
        cands = [c for c in cands if c[0] == FORCE_TILE]
    if not cands:
        return None
    key = _group_key([m[1] for m in ms])
    choice = cands[0]
    if TILE_PICKER is not None and FORCE_TILE < 0:
        choice = TILE_PICKER(key, cands)
    elif AUTOTUNE and x0.is_cuda and FORCE_TILE < 0:
        _load_default_tile_cache()
        choice = _tile_cache.get(key)
        if choice is not None and tuple(choice) not in cands:
            choice = None
        inputs = [t for m in ms for t in (m[3][0], m[3][1], m[3][4], m[3][5])]
        if choice is None and not _aliases(inputs, [m[2] for m in ms]) and not torch.cuda.is_current_stream_capturing():
            choice = _autotune_group(lib, arr, n, ds, cands, _stream(x0), key)
        if choice is None:
            choice = cands[0]
    for d in ds:
        d.tile = choice[0]
    _run(lib.aa_conv_gemm_group, arr, n, _stream(x0))
    if TRACE is not None:                                 # every member on its own: the roofline / launch-list accounting sees contractions
        for m in ms:
            TRACE.append((m[0], m[3]))
    return [m[2] for m in ms]


# ------------------------------------------------------------------------------------- norms
def groupnorm(x0: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, n_groups_img: int,
              tokens_per_group: int, num_groups: int = 32, eps: float = 1e-5, silu: bool = False,
              x1: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.get()
    _check(x0, x1, gamma, beta, out)
    c0 = x0.shape[-1]
    c1 = 0 if x1 is None else x1.shape[-1]
    y = torch.empty(n_groups_img * tokens_per_group, c0 + c1, dtype=x0.dtype, device=x0.device) if out is None else out
    d = AaGroupNorm()
    d.x0, d.x1, d.gamma, d.beta, d.y = _ptr(x0), _ptr(x1), _ptr(gamma), _ptr(beta), _ptr(y)
    d.c0, d.c1 = c0, c1
    d.n_groups_img, d.tokens_per_group, d.num_groups = n_groups_img, tokens_per_group, num_groups
    d.silu, d.dtype, d.eps = int(silu), _DT[x0.dtype], eps
    nbytes = lib.aa_groupnorm_workspace(C.byref(d))
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=x0.device)
    # one kernel (x kept in registers between statistics and normalisation) or the statistics + apply pair: the library offers
    # the single kernel wherever the shape allows; which of the two is faster is measured once per signature and kept with
    # the tile choices (key (-1, ...): tile_cache_gfx950.json)
    two_pass = False
    if AUTOTUNE and x0.is_cuda:
        key = (-1, d.dtype, c0, c1, n_groups_img, tokens_per_group, num_groups, int(silu))
        _load_default_tile_cache()
        choice = _tile_cache.get(key)
        if choice is None and y.data_ptr() != x0.data_ptr() and not torch.cuda.is_current_stream_capturing():
            choice = _autotune_groupnorm(lib, d, ws, nbytes, _stream(x0), key)
        two_pass = bool(choice and choice[0])
    if two_pass:
        lib.aa_set_groupnorm_two_pass(1)
    try:
        if GN_PLANS is not None:                          # (tests / bench breakdown) how this call runs: None = two kernels
            info = (C.c_int32 * 4)()
            GN_PLANS.append(tuple(info) if lib.aa_groupnorm_plan(C.byref(d), info) else None)
        _run(lib.aa_groupnorm, C.byref(d), _ptr(ws), nbytes, _stream(x0))
    finally:
        if two_pass:
            lib.aa_set_groupnorm_two_pass(0)
    return y


def groupnorm_coef(x0: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, n_groups_img: int, tokens_per_group: int, num_groups: int = 32,
                   eps: float = 1e-5) -> torch.Tensor:
    """The statistics pass of `groupnorm` alone: fp32 [n_groups_img, 2, C] = per-channel (scale, shift) of every image group, for
    linear_rows(affine=...) - the normalised tensor is never written."""
    lib = _lib.get()
    _check(x0, gamma, beta)
    c0 = x0.shape[-1]
    d = AaGroupNorm()
    d.x0, d.x1, d.gamma, d.beta, d.y = _ptr(x0), None, _ptr(gamma), _ptr(beta), None
    d.c0, d.c1 = c0, 0
    d.n_groups_img, d.tokens_per_group, d.num_groups = n_groups_img, tokens_per_group, num_groups
    d.silu, d.dtype, d.eps = 0, _DT[x0.dtype], eps
    nbytes = lib.aa_groupnorm_workspace(C.byref(d))
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=x0.device)
    coef = torch.empty(n_groups_img, 2, c0, dtype=torch.float32, device=x0.device)
    _run(lib.aa_groupnorm_coef, C.byref(d), _ptr(ws), nbytes, _ptr(coef), _stream(x0))
    return coef


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    lib = _lib.get()
    _check(x, gamma, beta)
    y = torch.empty_like(x)
    _run(lib.aa_layernorm, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), x.shape[0], x.shape[1], eps,
         _DT[x.dtype], _stream(x))
    return y


# ------------------------------------------------------------------------------------- attention
def _operand(t: torch.Tensor, col0: int, outer_stride: int, inner_stride: int, pos_stride: int, outer_div: int = 1):
    o = AaAttnOperand()
    o.ptr, o.ld, o.col0 = _ptr(t), t.stride(0), col0
    o.outer_stride, o.inner_stride, o.pos_stride, o.outer_div = outer_stride, inner_stride, pos_stride, outer_div
    return o


def attention(q: torch.Tensor, q_col0: int, k: torch.Tensor, k_col0: int, v: torch.Tensor, v_col0: int,
              heads: int, n_outer: int, n_inner: int, q_len: int, kv_len: int,
              q_strides, kv_strides, kv_outer_div: int = 1, scale: Optional[float] = None, head_dim: int = 64,
              kv_seq_mod: int = 0, causal: bool = False) -> torch.Tensor:
    """softmax(q k^T * scale) v for every (outer, inner, head).  `*_strides` = (outer, inner, pos)
    row strides of the token matrices; output rows use the q addressing, columns [0, heads*64)."""
    lib = _lib.get()
    for t in (q, k, v):                                   # operands may be column slices of wider matrices (ld = stride(0))
        if not _addressable(t) or t.stride(-1) != 1:
            raise RuntimeError("attention: operands must be GPU tensors with contiguous rows")
    out = torch.empty(q.shape[0], heads * head_dim, dtype=q.dtype, device=q.device)
    d = AaAttention()
    d.q = _operand(q, q_col0, *q_strides)
    d.k = _operand(k, k_col0, *kv_strides, outer_div=kv_outer_div)
    d.v = _operand(v, v_col0, *kv_strides, outer_div=kv_outer_div)
    d.o = _operand(out, 0, *q_strides)
    d.k.seq_mod = d.v.seq_mod = kv_seq_mod       # > 0: sequence number n reads K / V table entry n % kv_seq_mod
    d.causal = int(causal)                       # key position > query position masked (CLIP text encoder)
    d._pad = ATTN_FLAGS
    d.n_outer, d.n_inner, d.heads, d.head_dim = n_outer, n_inner, heads, head_dim
    d.q_len, d.kv_len, d.dtype = q_len, kv_len, _DT[q.dtype]
    d.scale = float(head_dim) ** -0.5 if scale is None else scale
    _run(lib.aa_attention, C.byref(d), _stream(q))
    return out


# ------------------------------------------------------------------------------------- short-sequence self-attention with the projections inside
SEQ_ATTN_DEBUG = 0     # profiling only: AaSeqSelfAttn.flags (timing ablations)


@dataclass
class SeqQKV:
    """Operands of aa_seq_self_attention: `w` [heads, 3, 64, C] (per head the to_k rows, the permuted to_v rows, the to_q rows; a
    LayerNorm's gamma folded in), `bias` fp32 [heads, 3, 64] = W beta of that LayerNorm (None without one), its epsilon."""
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    ln_eps: float


def pack_seq_qkv(wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor, ln=None) -> SeqQKV:
    """to_q / to_k / to_v [heads * 64, C] (no bias: diffusers Attention) -> the operands of aa_seq_self_attention.  The to_v rows of a
    head go in the order 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3) per 32-row half (a lane's 16 output registers are then 16
    consecutive channels).  `ln` = (gamma, beta, eps) folds the LayerNorm in front: LN(x) W^T = x~ W'^T + W beta with x~ the
    normalised rows (the kernel's part), W' = W diag(gamma) rounded to the storage type, the bias in fp32 (cf. pack_weight(ln=...))."""
    n, c = wq.shape
    assert n % 64 == 0 and wk.shape == (n, c) and wv.shape == (n, c)
    i = torch.arange(32, device=wq.device)
    perm = 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3)
    perm64 = torch.cat([perm, perm + 32])
    heads = n // 64

    def order(t):                                                     # [3, n, ...] (q, k, v) -> [heads, 3, 64, ...] (k, permuted v, q)
        q, k, v = (t[j].reshape((heads, 64) + tuple(t.shape[2:])) for j in range(3))
        return torch.stack([k, v[:, perm64], q], dim=1).contiguous()

    w3 = torch.stack([wq.detach(), wk.detach(), wv.detach()])
    bias, eps = None, 0.0
    if ln is not None:
        gamma, beta, eps = ln
        wf = w3.float()
        bias = order(wf @ beta.detach().float())                      # fp32 [heads, 3, 64]
        w3 = (wf * gamma.detach().float()[None, None, :]).to(wq.dtype)
    return SeqQKV(order(w3), bias, float(eps))


@dataclass
class SeqPre:
    """A linear layer run INSIDE aa_seq_self_attention in front of the normalisation (AaSeqSelfAttn.pre_w): `w` [C / 64, 64, C] = its rows
    in 64-row passes, each 32-row half in the order 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3); `bias` fp32 [C] in the same order."""
    w: torch.Tensor
    bias: Optional[torch.Tensor]


def pack_seq_pre(weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> SeqPre:
    """nn.Linear(C, C) (diffusers Transformer*Model.proj_in, Attention.to_out[0]) -> the `pre` operand of seq_self_attention."""
    n, c = weight.shape
    assert n == c and n % 64 == 0
    i = torch.arange(32, device=weight.device)
    perm = 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3)
    rows = (torch.arange(0, n, 32, device=weight.device)[:, None] + perm[None, :]).reshape(-1)
    b = None if bias is None else bias.detach().float()[rows].contiguous()
    return SeqPre(weight.detach()[rows].reshape(n // 64, 64, c).contiguous(), b)


def _seq_self_attn_desc(x, pk, out, n_outer, n_inner, seq_len, strides, scale):
    d = AaSeqSelfAttn()
    d.x, d.w, d.w_bias, d.o = _ptr(x), _ptr(pk.w), _ptr(pk.bias), _ptr(out)
    d.outer_stride, d.inner_stride, d.pos_stride = strides
    last = (n_outer - 1) * strides[0] + (n_inner - 1) * strides[1] + (seq_len - 1) * strides[2]
    d.x_bytes, d.o_bytes = (last + 1) * x.stride(0) * 2, (last + 1) * out.stride(0) * 2
    d.n_outer, d.n_inner, d.seq_len, d.channels = n_outer, n_inner, seq_len, x.shape[1]
    d.ldx, d.ldo = x.stride(0), out.stride(0)
    d.normalize, d.ln_eps, d.scale, d.dtype = int(pk.ln_eps > 0.0), float(pk.ln_eps), float(scale), _DT[x.dtype]
    d.flags = SEQ_ATTN_DEBUG
    return d


def seq_self_attention_ok(channels: int, seq_len: int, rows: int, dtype) -> bool:
    """Does aa_seq_self_attention cover a [rows, channels] token matrix with sequences of `seq_len` positions?"""
    d = AaSeqSelfAttn()
    d.channels, d.seq_len, d.n_outer, d.n_inner, d.ldx, d.ldo = channels, seq_len, 1, 1, channels, channels
    d.x_bytes = d.o_bytes = rows * channels * 2
    d.dtype = _DT.get(dtype, -1)
    return bool(_lib.get().aa_seq_self_attention_ok(C.byref(d)))


def seq_self_attention(x: torch.Tensor, pk: SeqQKV, n_outer: int, n_inner: int, seq_len: int, strides, scale: Optional[float] = None,
                       pre: Optional[SeqPre] = None, residual: Optional[torch.Tensor] = None):
    """softmax(q k^T * scale) v with [q | k | v] = LayerNorm(x) W^T for every (outer, inner) sequence and head (head_dim 64), in one
    kernel; `pk` from pack_seq_qkv (with the LayerNorm folded in, or without one), `strides` = (outer, inner, pos) row strides of x
    (and of the result, [rows, C]).
    `pre` (pack_seq_pre): the same kernel first runs x' = x W_pre^T + b_pre (+ residual), writes it and attends over LayerNorm(x') -
    the projection in front of the block (proj_in) or the previous attention layer's to_out + residual.  Returns (o, x') then."""
    lib = _lib.get()
    _check(x, pk.w, pk.bias, residual)
    if pk.w.dtype != x.dtype or pk.w.shape[-1] != x.shape[1]:
        raise RuntimeError("seq_self_attention: weights were packed for another dtype / width")
    out = torch.empty(x.shape[0], x.shape[1], dtype=x.dtype, device=x.device)
    d = _seq_self_attn_desc(x, pk, out, n_outer, n_inner, seq_len, strides, 64.0 ** -0.5 if scale is None else scale)
    x_pre = None
    if pre is not None:
        _check(pre.w, pre.bias)
        if pre.w.dtype != x.dtype or pre.w.shape[-1] != x.shape[1]:
            raise RuntimeError("seq_self_attention: the projection in front was packed for another dtype / width")
        x_pre = torch.empty_like(out)
        d.pre_w, d.pre_bias, d.pre_residual, d.pre_out = _ptr(pre.w), _ptr(pre.bias), _ptr(residual), _ptr(x_pre)
        d.ld_res, d.ld_pre = 0 if residual is None else residual.stride(0), x_pre.stride(0)
    elif residual is not None:
        raise RuntimeError("seq_self_attention: `residual` belongs to the projection in front (`pre`)")
    _run(lib.aa_seq_self_attention, C.byref(d), _stream(x))
    return out if pre is None else (out, x_pre)


# ------------------------------------------------------------------------------------- FeedForward + proj_out in one kernel
FF_FUSED_DEBUG = 0     # profiling only: AaFFFused.flags (timing ablations)


FF_STAGE_BYTES, FF_STAGES = 41984, 65          # include/aa_mi355.h: AA_FF_STAGE_BYTES, AA_FF_STAGES


@dataclass
class FFFused:
    """Operand of aa_ff_fused (include/aa_mi355.h): `w` = the weight stream, [65, 41984 / 2] of the storage type - the LDS stage images of
    GEGLU.proj (LayerNorm folded in), Wp W2 and Wp in the order the kernel consumes them, biases as (hi, lo) rows; see pack_ff_fused."""
    w: torch.Tensor
    ln_eps: float
    normalize: bool


def _bias_hi_lo(b: Optional[torch.Tensor], n: int, dtype, device) -> torch.Tensor:
    """fp32 bias [n] (None: zeros) -> [n, 8] of the storage type: (hi, lo, 0 x 6) with hi = round(b), lo = round(b - hi) - the A operand of the
    bias k-slice of aa_ff_fused (the matrix pipe adds hi * 1 + lo * 1 in fp32: the bias to 2^-22 (fp16) / 2^-16 (bf16) relative)."""
    out = torch.zeros(n, 8, dtype=dtype, device=device)
    if b is not None:
        hi = b.to(dtype)
        out[:, 0], out[:, 1] = hi, (b - hi.float()).to(dtype)
    return out


def _ff_stage_image(block: torch.Tensor, bias8: Optional[torch.Tensor], k_chunks: bool) -> torch.Tensor:
    """One LDS stage image [41984 / 2]: `block` = [64, 320] (64 weight rows x all K: five K chunks of 64) or [320, 64] (all rows x 64 K: five
    row chunks of 64); every chunk [64 rows][8 slots][8] with slot s of row r holding source slot s ^ ((r >> 1) & 7); then `bias8` [64, 8]
    (zeros if None)."""
    dev = block.device
    chunks = block.reshape(64, 5, 64).permute(1, 0, 2) if k_chunks else block.reshape(5, 64, 64)       # [5][64 rows][64 K]
    r = torch.arange(64, device=dev)[:, None]
    src_slot = torch.arange(8, device=dev)[None, :] ^ ((r >> 1) & 7)                                    # [64, 8]
    sw = torch.gather(chunks.reshape(5, 64, 8, 8), 2, src_slot[None, :, :, None].expand(5, 64, 8, 8))
    b = torch.zeros(64, 8, dtype=block.dtype, device=dev) if bias8 is None else bias8
    return torch.cat([sw.reshape(-1), b.reshape(-1)])


def pack_ff_fused(w1: torch.Tensor, b1: Optional[torch.Tensor], w2: torch.Tensor, b2: Optional[torch.Tensor],
                  wp: Optional[torch.Tensor] = None, bp: Optional[torch.Tensor] = None, ln=None) -> FFFused:
    """diffusers FeedForward = GEGLU.proj (w1 [8 C, C]: value rows, then gate rows; b1) -> value * gelu(gate) -> Linear (w2 [C, 4 C], b2), `+ x`
    behind it, and the transformer wrapper's proj_out (wp [C, C], bp; None: identity) -> the weight stream of ff_fused:
        out = [h | x] [Wp W2 | Wp]^T + (Wp b2 + bp) + outer.
    The product Wp W2 is formed in fp32 and rounded once (layers._MergedTail checks that this is harmless for the weights at hand).
    `ln` = (gamma, beta, eps) folds the LayerNorm in front of GEGLU.proj as pack_weight(ln=...) does."""
    c = w1.shape[1]
    hid = w2.shape[1]
    assert c == 320 and w1.shape == (2 * hid, c) and w2.shape == (c, hid) and hid == 4 * c
    dt, dev = w1.dtype, w1.device
    w1f = w1.detach().float()
    b1f = None if b1 is None else b1.detach().float()
    eps, normalize = 0.0, False
    if ln is not None:
        gamma, beta, eps = ln
        extra = w1f @ beta.detach().float()
        b1f = extra if b1f is None else b1f + extra
        w1f = w1f * gamma.detach().float()[None, :]
        normalize = True
    # W1 chunk ch of 64 rows: value rows of hidden units 32 ch .. + 31, then their gate rows
    idx = torch.arange(hid, device=dev).reshape(hid // 32, 32)
    rows1 = torch.cat([idx, idx + hid], dim=1).reshape(-1)
    w1p = w1f[rows1].to(dt)
    b1p = _bias_hi_lo(None if b1f is None else b1f[rows1], 2 * hid, dt, dev)
    wpf = torch.eye(c, device=dev) if wp is None else wp.detach().float()
    wh = wpf @ w2.detach().float()                                                  # [C, 4 C]
    bm = None
    if b2 is not None or bp is not None:
        bm = (0.0 if bp is None else bp.detach().float()) + (0.0 if b2 is None else wpf @ b2.detach().float())
    i = torch.arange(32, device=dev)
    perm = 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3)
    rows = (torch.arange(0, c, 32, device=dev)[:, None] + perm[None, :]).reshape(-1)
    # hidden axis: position 32 cc + 16 h + 8 t + e of every 64 holds unit 32 cc + (e & 3) + 4 h + 8 (e >> 2) + 16 t (the order in which a lane's
    # accumulator registers of value * gelu(gate) become the B operand of the second product)
    pz = torch.arange(64, device=dev)
    cc, hh, tt, ee = pz >> 5, (pz >> 4) & 1, (pz >> 3) & 1, pz & 7
    unit = 32 * cc + (ee & 3) + 4 * hh + 8 * (ee >> 2) + 16 * tt
    cols = (torch.arange(0, hid, 64, device=dev)[:, None] + unit[None, :]).reshape(-1)
    whp, wxp = wh[rows][:, cols].to(dt), wpf[rows].to(dt)
    bmp = _bias_hi_lo(None if bm is None else bm[rows], c, dt, dev)
    stage_x = lambda n: _ff_stage_image(wxp[64 * n:64 * n + 64], bmp[64 * n:64 * n + 64], True)
    stage_w1 = lambda ch: _ff_stage_image(w1p[64 * ch:64 * ch + 64], b1p[64 * ch:64 * ch + 64], True)
    stage_h = lambda g: _ff_stage_image(whp[:, 64 * g:64 * g + 64], None, False)
    npair = hid // 64
    seq = [stage_x(n) for n in range(c // 64)] + [stage_w1(0), stage_w1(1)]
    for g in range(1, npair):
        seq += [stage_w1(2 * g), stage_h(g - 1), stage_w1(2 * g + 1)]
    seq.append(stage_h(npair - 1))
    w = torch.stack(seq).contiguous()
    assert w.shape == (FF_STAGES, FF_STAGE_BYTES // 2)
    return FFFused(w, float(eps), normalize)


def _ff_fused_desc(x, pk, outer, out):
    d = AaFFFused()
    d.x, d.outer, d.out, d.w = _ptr(x), _ptr(outer), _ptr(out), _ptr(pk.w)
    d.rows, d.channels = x.shape[0], x.shape[1]
    d.ldx, d.ld_outer, d.ldo = x.stride(0), 0 if outer is None else outer.stride(0), out.stride(0)
    d.normalize, d.ln_eps, d.dtype, d.flags = int(pk.normalize), pk.ln_eps, _DT[x.dtype], FF_FUSED_DEBUG
    return d


def ff_fused_ok(channels: int, rows: int, dtype) -> bool:
    d = AaFFFused()
    d.rows, d.channels, d.ldx, d.ld_outer, d.ldo, d.dtype = rows, channels, channels, channels, channels, _DT.get(dtype, -1)
    return bool(_lib.get().aa_ff_fused_ok(C.byref(d)))


def ff_fused(x: torch.Tensor, pk: FFFused, outer: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[GEGLU(LayerNorm(x) W1^T + b1) | x] Wm^T + bm + outer in one kernel (pk from pack_ff_fused): the FeedForward of a transformer block, its
    residual, the wrapper's proj_out and the wrapper's residual; the [rows, 4 C] activation is never written."""
    lib = _lib.get()
    _check(x, outer, pk.w, out)
    if pk.w.dtype != x.dtype or x.shape[1] != 320:
        raise RuntimeError("ff_fused: weights were packed for another dtype / width")
    if out is None:
        out = torch.empty(x.shape[0], x.shape[1], dtype=x.dtype, device=x.device)
    elif out.shape != x.shape or out.dtype != x.dtype or out.stride(1) != 1:
        raise RuntimeError("ff_fused: `out` must have x's shape and dtype")
    d = _ff_fused_desc(x, pk, outer, out)
    _run(lib.aa_ff_fused, C.byref(d), _stream(x))
    return out


# ------------------------------------------------------------------------------------- K = C projections with the rows in registers
LR_STAGE_BYTES = 21504                          # include/aa_mi355.h: AA_LR_STAGE_BYTES
LINEAR_ROWS_DEBUG = int(os.environ.get("AA_LINEAR_ROWS_DEBUG", "0"))      # AaLinearRows.flags (1: plan for a 2-CU chip, 2: no stage split of the last round)


@dataclass
class LinearRows:
    """Operand of aa_linear_rows: `w` = the weight stream [n_out / 32, 21504 / 2] of the storage type (see pack_linear_rows)."""
    w: torch.Tensor
    n_out: int
    ln_eps: float
    normalize: bool


def pack_linear_rows(weight: torch.Tensor, bias: Optional[torch.Tensor] = None, ln=None) -> LinearRows:
    """nn.Linear(320, n_out) [+ the LayerNorm (gamma, beta, eps) in front of it] -> the weight stream of linear_rows: per 32 output channels the
    weight rows in the order 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3) (a lane's accumulator registers are then 16 consecutive channels),
    five [32][64] K chunks with the kernel's XOR swizzle applied, the biases as (hi, lo) rows (_bias_hi_lo)."""
    n, c = weight.shape
    assert c == 320 and n % 32 == 0
    dt, dev = weight.dtype, weight.device
    wf = weight.detach().float()
    bf = None if bias is None else bias.detach().float()
    eps, normalize = 0.0, False
    if ln is not None:
        gamma, beta, eps = ln
        extra = wf @ beta.detach().float()
        bf = extra if bf is None else bf + extra
        wf = wf * gamma.detach().float()[None, :]
        normalize = True
    i = torch.arange(32, device=dev)
    perm = 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3)
    rows = (torch.arange(0, n, 32, device=dev)[:, None] + perm[None, :]).reshape(-1)
    wp = wf[rows].to(dt).reshape(n // 32, 32, 5, 8, 8)                       # [stage][row][K chunk][slot][8]
    r = torch.arange(32, device=dev)[:, None]
    src_slot = torch.arange(8, device=dev)[None, :] ^ ((r >> 1) & 7)           # [32, 8]: slot s of row r holds source slot s ^ ((r >> 1) & 7)
    sw = torch.gather(wp.permute(0, 2, 1, 3, 4), 3, src_slot[None, None, :, :, None].expand(n // 32, 5, 32, 8, 8))     # [stage][chunk][row][slot][8]
    b8 = _bias_hi_lo(None if bf is None else bf[rows], n, dt, dev).reshape(n // 32, 32 * 8)
    pad = torch.zeros(n // 32, 256, dtype=dt, device=dev)
    w = torch.cat([sw.reshape(n // 32, -1), b8, pad], dim=1).contiguous()
    assert w.shape == (n // 32, LR_STAGE_BYTES // 2)
    return LinearRows(w, n, float(eps), normalize)


def linear_rows_ok(channels: int, n_out: int, rows: int, dtype, rows_per_group: int = 0) -> bool:
    """`rows_per_group` > 0: with a GroupNorm's coefficients in front (linear_rows(affine=...))."""
    d = AaLinearRows()
    d.rows, d.channels, d.n_out, d.ldx, d.ld_res, d.ldo, d.dtype = rows, channels, n_out, channels, n_out, n_out, _DT.get(dtype, -1)
    if rows_per_group:
        d.row_affine, d.rows_per_group = 16, rows_per_group          # (any non-null pointer: the check reads the geometry only)
    return bool(_lib.get().aa_linear_rows_ok(C.byref(d)))


def linear_rows(x: torch.Tensor, pk: LinearRows, residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, affine=None) -> torch.Tensor:
    """[LayerNorm](x) W^T + b (+ residual) for 320-channel token rows, rows in registers (pk from pack_linear_rows).
    `affine` = (groupnorm_coef(...), rows per image group): the GroupNorm in front of this layer, applied to the rows in the registers."""
    lib = _lib.get()
    _check(x, residual, pk.w, out)
    if pk.w.dtype != x.dtype or x.shape[1] != 320:
        raise RuntimeError("linear_rows: weights were packed for another dtype / width")
    if out is None:
        out = torch.empty(x.shape[0], pk.n_out, dtype=x.dtype, device=x.device)
    d = AaLinearRows()
    d.x, d.residual, d.out, d.w = _ptr(x), _ptr(residual), _ptr(out), _ptr(pk.w)
    d.rows, d.channels, d.n_out = x.shape[0], x.shape[1], pk.n_out
    d.ldx, d.ld_res, d.ldo = x.stride(0), 0 if residual is None else residual.stride(0), out.stride(0)
    d.normalize, d.ln_eps, d.dtype, d.flags = int(pk.normalize), pk.ln_eps, _DT[x.dtype], LINEAR_ROWS_DEBUG
    if affine is not None:
        coef, per = affine
        if coef.dtype != torch.float32 or not coef.is_contiguous() or coef.shape[-1] != x.shape[1] or coef.shape[0] * per < x.shape[0] or coef.device != x.device:
            raise RuntimeError("linear_rows: `affine` must be groupnorm_coef's fp32 [groups, 2, channels] covering every row")
        d.row_affine, d.rows_per_group = _ptr(coef), per
    _run(lib.aa_linear_rows, C.byref(d), _stream(x))
    return out


# ------------------------------------------------------------------------------------- fp8 (e4m3) linear layers
FP8_MAX = 448.0          # largest finite OCP e4m3 value
FP8_TINY = 1e-12         # include/aa_mi355.h: AA_FP8_TINY


def _fp8_row_perm(n: int, device) -> torch.Tensor:
    """Row order of aa_linear_fp8's weight operand: inside every block of 32 rows, row i holds channel 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3)."""
    i = torch.arange(32, device=device)
    perm = 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3)
    return (torch.arange(0, n, 32, device=device)[:, None] + perm[None, :]).reshape(-1)


@dataclass
class PackedWeightFp8:
    """Operands of aa_linear_fp8: `w` uint8 [n, k] e4m3 bytes in the kernel's row order, `scale` / `bias` fp32 [n] in channel order
    (geglu: value / gate blocks of 32 alternating, like pack_weight(geglu=True))."""
    w: torch.Tensor
    scale: torch.Tensor
    bias: Optional[torch.Tensor]
    n: int
    k: int
    geglu: bool

    @property
    def n_out(self):
        return self.n // 2 if self.geglu else self.n


def pack_weight_fp8(weight: torch.Tensor, bias: Optional[torch.Tensor] = None, geglu: bool = False) -> PackedWeightFp8:
    """nn.Linear [n, k] -> e4m3 bytes with one fp32 scale per output channel: scale = max(absmax(row), FP8_TINY) / 448,
    byte = float8_e4m3fn(weight / scale) (round to nearest even; |weight / scale| <= 448 by construction)."""
    n, k = weight.shape
    if k % 128 or n % 64 or (geglu and (n // 2) % 32):
        raise RuntimeError(f"pack_weight_fp8: n={n} k={k} (k a multiple of 128, n of 64)")
    dev = weight.device
    wf = weight.detach().float()
    b = None if bias is None else bias.detach().float()
    if geglu:
        d = n // 2
        val = torch.arange(d, device=dev).reshape(d // 32, 1, 32)
        src = torch.cat([val, val + d], dim=1).reshape(-1)
        wf = wf[src]
        b = None if b is None else b[src]
    scale = wf.abs().amax(dim=1).clamp_min(FP8_TINY) / FP8_MAX
    q = (wf / scale[:, None]).clamp(-FP8_MAX, FP8_MAX).cpu().to(torch.float8_e4m3fn).view(torch.uint8).to(dev)
    return PackedWeightFp8(q[_fp8_row_perm(n, dev)].contiguous(), scale.contiguous(), None if b is None else b.contiguous(), n, k, bool(geglu))


def quant_rows_fp8(x: torch.Tensor, ln=None, out=None):
    """Per-row dynamic quantisation of a token matrix [M, K] to e4m3: (q uint8 [M, K], scale fp32 [M]) with scale = max(absmax(row), FP8_TINY) / 448.
    `ln` = (gamma, beta, eps): the rows of LayerNorm(x) are quantised instead (one pass, statistics in fp32).  `out` = (q, scale) buffers to fill."""
    lib = _lib.get()
    gamma, beta, eps = ln if ln is not None else (None, None, 0.0)
    q, scale = out if out is not None else (torch.empty(x.shape, dtype=torch.uint8, device=x.device),
                                            torch.empty(x.shape[0], dtype=torch.float32, device=x.device))
    _check(x, gamma, beta, q, scale)
    if q.dtype != torch.uint8 or scale.dtype != torch.float32 or tuple(q.shape) != tuple(x.shape) or scale.numel() != x.shape[0]:
        raise RuntimeError("quant_rows_fp8: `out` must be (uint8 [M, K], fp32 [M])")
    if ln is not None and (gamma.dtype != x.dtype or (beta is not None and beta.dtype != x.dtype) or gamma.numel() != x.shape[1]):
        raise RuntimeError("quant_rows_fp8: LayerNorm parameters must match x")
    d = AaQuantRowsFp8()
    d.x, d.gamma, d.beta, d.q, d.scale = _ptr(x), _ptr(gamma), _ptr(beta), _ptr(q), _ptr(scale)
    d.rows, d.channels, d.ldx, d.ldq, d.ln_eps, d.dtype = x.shape[0], x.shape[1], x.stride(0), q.stride(0), float(eps), _DT[x.dtype]
    _run(lib.aa_quant_rows_fp8, C.byref(d), _stream(x))
    return q, scale


def linear_fp8(q: torch.Tensor, scale: torch.Tensor, packed: PackedWeightFp8, residual: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, dtype=None) -> torch.Tensor:
    """(q scale) W^T + b (+ residual) on the block-scaled e4m3 matrix form (q, scale from quant_rows_fp8, `packed` from pack_weight_fp8);
    a geglu pack gives value * gelu(gate), [M, n / 2].  The output type is the residual's / `out`'s, or `dtype`."""
    lib = _lib.get()
    _check(q, scale, packed.w, packed.scale, packed.bias, residual, out)
    if q.dtype != torch.uint8 or q.dim() != 2 or q.shape[1] != packed.k or scale.dtype != torch.float32 or scale.numel() != q.shape[0]:
        raise RuntimeError("linear_fp8: (q, scale) must be quant_rows_fp8's uint8 [M, K] / fp32 [M] with the K of the packed weights")
    if out is None:
        dt = residual.dtype if residual is not None else dtype
        if dt is None:
            raise RuntimeError("linear_fp8: give `out`, `residual` or `dtype`")
        out = torch.empty(q.shape[0], packed.n_out, dtype=dt, device=q.device)
    if residual is not None and (residual.dtype != out.dtype or residual.shape != out.shape):
        raise RuntimeError("linear_fp8: the residual must have the output's type and shape")
    d = AaLinearFp8()
    d.a, d.a_scale, d.w, d.w_scale, d.bias = _ptr(q), _ptr(scale), _ptr(packed.w), _ptr(packed.scale), _ptr(packed.bias)
    d.residual, d.out, d.rows, d.n, d.k = _ptr(residual), _ptr(out), q.shape[0], packed.n, packed.k
    d.ld_res, d.ldo, d.geglu, d.dtype = 0 if residual is None else residual.stride(0), out.stride(0), int(packed.geglu), _DT[out.dtype]
    _run(lib.aa_linear_fp8, C.byref(d), _stream(q))
    return out


def softmax_rows(x: torch.Tensor, dtype, cols: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row softmax of fp32 scores over the first `cols` columns; `out` may be wider (its padding is
    left untouched)."""
    lib = _lib.get()
    _check(x, out)
    assert x.dtype == torch.float32
    cols = x.shape[1] if cols is None else cols
    y = torch.empty(x.shape, dtype=dtype, device=x.device) if out is None else out
    _run(lib.aa_softmax_rows, _ptr(x), _ptr(y), x.shape[0], cols, x.stride(0), y.stride(0), _DT[y.dtype], _stream(x))
    return y


def cfg_dpm_step(eps_uncond, eps_text, latents, x0_prev, latents_lp, guidance, sigma_s, alpha_s, c_x, c_d0, c_d1):
    lib = _lib.get()
    _check(eps_uncond, eps_text, latents, x0_prev, latents_lp)
    d = AaDpmStep()
    d.eps_uncond, d.eps_text = _ptr(eps_uncond), _ptr(eps_text)
    d.latents, d.x0_prev, d.latents_lp = _ptr(latents), _ptr(x0_prev), _ptr(latents_lp)
    d.n = latents.numel()
    d.guidance, d.sigma_s, d.alpha_s, d.c_x, d.c_d0, d.c_d1 = guidance, sigma_s, alpha_s, c_x, c_d0, c_d1
    d.dtype = _DT[eps_uncond.dtype]
    _run(lib.aa_cfg_dpm_step, C.byref(d), _stream(latents))


# ------------------------------------------------------------------------------------- step glue
def timestep_embedding(t: torch.Tensor, dim: int, dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """diffusers Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0) of the fp32 DEVICE array `t` [n] -> [n, dim]."""
    lib = _lib.get()
    _check(t, out)
    assert t.dtype == torch.float32 and t.dim() == 1
    y = torch.empty(t.shape[0], dim, dtype=dtype, device=t.device) if out is None else out
    _run(lib.aa_timestep_embedding, _ptr(t), _ptr(y), t.shape[0], dim, _DT[y.dtype], _stream(t))
    return y


def pack_latents(sample: torch.Tensor, cond: torch.Tensor, mask: Optional[torch.Tensor], batch: int, dtype,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sample [Bs,C,T,h,w] (fp32 or `dtype`), cond [Bc,C,1,h,w], mask [Bm,1,1,h,w] or None -> tokens [batch*(T+1)*h*w, 8]."""
    lib = _lib.get()
    _check(sample, cond, mask, out)
    bs, c, frames, h, w = sample.shape
    y = torch.empty(batch * (frames + 1) * h * w, 8, dtype=dtype, device=sample.device) if out is None else out
    d = AaPackLatents()
    d.sample, d.cond, d.mask, d.out = _ptr(sample), _ptr(cond), _ptr(mask), _ptr(y)
    d.batch, d.sample_batch, d.cond_batch = batch, bs, cond.shape[0]
    d.mask_batch = 0 if mask is None else mask.shape[0]
    d.channels, d.frames, d.hw = c, frames, h * w
    d.dtype, d.sample_dtype = _DT[dtype], _DT[sample.dtype]
    assert cond.dtype == dtype and (mask is None or mask.dtype == dtype)
    _run(lib.aa_pack_latents, C.byref(d), _stream(sample))
    return y


def _step_tok_common(name, d, tokens, latents, latents_lp, guidance, next_t, next_t_value, state=()):
    """What the three UNet3D token steps share: the operand checks and the descriptor fields for the token matrix, the fp32
    latents, their 16-bit copy, the next-timestep deposit, the geometry and the guidance.  `state`: (what, tensor or None) pairs of
    the sampler's further fp32 operands in the latents' shape.  Returns (library, stream)."""
    lib = _lib.get()
    _check(tokens, latents, latents_lp, next_t, *(t for _, t in state))
    if latents.dtype != torch.float32 or latents.dim() != 5:
        raise RuntimeError(f"{name}: latents must be fp32 [clips, C, T, h, w]")
    for what, t in state:
        if t is not None and (t.shape != latents.shape or t.dtype != torch.float32):
            raise RuntimeError(f"{name}: {what} must be fp32 in the latents' shape")
    if latents_lp is not None and (latents_lp.shape != latents.shape or latents_lp.dtype != tokens.dtype):
        raise RuntimeError(f"{name}: latents_lp must have the latents' shape and the tokens' dtype")
    if next_t is not None and next_t.dtype != torch.float32:
        raise RuntimeError(f"{name}: next_t must be fp32")
    clips, c, frames, h, w = latents.shape
    rows = (2 if guidance is not None else 1) * clips * (frames + 1) * h * w
    if tokens.dim() != 2 or tokens.shape[0] < rows or tokens.shape[1] < c:
        raise RuntimeError(f"{name}: tokens {tuple(tokens.shape)} do not hold {rows} rows of {c} channels")
    if isinstance(d, AaDpmStepTok):
        d.eps_tokens, d.eps_ld = _ptr(tokens), tokens.stride(0)
    else:
        d.tokens, d.ld = _ptr(tokens), tokens.stride(0)
    d.latents, d.latents_lp = _ptr(latents), _ptr(latents_lp)
    d.next_t, d.next_t_count, d.next_t_value = _ptr(next_t), 0 if next_t is None else next_t.numel(), float(next_t_value)
    d.clips, d.channels, d.frames, d.hw = clips, c, frames, h * w
    d.guidance_on, d.guidance = int(guidance is not None), float(guidance or 0.0)
    d.dtype = _DT[tokens.dtype]
    return lib, _stream(latents)


def cfg_dpm_step_tokens(eps_tokens, latents, x0_prev, latents_lp, guidance, coeffs, next_t=None, next_t_value=0.0):
    """Fused CFG + DPM-Solver++ update reading the UNet's token-layout output [(2*)clips*(T+1)*hw, eps_ld]."""
    d = AaDpmStepTok()
    lib, stream = _step_tok_common("cfg_dpm_step_tokens", d, eps_tokens, latents, latents_lp, guidance, next_t, next_t_value,
                                   (("x0_prev", x0_prev),))
    d.x0_prev = _ptr(x0_prev)
    d.sigma_s, d.alpha_s, d.c_x, d.c_d0, d.c_d1 = (coeffs[k] for k in ("sigma_s", "alpha_s", "c_x", "c_d0", "c_d1"))
    _run(lib.aa_cfg_dpm_step_tokens, C.byref(d), stream)


# ------------------------------------------------------------------------------------- Stable-Video-Diffusion glue
def blend(x: torch.Tensor, y: Optional[torch.Tensor] = None, a: float = 1.0, b: float = 1.0,
          rowvec: Optional[torch.Tensor] = None, rowvec_div: int = 1, rowvec_mod: int = 0, act: int = AA_ACT_NONE,
          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(a*x + b*y + rowvec[(row // rowvec_div) % rowvec_mod]) on [rows, C] token matrices (diffusers AlphaBlender etc.)."""
    lib = _lib.get()
    _check(x, y, out)
    if rowvec is not None and (not _addressable(rowvec) or rowvec.stride(-1) != 1):
        raise RuntimeError("blend: rowvec must be a GPU tensor with contiguous rows")
    o = torch.empty_like(x) if out is None else out
    d = AaBlend()
    d.x, d.y, d.rowvec, d.out = _ptr(x), _ptr(y), _ptr(rowvec), _ptr(o)
    d.rows, d.channels = x.shape[0], x.shape[1]
    d.rowvec_div, d.rowvec_mod = rowvec_div, rowvec_mod
    d.rowvec_ld = 0 if rowvec is None or rowvec.dim() < 2 else rowvec.stride(0)
    d.a, d.b, d.act, d.dtype = float(a), float(b), act, _DT[x.dtype]
    _run(lib.aa_blend, C.byref(d), _stream(x))
    return o


def pack_frames(sources, batch: int, dtype, scale: Optional[torch.Tensor] = None, scaled_src: int = -1,
                out_channels: int = 16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cat(sources, dim=2) of [Bs, F, Cs, h, w] tensors (fp32 or `dtype`) -> tokens [batch*F*h*w, out_channels];
    source `scaled_src` is multiplied by the DEVICE scalar `scale` (EulerDiscreteScheduler.scale_model_input)."""
    lib = _lib.get()
    srcs = [s_ for s_ in sources if s_ is not None]
    _check(*srcs, scale, out)
    assert 1 <= len(srcs) <= 3
    _, frames, _, h, w = srcs[0].shape
    y = torch.empty(batch * frames * h * w, out_channels, dtype=dtype, device=srcs[0].device) if out is None else out
    d = AaPackFrames()
    k = 0
    for i, s_ in enumerate(sources):
        if s_ is None:
            continue
        assert s_.shape[1] == frames and s_.shape[3:] == (h, w) and s_.dtype in (torch.float32, dtype)
        d.src[k], d.src_channels[k], d.src_batch[k], d.src_f32[k] = _ptr(s_), s_.shape[2], s_.shape[0], int(s_.dtype == torch.float32)
        if i == scaled_src:
            d.scaled_src = k
        k += 1
    if scaled_src < 0 or scale is None:
        d.scaled_src = -1
    d.scale, d.out = _ptr(scale), _ptr(y)
    d.batch, d.frames, d.hw, d.out_channels, d.dtype = batch, frames, h * w, out_channels, _DT[dtype]
    _run(lib.aa_pack_frames, C.byref(d), _stream(srcs[0]))
    return y


def cfg_euler_step_tokens(v_tokens, latents, guidance, c_x, c_v, next_t=None, next_t_value=0.0, next_scale=None,
                          next_scale_value=1.0):
    """Per-frame guidance + Euler (v-prediction) update x' = c_x x + c_v v, reading the UNet's token-layout output;
    latents fp32 [clips, F, C, h, w] updated in place; `guidance` DEVICE fp32 [F] or None."""
    lib = _lib.get()
    _check(v_tokens, latents, guidance, next_t, next_scale)
    clips, frames, c, h, w = latents.shape
    assert latents.dtype == torch.float32 and (guidance is None or (guidance.dtype == torch.float32 and guidance.numel() == frames))
    d = AaEulerStepTok()
    d.v_tokens, d.latents, d.guidance = _ptr(v_tokens), _ptr(latents), _ptr(guidance)
    d.next_t, d.next_t_count, d.next_t_value = _ptr(next_t), 0 if next_t is None else next_t.numel(), float(next_t_value)
    d.next_scale, d.next_scale_value = _ptr(next_scale), float(next_scale_value)
    d.clips, d.channels, d.frames, d.hw, d.ld = clips, c, frames, h * w, v_tokens.stride(0)
    d.c_x, d.c_v, d.dtype = float(c_x), float(c_v), _DT[v_tokens.dtype]
    _run(lib.aa_cfg_euler_step_tokens, C.byref(d), _stream(latents))


def cfg_ddim_step_tokens(tokens, latents, latents_lp, guidance, coeffs, noise=None, next_t=None, next_t_value=0.0):
    """Fused CFG + DDIM update reading the UNet's token-layout output [(2*)clips*(T+1)*hw, ld]; latents fp32 [clips, C, T, h, w]
    updated in place.  `coeffs` is schedulers.DDIMScheduler.coefficients(); `noise` (fp32, the latents' shape) is needed when
    coeffs["c_n"] != 0 (eta > 0)."""
    d = AaDdimStepTok()
    lib, stream = _step_tok_common("cfg_ddim_step_tokens", d, tokens, latents, latents_lp, guidance, next_t, next_t_value,
                                   (("noise", noise),))
    d.noise = _ptr(noise)
    d.a_x, d.a_m, d.e_x, d.e_m, d.q_x, d.q_0 = (coeffs[k] for k in ("a_x", "a_m", "e_x", "e_m", "q_x", "q_0"))
    d.c_0, d.c_e, d.c_n = (coeffs[k] for k in ("c_0", "c_e", "c_n"))
    d.clip_on, d.clip, d.eps_from_x0 = int(coeffs["clip"] is not None), float(coeffs["clip"] or 0.0), int(coeffs["eps_from_x0"])
    _run(lib.aa_cfg_ddim_step_tokens, C.byref(d), stream)


def cfg_unipc_step_tokens(tokens, latents, latents_lp, guidance, coeffs, last_sample, history, next_t=None, next_t_value=0.0):
    """Fused CFG + UniPC step (corrector of the step before + predictor) reading the UNet's token-layout output
    [(2*)clips*(T+1)*hw, ld]; latents fp32 [clips, C, T, h, w] updated in place.  `coeffs` is
    schedulers.UniPCMultistepScheduler.coefficients(); `last_sample` (fp32, the latents' shape) receives the corrected sample;
    `history` = (m of the previous step, of the second previous, of the third previous), fp32 in the latents' shape, an entry
    may be None where its coefficients are zero.  The kernel writes this step's m into the last entry that is not None;
    returns the history rotated for the next step."""
    history = tuple(history)
    if len(history) != 3:
        raise RuntimeError("cfg_unipc_step_tokens: history must hold three entries (tensors or None)")
    if last_sample is None:
        raise RuntimeError("cfg_unipc_step_tokens: last_sample must be fp32 in the latents' shape")
    d = AaUnipcStepTok()
    lib, stream = _step_tok_common("cfg_unipc_step_tokens", d, tokens, latents, latents_lp, guidance, next_t, next_t_value,
                                   (("last_sample", last_sample),) + tuple(("history buffers", hbuf) for hbuf in history))
    d.last_sample = _ptr(last_sample)
    d.hist1, d.hist2, d.hist3 = (_ptr(hbuf) for hbuf in history)
    d.a_x, d.a_m, d.corr_on = coeffs["a_x"], coeffs["a_m"], int(bool(coeffs["corr_on"]))
    d.q_l, d.q_1, d.q_2, d.q_3, d.q_n = (coeffs[k] for k in ("q_l", "q_1", "q_2", "q_3", "q_n"))
    d.p_x, d.p_0, d.p_1, d.p_2 = (coeffs[k] for k in ("p_x", "p_0", "p_1", "p_2"))
    _run(lib.aa_cfg_unipc_step_tokens, C.byref(d), stream)
    live = [hbuf for hbuf in history if hbuf is not None]
    return tuple(live[-1:] + live[:-1]) + (None,) * (3 - len(live))


# ------------------------------------------------------------------------------------- FreeU
_FREEU_TRIG = {}


def freeu_trig_table(h: int, w: int, device) -> torch.Tensor:
    """fp32 [h*w, 4] = (cos ty, sin ty, cos tx, sin tx) per pixel (row-major), ty = 2 pi row / h, tx = 2 pi col / w, evaluated in
    float64 on the host; zeros along a 1-pixel axis (aa_mi355.h AaFreeU).  Cached per (h, w, device)."""
    key = (int(h), int(w), str(torch.device(device)))
    t = _FREEU_TRIG.get(key)
    if t is None:
        ty = 2.0 * math.pi * torch.arange(h, dtype=torch.float64) / h
        tx = 2.0 * math.pi * torch.arange(w, dtype=torch.float64) / w
        one = lambda f, a, n: f(a) if n > 1 else torch.zeros(n, dtype=torch.float64)
        rows = torch.stack([one(torch.cos, ty, h), one(torch.sin, ty, h)], dim=1)[:, None, :].expand(h, w, 2)
        cols = torch.stack([one(torch.cos, tx, w), one(torch.sin, tx, w)], dim=1)[None, :, :].expand(h, w, 2)
        t = _FREEU_TRIG[key] = torch.cat([rows, cols], dim=2).reshape(h * w, 4).to(torch.float32).contiguous().to(device)
    return t


def freeu(hidden: torch.Tensor, skip: torch.Tensor, images: int, h: int, w: int, b: float, s: float,
          hidden_out: Optional[torch.Tensor] = None, skip_out: Optional[torch.Tensor] = None):
    """FreeU on the operands of an up-block resnet, token layout [images*h*w, C] (rows may be pitched: stride(0) >= C, stride(1) == 1):
    hidden[:, :C_hidden // 2] * b and the Fourier filter of diffusers (threshold 1, scale s) on every (image, channel) plane of
    `skip`, one launch (aa_freeu_tokens).  An output may be its input (in place) or None (a new dense tensor).
    Returns (hidden_out, skip_out)."""
    lib = _lib.get()
    rows = int(images) * int(h) * int(w)
    for name, t in (("hidden", hidden), ("skip", skip), ("hidden_out", hidden_out), ("skip_out", skip_out)):
        if t is None:
            continue
        _check_token_matrix("freeu", name, t, hidden, "all")
        if h >= 1 and w >= 1 and images >= 1 and t.shape[0] != rows:
            raise RuntimeError(f"freeu: {name} has {t.shape[0]} rows, images * h * w = {rows}")
    ho = torch.empty(hidden.shape, dtype=hidden.dtype, device=hidden.device) if hidden_out is None else hidden_out
    so = torch.empty(skip.shape, dtype=skip.dtype, device=skip.device) if skip_out is None else skip_out
    if ho.shape != hidden.shape or so.shape != skip.shape:
        raise RuntimeError("freeu: an output must have its input's shape")
    d = AaFreeU()
    d.hidden, d.hidden_out, d.skip, d.skip_out = _ptr(hidden), _ptr(ho), _ptr(skip), _ptr(so)
    d.trig = _ptr(freeu_trig_table(max(int(h), 1), max(int(w), 1), hidden.device))      # (h or w < 1: the entry point refuses)
    d.images, d.h, d.w, d.c_hidden, d.c_skip = int(images), int(h), int(w), hidden.shape[1], skip.shape[1]
    d.hidden_ld, d.hidden_out_ld, d.skip_ld, d.skip_out_ld = hidden.stride(0), ho.stride(0), skip.stride(0), so.stride(0)
    d.b, d.s, d.dtype = float(b), float(s), _DT[hidden.dtype]
    _run(lib.aa_freeu_tokens, C.byref(d), _stream(hidden))
    return ho, so


# ------------------------------------------------------------------------------------- guidance rescale
_CFG_RESCALE_WS = {}


def cfg_rescale_tokens(tokens: torch.Tensor, clips: int, channels: int, frames: int, hw: int, guidance: float, rescale: float,
                       out: Optional[torch.Tensor] = None, factor: Optional[torch.Tensor] = None) -> torch.Tensor:
    """guidance_rescale (diffusers `rescale_noise_cfg`, per clip) on the UNet's token-layout output `tokens`
    [2*clips*(frames+1)*hw, >= channels] (unconditional clips first; rows may be pitched: stride(0) >= channels, stride(1) == 1):
    k_b * (u + guidance * (t - u)) with k_b = 1 + rescale * (std(t) / std(u + guidance * (t - u)) - 1) over frames 1..frames and columns
    [0, channels) of clip b, written to `out` [clips*(frames+1)*hw, >= channels] - None: in place, over the unconditional half of
    `tokens` - for the step kernel to read with guidance off (aa_cfg_rescale_tokens: two launches).  `factor`: fp32 [clips], receives
    k_b.  A constant guided clip keeps k_b = 1 (diffusers: NaN).  The fp64 workspace is kept per (device, geometry).  Returns `out`."""
    lib = _lib.get()
    clips, channels, frames, hw = int(clips), int(channels), int(frames), int(hw)
    rows = clips * (frames + 1) * hw
    if out is None:
        out = tokens[:max(rows, 0)] if tokens.dim() == 2 else tokens
    for name, t, need in (("tokens", tokens, 2 * rows), ("out", out, rows)):        # (a bad geometry is the entry point's to refuse)
        _check_token_matrix("cfg_rescale_tokens", name, t, tokens, "both", ("tokens", tokens), need if min(clips, channels, frames, hw) >= 1 else None, channels)
    if factor is not None:
        _check(factor)
        if factor.dtype != torch.float32 or factor.numel() != max(clips, 0) or factor.device != tokens.device:
            raise RuntimeError("cfg_rescale_tokens: factor must be fp32 [clips] on the tokens' device")
    d = AaCfgRescale()
    d.tokens, d.out, d.factor = _ptr(tokens), _ptr(out), _ptr(factor)
    d.clips, d.channels, d.frames, d.hw = clips, channels, frames, hw
    d.ld, d.out_ld = tokens.stride(0), out.stride(0)
    d.guidance, d.rescale, d.dtype = float(guidance), float(rescale), _DT[tokens.dtype]
    nbytes = lib.aa_cfg_rescale_workspace(C.byref(d))
    key = (str(tokens.device), clips, channels, frames, hw)
    ws = _CFG_RESCALE_WS.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = _CFG_RESCALE_WS[key] = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=tokens.device)
    _run(lib.aa_cfg_rescale_tokens, C.byref(d), _ptr(ws), ws.numel() * 8, _stream(tokens))
    return out


# ------------------------------------------------------------------------------------- adaptive projected guidance
_APG_WS = {}


def apg_tokens(tokens: torch.Tensor, clips: int, channels: int, frames: int, hw: int, guidance: float, eta: float, norm_threshold: float,
               momentum: float, momentum_buf: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
               stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adaptive Projected Guidance (Sadat et al. 2024, per clip) on the UNet's token-layout output `tokens`
    [2*clips*(frames+1)*hw, >= channels] (unconditional clips first; rows may be pitched: stride(0) >= channels, stride(1) == 1): with
    d = t - u (momentum != 0: d = r = d + momentum * r_prev, `momentum_buf` - fp32, clips*frames*hw*channels elements, dense - holding
    r_prev and receiving r), s = min(1, norm_threshold / |d|) (norm_threshold 0: 1) and p = s <d, t> / <t, t> over frames 1..frames and
    columns [0, channels) of clip b, (1 + (guidance - 1)(eta - 1) p) t + (guidance - 1) s d is written to `out`
    [clips*(frames+1)*hw, >= channels] - None: in place, over the unconditional half of `tokens` - for the step kernel to read with
    guidance off (aa_apg_tokens: two launches).  `stats`: fp32 [clips, 2], receives (s_b, p_b).  The fp64 workspace is kept per
    (device, geometry).  Returns `out`."""
    lib = _lib.get()
    clips, channels, frames, hw = int(clips), int(channels), int(frames), int(hw)
    rows = clips * (frames + 1) * hw
    if out is None:
        out = tokens[:max(rows, 0)] if tokens.dim() == 2 else tokens
    for name, t, need in (("tokens", tokens, 2 * rows), ("out", out, rows)):        # (a bad geometry is the entry point's to refuse)
        _check_token_matrix("apg_tokens", name, t, tokens, "both", ("tokens", tokens), need if min(clips, channels, frames, hw) >= 1 else None, channels)
    for name, t, count in (("momentum_buf", momentum_buf, clips * frames * hw * channels), ("stats", stats, 2 * clips)):
        if t is None:
            continue
        _check(t)
        if t.dtype != torch.float32 or t.numel() != max(count, 0) or t.device != tokens.device or not t.is_contiguous():
            raise RuntimeError(f"apg_tokens: {name} must be fp32, contiguous, {max(count, 0)} elements, on the tokens' device")
    d = AaApg()
    d.tokens, d.out, d.momentum_buf, d.stats = _ptr(tokens), _ptr(out), _ptr(momentum_buf), _ptr(stats)
    d.clips, d.channels, d.frames, d.hw = clips, channels, frames, hw
    d.ld, d.out_ld = tokens.stride(0), out.stride(0)
    d.guidance, d.eta, d.norm_threshold, d.momentum, d.dtype = float(guidance), float(eta), float(norm_threshold), float(momentum), _DT[tokens.dtype]
    nbytes = lib.aa_apg_workspace(C.byref(d))
    key = (str(tokens.device), clips, channels, frames, hw)
    ws = _APG_WS.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = _APG_WS[key] = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=tokens.device)
    _run(lib.aa_apg_tokens, C.byref(d), _ptr(ws), ws.numel() * 8, _stream(tokens))
    return out


# ------------------------------------------------------------------------------------- context windows
def window_desc(window) -> AaWindow:
    """One window of schedulers.context_windows - (frame_indices, normalised_weights, first_flags, last_flags) - as the by-value
    block both window descriptors carry.  An AaWindow passes through.  The slot count is left to the entry points to judge (one past
    AA_WINDOW_MAX is recorded as such and refused there)."""
    if isinstance(window, AaWindow):
        return window
    frames, weights, first, last = window
    n = len(frames)
    if not (len(weights) == len(first) == len(last) == n):
        raise RuntimeError("window_desc: frame indices, weights and flags differ in length")
    w = AaWindow()
    w.window_frames = n
    for j in range(min(n, _lib.AA_WINDOW_MAX)):
        w.frame[j], w.weight[j], w.first[j], w.last[j] = int(frames[j]), float(weights[j]), int(bool(first[j])), int(bool(last[j]))
    return w


def window_gather_latents(src: torch.Tensor, window, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b, c, j] = src[b, c, frame[j]] on fp32 latents [clips, C, frames, h, w] (aa_window_gather_latents, bit-exact): the window's
    frames into `out` [clips, C, window_frames, h, w] - the UNet session's `sample` input; None: a new tensor.  Returns `out`."""
    lib = _lib.get()
    w = window_desc(window)
    if src.dim() != 5 or src.dtype != torch.float32:
        raise RuntimeError("window_gather_latents: src must be fp32 [clips, C, frames, h, w]")
    clips, c, frames, h, wd = src.shape
    if out is None:
        out = torch.empty((clips, c, max(w.window_frames, 0), h, wd), dtype=torch.float32, device=src.device)
    _check(src, out)
    if out.dtype != torch.float32 or tuple(out.shape) != (clips, c, w.window_frames, h, wd) or out.device != src.device:
        raise RuntimeError(f"window_gather_latents: out must be fp32 {(clips, c, w.window_frames, h, wd)} on the source's device")
    d = AaWindowGather()
    d.src, d.dst = _ptr(src), _ptr(out)
    d.clips, d.channels, d.total_frames, d.hw = clips, c, frames, h * wd
    d.window = w
    _run(lib.aa_window_gather_latents, C.byref(d), _stream(src))
    return out


def window_merge_tokens(tokens: torch.Tensor, acc: torch.Tensor, merged: torch.Tensor, window, guidance) -> torch.Tensor:
    """One window's share of a context-window step (aa_window_merge_tokens; one call per window, in schedule order): the guided
    prediction of the window - `tokens` [(2*)clips*(window_frames+1)*hw, >= C], the UNet's token-layout output read as the step
    kernels read it, `guidance` None = off - times the slot's weight into `acc` (fp32 [clips, frames, hw, C]: written by a frame's
    first window, added to after), and by a frame's last window rounded into `merged` [(2*)clips*(frames+1)*hw, >= C] (the tokens'
    dtype; both halves under guidance), which the step kernel then reads with the SAME guidance: a frame held by one window is copied
    bit for bit, u and t alike, without touching `acc`; a blended frame's value goes to both halves, where guidance leaves it as it is.
    Rows may be pitched (stride(0) >= C, stride(1) == 1).  Returns `merged`."""
    lib = _lib.get()
    w = window_desc(window)
    if acc.dim() != 4 or acc.dtype != torch.float32:
        raise RuntimeError("window_merge_tokens: acc must be fp32 [clips, frames, hw, C]")
    _check(acc)
    clips, frames, hw, c = acc.shape
    halves = 2 if guidance is not None else 1
    for name, t, need in (("tokens", tokens, halves * clips * (w.window_frames + 1) * hw), ("merged", merged, halves * clips * (frames + 1) * hw)):
        _check_token_matrix("window_merge_tokens", name, t, tokens, "both", ("acc", acc), need, c)
    d = AaWindowMerge()
    d.tokens, d.acc, d.merged = _ptr(tokens), _ptr(acc), _ptr(merged)
    d.clips, d.channels, d.total_frames, d.hw = clips, c, frames, hw
    d.ld, d.out_ld = tokens.stride(0), merged.stride(0)
    d.guidance_on, d.guidance, d.dtype = int(guidance is not None), float(guidance or 0.0), _DT[tokens.dtype]
    d.window = w
    _run(lib.aa_window_merge_tokens, C.byref(d), _stream(acc))
    return merged


# ------------------------------------------------------------------------------------- FreeInit
_FREE_INIT_TABLES = {}
_FREE_INIT_WS = {}


class FreeInitTables:
    """What aa_freeinit_mix reads besides the latents: `mask` fp32 [T, h, w] (unshifted, symmetrised) and `twiddle` fp32 [T + h + w, 2]."""

    def __init__(self, mask, twiddle):
        self.mask, self.twiddle = mask, twiddle
        self.shape = tuple(mask.shape)


def free_init_tables(T: int, h: int, w: int, mask: torch.Tensor, device) -> FreeInitTables:
    """The tables of aa_freeinit_mix for a volume of T x h x w from the float64 low-pass `mask` in SHIFTED order
    (schedulers.free_init_filter): the mask unshifted and symmetrised (schedulers.free_init_symmetric_mask) and the pairs
    (cos 2 pi j / n, sin 2 pi j / n) for n = T, h, w in one array, both evaluated in float64 on the host and rounded once to fp32.
    Cached per (T, h, w, device) and mask values."""
    from .schedulers import free_init_symmetric_mask
    T, h, w = int(T), int(h), int(w)
    if tuple(mask.shape) != (T, h, w):
        raise RuntimeError(f"free_init_tables: mask {tuple(mask.shape)} is not [T, h, w] = {(T, h, w)}")
    mask = mask.detach().to(device="cpu", dtype=torch.float64)
    key = (T, h, w, str(torch.device(device)))
    kept = _FREE_INIT_TABLES.setdefault(key, [])
    for m, tables in kept:
        if torch.equal(m, mask):
            return tables
    tw = []
    for n in (T, h, w):
        ang = 2.0 * math.pi * torch.arange(n, dtype=torch.float64) / n
        tw.append(torch.stack([torch.cos(ang), torch.sin(ang)], dim=1))
    tables = FreeInitTables(free_init_symmetric_mask(mask).to(torch.float32).contiguous().to(device),
                            torch.cat(tw).to(torch.float32).contiguous().to(device))
    del kept[:-3]                                                 # (a handful of filters per shape at most)
    kept.append((mask.clone(), tables))
    return tables


def freeinit_mix(x: torch.Tensor, n0: torch.Tensor, z: torch.Tensor, a: float, s: float, tables: FreeInitTables,
                 out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FreeInit's re-initialisation out = z + LP(a * x + s * n0 - z) on fp32 latents [..., T, h, w] (aa_freeinit_mix: five launches,
    direct DFTs per axis, LP the 3-d low-pass of `tables`): x the previous iteration's result, n0 the run's initial noise, z fresh
    noise, a / s = sqrt(abar) / sqrt(1 - abar) at the last training timestep.  `out`: None (a new tensor) or a tensor of x's shape - x
    itself is allowed, nothing else may overlap.  `workspace`: None (kept per device and geometry) or an fp32 tensor of at least
    2 * x.numel() elements.  Returns `out`."""
    lib = _lib.get()
    if out is None:
        out = torch.empty_like(x)
    _check(x, n0, z, out, tables.mask, tables.twiddle, workspace)
    T, h, w = tables.shape
    for name, t in (("x", x), ("n0", n0), ("z", z), ("out", out)):
        if t.dtype != torch.float32 or t.shape != x.shape or t.device != x.device:
            raise RuntimeError(f"freeinit_mix: {name} must be fp32 of x's shape {tuple(x.shape)} on x's device")
    if x.dim() < 3 or tuple(x.shape[-3:]) != (T, h, w) or x.numel() == 0:
        raise RuntimeError(f"freeinit_mix: x {tuple(x.shape)} does not end in the tables' [T, h, w] = {(T, h, w)}")
    if tables.mask.device != x.device:
        raise RuntimeError(f"freeinit_mix: the tables are on {tables.mask.device}, x on {x.device}")
    d = AaFreeInit()
    d.x, d.n0, d.z, d.out, d.mask, d.twiddle = _ptr(x), _ptr(n0), _ptr(z), _ptr(out), _ptr(tables.mask), _ptr(tables.twiddle)
    d.volumes, d.frames, d.h, d.w = x.numel() // (T * h * w), T, h, w
    d.a, d.s = float(a), float(s)
    if workspace is None:
        nbytes = lib.aa_freeinit_workspace(C.byref(d))
        key = (str(x.device), d.volumes, T, h, w)
        workspace = _FREE_INIT_WS.get(key)
        if workspace is None or workspace.numel() * 4 < nbytes:
            workspace = _FREE_INIT_WS[key] = torch.empty(max(nbytes // 4, 2), dtype=torch.float32, device=x.device)
    elif workspace.dtype != torch.float32 or workspace.device != x.device:
        raise RuntimeError("freeinit_mix: the workspace must be fp32 on x's device")
    _run(lib.aa_freeinit_mix, C.byref(d), _ptr(workspace), workspace.numel() * 4, _stream(x))
    return out


# ------------------------------------------------------------------------------------- known-region blend
def keep_blend(x: torch.Tensor, known: torch.Tensor, mask: torch.Tensor, a: float, s: float, noise: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The known-region blend of inpainting samplers on fp32 planes x [clips, C, T, h, w] (or [clips, C, T, hw]), one launch
    (aa_keep_blend): with kn = a * known + s * noise (noise None: s must be 0), out = x where mask >= 1, kn where mask <= 0 and
    mask * x + (1 - mask) * kn between - the endpoints by selection: a mask of 1 hands x through bit for bit, a mask of 0 yields kn
    whatever x holds.  `known`: fp32 / fp16 / bf16 [1 | clips, C, 1 | T, ...]; `mask`: fp32 / fp16 / bf16 [1 | clips, 1 | T, ...], or
    the same with a channel axis of one, [1 | clips, 1, 1 | T, ...] (the motion mask's layout); `noise`: fp32 of x's shape.  A count of
    one is broadcast.  `out`: None - in place, over x - or an fp32 tensor of x's shape that overlaps no operand.  Returns `out`, or x."""
    lib = _lib.get()
    if out is None:
        out = x
    _check(x, known, mask, noise, out)
    if x.dim() not in (4, 5) or x.dtype != torch.float32 or x.numel() == 0:
        raise RuntimeError("keep_blend: x must be fp32 [clips, C, T, h, w] or [clips, C, T, hw]")
    clips, c, frames = x.shape[:3]
    space = tuple(x.shape[3:])
    for name, t in (("noise", noise), ("out", out)):
        if t is not None and (t.dtype != torch.float32 or t.shape != x.shape or t.device != x.device):
            raise RuntimeError(f"keep_blend: {name} must be fp32 of x's shape {tuple(x.shape)} on x's device")
    for name, t in (("known", known), ("mask", mask)):
        if t.dtype not in _DT or t.device != x.device:
            raise RuntimeError(f"keep_blend: {name} must be fp32, fp16 or bf16 on x's device")
    if known.dim() != x.dim() or known.shape[0] not in (1, clips) or known.shape[1] != c or known.shape[2] not in (1, frames) or tuple(known.shape[3:]) != space:
        raise RuntimeError(f"keep_blend: known {tuple(known.shape)} is not [1 | {clips}, {c}, 1 | {frames}, {', '.join(map(str, space))}]")
    m = mask
    if m.dim() == x.dim() and m.shape[1] == 1:
        m = m[:, 0]                                               # (a size-one axis: the memory is the same)
    if m.dim() != x.dim() - 1 or m.shape[0] not in (1, clips) or m.shape[1] not in (1, frames) or tuple(m.shape[2:]) != space:
        raise RuntimeError(f"keep_blend: mask {tuple(mask.shape)} is not [1 | {clips}, (1,) 1 | {frames}, {', '.join(map(str, space))}]")
    if noise is None and float(s) != 0.0:
        raise RuntimeError("keep_blend: s != 0 needs the noise operand")
    d = AaKeepBlend()
    d.x, d.out, d.known, d.mask, d.noise = _ptr(x), _ptr(out), _ptr(known), _ptr(mask), _ptr(noise)
    d.clips, d.channels, d.frames, d.hw = clips, c, frames, x[0, 0, 0].numel()
    d.known_clips, d.known_frames, d.mask_clips, d.mask_frames = known.shape[0], known.shape[2], m.shape[0], m.shape[1]
    d.known_dtype, d.mask_dtype = _DT[known.dtype], _DT[mask.dtype]
    d.a, d.s = float(a), float(s)
    _run(lib.aa_keep_blend, C.byref(d), _stream(x))
    return out
