"""aa_conv_gemm_group: 2..4 independent contractions as ONE launch of one hand-scheduled tile.

The yardstick is bit equality: torch.equal(grouped outputs, the same descriptors launched one by one on the same tile with one K
range) - a member's workgroups see the (workgroup count, workgroup id) of a launch of their own, so nothing about its arithmetic may
change.  Every case runs once per tile the grouped kernel is instantiated for (39, 46, 47, 49) that the case's packed widths admit, pinned
through ops.TILE_PICKER, in fp16 and bf16, on the emulator build and (`-m gpu`) on the MI355X."""
import ctypes as C
import dataclasses

import pytest
import torch

from animate_anything_amd import _lib, ops
from animate_anything_amd._lib import AaConvGemm

GROUP_TILES = (39, 46, 47, 49)
SENTINEL = -77.0
AA_E_SHAPE = -1


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


DEV = "cpu"


def rnd(dt, *shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt).to(DEV)


def widen(pw, n_pad):
    """The same packed weights with zero rows up to `n_pad` packed columns (a 64-column output on a 128-column tile)."""
    w = torch.zeros(n_pad, pw.w.shape[1], dtype=pw.w.dtype, device=pw.w.device)
    w[:pw.w.shape[0]] = pw.w
    return dataclasses.replace(pw, w=w)


def pinned(tile):
    """ops.TILE_PICKER: every group on `tile`, every single call on `tile` with ONE K range."""
    seen = []

    def pick(key, cands):
        seen.append(key[0] == "group")
        if key[0] == "group":
            assert (tile, 0) in cands, (tile, cands)
            return (tile, 0)
        assert any(c[0] == tile for c in cands), (tile, cands)
        return (tile, 1)
    pick.seen = seen
    return pick


def descs(calls):
    """The members' descriptors as ops.conv_gemm_group hands them over: no ticket array (ops.USE_TICKETS may be on)."""
    ds = [ops._conv_gemm_desc(**kw)[0] for kw in calls]
    for d in ds:
        d.tickets, d.tickets_len = None, 0
    return ds


def offered(calls):
    """The grouped tiles the library offers for these calls (the outputs are not touched)."""
    ds = descs(calls)
    arr = (C.POINTER(AaConvGemm) * len(ds))(*[C.pointer(d) for d in ds])
    return [t for t in GROUP_TILES if _lib.get().aa_conv_gemm_group_ok(arr, len(ds), t)]


def with_outputs(calls, fresh):
    """`calls` with their `out` tensors replaced: tensors that share storage in `calls` share one fresh tensor."""
    new = {}
    res = []
    for kw in calls:
        o = kw["out"]
        if id(o) not in new:
            new[id(o)] = fresh(o)
        res.append(dict(kw, out=new[id(o)][:o.shape[0]]))
    return res, list(new.values())


def check_group(calls, tiles_expected):
    """Grouped == one by one, bit for bit, on every offered tile; rows behind each output (where stray rows, padding columns of the
    last row or a neighbouring class would land) keep their sentinel."""
    tiles = offered(calls)
    assert set(tiles) == set(tiles_expected), (tiles, tiles_expected)
    fresh = lambda o: torch.full((o.shape[0] + 3, o.shape[1]), SENTINEL, dtype=o.dtype, device=o.device)
    for tile in tiles:
        ops.TILE_PICKER = pick = pinned(tile)
        try:
            one, one_bufs = with_outputs(calls, fresh)
            for kw in one:
                ops.conv_gemm(**kw)
            grp, grp_bufs = with_outputs(calls, fresh)
            outs = ops.conv_gemm_group(grp)
        finally:
            ops.TILE_PICKER = None
        assert outs is not None and pick.seen.count(True) == 1
        for a, b in zip(grp_bufs, one_bufs):
            assert torch.equal(a, b), tile
            assert (a[-3:] == SENTINEL).all() and torch.isfinite(a[:-3].float()).all(), tile
            assert not (a[:-3] == SENTINEL).all(dim=1).any(), tile       # every row of every member was written
    return tiles


def upsampler_calls(dt, n, h, w, cin, cout, n_pad=None, classes=4, seed=0):
    x = rnd(dt, n * h * w, cin, seed=seed)
    wt, b = rnd(dt, cout, cin, 3, 3, scale=0.05, seed=seed + 1), rnd(dt, cout, seed=seed + 2)
    out = torch.empty(n * 4 * h * w, cout, dtype=dt, device=DEV)
    calls = []
    for (a, bb), pw in list(ops.pack_upsample2x_weights(wt, b).items())[:classes]:
        pw = pw if n_pad is None else widen(pw, n_pad)
        calls.append(dict(x0=x, pw=pw, g=ops.Geom(n, h, w, h, w, 1, 1 - a, 1 - bb), out=out, out_map=(2, 2, a, bb)))
    return calls


DTYPES = [torch.float16, torch.bfloat16]


@pytest.mark.parametrize("dt", DTYPES)
def test_four_upsampler_classes_partial_tiles(backend, dt):
    """3 images of 5 x 7 stored pixels, 128 -> 64 channels: each member is one partial tile (105 rows, 64 of 128 packed columns); the
    classes interleave rows of ONE output, so a class that strays writes over another class's rows."""
    assert check_group(upsampler_calls(dt, 3, 5, 7, 128, 64, n_pad=128, seed=10), [47]) == [47]


@pytest.mark.parametrize("dt", DTYPES)
def test_four_upsampler_classes_several_tiles(backend, dt):
    """5 images of 13 x 11, 128 -> 640 channels: 715 rows = several row tiles with a ragged last one, 2 (5) column tiles, and member
    ranges of 6 / 8 (256 x 320), 8 (192 x 320) and 30 (128 x 128) workgroups: the first needs padding to a multiple of 8."""
    check_group(upsampler_calls(dt, 5, 13, 11, 128, 640, seed=20), [39, 47, 49])


@pytest.mark.parametrize("classes", [2, 3])
def test_member_counts(backend, classes):
    """Groups of 2 and 3 members (4: the upsampler cases): the classes left out keep their sentinel rows."""
    calls = upsampler_calls(torch.float16, 2, 6, 5, 64, 128, classes=classes, seed=30)
    fresh = lambda o: torch.full((o.shape[0] + 3, o.shape[1]), SENTINEL, dtype=o.dtype, device=o.device)
    ops.TILE_PICKER = pinned(47)
    try:
        one, (ref,) = with_outputs(calls, fresh)
        for kw in one:
            ops.conv_gemm(**kw)
        grp, (got,) = with_outputs(calls, fresh)
        assert ops.conv_gemm_group(grp) is not None
    finally:
        ops.TILE_PICKER = None
    assert torch.equal(got, ref)
    untouched = (got == SENTINEL).all(dim=1).sum().item()
    assert untouched == 3 + (4 - classes) * 2 * 6 * 5             # the rows of the other parity classes and behind the grid


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,h,w", [(2, 9, 10), (4, 16, 13)])
def test_shortcut_next_to_conv1(backend, dt, n, h, w):
    """ResnetBlock2D's pair: a two-source 1x1 member (c0 = 64, c1 = 128, bias) and a 3x3 member with K = 9 x 192, a row vector (time
    embedding) and rowvec_div - different K lengths, epilogues and tile counts (M = 180 and 832)."""
    M, cout = n * h * w, 256
    x0, x1, hh = rnd(dt, M, 64, seed=40), rnd(dt, M, 128, seed=41), rnd(dt, M, 192, seed=42)
    w1, b1 = rnd(dt, cout, 192, 1, 1, scale=0.05, seed=43), rnd(dt, cout, seed=44)
    w3, b3 = rnd(dt, cout, 192, 3, 3, scale=0.03, seed=45), rnd(dt, cout, seed=46)
    temb = rnd(dt, n // 2, cout, seed=47)
    conv1 = dict(x0=hh, pw=ops.pack_weight(w3, b3), g=ops.conv3x3_geom(n, h, w), rowvec=temb, rowvec_div=2 * h * w,
                 out=torch.empty(M, cout, dtype=dt, device=DEV))
    shortcut = dict(x0=x0, x1=x1, pw=ops.pack_weight(w1, b1), g=ops.linear_geom(M), out=torch.empty(M, cout, dtype=dt, device=DEV))
    check_group([shortcut, conv1], [46, 47])                     # (the library orders the members itself: longest K first)


@pytest.mark.parametrize("dt", DTYPES)
def test_wide_output_next_to_a_narrow_one(backend, dt):
    """2560 columns at K = 64 next to a 64-column member: 20 column tiles of 128 - the grouped tile order inside a member (>= 8 column
    tiles) next to a member of one partial tile.  300 rows: three row tiles, so the panels of the grouped order hold more than one."""
    M = 300
    xa, xb = rnd(dt, M, 64, seed=50), rnd(dt, M, 64, seed=51)
    wide = dict(x0=xa, pw=ops.pack_weight(rnd(dt, 2560, 64, scale=0.1, seed=52), rnd(dt, 2560, seed=53)), g=ops.linear_geom(M),
                out=torch.empty(M, 2560, dtype=dt, device=DEV))
    narrow = dict(x0=xb, pw=widen(ops.pack_weight(rnd(dt, 64, 64, scale=0.1, seed=54), rnd(dt, 64, seed=55)), 128), g=ops.linear_geom(M),
                  out=torch.empty(M, 64, dtype=dt, device=DEV))
    check_group([narrow, wide], [47])


@pytest.mark.parametrize("dt", DTYPES)
def test_wide_output_on_every_grouped_tile(backend, dt):
    """The same on all four tiles: 2560 columns (8 / 10 / 20 column tiles) next to a 1280-column member, both with a residual."""
    M = 200
    xa, xb = rnd(dt, M, 64, seed=60), rnd(dt, M, 128, seed=61)
    ra, rb = rnd(dt, M, 2560, seed=62), rnd(dt, M, 1280, seed=63)
    wide = dict(x0=xa, pw=ops.pack_weight(rnd(dt, 2560, 64, scale=0.1, seed=64), rnd(dt, 2560, seed=65)), g=ops.linear_geom(M), residual=ra,
                out=torch.empty(M, 2560, dtype=dt, device=DEV))
    other = dict(x0=xb, pw=ops.pack_weight(rnd(dt, 1280, 128, scale=0.1, seed=66)), g=ops.linear_geom(M), residual=rb, out_scale=0.5,
                 out=torch.empty(M, 1280, dtype=dt, device=DEV))
    check_group([wide, other], GROUP_TILES)


def _raw(calls, tile=47):
    ds = descs(calls)
    for d in ds:
        d.tile, d.k_splits = tile, 1
    return ds


def _launch(ds, n=None):
    n = len(ds) if n is None else n
    arr = (C.POINTER(AaConvGemm) * len(ds))(*[C.pointer(d) for d in ds])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if DEV == "cuda" else None
    rc = _lib.get().aa_conv_gemm_group(arr, n, stream)
    if DEV == "cuda":
        torch.cuda.synchronize()
    return rc


def test_rejections_launch_nothing(backend):
    """n = 1 and n = 5, mixed dtypes, a member with k_splits > 1, tickets or row_stats: AA_E_SHAPE, and every output keeps its sentinel."""
    def pair(dt_a=torch.float16, dt_b=torch.float16):
        mk = lambda dt, s: dict(x0=rnd(dt, 70, 64, seed=s), pw=ops.pack_weight(rnd(dt, 128, 64, scale=0.1, seed=s + 1)), g=ops.linear_geom(70),
                                out=torch.full((70, 128), SENTINEL, dtype=dt, device=DEV))
        return [mk(dt_a, 70), mk(dt_b, 72)]

    def rejected(calls, ds, n=None):
        assert _launch(ds, n) == AA_E_SHAPE
        assert _lib.get().aa_last_error()
        assert all((kw["out"] == SENTINEL).all() for kw in calls)

    calls = pair()
    ds = _raw(calls)
    assert _launch(ds) == 0 and not any((kw["out"] == SENTINEL).any() for kw in calls)      # the pair itself is a valid group
    calls = pair()
    rejected(calls, _raw(calls), n=1)
    calls = pair() + pair() + pair()
    rejected(calls[:5], _raw(calls[:5]))
    calls = pair(torch.float16, torch.bfloat16)
    rejected(calls, _raw(calls))
    calls = pair()
    ds = _raw(calls)
    ds[1].k_splits = 2
    rejected(calls, ds)
    calls = pair()
    ds = _raw(calls)
    tickets = torch.zeros(64, dtype=torch.int32, device=DEV)
    ds[0].tickets, ds[0].tickets_len = C.c_void_p(tickets.data_ptr()), 64
    rejected(calls, ds)
    calls = pair()
    ds = _raw(calls)
    stats = torch.zeros(70, 2, 2, dtype=torch.float32, device=DEV)
    ds[1].row_stats, ds[1].row_stats_parts = C.c_void_p(stats.data_ptr()), 2
    rejected(calls, ds)
    assert (stats == 0).all()


def test_host_falls_back_when_no_tile_is_offered(backend):
    """64 packed columns: no grouped tile divides them - ops.conv_gemm_group returns None and launches nothing."""
    mk = lambda s: dict(x0=rnd(torch.float16, 70, 64, seed=s), pw=ops.pack_weight(rnd(torch.float16, 64, 64, scale=0.1, seed=s + 1)),
                        g=ops.linear_geom(70), out=torch.full((70, 64), SENTINEL, dtype=torch.float16, device=DEV))
    calls = [mk(80), mk(82)]
    assert ops.conv_gemm_group(calls) is None
    assert all((kw["out"] == SENTINEL).all() for kw in calls)


@pytest.mark.gpu
def test_benchmark_shapes_of_the_16x16_level():
    """The groups of the flagship step at the 34 x 16 x 16 level (8704 rows, 1280 columns), where a member is 230 workgroups of the
    192 x 256 tile - less than one residency round, so the one-by-one launches have no split-off last round and bit equality holds -
    and a group is 3.6 rounds: the four upsampler classes (K = 5120), and a two-source shortcut (1280 + 1280) next to conv1 (K = 9 x 2560)."""
    global DEV
    DEV = "cuda"
    try:
        dt, n, h, w = torch.float16, 34, 16, 16
        check_group(upsampler_calls(dt, n, h, w, 1280, 1280, seed=100), GROUP_TILES)
        M = n * h * w
        x0, x1, hh = rnd(dt, M, 1280, seed=110), rnd(dt, M, 1280, seed=111), rnd(dt, M, 2560, seed=112)
        conv1 = dict(x0=hh, pw=ops.pack_weight(rnd(dt, 1280, 2560, 3, 3, scale=0.01, seed=113), rnd(dt, 1280, seed=114)), g=ops.conv3x3_geom(n, h, w),
                     rowvec=rnd(dt, 2, 1280, seed=115), rowvec_div=17 * h * w, out=torch.empty(M, 1280, dtype=dt, device=DEV))
        shortcut = dict(x0=x0, x1=x1, pw=ops.pack_weight(rnd(dt, 1280, 2560, 1, 1, scale=0.02, seed=116), rnd(dt, 1280, seed=117)),
                        g=ops.linear_geom(M), out=torch.empty(M, 1280, dtype=dt, device=DEV))
        check_group([conv1, shortcut], GROUP_TILES)
    finally:
        DEV = "cpu"


def test_group_signatures_survive_the_tile_cache(emu, tmp_path, monkeypatch):
    """A group's signature (words and numbers, flat) is written next to the single calls' and read back as the same key."""
    key = ops._group_key([(0, 2, 9, 10, True, "ln"), (0, 1, 1, 180, False)])
    monkeypatch.setattr(ops, "_tile_cache", {key: (47, 0), (0, 1, 1, 180, False): (1, 0), (0, 1, 1, 180, True, "ln"): (36, 2)})
    path = str(tmp_path / "tiles.json")
    ops.save_tile_cache(path)
    saved = dict(ops._tile_cache)
    ops._tile_cache.clear()
    assert ops.load_tile_cache(path) is True and ops._tile_cache == saved


@pytest.mark.gpu
def test_grouped_call_in_a_captured_graph():
    """The launch carries the descriptors by value: captured in a torch.cuda.graph and replayed twice it equals the eager result."""
    global DEV
    DEV = "cuda"
    try:
        calls = upsampler_calls(torch.float16, 5, 13, 11, 128, 640, seed=90)
        ops.TILE_PICKER = pinned(49)
        try:
            eager = ops.conv_gemm_group(calls)[0].clone()
            torch.cuda.synchronize()
            static, (buf,) = with_outputs(calls, lambda o: torch.full_like(o, SENTINEL))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ops.conv_gemm_group(static)
            for _ in range(2):
                buf.fill_(SENTINEL)
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(buf, eager)
        finally:
            ops.TILE_PICKER = None
    finally:
        DEV = "cpu"


def test_tiny_unet_grouped_equals_ungrouped(backend, monkeypatch):
    """Model level: the tiny UNet with AA_GROUP on equals the same forward with it off bit for bit - every call and every group pinned to
    the 128 x 128 tile (where it fits), one K range."""
    from animate_anything_amd.unet3d import UNet3DConditionModel
    from util import TINY_UNET, seeded_state, unet_inputs
    import oracle
    torch.manual_seed(0)
    state = seeded_state(oracle.UNet3DConditionModel(**TINY_UNET).eval())
    net = UNet3DConditionModel(**TINY_UNET).eval()
    net.load_state_dict(state)
    net = net.half().to(DEV)
    i = unet_inputs(h=6, w=6, text_len=9)
    dev = lambda t: t.half().to(DEV)
    groups = []

    def pick(key, cands):
        if key[0] == "group":
            groups.append(key)
            return (47, 0) if (47, 0) in cands else cands[0]
        return (47, 1) if any(c[0] == 47 for c in cands) else cands[0]

    def forward(group):
        monkeypatch.setattr(ops, "GROUP", group)
        ops.TILE_PICKER = pick
        try:
            with torch.no_grad():
                return net(dev(i["sample"]), i["t"], dev(i["text"]), dev(i["cond"]), dev(i["mask"]), motion=i["motion"]).sample.cpu()
        finally:
            ops.TILE_PICKER = None

    off = forward(0)
    assert not groups
    on = forward(3)
    assert any(k[1] == 4 for k in groups) and any(k[1] == 2 for k in groups), groups      # both call sites really grouped
    assert torch.isfinite(on.float()).all() and torch.equal(on, off)
