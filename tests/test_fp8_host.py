"""Host side of the opt-in e4m3 FeedForward path: which layers the switch flags, the default, the tile-cache file under the new library version."""
import torch

from animate_anything_amd import layers, ops


def _default_unet():
    from animate_anything_amd.unet3d import UNet3DConditionModel
    with torch.device("meta"):
        return UNet3DConditionModel(motion_mask=True, motion_strength=True)


def _ffs(net):
    return [m for m in net.modules() if isinstance(m, layers.FeedForward)]


def test_switch_flags_exactly_the_wide_feedforwards():
    """Default architecture (320, 640, 1280, 1280 channels; two transformer pairs per down level, three per up level, one in the middle, plus
    transformer_in): every spatial / temporal FeedForward with dim >= min_dim and no other."""
    net = _default_unet()
    ffs = _ffs(net)
    by_dim = {}
    for m in ffs:
        by_dim[m.dim] = by_dim.get(m.dim, 0) + 1
    assert set(by_dim) == {320, 512, 640, 1280}, by_dim        # (512: transformer_in, 8 heads x 64)
    assert not any(m.fp8 for m in ffs)
    n = net.enable_fp8_feedforward()
    assert n == by_dim[640] + by_dim[1280] == sum(m.fp8 for m in ffs)
    assert all(m.fp8 == (m.dim >= 640) for m in ffs)
    assert net.enable_fp8_feedforward(min_dim=1280) == by_dim[1280]
    assert all(m.fp8 == (m.dim >= 1280) for m in ffs)
    net.disable_fp8_feedforward()
    assert not any(m.fp8 for m in ffs)
    # spatial and temporal transformers alike
    net.enable_fp8_feedforward()
    kinds = {type(t).__name__ for t in net.modules() if isinstance(t, (layers.Transformer2DModel, layers.TransformerTemporalModel))
             and t.transformer_blocks[-1].ff.fp8}
    assert kinds == {"Transformer2DModel", "TransformerTemporalModel"}
    # a flagged last block ends in its own contraction: no merged tail, no fused kernel
    assert all(t.merged_tail() is None and t.fused_ff() is None for t in net.modules()
               if isinstance(t, (layers.Transformer2DModel, layers.TransformerTemporalModel)) and t.transformer_blocks[-1].ff.fp8)


def test_knob_unset_flags_nothing(monkeypatch):
    """AA_FP8_FF is read once at import (like the other knobs of layers.py): unset or "0" means off, and a model built then has no flagged layer;
    with the knob on, a model flags itself at construction."""
    import os
    assert layers.AA_FP8_FF == (os.environ.get("AA_FP8_FF", "0") == "1")
    monkeypatch.setattr(layers, "AA_FP8_FF", False)
    assert not any(m.fp8 for m in _ffs(_default_unet()))
    monkeypatch.setattr(layers, "AA_FP8_FF", True)
    ffs = _ffs(_default_unet())
    assert any(m.fp8 for m in ffs) and all(m.fp8 == (m.dim >= layers.FP8_FF_MIN_DIM) for m in ffs)


def test_tile_cache_loads_under_the_new_version(emu_lib):
    from animate_anything_amd import _lib
    assert emu_lib.aa_version() == 110
    with _lib.use_library(emu_lib, host_pointers=True):
        assert ops.load_tile_cache(ops.DEFAULT_TILE_CACHE) is True
