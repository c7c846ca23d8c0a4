"""FreeU without a GPU: the FFT-free seven-basis form against diffusers' FFT form, the UNet / pipeline / eval plumbing, and the product
UNet with FreeU on against the oracle carrying diffusers' `apply_freeu` as forward-pre-hooks (SIMT emulator)."""
import pytest
import torch

import oracle
from animate_anything_amd.unet3d import UNet3DConditionModel
from freeu_util import FREEU, PLANES, fourier_filter_basis, fourier_filter_fft, hook_oracle
from util import TINY_UNET, rel_err, seeded_state, unet_inputs


@pytest.mark.parametrize("h,w", PLANES)
def test_seven_basis_form_equals_the_fft_form(h, w):
    g = torch.Generator().manual_seed(100 * h + w)
    for mean in (0.7, 50.0):
        x = torch.randn(3, 5, h, w, generator=g, dtype=torch.float64) + mean
        for s in (0.9, 0.2):
            want = fourier_filter_fft(x, 1, s)
            got = fourier_filter_basis(x, s)
            assert (got - want).abs().max().item() < 1e-11, (h, w, mean, s)
            if h * w > 1:                                      # the filter does something: the mean alone moves by (s - 1) * mean
                assert (want - x).abs().max().item() > 0.05


def _pair(seed=0):
    torch.manual_seed(seed)
    ref = oracle.UNet3DConditionModel(**TINY_UNET).eval()
    state = seeded_state(ref)
    ref.load_state_dict(state)
    net = UNet3DConditionModel(**TINY_UNET).eval()
    net.load_state_dict(state)
    return ref, net.half()


def _run(net, i):
    with torch.no_grad():
        return net(i["sample"].half(), i["t"], i["text"].half(), i["cond"].half(), i["mask"].half(), motion=i["motion"]).sample


def _run_ref(ref, i):
    with torch.no_grad():
        return ref(i["sample"], i["t"], i["text"], i["cond"], i["mask"], motion=i["motion"]).sample


def test_enable_and_disable_set_the_attributes_and_drop_captured_sessions():
    net = UNet3DConditionModel(**TINY_UNET).eval()
    assert [b.resolution_idx for b in net.up_blocks] == [0, 1]
    assert all(getattr(b, k) is None for b in net.up_blocks for k in FREEU)
    net.enable_graph()
    net._graph["a captured session"] = object()
    net.enable_freeu(**FREEU)
    assert net._graph == {}
    assert all(getattr(b, k) == v for b in net.up_blocks for k, v in FREEU.items())
    assert net.up_blocks[0]._freeu() == (FREEU["b1"], FREEU["s1"]) and net.up_blocks[1]._freeu() == (FREEU["b2"], FREEU["s2"])
    net._graph["a captured session"] = object()
    net.disable_freeu()
    assert net._graph == {}
    assert all(getattr(b, k) is None for b in net.up_blocks for k in FREEU) and all(b._freeu() is None for b in net.up_blocks)
    net.enable_freeu(0.9, 0.2, 1.2, 0)                         # diffusers' condition: all four set and non-zero
    assert all(b._freeu() is None for b in net.up_blocks)
    net.enable_freeu(s1=0.9, s2=0.2, b1=1.2, b2=1.4)           # diffusers' signature (s1, s2, b1, b2)
    deep = UNet3DConditionModel(block_out_channels=(64, 64, 64), down_block_types=("DownBlock3D",) * 3, up_block_types=("UpBlock3D",) * 3,
                                layers_per_block=1, cross_attention_dim=64)
    deep.enable_freeu(**FREEU)
    assert [b._freeu() is not None for b in deep.up_blocks] == [True, True, False]    # resolution_idx 0 and 1 only


@pytest.mark.parametrize("h,w", [(8, 8), (5, 7)])
def test_tiny_unet_with_freeu_matches_the_hooked_oracle(emu, monkeypatch, h, w):
    """Product with FreeU on against the oracle with diffusers' apply_freeu hooked in; one launch per layer of the two top up blocks, in
    place, none with FreeU off; at 5x7 also: disable_freeu() restores the never-enabled output bit for bit."""
    from animate_anything_amd import ops
    calls = []
    real = ops.freeu
    monkeypatch.setattr(ops, "freeu", lambda *a, **k: calls.append((a[2:7], k["hidden_out"] is a[0], k["skip_out"] is a[1])) or real(*a, **k))
    ref, net = _pair()
    i = unet_inputs(h=h, w=w, text_len=9)
    never = _run(net, i) if h == 5 else None
    assert calls == []
    want_off = _run_ref(ref, i)
    handles = hook_oracle(ref, **FREEU)
    assert len(handles) == 4
    want = _run_ref(ref, i)
    for hd in handles:
        hd.remove()
    net.enable_freeu(**FREEU)
    got = _run(net, i)
    images, lo = 2 * 3, ((h + 1) // 2, (w + 1) // 2)
    assert calls == [((images,) + lo + (1.2, 0.9), True, True)] * 2 + [((images, h, w, 1.4, 0.2), True, True)] * 2
    err, mse = rel_err(got, want), ((got.float() - want) ** 2).mean().item()
    off_err, off_mse = rel_err(want_off, want), ((want_off - want) ** 2).mean().item()
    print(f"{h}x{w}: product-on vs oracle-on rel_err {err:.4g} mse {mse:.4g}; oracle-off vs oracle-on {off_err:.4g} / {off_mse:.4g}")
    assert off_err > 3e-2 and off_mse > 1e-3                   # the hooks act: a no-op implementation cannot pass
    assert err < 3e-2 and mse < 1e-3, (err, mse)
    if never is not None:
        net.disable_freeu()
        again = _run(net, i)
        assert len(calls) == 4
        assert torch.equal(again.view(torch.int16), never.view(torch.int16))
        assert not torch.equal(got, never)


def test_pipeline_methods_forward_to_the_unet():
    from animate_anything_amd.pipeline import LatentToVideoPipeline
    net = UNet3DConditionModel(**TINY_UNET).eval()
    pipe = LatentToVideoPipeline(vae=None, unet=net)
    pipe.enable_freeu(s1=0.9, s2=0.2, b1=1.2, b2=1.4)
    assert all(getattr(b, k) == v for b in net.up_blocks for k, v in FREEU.items())
    pipe.enable_freeu(0.6, 0.4, 1.1, 1.2)                      # positional order s1, s2, b1, b2
    assert (net.up_blocks[0].s1, net.up_blocks[0].s2, net.up_blocks[0].b1, net.up_blocks[0].b2) == (0.6, 0.4, 1.1, 1.2)
    pipe.disable_freeu()
    assert all(getattr(b, k) is None for b in net.up_blocks for k in FREEU)


def test_eval_validates_the_freeu_key_before_any_model_is_loaded(tmp_path):
    from animate_anything_amd import eval as aa_eval
    missing = str(tmp_path / "no_such_checkpoint")
    bad = [dict(s1=0.9, s2=0.2, b1=1.2), dict(FREEU, b3=1.0), dict(FREEU, s1="strong"), dict(FREEU, b2=None), dict(FREEU, b1=True),
           [0.9, 0.2, 1.2, 1.4], 0.9]
    for freeu in bad:
        with pytest.raises(ValueError, match="freeu"):
            aa_eval.main_eval(missing, {}, freeu=freeu)
    assert aa_eval._check_freeu(dict(FREEU, s1=1)) == dict(FREEU, s1=1.0)
    # the YAML key and dot-list overrides
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text("pretrained_model_path: x\nvalidation_data: {}\nfreeu: {s1: 0.9, s2: 0.2, b1: 1.2, b2: 1.4}\n")
    cfg = aa_eval.load_config(str(cfg_path), ["freeu.b2=1.6", "freeu.s1=1"])
    assert aa_eval._check_freeu(cfg["freeu"]) == dict(s1=1.0, s2=0.2, b1=1.2, b2=1.6)
    cfg = aa_eval.load_config(str(cfg_path), ["freeu.b2=much"])
    with pytest.raises(ValueError, match="freeu.b2"):
        aa_eval.main_eval(**cfg)
    assert aa_eval._check_freeu(None) is None
