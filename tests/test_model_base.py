"""animate_anything_amd/_model.py: the loading / saving protocol, the cache and session store and the batched projections that
the model and pipeline classes share.  The expected file contents below are what the classes wrote BEFORE they shared a base
(recorded from that commit, not from the code under test): keys, key order and the literal class names are part of the
checkpoint format."""
import json
import os

import pytest
import torch

from animate_anything_amd import ops
from animate_anything_amd.clip import CLIPTextModel, CLIPVisionModelWithProjection
from animate_anything_amd.layerdiffuse import MaskedLatentToVideoPipeline
from animate_anything_amd.pipeline import LatentToVideoPipeline
from animate_anything_amd.svd_pipeline import MaskStableVideoDiffusionPipeline, StableVideoDiffusionPipeline
from animate_anything_amd.svd_unet import UNetSpatioTemporalConditionModel
from animate_anything_amd.svd_vae import AutoencoderKLTemporalDecoder
from animate_anything_amd.unet3d import UNet3DConditionModel
from animate_anything_amd.vae import AutoencoderKL
from test_clip import TINY_CLIP
from test_svd import TINY_SVD_UNET, TINY_SVD_VAE
from util import TINY_UNET, TINY_VAE

TINY_VISION = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, image_size=42, patch_size=14,
                   projection_dim=48, hidden_act="quick_gelu")

# class -> (constructor arguments, the config.json it writes as ordered (key, value) pairs, the weight file)
MODELS = {
    UNet3DConditionModel: (TINY_UNET, [
        ("sample_size", None), ("in_channels", 4), ("out_channels", 4), ("down_block_types", ["CrossAttnDownBlock3D", "DownBlock3D"]),
        ("up_block_types", ["UpBlock3D", "CrossAttnUpBlock3D"]), ("block_out_channels", [64, 128]), ("layers_per_block", 1),
        ("downsample_padding", 1), ("mid_block_scale_factor", 1), ("act_fn", "silu"), ("norm_num_groups", 32), ("norm_eps", 1e-05),
        ("cross_attention_dim", 64), ("attention_head_dim", 64), ("motion_mask", True), ("motion_strength", True),
        ("_class_name", "UNet3DConditionModel")], "diffusion_pytorch_model.safetensors"),
    UNetSpatioTemporalConditionModel: (TINY_SVD_UNET, [
        ("sample_size", None), ("in_channels", 9), ("out_channels", 4),
        ("down_block_types", ["CrossAttnDownBlockSpatioTemporal", "DownBlockSpatioTemporal"]),
        ("up_block_types", ["UpBlockSpatioTemporal", "CrossAttnUpBlockSpatioTemporal"]), ("block_out_channels", [64, 128]),
        ("addition_time_embed_dim", 32), ("projection_class_embeddings_input_dim", 96), ("layers_per_block", 1),
        ("cross_attention_dim", 64), ("transformer_layers_per_block", 1), ("num_attention_heads", [1, 2]), ("num_frames", 3),
        ("_class_name", "UNetSpatioTemporalConditionModel")], "diffusion_pytorch_model.safetensors"),
    AutoencoderKL: (TINY_VAE, [
        ("in_channels", 3), ("out_channels", 3), ("block_out_channels", [32, 64]), ("layers_per_block", 1), ("latent_channels", 4),
        ("norm_num_groups", 32), ("scaling_factor", 0.18215), ("force_upcast", True), ("_class_name", "AutoencoderKL")],
        "diffusion_pytorch_model.safetensors"),
    AutoencoderKLTemporalDecoder: (TINY_SVD_VAE, [
        ("in_channels", 3), ("out_channels", 3), ("block_out_channels", [32, 64]), ("layers_per_block", 1), ("latent_channels", 4),
        ("scaling_factor", 0.18215), ("force_upcast", True), ("_class_name", "AutoencoderKLTemporalDecoder")],
        "diffusion_pytorch_model.safetensors"),
    CLIPTextModel: (TINY_CLIP, [
        ("vocab_size", 120), ("hidden_size", 128), ("intermediate_size", 256), ("num_hidden_layers", 2), ("num_attention_heads", 2),
        ("max_position_embeddings", 24), ("hidden_act", "gelu"), ("layer_norm_eps", 1e-05), ("eos_token_id", 2),
        ("architectures", ["CLIPTextModel"]), ("model_type", "clip_text_model")], "model.safetensors"),
    CLIPVisionModelWithProjection: (TINY_VISION, [
        ("hidden_size", 64), ("intermediate_size", 128), ("projection_dim", 48), ("num_hidden_layers", 2), ("num_attention_heads", 1),
        ("num_channels", 3), ("image_size", 42), ("patch_size", 14), ("hidden_act", "quick_gelu"), ("layer_norm_eps", 1e-05),
        ("architectures", ["CLIPVisionModelWithProjection"]), ("model_type", "clip_vision_model")], "model.safetensors"),
}
UNETS = [UNet3DConditionModel, UNetSpatioTemporalConditionModel]
ids = lambda v: getattr(v, "__name__", None)                    # classes by name, everything else as pytest names it


def _read(path):
    """(text, ordered pairs) of a JSON file."""
    with open(path) as f:
        text = f.read()
    return text, list(json.loads(text).items())


# ------------------------------------------------------------------------------------------- written files
@pytest.mark.parametrize("cls", list(MODELS), ids=ids)
def test_config_json_is_written_as_before_and_loads_back(cls, tmp_path):
    cfg, want, weights = MODELS[cls]
    torch.manual_seed(0)
    net = cls(**cfg)
    net.save_pretrained(str(tmp_path / "m"))
    assert sorted(os.listdir(tmp_path / "m")) == ["config.json", weights]
    text, got = _read(tmp_path / "m" / "config.json")
    assert got == want                                           # keys, values AND order
    assert text == json.dumps(dict(want), indent=2)
    again = cls.from_pretrained(str(tmp_path), subfolder="m")
    assert json.dumps(vars(again.config)) == json.dumps(vars(net.config))       # (a tuple the constructor keeps as given comes back a list)
    assert list(again.state_dict()) == list(net.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), again.state_dict().values()))
    half = cls.from_pretrained(str(tmp_path / "m"), torch_dtype=torch.float16)
    assert half.dtype == torch.float16 and half.device == torch.device("cpu")


@pytest.mark.parametrize("cls", [UNet3DConditionModel, CLIPTextModel], ids=ids)
def test_variant_weight_files_are_found(cls, tmp_path):
    cfg, _, weights = MODELS[cls]
    net = cls(**cfg)
    net.save_pretrained(str(tmp_path))
    os.rename(tmp_path / weights, tmp_path / weights.replace(".safetensors", ".fp16.safetensors"))
    with pytest.raises(FileNotFoundError):
        cls.from_pretrained(str(tmp_path))
    again = cls.from_pretrained(str(tmp_path), variant="fp16")
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), again.state_dict().values()))


@pytest.mark.parametrize("cls,unet,name,scheduler", [
    (LatentToVideoPipeline, UNet3DConditionModel, "LatentToVideoPipeline", "DPMSolverMultistepScheduler"),
    (MaskedLatentToVideoPipeline, UNet3DConditionModel, "LatentToVideoPipeline", "DPMSolverMultistepScheduler"),
    (StableVideoDiffusionPipeline, UNetSpatioTemporalConditionModel, "StableVideoDiffusionPipeline", "EulerDiscreteScheduler"),
    (MaskStableVideoDiffusionPipeline, UNetSpatioTemporalConditionModel, "StableVideoDiffusionPipeline", "EulerDiscreteScheduler")],
    ids=ids)
def test_model_index_json_is_written_as_before(cls, unet, name, scheduler, tmp_path):
    """A subclass writes its parent's name; absent components are left out; the scheduler's file ends with its class name."""
    pipe = cls(vae=None, unet=unet(**MODELS[unet][0]))
    pipe.save_pretrained(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["model_index.json", "scheduler", "unet"]
    want = [("_class_name", name), ("unet", ["animate_anything_amd", unet.__name__]), ("scheduler", ["animate_anything_amd", scheduler])]
    text, got = _read(tmp_path / "model_index.json")
    assert got == want and text == json.dumps(dict(want), indent=2)
    text, got = _read(tmp_path / "scheduler" / "scheduler_config.json")
    assert got == list(vars(pipe.scheduler.config).items()) + [("_class_name", scheduler)]
    assert text == json.dumps(dict(got), indent=2)
    assert _read(tmp_path / "unet" / "config.json")[1] == MODELS[unet][1]
    assert pipe.to("cpu", torch.float16) is pipe and pipe.unet.dtype == torch.float16


# ------------------------------------------------------------------------------------------- from_config
# class -> a constructor argument, its value in the file, the value the caller overrides it with
OVERRIDES = {UNet3DConditionModel: ("sample_size", 8, 16), UNetSpatioTemporalConditionModel: ("sample_size", 8, 16),
             AutoencoderKL: ("scaling_factor", 0.5, 0.25), AutoencoderKLTemporalDecoder: ("scaling_factor", 0.5, 0.25),
             CLIPTextModel: ("layer_norm_eps", 3e-5, 1e-6), CLIPVisionModelWithProjection: ("layer_norm_eps", 3e-5, 1e-6)}


@pytest.mark.parametrize("cls", list(MODELS), ids=ids)
def test_from_config_drops_unknown_and_private_keys_and_overrides_win(cls):
    cfg = MODELS[cls][0]
    key, in_file, override = OVERRIDES[cls]
    file = dict(cfg, _class_name="SomethingElse", _diffusers_version="0.24.0", not_a_constructor_argument=7, **{key: in_file})
    want = vars(cls(**cfg).config)
    for net, value in ((cls.from_config(file), in_file), (cls.from_config(file, **{key: override}), override),
                       (cls.from_config(file, also_not_an_argument=1, **{key: override}), override)):
        got = vars(net.config)
        assert list(got) == list(want)
        for k in got:
            assert got[k] == (value if k == key else want[k]), k


@pytest.mark.parametrize("cls,section", [(CLIPTextModel, "text_config"), (CLIPVisionModelWithProjection, "vision_config")], ids=ids)
def test_from_config_folds_the_nested_clip_section_under_the_top_level(cls, section):
    cfg = MODELS[cls][0]
    composite = {section: dict(cfg, num_hidden_layers=5, _name_or_path="x"), "num_hidden_layers": 1, "model_type": "clip",
                 "text_config" if section == "vision_config" else "vision_config": {"hidden_size": 999}}
    net = cls.from_config(composite)
    assert net.config.num_hidden_layers == 1                         # the top level wins
    assert net.config.hidden_size == cfg["hidden_size"] and net.config.intermediate_size == cfg["intermediate_size"]
    assert cls.from_config(composite, num_hidden_layers=2).config.num_hidden_layers == 2
    assert cls.from_config({section: None, **cfg}).config.hidden_size == cfg["hidden_size"]


# ------------------------------------------------------------------------------------------- caches and sessions
def _session(net, h):
    if isinstance(net, UNet3DConditionModel):
        return net.session(2, 2, h, 6, (9, 64), True, True, False, torch.float32, 2, 2, 1, "cpu")
    return net.session(2, 3, h, 6, (1, 64), ((2, 9, torch.float32),), "cpu")


@pytest.mark.parametrize("cls", UNETS, ids=ids)
def test_session_store(cls):
    """Eager: at most one session (they hold only input buffers).  Graphs enabled: one per key, in `net._graph`."""
    net = cls(**MODELS[cls][0])
    assert net._graph is None
    a = _session(net, 4)
    assert _session(net, 4) is a and a.net is net and a.graph is None and a.out is None
    assert list(net.__dict__["_eager_sessions"].values()) == [a]
    b = _session(net, 5)
    assert b is not a and list(net.__dict__["_eager_sessions"].values()) == [b]      # the second key evicted the first
    assert _session(net, 4) is not a and net._graph is None
    net.enable_graph()
    assert net._graph == {}
    c, d = _session(net, 4), _session(net, 5)
    assert c is not d and _session(net, 4) is c and _session(net, 5) is d and set(net._graph.values()) == {c, d}
    assert len(net.__dict__["_eager_sessions"]) == 1                                 # untouched by the graph store
    src = torch.full((1, 1, 64), 2.0)
    c.load(text=src, t=None)                                                         # broadcast into the static buffer; None: left alone
    assert torch.equal(c.inputs["text"], src.expand(c.inputs["text"].shape)) and c.inputs["text"].dtype == net.dtype
    net.enable_graph(False)
    assert net._graph is None


def _invalidating_calls(net):
    calls = {"to": lambda: net.to(torch.float16), "load_state_dict": lambda: net.load_state_dict(net.state_dict()),
             "invalidate_caches": net.invalidate_caches}
    if isinstance(net, UNet3DConditionModel):
        calls.update(enable_freeu=lambda: net.enable_freeu(0.9, 0.2, 1.2, 1.4), disable_freeu=net.disable_freeu,
                     enable_fp8_feedforward=net.enable_fp8_feedforward, disable_fp8_feedforward=net.disable_fp8_feedforward)
    return calls


@pytest.mark.parametrize("cls", UNETS, ids=ids)
def test_every_invalidating_call_empties_the_graph_store_and_drops_the_packs(cls):
    net = cls(**MODELS[cls][0])
    packs = ("_temb_pack", "_text_pack") + (("_co_pack",) if cls is UNet3DConditionModel else ())
    assert tuple(net._packs) == packs
    for graph in (True, False):
        net.enable_graph(graph)
        for name, call in _invalidating_calls(net).items():
            if graph:
                net._graph["a captured session"] = object()
            for p in packs:
                setattr(net, p, ("a stale pack",))
            call()
            assert net._graph == ({} if graph else None), name
            assert all(getattr(net, p) is None for p in packs), name


# one resolution level (a cross-attention down block, the mid block, a cross-attention up block): every kind of cache, a third of the launches
ONE_LEVEL = {UNet3DConditionModel: dict(block_out_channels=(64,), down_block_types=("CrossAttnDownBlock3D",),
                                        up_block_types=("CrossAttnUpBlock3D",)),
             UNetSpatioTemporalConditionModel: dict(block_out_channels=(64,), down_block_types=("CrossAttnDownBlockSpatioTemporal",),
                                                    up_block_types=("CrossAttnUpBlockSpatioTemporal",), num_attention_heads=(1,))}


def _forward(net):
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g).half()
    with torch.no_grad():
        if isinstance(net, UNet3DConditionModel):
            return net(r(1, 4, 1, 4, 4), 501, r(1, 3, 64), r(1, 4, 1, 4, 4), torch.ones(1, 1, 1, 4, 4).half(), motion=torch.tensor([3.0])).sample
        return net(r(1, 2, 9, 4, 4), 1.2, r(1, 1, 64), torch.tensor([[6.0, 127.0, 0.02]])).sample


@pytest.mark.parametrize("cls", UNETS, ids=ids)
def test_caches_are_not_state(emu, cls):
    """The module lists, packs and sessions a forward leaves behind are plain attributes: no new state-dict key, submodule,
    parameter or buffer - a checkpoint saved after a forward is the checkpoint saved before it."""
    torch.manual_seed(0)
    net = cls(**dict(MODELS[cls][0], **ONE_LEVEL[cls])).eval().half()
    before = (list(net.state_dict()), [n for n, _ in net.named_modules()], [n for n, _ in net.named_buffers()])
    assert torch.isfinite(_forward(net)).all()
    assert net._temb_pack is not None and net._text_pack is not None and len(net.__dict__["_eager_sessions"]) == 1
    assert net.__dict__["_temb_pack_modules"] and net.__dict__["_text_pack_modules"]
    assert (list(net.state_dict()), [n for n, _ in net.named_modules()], [n for n, _ in net.named_buffers()]) == before


# ------------------------------------------------------------------------------------------- batched projections
@pytest.mark.parametrize("cls", UNETS, ids=ids)
def test_batched_projections_equal_each_modules_own_contraction(emu, cls):
    """`_project_text` / `_project_time_embeddings`: every module's column slice of the ONE wide contraction is, bit for bit, that
    module's own weights applied alone (ops.conv_gemm over the same rows: the sum over K of one output column does not depend on
    how many columns the launch has); modules are taken in `self.modules()` order, K rows in front of V rows."""
    from animate_anything_amd.layers import Attention, ResnetBlock2D
    from animate_anything_amd.svd_unet import TemporalResnetBlock
    torch.manual_seed(0)
    net = cls(**MODELS[cls][0]).eval().half()
    g = torch.Generator().manual_seed(3)
    text = torch.randn(2 * 5, 64, generator=g).half()
    temb = torch.randn(2, 4 * 64, generator=g).half()
    cross = [m for m in net.modules() if isinstance(m, Attention) and m.is_cross]
    kinds = (ResnetBlock2D, TemporalResnetBlock) if cls is UNetSpatioTemporalConditionModel else ResnetBlock2D
    blocks = [m for m in net.modules() if isinstance(m, kinds) and m.time_emb_proj is not None]
    assert len(cross) >= 3 and len(blocks) >= 5 and (kinds is ResnetBlock2D or any(isinstance(b, TemporalResnetBlock) for b in blocks))

    def check():
        with torch.no_grad():
            net._project_text(text)
            net._project_time_embeddings(temb)
            for a in cross:
                alone = ops.conv_gemm(text, ops.pack_weight(torch.cat([a.to_k.weight, a.to_v.weight])), ops.linear_geom(text.shape[0]))
                assert a.kv.shape == (10, 2 * a.inner) and torch.equal(a.kv, alone)
            for b in blocks:
                alone = ops.conv_gemm(temb, ops.pack_weight(b.time_emb_proj.weight, b.time_emb_proj.bias), ops.linear_geom(2))
                assert b.tproj.shape == (2, b.time_emb_proj.weight.shape[0]) and torch.equal(b.tproj, alone)
        return net._text_pack, net._temb_pack

    first = check()
    assert first[0][2] == cross and first[1][2] == blocks                       # the module order
    again = check()
    assert again[0] is first[0] and again[1] is first[1]                         # unchanged weights: the packs are reused
    kv_before = cross[1].kv.clone()
    with torch.no_grad():                                                       # an in-place edit changes the key: repacked
        cross[1].to_v.weight.mul_(0.5)
        blocks[2].time_emb_proj.bias.add_(0.25)
    edited = check()
    assert edited[0] is not first[0] and edited[1] is not first[1]
    assert edited[0][1] is not first[0][1] and not torch.equal(cross[1].kv, kv_before)
