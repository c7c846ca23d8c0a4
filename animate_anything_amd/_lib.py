"""ctypes binding of libaa_mi355.so (C ABI: include/aa_mi355.h).

The library is the only compute backend of this package: if it cannot be loaded the import of any
op fails loudly (RuntimeError) -- there is no eager/PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede the dlopen below: libaa_mi355.so has to bind to the HIP runtime
#                           torch already loaded, otherwise two runtimes end up in one process)

AA_F16, AA_BF16, AA_F32 = 0, 1, 2
AA_ACT_NONE, AA_ACT_SILU, AA_ACT_GELU, AA_ACT_QUICK_GELU = 0, 1, 2, 3


class AaConvGemm(C.Structure):
    _fields_ = [
        ("a0", C.c_void_p), ("a1", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p),
        ("rowvec", C.c_void_p), ("residual", C.c_void_p), ("out", C.c_void_p),
        ("c0", C.c_int32), ("c1", C.c_int32),
        ("n_img", C.c_int32), ("h_in", C.c_int32), ("w_in", C.c_int32), ("h_virt", C.c_int32),
        ("w_virt", C.c_int32), ("h_out", C.c_int32), ("w_out", C.c_int32),
        ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("pad_h", C.c_int32), ("pad_w", C.c_int32),
        ("n_out", C.c_int32), ("n_pad", C.c_int32), ("k_pad", C.c_int32),
        ("rowvec_div", C.c_int32), ("ldo", C.c_int32), ("ldr", C.c_int32),
        ("act", C.c_int32), ("geglu", C.c_int32), ("bias_per_row", C.c_int32),
        ("dtype", C.c_int32), ("out_dtype", C.c_int32), ("out_scale", C.c_float), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("k_order", C.c_int32), ("debug", C.c_int32), ("tile", C.c_int32), ("k_splits", C.c_int32), ("rowvec_ld", C.c_int32), ("acc_scale", C.c_float),
        ("out_sy", C.c_int32), ("out_sx", C.c_int32), ("out_oy", C.c_int32), ("out_ox", C.c_int32),
        ("ln_stats", C.c_void_p), ("ln_cols", C.c_void_p), ("ln_parts", C.c_int32), ("ln_eps", C.c_float),
        ("row_stats", C.c_void_p), ("row_stats_parts", C.c_int32), ("tickets_len", C.c_int32), ("tickets", C.c_void_p),
        ("row_coef", C.c_void_p), ("row_coef_eps", C.c_float), ("_reserved107", C.c_int32),
    ]


class AaGroupNorm(C.Structure):
    _fields_ = [
        ("x0", C.c_void_p), ("x1", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("y", C.c_void_p),
        ("c0", C.c_int32), ("c1", C.c_int32), ("n_groups_img", C.c_int32), ("tokens_per_group", C.c_int32),
        ("num_groups", C.c_int32), ("silu", C.c_int32), ("dtype", C.c_int32), ("eps", C.c_float),
    ]


class AaAttnOperand(C.Structure):
    _fields_ = [
        ("ptr", C.c_void_p), ("outer_stride", C.c_int64), ("inner_stride", C.c_int64), ("pos_stride", C.c_int64),
        ("ld", C.c_int32), ("col0", C.c_int32), ("outer_div", C.c_int32), ("seq_mod", C.c_int32),
    ]


class AaAttention(C.Structure):
    _fields_ = [
        ("q", AaAttnOperand), ("k", AaAttnOperand), ("v", AaAttnOperand), ("o", AaAttnOperand),
        ("n_outer", C.c_int32), ("n_inner", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32),
        ("q_len", C.c_int32), ("kv_len", C.c_int32), ("dtype", C.c_int32), ("scale", C.c_float), ("causal", C.c_int32), ("_pad", C.c_int32),
    ]


class AaSeqSelfAttn(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p), ("w_bias", C.c_void_p), ("pre_w", C.c_void_p), ("pre_bias", C.c_void_p), ("pre_residual", C.c_void_p), ("pre_out", C.c_void_p), ("o", C.c_void_p),
        ("outer_stride", C.c_int64), ("inner_stride", C.c_int64), ("pos_stride", C.c_int64), ("x_bytes", C.c_int64), ("o_bytes", C.c_int64),
        ("n_outer", C.c_int32), ("n_inner", C.c_int32), ("seq_len", C.c_int32), ("channels", C.c_int32), ("ldx", C.c_int32), ("ldo", C.c_int32), ("ld_res", C.c_int32), ("ld_pre", C.c_int32),
        ("normalize", C.c_int32), ("ln_eps", C.c_float), ("scale", C.c_float), ("dtype", C.c_int32), ("flags", C.c_int32),
    ]


class AaFFFused(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("outer", C.c_void_p), ("out", C.c_void_p), ("w", C.c_void_p), ("rows", C.c_int64),
        ("channels", C.c_int32), ("ldx", C.c_int32), ("ld_outer", C.c_int32), ("ldo", C.c_int32),
        ("normalize", C.c_int32), ("ln_eps", C.c_float), ("dtype", C.c_int32), ("flags", C.c_int32),
    ]


class AaLinearRows(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("residual", C.c_void_p), ("out", C.c_void_p), ("w", C.c_void_p), ("rows", C.c_int64),
        ("channels", C.c_int32), ("n_out", C.c_int32), ("ldx", C.c_int32), ("ld_res", C.c_int32), ("ldo", C.c_int32),
        ("normalize", C.c_int32), ("ln_eps", C.c_float), ("dtype", C.c_int32), ("flags", C.c_int32),
        ("row_affine", C.c_void_p), ("rows_per_group", C.c_int32), ("_pad", C.c_int32),
    ]


class AaQuantRowsFp8(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("q", C.c_void_p), ("scale", C.c_void_p), ("rows", C.c_int64),
        ("channels", C.c_int32), ("ldx", C.c_int32), ("ldq", C.c_int32), ("ln_eps", C.c_float), ("dtype", C.c_int32), ("_pad", C.c_int32),
    ]


class AaLinearFp8(C.Structure):
    _fields_ = [
        ("a", C.c_void_p), ("a_scale", C.c_void_p), ("w", C.c_void_p), ("w_scale", C.c_void_p), ("bias", C.c_void_p),
        ("residual", C.c_void_p), ("out", C.c_void_p), ("rows", C.c_int64),
        ("n", C.c_int32), ("k", C.c_int32), ("ld_res", C.c_int32), ("ldo", C.c_int32), ("geglu", C.c_int32), ("dtype", C.c_int32),
    ]


class AaDpmStep(C.Structure):
    _fields_ = [
        ("eps_uncond", C.c_void_p), ("eps_text", C.c_void_p), ("latents", C.c_void_p), ("x0_prev", C.c_void_p),
        ("latents_lp", C.c_void_p), ("n", C.c_int64),
        ("guidance", C.c_float), ("sigma_s", C.c_float), ("alpha_s", C.c_float),
        ("c_x", C.c_float), ("c_d0", C.c_float), ("c_d1", C.c_float), ("dtype", C.c_int32),
    ]


class AaPackLatents(C.Structure):
    _fields_ = [
        ("sample", C.c_void_p), ("cond", C.c_void_p), ("mask", C.c_void_p), ("out", C.c_void_p),
        ("batch", C.c_int32), ("sample_batch", C.c_int32), ("cond_batch", C.c_int32), ("mask_batch", C.c_int32),
        ("channels", C.c_int32), ("frames", C.c_int32), ("hw", C.c_int32), ("dtype", C.c_int32), ("sample_dtype", C.c_int32),
    ]


class AaDpmStepTok(C.Structure):
    _fields_ = [
        ("eps_tokens", C.c_void_p), ("latents", C.c_void_p), ("x0_prev", C.c_void_p), ("latents_lp", C.c_void_p),
        ("next_t", C.c_void_p), ("next_t_count", C.c_int32), ("next_t_value", C.c_float),
        ("clips", C.c_int32), ("channels", C.c_int32), ("frames", C.c_int32), ("hw", C.c_int32),
        ("eps_ld", C.c_int32), ("guidance_on", C.c_int32),
        ("guidance", C.c_float), ("sigma_s", C.c_float), ("alpha_s", C.c_float),
        ("c_x", C.c_float), ("c_d0", C.c_float), ("c_d1", C.c_float), ("dtype", C.c_int32),
    ]


class AaBlend(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("y", C.c_void_p), ("rowvec", C.c_void_p), ("out", C.c_void_p), ("rows", C.c_int64),
        ("channels", C.c_int32), ("rowvec_div", C.c_int32), ("rowvec_mod", C.c_int32), ("rowvec_ld", C.c_int32),
        ("a", C.c_float), ("b", C.c_float), ("act", C.c_int32), ("dtype", C.c_int32),
    ]


class AaPackFrames(C.Structure):
    _fields_ = [
        ("src", C.c_void_p * 3), ("src_channels", C.c_int32 * 3), ("src_batch", C.c_int32 * 3), ("src_f32", C.c_int32 * 3),
        ("scale", C.c_void_p), ("scaled_src", C.c_int32), ("out", C.c_void_p),
        ("batch", C.c_int32), ("frames", C.c_int32), ("hw", C.c_int32), ("out_channels", C.c_int32), ("dtype", C.c_int32),
    ]


class AaEulerStepTok(C.Structure):
    _fields_ = [
        ("v_tokens", C.c_void_p), ("latents", C.c_void_p), ("guidance", C.c_void_p), ("next_t", C.c_void_p),
        ("next_t_count", C.c_int32), ("next_t_value", C.c_float), ("next_scale", C.c_void_p), ("next_scale_value", C.c_float),
        ("clips", C.c_int32), ("channels", C.c_int32), ("frames", C.c_int32), ("hw", C.c_int32), ("ld", C.c_int32),
        ("c_x", C.c_float), ("c_v", C.c_float), ("dtype", C.c_int32),
    ]


class AaDdimStepTok(C.Structure):
    _fields_ = [
        ("tokens", C.c_void_p), ("latents", C.c_void_p), ("latents_lp", C.c_void_p), ("noise", C.c_void_p), ("next_t", C.c_void_p),
        ("next_t_count", C.c_int32), ("next_t_value", C.c_float),
        ("clips", C.c_int32), ("channels", C.c_int32), ("frames", C.c_int32), ("hw", C.c_int32), ("ld", C.c_int32),
        ("guidance_on", C.c_int32), ("guidance", C.c_float), ("a_x", C.c_float), ("a_m", C.c_float),
        ("clip_on", C.c_int32), ("clip", C.c_float), ("eps_from_x0", C.c_int32),
        ("e_x", C.c_float), ("e_m", C.c_float), ("q_x", C.c_float), ("q_0", C.c_float),
        ("c_0", C.c_float), ("c_e", C.c_float), ("c_n", C.c_float), ("dtype", C.c_int32),
    ]


class AaUnipcStepTok(C.Structure):
    _fields_ = [
        ("tokens", C.c_void_p), ("latents", C.c_void_p), ("latents_lp", C.c_void_p), ("last_sample", C.c_void_p),
        ("hist1", C.c_void_p), ("hist2", C.c_void_p), ("hist3", C.c_void_p), ("next_t", C.c_void_p),
        ("next_t_count", C.c_int32), ("next_t_value", C.c_float),
        ("clips", C.c_int32), ("channels", C.c_int32), ("frames", C.c_int32), ("hw", C.c_int32), ("ld", C.c_int32),
        ("guidance_on", C.c_int32), ("guidance", C.c_float), ("a_x", C.c_float), ("a_m", C.c_float),
        ("corr_on", C.c_int32), ("q_l", C.c_float), ("q_1", C.c_float), ("q_2", C.c_float), ("q_3", C.c_float), ("q_n", C.c_float),
        ("p_x", C.c_float), ("p_0", C.c_float), ("p_1", C.c_float), ("p_2", C.c_float), ("dtype", C.c_int32),
    ]


class AaFreeU(C.Structure):
    _fields_ = [
        ("hidden", C.c_void_p), ("hidden_out", C.c_void_p), ("skip", C.c_void_p), ("skip_out", C.c_void_p), ("trig", C.c_void_p),
        ("images", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("c_hidden", C.c_int32), ("c_skip", C.c_int32),
        ("hidden_ld", C.c_int32), ("hidden_out_ld", C.c_int32), ("skip_ld", C.c_int32), ("skip_out_ld", C.c_int32),
        ("b", C.c_float), ("s", C.c_float), ("dtype", C.c_int32),
    ]


class AaCfgRescale(C.Structure):
    _fields_ = [
        ("tokens", C.c_void_p), ("out", C.c_void_p), ("factor", C.c_void_p),
        ("clips", C.c_int32), ("channels", C.c_int32), ("frames", C.c_int32), ("hw", C.c_int32), ("ld", C.c_int32), ("out_ld", C.c_int32),
        ("guidance", C.c_float), ("rescale", C.c_float), ("dtype", C.c_int32),
    ]


class AaApg(C.Structure):
    _fields_ = [
        ("tokens", C.c_void_p), ("out", C.c_void_p), ("momentum_buf", C.c_void_p), ("stats", C.c_void_p),
        ("clips", C.c_int32), ("channels", C.c_int32), ("frames", C.c_int32), ("hw", C.c_int32), ("ld", C.c_int32), ("out_ld", C.c_int32),
        ("guidance", C.c_float), ("eta", C.c_float), ("norm_threshold", C.c_float), ("momentum", C.c_float), ("dtype", C.c_int32),
    ]


AA_WINDOW_MAX = 64


class AaWindow(C.Structure):
    _fields_ = [
        ("window_frames", C.c_int32), ("frame", C.c_int32 * AA_WINDOW_MAX), ("weight", C.c_float * AA_WINDOW_MAX),
        ("first", C.c_int32 * AA_WINDOW_MAX), ("last", C.c_int32 * AA_WINDOW_MAX),
    ]


class AaWindowGather(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("dst", C.c_void_p),
        ("clips", C.c_int32), ("channels", C.c_int32), ("total_frames", C.c_int32), ("hw", C.c_int32),
        ("window", AaWindow),
    ]


class AaWindowMerge(C.Structure):
    _fields_ = [
        ("tokens", C.c_void_p), ("acc", C.c_void_p), ("merged", C.c_void_p),
        ("clips", C.c_int32), ("channels", C.c_int32), ("total_frames", C.c_int32), ("hw", C.c_int32), ("ld", C.c_int32), ("out_ld", C.c_int32),
        ("guidance_on", C.c_int32), ("guidance", C.c_float), ("dtype", C.c_int32),
        ("window", AaWindow),
    ]


class AaFreeInit(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("n0", C.c_void_p), ("z", C.c_void_p), ("out", C.c_void_p), ("mask", C.c_void_p), ("twiddle", C.c_void_p),
        ("volumes", C.c_int32), ("frames", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("a", C.c_float), ("s", C.c_float),
    ]


class AaKeepBlend(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("out", C.c_void_p), ("known", C.c_void_p), ("mask", C.c_void_p), ("noise", C.c_void_p),
        ("clips", C.c_int32), ("channels", C.c_int32), ("frames", C.c_int32), ("hw", C.c_int32),
        ("known_clips", C.c_int32), ("known_frames", C.c_int32), ("mask_clips", C.c_int32), ("mask_frames", C.c_int32),
        ("known_dtype", C.c_int32), ("mask_dtype", C.c_int32),
        ("a", C.c_float), ("s", C.c_float),
    ]


_I, _I32, _I64, _F, _V, _Z, _P = C.c_int, C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_size_t, C.POINTER


def _launch(desc):
    """int f(const Desc* d, void* stream)"""
    return _I, [_P(desc), _V]


# The C ABI, in the order of include/aa_mi355.h: name -> (restype, argtypes).  A new entry point is one row here
# (tests/test_abi.py holds the rows and the structures above against the header).
PROTOTYPES = {
    "aa_version": (_I, []),
    "aa_last_error": (C.c_char_p, []),
    "aa_conv_gemm_workspace": (_Z, [_P(AaConvGemm)]),
    "aa_conv_gemm": _launch(AaConvGemm),
    "aa_conv_gemm_group": (_I, [_P(_P(AaConvGemm)), _I32, _V]),
    "aa_conv_gemm_group_ok": (_I, [_P(_P(AaConvGemm)), _I32, _I32]),
    "aa_conv_gemm_launch_count": (_I, [_P(AaConvGemm)]),
    "aa_conv_gemm_tickets": (_I, [_P(AaConvGemm)]),
    "aa_conv_gemm_reduce_launches": (_I, [_P(AaConvGemm)]),
    "aa_conv_gemm_row_stats_parts": (_I, [_P(AaConvGemm)]),
    "aa_conv_gemm_row_coef_ok": (_I, [_P(AaConvGemm)]),
    "aa_ln_finalize": (_I, [_V, _I32, _V, _I64, _I32, _F, _V]),
    "aa_conv_gemm_tile_info": (_I, [_I, _P(_I32)]),
    "aa_conv_gemm_tile_flags": (_I, [_I]),
    "aa_conv_gemm_tile_ok": (_I, [_P(AaConvGemm), _I]),
    "aa_set_tile_override": (None, [_I]),
    "aa_groupnorm_workspace": (_Z, [_P(AaGroupNorm)]),
    "aa_set_groupnorm_two_pass": (None, [_I]),
    "aa_groupnorm_plan": (_I, [_P(AaGroupNorm), _P(_I32)]),
    "aa_groupnorm": (_I, [_P(AaGroupNorm), _V, _Z, _V]),
    "aa_groupnorm_coef": (_I, [_P(AaGroupNorm), _V, _Z, _V, _V]),
    "aa_layernorm": (_I, [_V, _V, _V, _V, _I64, _I32, _F, _I32, _V]),
    "aa_attention": _launch(AaAttention),
    "aa_seq_self_attention_ok": (_I, [_P(AaSeqSelfAttn)]),
    "aa_seq_self_attention": _launch(AaSeqSelfAttn),
    "aa_ff_fused_ok": (_I, [_P(AaFFFused)]),
    "aa_ff_fused": _launch(AaFFFused),
    "aa_linear_rows_ok": (_I, [_P(AaLinearRows)]),
    "aa_linear_rows": _launch(AaLinearRows),
    "aa_quant_rows_fp8": _launch(AaQuantRowsFp8),
    "aa_linear_fp8": _launch(AaLinearFp8),
    "aa_softmax_rows": (_I, [_V, _V, _I64, _I32, _I32, _I32, _I32, _V]),
    "aa_cfg_dpm_step": _launch(AaDpmStep),
    "aa_timestep_embedding": (_I, [_V, _V, _I32, _I32, _I32, _V]),
    "aa_pack_latents": _launch(AaPackLatents),
    "aa_cfg_dpm_step_tokens": _launch(AaDpmStepTok),
    "aa_blend": _launch(AaBlend),
    "aa_pack_frames": _launch(AaPackFrames),
    "aa_cfg_euler_step_tokens": _launch(AaEulerStepTok),
    "aa_cfg_ddim_step_tokens": _launch(AaDdimStepTok),
    "aa_cfg_unipc_step_tokens": _launch(AaUnipcStepTok),
    "aa_freeu_tokens": _launch(AaFreeU),
    "aa_cfg_rescale_workspace": (_Z, [_P(AaCfgRescale)]),
    "aa_cfg_rescale_tokens": (_I, [_P(AaCfgRescale), _V, _Z, _V]),
    "aa_apg_workspace": (_Z, [_P(AaApg)]),
    "aa_apg_tokens": (_I, [_P(AaApg), _V, _Z, _V]),
    "aa_window_gather_latents": _launch(AaWindowGather),
    "aa_window_merge_tokens": _launch(AaWindowMerge),
    "aa_freeinit_workspace": (_Z, [_P(AaFreeInit)]),
    "aa_freeinit_mix": (_I, [_P(AaFreeInit), _V, _Z, _V]),
    "aa_keep_blend": _launch(AaKeepBlend),
}
SYMBOLS = tuple(PROTOTYPES)

DEFAULT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libaa_mi355.so")


def bind(path: str) -> C.CDLL:
    """dlopen `path` and attach the prototypes of include/aa_mi355.h."""
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -m animate_anything_amd.build` "
                           "(hipcc --offload-arch=gfx950); this package has no fallback backend")
    lib = C.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        if not hasattr(lib, name):
            raise RuntimeError(f"{path} does not export {name}")
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


_lib = None
_host_pointers_ok = False     # only the emulator build (tests/emu) accepts host memory


def get() -> C.CDLL:
    global _lib
    if _lib is None:
        _lib = bind(os.environ.get("AA_LIBRARY") or DEFAULT_PATH)      # AA_LIBRARY: another BUILD of this library (A/B and probe variants of build.py)
    return _lib


def host_pointers_ok() -> bool:
    return _host_pointers_ok


class use_library:
    """Test hook: route ops through another build of the same C ABI (the CPU SIMT emulator of
    tests/emu).  Never used by the product path."""

    def __init__(self, lib, host_pointers=False):
        self.lib, self.host = lib, host_pointers

    def __enter__(self):
        global _lib, _host_pointers_ok
        self.prev = (_lib, _host_pointers_ok)
        _lib, _host_pointers_ok = self.lib, self.host
        return self.lib

    def __exit__(self, *a):
        global _lib, _host_pointers_ok
        _lib, _host_pointers_ok = self.prev
