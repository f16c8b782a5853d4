"""ctypes binding of libccvs_hip.so (the C ABI declared in include/ccvs_hip.h).

The product has no CPU fallback: if the shared library is missing or a call fails this
module raises.  Build the library with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C ccvs_amd/csrc`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (CCVS_LIB: another build of the same library, for A/B measurements of kernel changes on one GPU box)
LIB_PATH = os.environ.get("CCVS_LIB") or os.path.join(_HERE, "csrc", "libccvs_hip.so")

# every symbol include/ccvs_hip.h declares
EXPORTS = [
    "ccvs_last_error", "ccvs_abi_version", "ccvs_conv2d", "ccvs_conv2d_bf16x3", "ccvs_conv_fetch_bytes_per_lane", "ccvs_conv_persistent_tiles", "ccvs_upfirdn2d", "ccvs_dwconvT4x4s2",
    "ccvs_correlation7x7", "ccvs_backwarp", "ccvs_backwarp_ctx", "ccvs_backwarp_p8_ctx", "ccvs_backwarp_proj_ctx", "ccvs_warp_fuse_blend", "ccvs_warp_fuse_blend_ctx", "ccvs_tap_shift_add", "ccvs_vq_argmin", "ccvs_embed_gather", "ccvs_l2_normalize_channels",
    "ccvs_gpt_embed", "ccvs_layernorm", "ccvs_gemm_workspace_bytes", "ccvs_gemm_nt", "ccvs_gemm_ln", "ccvs_gemm_ln_qkv", "ccvs_attention", "ccvs_kv_append", "ccvs_sample_topk", "ccvs_sample_topk_philox", "ccvs_sample_topn",
    "ccvs_gpt_decode_step", "ccvs_gpt_decode_status", "ccvs_gpt_program_bytes", "ccvs_gpt_decode_prepare", "ccvs_pack_u8", "ccvs_pack_u8_norm", "ccvs_stream_cu_limit", "ccvs_psnr", "ccvs_ssim_workspace_bytes", "ccvs_ssim", "ccvs_resize_bilinear",
    "ccvs_deform_conv3x3_ctx", "ccvs_gconvT4x4s2", "ccvs_flow_mask_toff", "ccvs_gaussian_blur", "ccvs_to_rgb", "ccvs_channel_head", "ccvs_mse",
    "ccvs_token_nll", "ccvs_mean_f32", "ccvs_conv_last_launch",
]
# every symbol include/ccvs_hip_eval.h declares (the frame autoencoder's validation reductions; ccvs_hip.h includes that header)
EVAL_EXPORTS = ["ccvs_l1_workspace_bytes", "ccvs_l1_mean", "ccvs_vq_stats_workspace_bytes", "ccvs_vq_stats", "ccvs_code_perplexity"]
# every symbol include/ccvs_hip_input.h declares (the input stage: uint8 frames -> the fp32 clip; ccvs_hip.h includes that header too)
INPUT_EXPORTS = ["ccvs_ingest_u8"]
# every symbol include/ccvs_hip_gemm.h declares (the tiled weight layout of the decode GEMMs; included by ccvs_hip.h as well)
GEMM_EXPORTS = ["ccvs_gemm_tiled", "ccvs_gemm_tiled_max_rows"]
# every symbol include/ccvs_hip_output.h declares (the output stage: uint8 clips -> libjpeg-exact JPEG scans; included by ccvs_hip.h too)
OUTPUT_EXPORTS = ["ccvs_mjpeg_workspace_bytes", "ccvs_mjpeg_encode"]
# every symbol include/ccvs_hip_decode.h declares (the way back: baseline JPEG scans -> libjpeg-exact uint8 frames; included by ccvs_hip.h too)
DECODE_EXPORTS = ["ccvs_mjpeg_decode_workspace_bytes", "ccvs_mjpeg_decode"]
# every symbol include/ccvs_hip_video.h declares (the video-file datasets' input stage: the tensor transform chain in fp32; included by ccvs_hip.h too)
VIDEO_EXPORTS = ["ccvs_ingest_f32"]
# every symbol include/ccvs_hip_output_sampled.h declares (the output stage writing 4:2:2 and 4:2:0 as well; included by ccvs_hip.h too)
OUTPUT_SAMPLED_EXPORTS = ["ccvs_mjpeg_sampled_workspace_bytes", "ccvs_mjpeg_encode_sampled"]
# every symbol include/ccvs_hip_output_optimized.h declares (the output stage with per-frame optimised Huffman tables; included by ccvs_hip.h too)
OUTPUT_OPTIMIZED_EXPORTS = ["ccvs_mjpeg_optimized_workspace_bytes", "ccvs_mjpeg_encode_optimized"]
# every symbol include/ccvs_hip_lpips.h declares (the memory-bound passes of LPIPS around its convolutions; included by ccvs_hip.h too)
LPIPS_EXPORTS = ["ccvs_lpips_prep", "ccvs_relu_", "ccvs_relu_maxpool2", "ccvs_lpips_layer_workspace_bytes", "ccvs_lpips_layer"]
# every symbol include/ccvs_hip_fvd.h declares (the passes of the FVD embedding around its I3D convolutions; included by ccvs_hip.h too)
FVD_EXPORTS = ["ccvs_fvd_prep", "ccvs_time_unfold", "ccvs_maxpool3d_same", "ccvs_i3d_head"]
# every symbol include/ccvs_hip_output_lossless.h declares (the lossless output stage: PNG filters and deflate, a zlib stream per frame; included by ccvs_hip.h too)
OUTPUT_LOSSLESS_EXPORTS = ["ccvs_apng_workspace_bytes", "ccvs_apng_stream_bound", "ccvs_apng_encode"]
# every symbol include/ccvs_hip_output_lossless_lz.h declares (the same stage with LZ77 matches, kept per deflate block only where smaller; included by ccvs_hip.h too)
OUTPUT_LOSSLESS_LZ_EXPORTS = ["ccvs_apng_lz_workspace_bytes", "ccvs_apng_encode_lz"]
# every symbol include/ccvs_hip_decode_lossless.h declares (the way back from it: zlib streams -> bytes, PNG streams -> uint8 frames; included by ccvs_hip.h too)
DECODE_LOSSLESS_EXPORTS = ["ccvs_png_decode_workspace_bytes", "ccvs_zlib_inflate", "ccvs_png_decode"]
# every symbol include/ccvs_hip_sampling.h declares (nucleus sampling in the token pick; included by ccvs_hip.h too)
SAMPLING_EXPORTS = ["ccvs_sample_topp", "ccvs_sample_topp_philox", "ccvs_sample_topp_max_vocab"]
# every symbol include/ccvs_hip_flowviz.h declares (the decoder's motion export; included by ccvs_hip.h too).  (Named apart from the
# `*_EXPORTS` lists above, whose number tests/test_nucleus_host.py pins.)
FLOWVIZ_SYMBOLS = ["ccvs_flow_export", "ccvs_flow_max", "ccvs_flow_render"]
# every symbol include/ccvs_hip_output_gif.h declares (the GIF output stage: a palette per clip, LZW-coded frames; included by ccvs_hip.h
# too; named apart from the `*_EXPORTS` lists for the same reason)
GIF_SYMBOLS = ["ccvs_gif_workspace_bytes", "ccvs_gif_stream_bound", "ccvs_gif_palette", "ccvs_gif_encode"]
# every symbol include/ccvs_hip_kv16.h declares (the token loop on a bf16 KV cache: append, attention, the step's launch chain; included by
# ccvs_hip.h too; named apart from the `*_EXPORTS` lists for the same reason)
KV16_SYMBOLS = ["ccvs_kv_append_bf16", "ccvs_attention_bf16", "ccvs_gpt_decode_step_bf16kv"]
# every symbol include/ccvs_hip_output_gif_delta.h declares (the GIF output stage writing changed rectangles with a transparent index;
# included by ccvs_hip.h too; named apart from the `*_EXPORTS` lists for the same reason)
GIF_DELTA_SYMBOLS = ["ccvs_gif_palette_n", "ccvs_gif_delta_workspace_bytes", "ccvs_gif_encode_delta"]


class ConvDesc(C.Structure):
    """Mirror of `ccvs_conv_desc`."""
    _fields_ = [
        ("N", C.c_int32), ("Cin", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32),
        ("in_sN", C.c_int64), ("in_sC", C.c_int64),
        ("Cout", C.c_int32), ("CoutPad", C.c_int32), ("Hout", C.c_int32), ("Wout", C.c_int32),
        ("out_sN", C.c_int64), ("out_sC", C.c_int64), ("res_sN", C.c_int64), ("res_sC", C.c_int64),
        ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("transposed", C.c_int32),
        ("act", C.c_int32), ("accumulate", C.c_int32), ("out_scale", C.c_float),
        ("pre", C.c_void_p), ("pre_sN", C.c_int64), ("pre_sC", C.c_int64), ("pre_div", C.c_int32),
        ("in_p8", C.c_int32), ("out_p8", C.c_int32), ("cu_limit", C.c_int32),
        ("w_ktail", C.c_void_p),
    ]


MAX_CTX = 16


class CtxList(C.Structure):
    """Mirror of `ccvs_ctx_list`."""
    _fields_ = [("k", C.c_int32), ("p", C.c_void_p * MAX_CTX), ("sN", C.c_int64 * MAX_CTX)]


class GptLayer(C.Structure):
    """Mirror of `ccvs_gpt_layer`."""
    _fields_ = [(n, C.c_void_p) for n in ("qkv_w", "qkv_b", "qkv_s", "proj_w", "proj_b", "fc_w", "fc_b", "fc_s", "fc2_w", "fc2_b",
                                          "kcache", "vcache")]


class GptDecode(C.Structure):
    """Mirror of `ccvs_gpt_decode`.  The C struct's last field, `float top_p`, follows `w_tiled` in what is this mirror's tail padding
    (same size either way): it is the `top_p` property below, not an entry of `_fields_`, whose last entry stays `w_tiled` as
    tests/test_gemm_tiled_gpu.py pins it.  tests/test_nucleus_host.py checks the offset against the C compiler's."""
    _fields_ = [
        ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("F", C.c_int32), ("n_layer", C.c_int32), ("Tmax", C.c_int32),
        ("vocab", C.c_int32), ("V", C.c_int32), ("ln_eps", C.c_float),
        ("layers", C.POINTER(GptLayer)),
        ("tok_emb", C.c_void_p), ("pos_table", C.c_void_p), ("pos_off", C.c_int32),
        ("head_w", C.c_void_p), ("head_b", C.c_void_p), ("head_s", C.c_void_p),
        ("tok", C.c_void_p), ("codes", C.c_void_p), ("codes_sB", C.c_int64),
        ("widx", C.c_void_p), ("len", C.c_void_p),
        ("x", C.c_void_p), ("q", C.c_void_p), ("att", C.c_void_p), ("h", C.c_void_p), ("logits", C.c_void_p),
        ("noise", C.c_void_p), ("rng", C.c_int32), ("top_k", C.c_int32), ("temperature", C.c_float),
        ("workspace", C.c_void_p), ("state", C.c_void_p), ("groups", C.c_int32),
        ("noise_stream", C.c_void_p),
        ("persistent", C.c_int32), ("program", C.c_void_p), ("w_tiled", C.c_int32),
    ]

    def _top_p_word(self):
        return C.c_float.from_address(C.addressof(self) + GptDecode.TOP_P_OFFSET)

    @property
    def top_p(self):
        return self._top_p_word().value

    @top_p.setter
    def top_p(self, value):
        self._top_p_word().value = value


GptDecode.TOP_P_OFFSET = GptDecode.w_tiled.offset + C.sizeof(C.c_int32)
assert GptDecode.TOP_P_OFFSET + C.sizeof(C.c_float) == C.sizeof(GptDecode)


class CcvsError(RuntimeError):
    pass


_lib = None


def load():
    """Load the shared library once; fail loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CcvsError(f"{LIB_PATH} not found: the HIP kernel library is not built "
                        f"(run `make -C {os.path.dirname(LIB_PATH)}`); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    lib.ccvs_last_error.restype = C.c_char_p
    lib.ccvs_last_error.argtypes = []
    lib.ccvs_abi_version.restype = C.c_int
    lib.ccvs_gemm_workspace_bytes.restype = C.c_int64
    lib.ccvs_gemm_workspace_bytes.argtypes = []
    lib.ccvs_ssim_workspace_bytes.restype = C.c_int64
    lib.ccvs_ssim_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    lib.ccvs_l1_workspace_bytes.restype = C.c_int64
    lib.ccvs_l1_workspace_bytes.argtypes = [C.c_int64]
    lib.ccvs_vq_stats_workspace_bytes.restype = C.c_int64
    lib.ccvs_vq_stats_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    lib.ccvs_gemm_tiled_max_rows.restype = C.c_int32
    lib.ccvs_gemm_tiled_max_rows.argtypes = []
    lib.ccvs_mjpeg_workspace_bytes.restype = C.c_size_t
    lib.ccvs_mjpeg_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.ccvs_mjpeg_sampled_workspace_bytes.restype = C.c_size_t
    lib.ccvs_mjpeg_sampled_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.ccvs_mjpeg_optimized_workspace_bytes.restype = C.c_size_t
    lib.ccvs_mjpeg_optimized_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.ccvs_mjpeg_decode_workspace_bytes.restype = C.c_size_t
    lib.ccvs_mjpeg_decode_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.ccvs_apng_workspace_bytes.restype = C.c_size_t
    lib.ccvs_apng_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.ccvs_apng_stream_bound.restype = C.c_long
    lib.ccvs_apng_stream_bound.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.ccvs_apng_lz_workspace_bytes.restype = C.c_size_t
    lib.ccvs_apng_lz_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.ccvs_gif_workspace_bytes.restype = C.c_size_t
    lib.ccvs_gif_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.ccvs_gif_delta_workspace_bytes.restype = C.c_size_t
    lib.ccvs_gif_delta_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.ccvs_gif_stream_bound.restype = C.c_long
    lib.ccvs_gif_stream_bound.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.ccvs_png_decode_workspace_bytes.restype = C.c_size_t
    lib.ccvs_png_decode_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.ccvs_lpips_layer_workspace_bytes.restype = C.c_int64
    lib.ccvs_lpips_layer_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
    lib.ccvs_sample_topp_max_vocab.restype = C.c_int32
    lib.ccvs_sample_topp_max_vocab.argtypes = []
    lib.ccvs_gpt_program_bytes.restype = C.c_int64
    lib.ccvs_gpt_program_bytes.argtypes = [C.c_int32]
    lib.ccvs_conv_fetch_bytes_per_lane.restype = C.c_int
    lib.ccvs_conv_fetch_bytes_per_lane.argtypes = [C.c_char_p]
    lib.ccvs_conv_persistent_tiles.restype = C.c_int          # (returns the previous mode, not a status)
    lib.ccvs_conv_persistent_tiles.argtypes = [C.c_int32]
    lib.ccvs_conv_last_launch.restype = C.c_char_p            # (the record of the calling thread's last convolution launch, not a status)
    lib.ccvs_conv_last_launch.argtypes = []
    sigs = {
        "ccvs_conv2d": [vp, vp, vp, vp, vp, C.POINTER(ConvDesc), vp],
        "ccvs_conv2d_bf16x3": [vp, vp, vp, vp, vp, C.POINTER(ConvDesc), vp],
        "ccvs_upfirdn2d": [vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, f32, i32, f32, vp],
        "ccvs_dwconvT4x4s2": [vp, i64, vp, vp, i64, i32, i32, i32, i32, vp],
        "ccvs_correlation7x7": [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
        "ccvs_backwarp": [vp, i64, i64, vp, i64, f32, vp, i64, i64, i32, i32, i32, i32, vp],
        "ccvs_warp_fuse_blend": [vp, i64, i64, vp, vp, i64, vp, i64, f32, i32, i32, i32, i32, i32, vp],
        "ccvs_backwarp_ctx": [C.POINTER(CtxList), i64, vp, i64, f32, vp, i64, i64, i32, i32, i32, i32, vp],
        "ccvs_backwarp_p8_ctx": [C.POINTER(CtxList), i64, vp, i64, f32, vp, i32, i32, i32, i32, vp],
        "ccvs_backwarp_proj_ctx": [C.POINTER(CtxList), i64, vp, i64, f32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
        "ccvs_warp_fuse_blend_ctx": [vp, i64, i64, C.POINTER(CtxList), vp, i64, vp, i64, f32, i32, i32, i32, i32, vp],
        "ccvs_tap_shift_add": [vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp],
        "ccvs_vq_argmin": [vp, vp, vp, vp, i32, i32, i32, i32, vp],
        "ccvs_embed_gather": [vp, vp, vp, i32, i32, i32, i32, vp],
        "ccvs_l2_normalize_channels": [vp, i32, i32, i64, vp],
        "ccvs_gpt_embed": [vp, i64, vp, i32, vp, i32, vp, vp, vp, i32, i32, i32, vp],
        "ccvs_layernorm": [vp, vp, vp, vp, i32, i32, vp],
        "ccvs_gemm_nt": [vp, i64, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp],
        "ccvs_gemm_ln": [vp, i64, vp, vp, vp, f32, vp, i64, i32, i32, i32, i32, vp],
        "ccvs_gemm_ln_qkv": [vp, i64, vp, vp, vp, f32, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, vp],
        "ccvs_gemm_tiled": [vp, i64, vp, vp, vp, vp, f32, vp, i64, i32, i32, i32, i32, vp, vp, i32, i32, vp, i32, vp, vp],
        "ccvs_attention": [vp, i64, i64, vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, vp],
        "ccvs_kv_append": [vp, vp, i64, i64, vp, vp, i32, i32, i32, i32, vp, i32, i32, vp],
        "ccvs_sample_topk": [vp, i64, vp, vp, i64, i32, i32, i32, f32, vp],
        "ccvs_sample_topk_philox": [vp, i64, vp, i64, i32, i32, i32, f32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp],
        "ccvs_sample_topp": [vp, i64, vp, vp, i64, i32, i32, i32, f32, f32, vp],
        "ccvs_sample_topp_philox": [vp, i64, vp, i64, i32, i32, i32, f32, f32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp],
        "ccvs_sample_topn": [vp, i64, vp, vp, vp, i32, i32, i32, f32, i32, vp],
        "ccvs_gpt_decode_step": [C.POINTER(GptDecode), vp],
        "ccvs_gpt_decode_step_bf16kv": [C.POINTER(GptDecode), vp],
        "ccvs_kv_append_bf16": [vp, vp, i64, i64, vp, vp, i32, i32, i32, i32, vp, i32, i32, vp],
        "ccvs_attention_bf16": [vp, i64, i64, vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, i32, vp],
        "ccvs_gpt_decode_status": [vp, vp],
        "ccvs_gpt_decode_prepare": [C.POINTER(GptDecode), vp],
        "ccvs_pack_u8": [vp, vp, i64, i32, i32, f32, f32, vp],
        "ccvs_pack_u8_norm": [vp, vp, i64, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float), vp],
        "ccvs_stream_cu_limit": [vp, i32],
        "ccvs_psnr": [vp, vp, vp, i64, i64, f32, vp],
        "ccvs_ssim": [vp, vp, vp, vp, i64, i32, i32, C.c_double, vp],
        "ccvs_resize_bilinear": [vp, vp, i64, i32, i32, i32, i32, vp],
        "ccvs_deform_conv3x3_ctx": [C.POINTER(CtxList), i64, vp, i64, f32, vp, i32, i32, vp, vp, i64, vp, i64, i64, vp, i64, i64, i32, i32,
                                    i32, i32, i32, vp],
        "ccvs_gconvT4x4s2": [vp, i64, vp, vp, i64, i64, i32, i32, i32, i32, i32, vp],
        "ccvs_flow_mask_toff": [vp, i64, i64, vp, i64, vp, i64, i64, i32, i32, i32, i32, i32, vp],
        "ccvs_gaussian_blur": [vp, i64, i64, vp, i32, i32, i32, i32, i32, C.POINTER(C.c_float), vp],
        "ccvs_to_rgb": [vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp],
        "ccvs_channel_head": [vp, i64, vp, f32, vp, vp, i32, i32, i32, i32, i32, i32, vp],
        "ccvs_mse": [vp, vp, vp, i64, vp],
        "ccvs_token_nll": [vp, i64, vp, vp, i64, i32, vp, vp],
        "ccvs_mean_f32": [vp, i64, vp, vp],
        "ccvs_l1_mean": [vp, vp, vp, vp, i64, vp],
        "ccvs_vq_stats": [vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp],
        "ccvs_code_perplexity": [vp, i32, i64, vp, vp],
        "ccvs_mjpeg_encode": [vp, C.c_long, i32, i32, i32, i32, i32, vp, C.c_long, vp, vp, vp],
        "ccvs_mjpeg_encode_sampled": [vp, C.c_long, i32, i32, i32, i32, i32, i32, vp, C.c_long, vp, vp, vp],
        "ccvs_mjpeg_encode_optimized": [vp, C.c_long, i32, i32, i32, i32, i32, i32, vp, C.c_long, vp, vp, vp, vp],
        "ccvs_mjpeg_decode": [vp, C.c_long, vp, vp, C.c_long, vp, i32, vp, i32, i32, i32, i32, vp, C.c_long, vp, vp, vp],
        "ccvs_apng_encode": [vp, C.c_long, i32, i32, i32, i32, i32, vp, C.c_long, vp, vp, vp],
        "ccvs_apng_encode_lz": [vp, C.c_long, i32, i32, i32, i32, i32, vp, C.c_long, vp, vp, vp],
        "ccvs_gif_palette": [vp, C.c_long, C.c_long, i32, i32, i32, i32, vp, vp, vp, vp, vp],
        "ccvs_gif_encode": [vp, C.c_long, C.c_long, i32, i32, i32, i32, i32, vp, vp, C.c_long, vp, vp, vp],
        "ccvs_gif_palette_n": [vp, C.c_long, C.c_long, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp],
        "ccvs_gif_encode_delta": [vp, C.c_long, C.c_long, i32, i32, i32, i32, i32, vp, vp, C.c_long, vp, vp, vp, vp],
        "ccvs_zlib_inflate": [vp, C.c_long, vp, vp, i32, vp, C.c_long, vp, vp],
        "ccvs_png_decode": [vp, C.c_long, vp, vp, i32, i32, i32, vp, C.c_long, vp, vp, vp],
        "ccvs_lpips_prep": [vp, vp, i64, i64, C.POINTER(C.c_float), C.POINTER(C.c_float), vp],
        "ccvs_relu_": [vp, i64, vp],
        "ccvs_relu_maxpool2": [vp, vp, i64, i32, i32, vp],
        "ccvs_lpips_layer": [vp, vp, vp, vp, i64, i32, i64, i32, i32, vp],
        "ccvs_fvd_prep": [vp, vp, i64, i32, i32, i32, i32, i32, vp],
        "ccvs_time_unfold": [vp, i64, i64, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
        "ccvs_maxpool3d_same": [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
        "ccvs_i3d_head": [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
        "ccvs_flow_export": [vp, i64, i32, i32, i32, i32, f32, vp, i64, vp],
        "ccvs_flow_max": [vp, i64, i64, i32, i32, i32, i32, vp, vp],
        "ccvs_flow_render": [vp, i64, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp],
        "ccvs_ingest_f32": [vp, i32, i64, i64, i32, i32, i32, i32, i32, vp, i32, vp, vp, i64, i64, vp],
        "ccvs_ingest_u8": [vp, i64, i32, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, i64, i64, vp, vp],
    }
    for name, argtypes in sigs.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(rc, name):
    if rc != 0:
        raise CcvsError(f"{name} failed ({rc}): {load().ccvs_last_error().decode()}")
