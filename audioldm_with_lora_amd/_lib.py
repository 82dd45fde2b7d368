"""ctypes binding of libaldm_hip.so (the C-ABI declared in include/aldm_hip.h).

The product path has NO fallback: if the HIP library is missing or a call fails, this raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ALDM_LIB") or os.path.join(_HERE, "libaldm_hip.so")   # ALDM_LIB: diagnostic builds only

ACT_NONE, ACT_SILU, ACT_LRELU, ACT_TANH, ACT_GELU = 0, 1, 2, 3, 4
OUT_BF16, OUT_F32 = 0, 1
TILE_AUTO, TILE_128x128, TILE_64x64, TILE_128x64, TILE_64x128 = 0, 1, 2, 3, 4    # ALDM_TILE_* (igemm_plan.TILES says what each one is)
TILE_128x128_W8, TILE_HALO_128x128, TILE_HALO_64x128, TILE_256x128_W8, TILE_64x128_W8, TILE_128x64_W8 = 6, 7, 8, 9, 10, 11
TILE_256x128_WS, TILE_64x128_WS, TILE_128x64_WS, TILE_HALO_128x128_WS, TILE_HALO_64x128_WS = 12, 13, 14, 15, 16
EPI_AUTO, EPI_LDS, EPI_DIRECT = 0, 0x10, 0x20                    # aldm_igemm_t.xcd_map bits 4-5: form of the standard epilogue
DEFER_ROWMAJOR, DEFER_PLANAR, DEFER_WRITE_THROUGH = 1, 2, 4     # aldm_igemm_t.defer_reduce flags
SLAB_ROWMAJOR, SLAB_PLANAR = 0, 1                               # slab layout as aldm_groupnorm_partials_layout is told it


class IgemmArgs(C.Structure):
    """Mirror of aldm_igemm_t (include/aldm_hip.h) -- field order and types must match exactly."""
    _fields_ = [
        ("x", C.c_void_p), ("x2", C.c_void_p),
        ("B", C.c_int), ("IH", C.c_int), ("IW", C.c_int), ("Cin", C.c_int), ("Cin2", C.c_int),
        ("UH", C.c_int), ("UW", C.c_int),
        ("in_dilate", C.c_int),
        ("w", C.c_void_p),
        ("Kpad", C.c_int),
        ("KH", C.c_int), ("KW", C.c_int), ("stride_h", C.c_int), ("stride_w", C.c_int),
        ("pad_h", C.c_int), ("pad_w", C.c_int), ("dil_h", C.c_int), ("dil_w", C.c_int),
        ("OH", C.c_int), ("OW", C.c_int), ("Cout", C.c_int),
        ("in_act", C.c_int), ("in_slope", C.c_float),
        ("ln_s", C.c_void_p), ("ln_sa", C.c_void_p), ("ln_ca", C.c_void_p), ("ln_eps", C.c_float),
        ("lora_a", C.c_void_p), ("lora_b", C.c_void_p),
        ("Rp", C.c_int),
        ("lora_t_out", C.c_void_p),
        ("bias", C.c_void_p), ("rowbias", C.c_void_p),
        ("rowbias_ld", C.c_int),
        ("geglu", C.c_int),
        ("out_act", C.c_int), ("out_slope", C.c_float),
        ("res", C.c_void_p), ("res2", C.c_void_p),
        ("alpha", C.c_float),
        ("post_act", C.c_int), ("post_slope", C.c_float), ("out2", C.c_void_p),
        ("out", C.c_void_p), ("out_dtype", C.c_int), ("out_ld", C.c_int),
        ("out_batch_stride", C.c_longlong),
        ("out_pix_stride", C.c_int), ("out_pix_offset", C.c_int),
        ("vt", C.c_void_p), ("vt_col0", C.c_int), ("vt_ld", C.c_int), ("vt_batch_stride", C.c_longlong),
        ("splits", C.c_int), ("workspace", C.c_void_p),
        ("tile", C.c_int),
        ("ring", C.c_int),
        ("defer_reduce", C.c_int),
        ("rowstat_out", C.c_void_p), ("ln_parts", C.c_void_p), ("ln_nparts", C.c_int),
        ("qstat_out", C.c_void_p),
        ("x3", C.c_void_p), ("x4", C.c_void_p), ("Cin3", C.c_int), ("Cin4", C.c_int),
        ("vt_dual", C.c_int),
        ("gnin_gamma", C.c_void_p), ("gnin_beta", C.c_void_p), ("gnin_q1", C.c_void_p), ("gnin_q2", C.c_void_p),
        ("gnin_bm1", C.c_int), ("gnin_tpi1", C.c_int), ("gnin_bm2", C.c_int), ("gnin_tpi2", C.c_int),
        ("gnin_groups", C.c_int), ("gnin_act", C.c_int), ("gnin_eps", C.c_float),
        ("xcd_map", C.c_int),
        ("lora_gate", C.c_void_p), ("gate_rows", C.c_int),
    ]


class IgemmVariant(C.Structure):
    """Mirror of aldm_igemm_variant_t: the kernel aldm_igemm would run (aldm_igemm_variant; no GPU needed)."""
    _fields_ = [(n, C.c_int) for n in ("family", "tile", "bm", "bn", "wm", "wn", "rp", "vt", "gate", "ring", "epi", "nl", "rs", "hp", "gnin",
                                       "ext", "transposed", "splits", "kt_per_split", "direct", "tiles_m", "tiles_n")] + \
               [("grid", C.c_uint), ("block", C.c_uint), ("lds", C.c_uint), ("name", C.c_char * 192)]


class IgemmTileInfo(C.Structure):
    """Mirror of aldm_igemm_tile_info_t: one row of the library's tile table (aldm_igemm_tile_info)."""
    _fields_ = [("tile", C.c_int), ("kind", C.c_int), ("bm", C.c_int), ("bn", C.c_int), ("wm", C.c_int), ("wn", C.c_int), ("blocks", C.c_int),
                ("rings", C.c_uint), ("ring", C.c_int), ("ring_lora", C.c_int), ("halo_rows", C.c_int), ("halo_rows_fused", C.c_int)]


IGEMM_TILE_KINDS = ("w4", "w8", "ws", "halo", "halo-ws")              # ALDM_IGEMM_KIND_*, as igemm_plan.Tile.kind spells them
IGEMM_FAMILIES = ("igemm_kernel", "igemm_pipe_kernel", "igemm_ws_kernel", "igemm_halo_kernel", "igemm_halo_ws_kernel")   # ALDM_IGEMM_*


class PgemmArgs(C.Structure):
    """Mirror of aldm_pgemm_t (include/aldm_hip.h) -- field order and types must match exactly."""
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p),
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("bias", C.c_void_p),
        ("ln_s", C.c_void_p), ("ln_sa", C.c_void_p), ("ln_ca", C.c_void_p), ("ln_eps", C.c_float),
        ("ln_parts", C.c_void_p), ("ln_nparts", C.c_int),
        ("lora_a", C.c_void_p), ("lora_b", C.c_void_p),
        ("Rp", C.c_int), ("ranks_used", C.c_int),
        ("geglu", C.c_int),
        ("res", C.c_void_p),
        ("out", C.c_void_p), ("out_ld", C.c_int),
        ("vt", C.c_void_p), ("vt_col0", C.c_int), ("vt_ld", C.c_int), ("vt_batch_stride", C.c_longlong), ("OHW", C.c_int),
        ("rowstat_out", C.c_void_p),
        ("mi", C.c_int), ("nt", C.c_int), ("tiles_per_range", C.c_int),
        ("max_ranges", C.c_int),
        ("waves", C.c_int),
        ("lora_t_out", C.c_void_p),
        ("vt_dual", C.c_int),
        ("lora_gate", C.c_void_p), ("gate_rows", C.c_int),
    ]


class WindowPlanArgs(C.Structure):
    """Mirror of aldm_window_plan_t (include/aldm_hip.h) -- field order and types must match exactly."""
    _fields_ = [
        ("offset", C.c_void_p), ("cover", C.c_void_p), ("weight", C.c_void_p),
        ("K", C.c_int), ("KC", C.c_int), ("rows", C.c_int), ("hw", C.c_int),
        ("offset_elems", C.c_longlong), ("cover_elems", C.c_longlong), ("weight_elems", C.c_longlong),
    ]


# name -> (restype, argtypes): every symbol include/aldm_hip.h declares
PROTOTYPES = {
    "aldm_version": (C.c_char_p, []),
    "aldm_last_error": (C.c_char_p, []),
    "aldm_igemm": (C.c_int, [C.POINTER(IgemmArgs), C.c_void_p]),
    "aldm_igemm_workspace_bytes": (C.c_size_t, [C.POINTER(IgemmArgs)]),
    "aldm_igemm_effective_splits": (C.c_int, [C.POINTER(IgemmArgs)]),
    "aldm_igemm_epilogue_form": (C.c_int, [C.POINTER(IgemmArgs)]),
    "aldm_igemm_variant": (C.c_int, [C.POINTER(IgemmArgs), C.POINTER(IgemmVariant)]),
    "aldm_igemm_tile_info": (C.c_int, [C.c_int, C.POINTER(IgemmTileInfo)]),
    "aldm_pgemm_supported": (C.c_int, [C.c_int]),
    "aldm_pgemm_plan": (C.c_int, [C.POINTER(PgemmArgs)]),
    "aldm_pgemm": (C.c_int, [C.POINTER(PgemmArgs), C.c_void_p]),
    "aldm_groupnorm_partials": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_groupnorm_partials_layout": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                                 C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "aldm_igemm_slab_offset": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "aldm_groupnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                 C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_groupnorm_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "aldm_gn_silu_conv3x3_small": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_layernorm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                 C.c_void_p]),
    "aldm_attention": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong,
                                 C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    "aldm_attention_prescaled": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "aldm_attn_block64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p]),
    "aldm_attn_block64_fp8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p]),
    # the block kernels with a per-sample gate table on the LoRA columns (multi-adapter routing): same list + lora_gate
    "aldm_attn_block64_gated": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "aldm_attn_block64_fp8_gated": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "aldm_attn_block256_gated": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "aldm_attn_block256": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p]),
    "aldm_hifigan_respair_supported": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "aldm_hifigan_respair": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "aldm_conv1d_to1": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_attention_wide": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong,
                                      C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "aldm_attention_fp8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    "aldm_attention_varlen": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p]),
    "aldm_embed_layernorm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_attention_lse": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p]),
    "aldm_attention_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "aldm_groupnorm_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "aldm_groupnorm_bwd_partials": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "aldm_layernorm_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "aldm_geglu_fwd": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_geglu_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_add_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "aldm_upsample_nearest_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p]),
    "aldm_tn_small": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_tn_batched": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "aldm_lora_pack": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "aldm_transpose_tokens": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_mse_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aldm_mse_grad_snr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                    C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aldm_softmax_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int,
                                    C.c_void_p]),
    "aldm_timestep_embedding": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_silu": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "aldm_nchw_f32_to_nhwc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "aldm_nhwc_to_nchw_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_f32_to_bf16": (C.c_int, [C.c_void_p, C.c_longlong, C.c_float, C.c_void_p, C.c_void_p]),
    "aldm_cfg_ddim_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_float,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aldm_philox_u32": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_ulonglong, C.c_void_p]),
    "aldm_randn": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p]),
    "aldm_add_noise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]),
    "aldm_add_noise_t": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]),
    "aldm_gaussian_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]),
    "aldm_train_noise_fused": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aldm_window_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_void_p, C.c_int, C.POINTER(WindowPlanArgs), C.c_void_p]),
    "aldm_window_blend": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.POINTER(WindowPlanArgs), C.c_void_p]),
    "aldm_sleep_us": (C.c_int, [C.c_int, C.c_void_p]),
    "aldm_gather_row": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "aldm_advance_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_log_mel": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                               C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "aldm_adamw_flat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_float,
                                  C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_void_p]),
    "aldm_sumsq_flat": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p]),
    "aldm_adamw_flat_clip": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_float, C.c_float, C.c_float,
                                       C.c_float, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_float, C.c_void_p,
                                       C.c_void_p]),
    "aldm_clip_flat": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "aldm_accum_flat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
    "aldm_resample_up3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "aldm_resample_poly": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_int, C.c_void_p]),
    "aldm_clip_segment_workspace_floats": (C.c_longlong, [C.c_int, C.c_int]),
    "aldm_clip_segment": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aldm_clip_normalize_parts": (C.c_int, [C.c_int, C.c_int]),
    "aldm_clip_normalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aldm_loudness_chunk": (C.c_int, []),
    "aldm_kweight_energy_workspace_doubles": (C.c_longlong, [C.c_int, C.c_int]),
    "aldm_kweight_energy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "aldm_loudness_gate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_peak_abs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_loudness_gain": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aldm_clap_log_mel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_clap_input": (C.c_int, [C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "aldm_aff_sum_pool": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aldm_aff_combine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p]),
    "aldm_window_attention": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    "aldm_patch_merge_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "aldm_token_mean": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# The eight fused scheduler steps share one argument frame (csrc/elementwise.hip launch_step_fused): eps, x, B, n_per_sample, cfg,
# guidance, coef, step_idx, x_in | the solver's operand (DDIM: none, DPM: hist, Euler-ancestral: the Philox state, UniPC: state) | table, row_elems,
# rowbias, timesteps, n_steps, t_out, ticket | masked: x0, noise, mask, blend, channels | stream.
_STEP_HEAD = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
_STEP_TAIL = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
_STEP_INPAINT = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
for _solver, _operand in (("ddim", []), ("dpm", [C.c_void_p]), ("euler_a", [C.c_void_p]), ("unipc", [C.c_void_p])):
    PROTOTYPES[f"aldm_{_solver}_step_fused"] = (C.c_int, _STEP_HEAD + _operand + _STEP_TAIL + [C.c_void_p])
    PROTOTYPES[f"aldm_{_solver}_step_fused_masked"] = (C.c_int, _STEP_HEAD + _operand + _STEP_TAIL + _STEP_INPAINT + [C.c_void_p])
    # the windowed steps (long-form generation): the unmasked list, then the window plan
    PROTOTYPES[f"aldm_{_solver}_step_fused_windowed"] = (C.c_int, _STEP_HEAD + _operand + _STEP_TAIL + [C.POINTER(WindowPlanArgs), C.c_void_p])
    # the masked windowed steps (audio-to-audio on a long latent): the windowed list, then the inpainting operands behind the plan
    PROTOTYPES[f"aldm_{_solver}_step_fused_windowed_masked"] = (C.c_int, _STEP_HEAD + _operand + _STEP_TAIL + [C.POINTER(WindowPlanArgs)]
                                                                + _STEP_INPAINT + [C.c_void_p])
# RePaint exists only masked: the Euler-ancestral masked lists (the operand is the Philox state; `noise` may be NULL)
PROTOTYPES["aldm_repaint_step_fused_masked"] = PROTOTYPES["aldm_euler_a_step_fused_masked"]
PROTOTYPES["aldm_repaint_step_fused_windowed_masked"] = PROTOTYPES["aldm_euler_a_step_fused_windowed_masked"]

_lib = None


class AldmError(RuntimeError):
    pass


def load():
    """Load the HIP library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AldmError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C audioldm_with_lora_amd/csrc`.  There is no CPU fallback on the product path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().aldm_last_error().decode()
        raise AldmError(f"{what} failed (rc={rc}): {msg}")
