"""ctypes binding of libtce_rvos.so (the C ABI declared in the headers of include/).

The product path has NO fallback: if the shared object is missing or a symbol is absent, importing this
module's `lib()` raises.  Build it with `python -m tce_rvos_amd.build` / `__graft_entry__.build()`.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TCE_LIB") or os.path.join(HERE, "lib", "libtce_rvos.so")  # TCE_LIB: A/B of two builds (tools)

c_f = C.c_void_p  # device pointers travel as integers
i32, i64, f32 = C.c_int32, C.c_int64, C.c_float


class GemmArgs(C.Structure):
    _fields_ = [("A", c_f), ("A2", c_f), ("W", c_f), ("bias", c_f), ("res", c_f), ("C", c_f),
                ("M", i32), ("N", i32), ("K", i32),
                ("lda", i32), ("lda2", i32), ("ldw", i32), ("ldc", i32), ("ldres", i32),
                ("act", i32), ("res_mode", i32), ("batch", i32),
                ("sA", i64), ("sA2", i64), ("sW", i64), ("sBias", i64), ("sC", i64), ("sRes", i64),
                ("conv", i32), ("T", i32), ("H", i32), ("Wd", i32), ("Cin", i32), ("Ho", i32), ("Wo", i32),
                ("kh", i32), ("kw", i32), ("stride", i32), ("pad", i32)]


class RowLinArgs(C.Structure):
    _fields_ = [("x", c_f), ("a2", c_f), ("packed", c_f), ("bias", c_f), ("res", c_f), ("out", c_f),
                ("g_in", c_f), ("be_in", c_f), ("g_out", c_f), ("be_out", c_f),
                ("ldx", i64), ("lda2", i64), ("ldres", i64), ("ldo", i64),
                ("sX", i64), ("sA2", i64), ("sRes", i64), ("sOut", i64),
                ("M", i32), ("N", i32), ("K", i32), ("batch", i32), ("a2_rows", i32), ("act", i32), ("res_mode", i32),
                ("eps_in", f32), ("eps_out", f32)]


class XattnArgs(C.Structure):
    _fields_ = [("x", c_f), ("a2", c_f), ("packed", c_f), ("bo", c_f), ("res", c_f), ("out", c_f),
                ("g_out", c_f), ("be_out", c_f),
                ("ldx", i64), ("lda2", i64), ("ldres", i64), ("ldo", i64),
                ("sX", i64), ("sRes", i64), ("sOut", i64), ("sW", i64),
                ("M", i32), ("batch", i32), ("a2_rows", i32), ("res_mode", i32), ("group", i32), ("eps_out", f32), ("w_div", i32)]



class XattnFfnArgs(C.Structure):
    _fields_ = [("packed", c_f), ("b2", c_f), ("g_out", c_f), ("be_out", c_f), ("mid", c_f), ("ldmid", i64), ("sMid", i64),
                ("hidden", i32), ("act", i32), ("eps_out", f32)]


class FewRowSeg(C.Structure):
    _fields_ = [("W", c_f), ("bias", c_f), ("out", c_f), ("N", i32), ("ldw", i32), ("ldo", i32), ("use_a2", i32), ("act", i32)]


class FewRowArgs(C.Structure):
    _fields_ = [("x", c_f), ("a2", c_f), ("res", c_f),
                ("ldx", i64), ("lda2", i64), ("ldres", i64),
                ("a2_rows", i32), ("R", i32), ("K", i32), ("nseg", i32), ("seg", FewRowSeg * 3),
                ("g_in", c_f), ("be_in", c_f), ("xn_out", c_f), ("ldxn", i64), ("eps_in", f32)]


class CopySeg(C.Structure):
    _fields_ = [("src", c_f), ("dst", c_f), ("rows", i64), ("row_words", i64), ("src_pitch_words", i64)]


class LabelObj(C.Structure):
    _fields_ = [("logits", c_f), ("masks", c_f)]


A2D_GROUP_MAX = 16  # TCE_A2D_GROUP_MAX: samples per tce_a2d_group_masks_u8 call


class A2dGroupSample(C.Structure):  # tceA2dGroupSample (include/tce_rvos_eval.h)
    _fields_ = [("masks", c_f), ("logits", c_f), ("out", c_f), ("scores", c_f), ("fh", i32), ("fw", i32), ("H0", i32), ("W0", i32),
                ("logit_stride", i32), ("reserved", i32)]


REFEXP_GROUP_MAX = 16   # TCE_REFEXP_GROUP_MAX: samples per tce_refexp_group_u8 call
REFEXP_MAX_CAND = 1024  # TCE_REFEXP_MAX_CAND: Q*K candidates per sample


class RefexpSample(C.Structure):  # tceRefexpSample (include/tce_rvos_refexp.h)
    _fields_ = [("logits", c_f), ("boxes_in", c_f), ("masks", c_f), ("scores", c_f), ("order", c_f), ("boxes_out", c_f), ("out", c_f),
                ("fh", i32), ("fw", i32), ("H0", i32), ("W0", i32)]


# name -> (restype, argtypes), one table per header of include/ (HEADERS): EVERY symbol of its header and no other (tests check this)
SIGNATURES = {
    "tce_abi_version": (i32, []),
    "tce_last_error": (C.c_char_p, []),
    "tce_gemm_f32": (i32, [C.POINTER(GemmArgs), c_f]),
    "tce_gemm_splitk_f32": (i32, [C.POINTER(GemmArgs), i32, c_f, c_f]),
    "tce_gemm_splitk_ln_f32": (i32, [C.POINTER(GemmArgs), i32, c_f, c_f, c_f, f32, c_f]),
    "tce_gemm_select_tile": (i32, [i32, i32, i32]),
    "tce_gemm_select_tile_ex": (i32, [i32, i32, i32, i32, i32]),
    "tce_set_gemm_mode": (i32, [i32]),
    "tce_set_gemm_mode_thread": (i32, [i32]),
    "tce_set_range_flag": (i32, [c_f]),
    "tce_get_gemm_mode": (i32, []),
    "tce_layernorm_f32": (i32, [c_f, c_f, c_f, c_f, c_f, i64, i32, f32, c_f]),
    "tce_groupnorm_nsplit": (i32, [i32]),
    "tce_groupnorm_f32": (i32, [c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, f32, i32, c_f]),
    "tce_groupnorm_up_add_f32": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, i32, f32, i32, c_f]),
    "tce_resnet_stem_f32": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, c_f]),
    "tce_maxpool3x3s2_cl_f32": (i32, [c_f, c_f, i32, i32, i32, i32, c_f]),
    "tce_resize_h_u8": (i32, [c_f, c_f, c_f, c_f, i64, i32, i32, i32, c_f]),
    "tce_resize_v_norm_f32": (i32, [c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, c_f]),
    "tce_patch_embed_f32": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, f32, c_f]),
    "tce_window_attn_f32": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, c_f]),
    "tce_window_attn3d_f32": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, c_f]),
    "tce_patch_merge_ln_f32": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, i32, f32, c_f]),
    "tce_mha_f32": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, i32, i32, i64, i64, i64, i64, c_f, f32, c_f]),
    "tce_mha_ws_bytes": (i64, [i32, i32, i32]),
    "tce_mha_ws_f32": (i32, [c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, i32, i32, i64, i64, i64, i64, c_f, f32, c_f]),
    "tce_ms_deform_attn_forward_f32": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, i32, c_f]),
    "tce_ms_deform_attn_backward_f32": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, i32, c_f]),
    "tce_msda_fused_f32": (i32, [c_f, c_f, c_f, c_f, C.POINTER(i32), i32, i32, i32, i32, i32, i32, i32, i32, c_f]),
    "tce_msda_fused_valid_f32": (i32, [c_f, c_f, c_f, c_f, C.POINTER(i32), C.POINTER(i32), i32, i32, i32, i32, i32, i32, i32,
                                       i32, c_f]),
    "tce_msda_fewq_raw_f32": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, C.POINTER(i32), C.POINTER(i32), i32, i32, i32, i32, i32, i32, i32,
                                    i32, c_f]),
    "tce_contrastive_f32": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, i32, c_f]),
    "tce_pos_sine2d_f32": (i32, [c_f, c_f, i32, i32, i32, i32, c_f]),
    "tce_pos_sine2d_valid_f32": (i32, [c_f, c_f, i32, i32, i32, i32, i32, i32, c_f]),
    "tce_resize_nearest_f32": (i32, [c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, c_f]),
    "tce_resize_bilinear_f32": (i32, [c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, c_f]),
    "tce_resize_bilinear_ln_f32": (i32, [c_f, c_f, c_f, c_f, f32, c_f, i32, i32, i32, i32, i32, i32, c_f]),
    "tce_add_f32": (i32, [c_f, c_f, c_f, i64, i64, c_f]),
    "tce_tile_f32": (i32, [c_f, c_f, i64, i64, c_f]),
    "tce_sigmoid_f32": (i32, [c_f, c_f, i64, c_f]),
    "tce_copy_segments": (i32, [C.POINTER(CopySeg), i32, c_f]),
    "tce_box_refine_f32": (i32, [c_f, c_f, c_f, i32, i32, c_f]),
    "tce_mask_pack_f32": (i32, [c_f, c_f, c_f, i32, i32, i32, i32, c_f]),
    "tce_mask_tail_f32": (i32, [c_f, c_f, c_f, i32, c_f, i32, i32, i32, i32, i32, f32, f32, i32, c_f]),
    "tce_select_masks_u8": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, i32, f32, c_f]),
    "tce_embed_ln_f32": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, f32, i32, c_f]),
    "tce_mha_small64_f32": (i32, [c_f, c_f, i32, i32, f32, c_f]),
    "tce_mha_small64_seqs_f32": (i32, [c_f, i32, c_f, c_f, i32, i32, i32, f32, c_f]),
    "tce_embed_ln_seqs_f32": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, f32, i32, c_f]),
    "tce_mha_small64_lens_f32": (i32, [c_f, i32, c_f, c_f, i32, i32, i32, f32, c_f, c_f]),
    "tce_caption_lens_f32": (i32, [c_f, i32, i32, i32, i32, c_f, c_f, c_f, c_f]),
    "tce_tanh_f32": (i32, [c_f, c_f, i64, c_f]),
    "tce_ffn_packed_bytes": (i64, [i32, i32]),
    "tce_ffn_pack_f32": (i32, [c_f, c_f, c_f, c_f, i32, i32, c_f]),
    "tce_ffn_fused_f32": (i32, [c_f, i64, c_f, c_f, c_f, c_f, f32, c_f, c_f, f32, c_f, i64, i32, i32, i32, i32, c_f]),
    "tce_ffn_split_ws_floats": (i64, [i32, i32, i32, i32]),
    "tce_ffn_split_counters": (i32, [i32, i32, i32, i32]),
    "tce_ffn_set_wg_cap": (i32, [i32]),
    "tce_ffn_capped_grid": (i32, [i32, i32, i32, C.POINTER(i32)]),
    "tce_ffn_fused_split_f32": (i32, [c_f, i64, c_f, c_f, c_f, c_f, f32, c_f, c_f, f32, c_f, i64, i32, i32, i32, i32, c_f, i64, c_f, i32, c_f]),
    "tce_xattn_prepare_f32": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, c_f]),
    "tce_ffn_pack_batched_f32": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, c_f]),
    "tce_xattn_fused_f32": (i32, [C.POINTER(XattnArgs), c_f]),
    "tce_xattn_ffn_fused_f32": (i32, [C.POINTER(XattnArgs), C.POINTER(XattnFfnArgs), c_f]),
    "tce_ffn_pack_chain_f32": (i32, [c_f, c_f, c_f, c_f, i32, i32, c_f]),
    "tce_xattn_pack_f32": (i32, [c_f, c_f, c_f, c_f, c_f, i32, i32, i32, c_f]),
    "tce_xattn_prepare_lens_f32": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, c_f, c_f]),
    "tce_xattn_pack_lens_f32": (i32, [c_f, c_f, c_f, c_f, c_f, i32, i32, i32, c_f, c_f]),
    "tce_rowlin_packed_bytes": (i64, [i32, i32]),
    "tce_rowlin_pack_f32": (i32, [c_f, i64, c_f, i32, i32, c_f]),
    "tce_rowlin_f32": (i32, [C.POINTER(RowLinArgs), c_f]),
    "tce_conv3x3_packed_bytes": (i64, [i32, i32]),
    "tce_conv3x3_pack_f32": (i32, [c_f, c_f, i32, i32, c_f]),
    "tce_conv3x3_f32": (i32, [c_f, i64, c_f, c_f, c_f, i64, i32, i32, i32, i32, i32, c_f]),
    "tce_conv3x3_split_ws_floats": (i64, [i32, i32, i32]),
    "tce_conv3x3_split_pieces": (i32, [i32, i32, i32]),
    "tce_conv3x3_split_kstep": (i32, [i32, i32]),
    "tce_conv3x3_split_f32": (i32, [c_f, i64, c_f, c_f, c_f, i64, i32, i32, i32, i32, i32, c_f, i64, c_f]),
    "tce_fewrow_linear_f32": (i32, [C.POINTER(FewRowArgs), c_f]),
    "tce_thin_linear_splits": (i32, [i32, i32, i32]),
    "tce_thin_partials_f32": (i32, [c_f, i64, i32, c_f, i32, c_f, i64, c_f, i32, i32, i32, c_f]),
    "tce_splitk_reduce_f32": (i32, [c_f, i32, i32, i32, c_f, i32, c_f, i32, i32, c_f, i32, c_f, c_f, f32, c_f]),
    "tce_mha_small64_splits_f32": (i32, [c_f, i32, c_f, c_f, i32, i32, f32, c_f]),
    "tce_swin_attn_packed_bytes": (i64, [i32]),
    "tce_swin_attn_pack_f32": (i32, [c_f, c_f, c_f, i32, c_f]),
    "tce_swin_attn_fused_f32": (i32, [c_f, i64, c_f, c_f, c_f, c_f, c_f, c_f, f32, c_f, i64, i32, i32, i32, i32, i32, c_f]),
    "tce_graph_begin": (i32, [c_f]),
    "tce_graph_end": (i32, [c_f, C.POINTER(C.c_void_p)]),
    "tce_graph_launch": (i32, [C.c_void_p, c_f]),
    "tce_graph_destroy": (i32, [C.c_void_p]),
    "tce_graph_group": (i32, [C.POINTER(C.c_void_p), i32, C.POINTER(C.c_void_p)]),
}

# include/tce_rvos_debug.h: tuning / diagnostic entry points (tools/ only)
DEBUG_SIGNATURES = {
    "tce_gemm_force_tile": (i32, [i32]),
    "tce_debug_set_stamp_buffer": (i32, [c_f]),
    "tce_debug_set_epilogue": (i32, [i32]),
    "tce_debug_ffn_set_stamp_buffer": (i32, [c_f]),
    "tce_debug_ffn_set_half": (i32, [i32]),
    "tce_debug_msda_set_lds": (i32, [i32]),
    "tce_debug_window_attn_set_mfma": (i32, [i32]),
    "tce_debug_mha_set_split": (i32, [i32]),
    "tce_debug_msda_set_fewq": (i32, [i32]),
    "tce_debug_conv3x3_set_waves": (i32, [i32]),
    "tce_debug_conv3x3_set_pieces": (i32, [i32]),
}

# include/tce_rvos_video.h: driver-stage entry points (what the reference's inference drivers do with the outputs of several forwards)
VIDEO_SIGNATURES = {
    # objs (host table), n, labels, best_query, T, Q, K, h, w, H0, W0, threshold, background
    "tce_label_objects_u8": (i32, [C.POINTER(LabelObj), i32, c_f, c_f, i32, i32, i32, i32, i32, i32, i32, f32, f32, c_f]),
}

# include/tce_rvos_eval.h: evaluation-stage entry points (the A2D-Sentences / JHMDB-Sentences post-processor)
EVAL_SIGNATURES = {
    # masks [N,h,w], out [N,H0,W0], N, h, w, fh, fw, H0, W0, threshold
    "tce_a2d_masks_u8": (i32, [c_f, c_f, i32, i32, i32, i32, i32, i32, i32, f32, c_f]),
    "tce_rle_ws_bytes": (i64, [i32, i32, i32]),
    # masks [P,H,W] u8, counts [P,H*W+1] u32, nruns [P] i32, ws, P, H, W
    "tce_rle_counts_u32": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, c_f]),
    # samples (host table), B, N, h, w, threshold: the masks and scores of up to A2D_GROUP_MAX samples in one launch
    "tce_a2d_group_masks_u8": (i32, [C.POINTER(A2dGroupSample), i32, i32, i32, i32, f32, c_f]),
}

# include/tce_rvos_score.h: scoring-stage entry points (the counts behind Ref-DAVIS J&F and behind A2D / JHMDB precision, IoU and AP)
SCORE_SIGNATURES = {
    "tce_jf_ws_bytes": (i64, [i32, i32, i32, i32, i32]),  # T, n, H, W, radius
    # pred [T,H,W] u8, gt [T,H,W] u8, counts [n,T,6] i32, ws, T, n, H, W, radius
    "tce_jf_counts_i32": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, c_f]),
    "tce_rle_decode_ws_bytes": (i64, [i32, i32, i32, i32]),  # P, H, W, stride
    # counts [P,stride] u32, nruns [P] i32, out [P,H,W] u8, ws, P, H, W, stride
    "tce_rle_decode_u8": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, i32, c_f]),
    "tce_mask_overlap_ws_bytes": (i64, [i32, i32, i32]),  # N, H, W
    # pred [N,H,W] u8, gt [H,W] u8, counts [N,3] i32, ws, N, H, W
    "tce_mask_overlap_i32": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, c_f]),
}

# include/tce_rvos_png.h: PNG-writing stage entry points (the zlib stream of every output plane, with the fixed Huffman code or with
# the cheaper of the fixed code and a code of its own per strip)
PNG_SIGNATURES = {
    "tce_png_stream_bound": (i64, [i32, i32, i32]),  # H, W, rows_per_strip
    "tce_png_ws_bytes": (i64, [i32, i32, i32, i32]),  # P, H, W, rows_per_strip
    # planes [P,H,W] u8, streams [P,bound] u8, nbytes [P] i32, ws, P, H, W, rows_per_strip, nonzero_value
    "tce_png_deflate_u8": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, c_f]),
    "tce_png_deflate_dyn_u8": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, c_f]),
}

# include/tce_rvos_vis.h: visualisation-stage entry points (the --visualize images drawn on the device and their RGB PNG streams)
VIS_SIGNATURES = {
    # frames [N,H0,W0,3] u8, out, masks [L,N,H0,W0] u8 | NULL, boxes [L,N,4] | NULL, points [L,N,2] | NULL, colors [L,3] u8, L, N, H0, W0
    "tce_vis_overlay_u8": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, c_f]),
    # img [P,H,W,3] u8, rows [P,H,1+3W] u8, P, H, W
    "tce_png_filter_rgb_u8": (i32, [c_f, c_f, i32, i32, i32, c_f]),
    # rows [P,H,R] u8, streams [P,bound] u8, nbytes [P] i32, ws, P, H, R, rows_per_strip
    "tce_png_deflate_rows_u8": (i32, [c_f, c_f, c_f, c_f, i32, i32, i32, i32, c_f]),
}

# include/tce_rvos_pngfile.h: PNG-file stage entry points (the IDAT chunk's CRC-32 and the chunk framing around the streams, on the
# device)
PNGFILE_SIGNATURES = {
    "tce_png_file_bound": (i64, [i32, i64]),  # head_bytes, stream_stride
    "tce_png_file_ws_bytes": (i64, [i32, i64]),  # P, stream_stride
    # streams [P,stream_stride] u8, nbytes [P] i32, head [head_bytes] u8, head_bytes, files [P,file_stride] u8, file_bytes [P] i32, ws,
    # P, stream_stride, file_stride
    "tce_png_file_u8": (i32, [c_f, c_f, c_f, i32, c_f, c_f, c_f, i32, i64, i64, c_f]),
}

# include/tce_rvos_refexp.h: RefCOCO evaluation-stage entry points (the box / mask post-processors for a group of samples, the
# generalised IoU behind precision@k)
REFEXP_SIGNATURES = {
    # samples (host table), B, Q, K, h, w, threshold
    "tce_refexp_group_u8": (i32, [C.POINTER(RefexpSample), i32, i32, i32, i32, i32, f32, c_f]),
    # boxes [M,Q,4], gt [M,4], giou [M,Q], best [M,Q], M, Q
    "tce_refexp_giou_f32": (i32, [c_f, c_f, c_f, c_f, i32, i32, c_f]),
}

# header of include/ -> its table.  The set is closed over include/: a header there without a row here, or a row without its header,
# fails tests/test_host_cpu.py, so a new stage adds its header, its table and this row
HEADERS = {"tce_rvos.h": SIGNATURES, "tce_rvos_debug.h": DEBUG_SIGNATURES, "tce_rvos_video.h": VIDEO_SIGNATURES,
           "tce_rvos_eval.h": EVAL_SIGNATURES, "tce_rvos_score.h": SCORE_SIGNATURES, "tce_rvos_png.h": PNG_SIGNATURES,
           "tce_rvos_vis.h": VIS_SIGNATURES, "tce_rvos_pngfile.h": PNGFILE_SIGNATURES, "tce_rvos_refexp.h": REFEXP_SIGNATURES}

_LIB = None


class TceError(RuntimeError):
    pass


def lib():
    """Loads the shared object (once).  Raises if it is missing: there is no CPU / PyTorch fallback."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise TceError(f"{LIB_PATH} not found: build the HIP extension first "
                           f"(python -c 'import __graft_entry__ as g; g.build()'); there is no fallback path")
        hwq = os.environ.get("GPU_MAX_HW_QUEUES")
        if hwq not in (None, "", "4"):  # measured, profiles/r03_clip_groups.txt: 1-3 abort the HIP runtime at start-up,
            import warnings             # 5-16 double the clip time (every graph edge becomes a cross-queue signal)
            warnings.warn(f"tce_rvos_amd: GPU_MAX_HW_QUEUES={hwq} is set; the HIP runtime's default (4) is the only value this "
                          f"launch program runs well with (1-3 crash the runtime, 5-16 double the clip time)", RuntimeWarning)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in [kv for table in HEADERS.values() for kv in table.items()]:
            fn = getattr(l, name)  # AttributeError if the symbol is absent
            fn.restype, fn.argtypes = res, args
        _LIB = l
    return _LIB


def lib_raw():
    """The CDLL itself even while hazard.recording() has a recording proxy standing in for it."""
    l = lib()
    return l.__dict__.get("_real", l)


def check(status, what=""):
    if status != 0:
        msg = lib().tce_last_error().decode(errors="replace")
        raise TceError(f"{what} failed ({status}): {msg}")
