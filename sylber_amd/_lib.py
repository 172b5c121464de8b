"""ctypes binding of libsylber_hip.so (include/sylber_hip.h).  There is no CPU fallback: if the
HIP library is missing or fails to load, importing the product path raises."""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product loads the in-tree build and nothing else: no environment variable swaps the library (round 6; development A/Bs of
# two builds go through tools/with_lib.py, which calls use_library() before anything is loaded)
LIB_PATH = os.path.join(_HERE, "libsylber_hip.so")
_DEV_LIB = False        # set by use_library(): an older A/B build may lack the newest entry points
MAX_LAYERS = 12

c_float_p = POINTER(c_float)


class SylberLayerWeights(ctypes.Structure):
    _fields_ = [(n, c_float_p) for n in (
        "q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "o_w", "o_b", "ln1_w", "ln1_b",
        "ff1_w", "ff1_b", "ff2_w", "ff2_b", "ln2_w", "ln2_b")]


class SylberMlpHidden(ctypes.Structure):
    _fields_ = [(n, c_float_p) for n in ("lin_w", "lin_b", "ff1_w", "ff1_b", "ff2_w", "ff2_b", "ln_w", "ln_b")]


class SylberMlpWeights(ctypes.Structure):
    """mirror of SylberMlpWeights in include/sylber_hip.h"""
    _fields_ = [("input_dim", c_int32), ("output_dim", c_int32), ("num_hidden", c_int32), ("hidden_dims", c_int32 * 4),
                ("hidden", SylberMlpHidden * 4), ("out_w", c_float_p), ("out_b", c_float_p)]


CFM_DEPTH = 8


class SylberCfmLayer(ctypes.Structure):
    """mirror of SylberCfmLayer in include/sylber_hip.h"""
    _fields_ = [(n, c_float_p) for n in (
        "attn_gamma_w", "attn_gamma_b", "attn_beta_w", "attn_beta_b", "q_gamma", "k_gamma", "qkv_w", "out_w",
        "ff_gamma_w", "ff_gamma_b", "ff_beta_w", "ff_beta_b", "ff1_w", "ff1_b", "ff2_w", "ff2_b")]


class SylberCfmWeights(ctypes.Structure):
    """mirror of SylberCfmWeights in include/sylber_hip.h"""
    _fields_ = [(n, c_float_p) for n in ("proj_in_w", "proj_in_b", "time_freq", "time_w", "time_b", "to_embed_w", "to_embed_b",
                                         "conv_w", "conv_b", "register_tokens", "rotary_inv_freq")] + \
               [("layers", SylberCfmLayer * CFM_DEPTH), ("final_gamma", c_float_p), ("to_pred_w", c_float_p)]


class SylberWeights(ctypes.Structure):
    _fields_ = [("num_layers", c_int32), ("conv_w", c_float_p * 7), ("gn_w", c_float_p), ("gn_b", c_float_p),
                ("fp_ln_w", c_float_p), ("fp_ln_b", c_float_p), ("fp_w", c_float_p), ("fp_b", c_float_p),
                ("pos_w", c_float_p), ("pos_b", c_float_p), ("enc_ln_w", c_float_p), ("enc_ln_b", c_float_p),
                ("layers", SylberLayerWeights * MAX_LAYERS)]


EXPORTS = {
    "sylber_num_frames": (c_int32, [c_int32]),
    "sylber_padded_frames": (c_int32, [c_int32]),
    "sylber_set_option": (c_int, [c_void_p, c_int32, c_int32]),
    "sylber_create": (c_int, [POINTER(SylberWeights), c_int, c_int, POINTER(c_void_p)]),
    "sylber_destroy": (None, [c_void_p]),
    "sylber_last_error": (c_char_p, []),
    "sylber_forward": (c_int, [c_void_p, c_void_p, POINTER(c_int32), c_int32, c_int32, c_void_p, c_void_p]),
    "sylber_segment": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_float, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    "sylber_segment_frames": (c_int, [c_void_p, c_void_p, POINTER(c_int32), c_int32, c_int32, c_int32, c_float, c_float, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
    "sylber_set_stop_stage": (c_int, [c_void_p, c_int32]),
    "sylber_set_profiling": (c_int, [c_void_p, c_int32]),
    "sylber_set_graph_mode": (c_int, [c_void_p, c_int32]),
    "sylber_get_profile": (c_int, [c_void_p, POINTER(c_char_p), POINTER(c_float), c_int32]),
    "sylber_workspace_bytes": (c_int64, [c_void_p]),
    "sylber_get_fp16_audit": (c_int, [c_void_p, POINTER(c_char_p), POINTER(ctypes.c_uint32), POINTER(c_float), c_int32]),
    "sylber_op_linear": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                 c_int32, c_void_p]),
    "sylber_op_linear16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                   c_int32, c_void_p]),
    "sylber_op_conv3": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "sylber_op_linear_resln": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                       c_int32, c_void_p]),
    "sylber_op_mx_quantize": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "sylber_op_layernorm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "sylber_ingest_num_frames": (c_int64, [c_int64, c_int32]),
    "sylber_ingest_workspace_bytes": (c_int64, [c_int32]),
    "sylber_ingest": (c_int, [c_void_p, c_int32, c_int32, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "sylber_flac_info": (c_int, [c_void_p, c_int64, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int64)]),
    "sylber_flac_decode": (c_int, [c_void_p, c_int64, c_void_p, c_int64, POINTER(c_int64)]),
    "sylber_km_workspace_floats": (c_int64, [c_int32, c_int32, c_int32]),
    "sylber_km_assign": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "sylber_km_decode": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "sylber_km_residual_workspace_floats": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "sylber_km_assign_residual": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "sylber_km_decode_residual": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "sylber_km_normalize": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "sylber_kmeans_assign_workspace_floats": (c_int64, [c_int32, c_int32, c_int32]),
    "sylber_kmeans_assign": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    "sylber_kmeans_update_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "sylber_kmeans_update": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_kmeans_seed_workspace_floats": (c_int64, [c_int32]),
    "sylber_kmeans_seed": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_knn_splits": (c_int32, [c_int32, c_int32, c_int32]),
    "sylber_knn_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "sylber_knn_row_norms": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "sylber_knn_unit_rows": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "sylber_knn_search": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                  c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_knn16_pack": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "sylber_knn16_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "sylber_knn16_scan": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                  c_void_p, c_void_p, c_void_p]),
    "sylber_knn_rerank": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p,
                                  c_void_p, c_void_p]),
    "sylber_pq_encode": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "sylber_pq_decode": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "sylber_pq_lut": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "sylber_pq_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "sylber_pq_scan": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                               c_void_p, c_void_p, c_void_p]),
    "sylber_ivf_work_items": (c_int32, [POINTER(c_int32), POINTER(c_int32), c_int32, c_int32, POINTER(c_int32), c_int32, POINTER(c_int32)]),
    "sylber_ivf_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "sylber_ivf_search": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                  c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_ivfpq_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "sylber_ivfpq_scan": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                  c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_ivfpq_list_terms": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p]),
    "sylber_ivfpq_recon_norms": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "sylber_ivfpq_decode": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "sylber_ivfpq_scan_residual": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                           c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p]),
    "sylber_dtw_plan": (c_int32, [POINTER(c_int32), c_int32, POINTER(c_int32), c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), c_int32,
                                  POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "sylber_dtw_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "sylber_dtw_search": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p,
                                  c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
    "sylber_dtw16_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "sylber_dtw16_scan": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p,
                                  c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    "sylber_dtw_rerank": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int32,
                                  c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_dtw_occurrences": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p,
                                       c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p]),
    "sylber_dtw_occ_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "sylber_dtw_local": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p,
                                 c_int32, c_int32, c_float, c_float, c_float, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_dtw_rerank_occurrences": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p,
                                              c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p]),
    "sylber_dtw_align_workspace_bytes": (c_int64, [c_int32, c_int32]),
    "sylber_dtw_align": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int32,
                                 c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_dtw_strings_workspace_bytes": (c_int64, [POINTER(c_int32), POINTER(c_int32), c_int32, c_int32]),
    "sylber_dtw_strings_align": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, POINTER(c_int32),
                                         POINTER(c_int32), c_int32, c_int32, POINTER(c_int64), c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "sylber_dtw_strings_split_workspace_bytes": (c_int64, [POINTER(c_int32), POINTER(c_int32), c_int32, c_int32, c_int32, c_int32]),
    "sylber_dtw_strings_align_split": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, POINTER(c_int32),
                                               POINTER(c_int32), c_int32, c_int32, POINTER(c_int64), c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_int32, c_int32, c_void_p, c_void_p]),
    "sylber_dtw_strings_local_workspace_bytes": (c_int64,[POINTER(c_int32), POINTER(c_int32), c_int32]),
    "sylber_dtw_strings_local": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, POINTER(c_int32),
                                         POINTER(c_int32), POINTER(c_int32), c_int32, c_float, c_float, c_float, c_int32, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "sylber_dtw_rerank_codes": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                        c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                        c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_dtw_rerank_occurrences_codes": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                                    c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                                    c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                                    c_void_p]),
    "sylber_dtw_align_codes": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                       c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32,
                                       c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_dtwpq_scan": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                  c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_phrase_vote": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p,
                                   c_int32, c_void_p, c_void_p, c_void_p]),
    "sylber_unit_workspace_bytes": (c_int64, [POINTER(c_int32), c_int32, POINTER(c_int32), c_int32, c_int32, c_int32]),
    "sylber_unit_search": (c_int, [c_void_p, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), c_int32, c_void_p, c_int32,
                                   POINTER(c_int32), c_int32, c_void_p, POINTER(c_int32), c_void_p, c_int32, c_int32, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p]),
    "sylber_unit_occurrences": (c_int, [c_void_p, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), c_int32, c_void_p,
                                        c_int32, POINTER(c_int32), c_int32, c_void_p, POINTER(c_int32), c_void_p, c_int32, c_int32, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_unit_align_workspace_bytes": (c_int64, [c_int32, c_int32]),
    "sylber_unit_align": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32,
                                  c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_unit_strings_workspace_bytes": (c_int64, [POINTER(c_int32), POINTER(c_int32), c_int32, c_int32]),
    "sylber_unit_strings_align": (c_int, [c_void_p, POINTER(c_int32), c_void_p, POINTER(c_int32), c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_unit_local_workspace_bytes": (c_int64, [POINTER(c_int32), POINTER(c_int32), c_int32]),
    "sylber_unit_local_align": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), c_int32, c_int32,
                                        c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_unit_local_all_workspace_bytes": (c_int64, [POINTER(c_int32), POINTER(c_int32), c_int32]),
    "sylber_unit_local_align_all": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                            c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_lq_norm": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_int64,
                               c_int32, c_void_p]),
    "sylber_ffenc_workspace_floats": (c_int64, [c_int32, c_int32, POINTER(c_int32)]),
    "sylber_ffenc": (c_int, [c_void_p, c_int32, c_int32, POINTER(c_int32), POINTER(c_void_p), c_void_p, c_void_p, c_void_p]),
    "sylber_rvq_prepare": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "sylber_rvq_workspace_floats": (c_int64, [c_int32, c_int32, c_int32]),
    "sylber_rvq_assign": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p,
                                  c_int64, c_void_p, c_void_p]),
    "sylber_rvq_decode": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p]),
    "sylber_mlp_create": (c_int, [POINTER(SylberMlpWeights), c_int, POINTER(c_void_p)]),
    "sylber_mlp_destroy": (None, [c_void_p]),
    "sylber_condition_workspace_floats": (c_int64, [c_void_p, c_int32, c_int32]),
    "sylber_condition": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "sylber_condition_features": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "sylber_condition_units_workspace_floats": (c_int64, [c_void_p, c_int32, c_int32]),
    "sylber_condition_units": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                       c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "sylber_expand_units": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "sylber_cfm_create": (c_int, [POINTER(SylberCfmWeights), c_int, c_int, POINTER(c_void_p)]),
    "sylber_cfm_destroy": (None, [c_void_p]),
    "sylber_cfm_workspace_bytes": (c_int64, [c_void_p, c_int32, c_int32]),
    "sylber_cfm_sample": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "sylber_cfm_sample_frames": (c_int, [c_void_p, c_void_p, POINTER(c_int32), c_int32, c_int32, c_int32, c_void_p, c_float, c_void_p,
                                         c_void_p, c_void_p]),
    "sylber_cfm_eval": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "sylber_packed_layout": (c_int, [POINTER(c_int32), c_int32, POINTER(c_int32), POINTER(c_int32)]),
    "sylber_forward_packed": (c_int, [c_void_p, c_void_p, POINTER(c_int32), c_int32, c_void_p, c_void_p]),
    "sylber_packed_gather": (c_int, [c_void_p, POINTER(c_int32), c_int32, c_void_p, c_void_p]),
    "sylber_segment_packed": (c_int, [c_void_p, c_void_p, POINTER(c_int32), c_int32, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "sylber_cfm_packed_layout": (c_int, [POINTER(c_int32), c_int32, POINTER(c_int32)]),
    "sylber_cfm_workspace_bytes_packed": (c_int64, [c_void_p, POINTER(c_int32), c_int32]),
    "sylber_cfm_sample_packed": (c_int, [c_void_p, c_void_p, POINTER(c_int32), c_int32, c_int32, c_void_p, c_float, c_void_p, c_void_p,
                                         c_void_p]),
    "sylber_condition_packed_workspace_floats": (c_int64, [c_void_p, c_int32, c_int32]),
    "sylber_condition_packed": (c_int, [c_void_p, c_void_p, POINTER(c_int32), POINTER(c_int32), c_int32, c_void_p, c_void_p, c_void_p,
                                        c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sylber_condition_units_packed": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                              POINTER(c_int32), c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "sylber_op_attention": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                    c_int32, c_void_p]),
}
# include/sylber_hip_dev.h: development aids (tools/ only)
DEV_EXPORTS = {
    "sylber_debug_gemm_bench": (c_int, [c_int32] * 8 + [POINTER(c_float)]),
    "sylber_debug_gemm_pick": (c_int, [c_int32] * 8),
    "sylber_debug_gemm_resolve": (c_int, [c_int32] * 12 + [ctypes.c_char_p, c_int32]),
    "sylber_debug_gemm_trace": (c_int, [c_int32] * 6 + [POINTER(ctypes.c_uint64), POINTER(c_float)]),
    "sylber_debug_attention_bench": (c_int, [c_int32] * 4 + [POINTER(c_float)]),
    "sylber_debug_poison_workspace": (c_int, [c_void_p, c_int32]),
    "sylber_debug_conv0_scale_shift": (c_int, [c_void_p, c_int32, c_void_p]),
    "sylber_debug_conv_rows": (c_int, [c_int32, POINTER(c_int32), POINTER(c_int32)]),
    "sylber_cfm_set_tap": (c_int, [c_void_p, c_int32, c_void_p, c_int64]),
    "sylber_cfm_tap_floats": (c_int64, [c_void_p, c_int32, c_int32, c_int32]),
    "sylber_cfm_tap_floats_packed": (c_int64, [c_void_p, c_int32, POINTER(c_int32), c_int32]),
    "sylber_debug_segment_scalars": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                             c_void_p, c_void_p]),
}
# taps inside the resynthesis decoder (include/sylber_hip_dev.h SYLBER_CFM_TAP_* / SYLBER_CFM_BTAP_*): the front stages, and launch k of block li
CFM_TAP_CONDX, CFM_TAP_GB, CFM_TAP_XE, CFM_TAP_X0 = 1, 2, 3, 4
(CFM_BTAP_H_ATTN, CFM_BTAP_QKV, CFM_BTAP_Q, CFM_BTAP_K, CFM_BTAP_VT, CFM_BTAP_QKVF, CFM_BTAP_CTX, CFM_BTAP_X_ATTN, CFM_BTAP_H_FF, CFM_BTAP_FF,
 CFM_BTAP_G, CFM_BTAP_X_FF) = range(12)


def CFM_TAP(block: int, k: int) -> int:
    """the tap stage behind launch k (CFM_BTAP_*) of decoder block ``block``"""
    return 16 * (int(block) + 1) + int(k)
OPT_GEMM_TILE, OPT_ATTN_QUERIES_PER_WAVE, OPT_GEMM_PERSISTENT = 1, 2, 3
OPT_FUSE_OUTPROJ_LN, OPT_CONV0_VALU = 4, 5
OPT_FP8_ATTENTION, OPT_SEGMENT, OPT_PER_UTTERANCE = 7, 9, 14
OPT_GEMM_MODEL, OPT_GEMM_MFMA16 = 12, 13
# negative stop stages of sylber_set_stop_stage: taps inside the front half (include/sylber_hip.h SYLBER_TAP_*)
TAP_CONV0, TAP_PROJ, TAP_POSCONV = -1, -2, -3
# taps inside encoder layer l (SYLBER_TAP_LAYER / SYLBER_LTAP_*): the forward ends after launch k of the layer
LTAP_QKV, LTAP_CTX, LTAP_ATTN_SUM, LTAP_LN1, LTAP_FFN1, LTAP_FFN2_SUM = 0, 1, 2, 3, 4, 5
LTAP_WIDTH = {LTAP_QKV: 2304, LTAP_CTX: 768, LTAP_ATTN_SUM: 768, LTAP_LN1: 768, LTAP_FFN1: 3072, LTAP_FFN2_SUM: 768}


def ltap_width(k: int, precision: str = "bf16", fp8_attention: bool = True) -> int:
    """floats per frame that tap k returns.  The fp8 precision returns its MXFP8 buffers as W dequantised values followed by W block
    exponents (2 W); its fp32 sums, and q | k | v where the attention core runs on bf16 operands (OPT_FP8_ATTENTION < 0), keep W"""
    w = LTAP_WIDTH.get(int(k), 768)
    if precision != "fp8" or k in (LTAP_ATTN_SUM, LTAP_FFN2_SUM) or (k == LTAP_QKV and not fp8_attention):
        return w
    return 2 * w


def TAP_LAYER(l: int, k: int) -> int:
    """the stop stage of tap k (LTAP_*) of encoder layer l"""
    return -(8 * (int(l) + 1) + int(k))


def TAP_CONV(i: int) -> int:
    """the stop stage of the tap behind conv layer i = 1..6 (SYLBER_TAP_CONV): every row of its output buffer, [B, padded_frames << (6 - i), 512]"""
    return -(1024 + int(i))


_LIB = None


class SylberHipError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise SylberHipError(
                "libsylber_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `python sylber_amd/build.py`; there is no CPU fallback on the product path." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in list(EXPORTS.items()) + list(DEV_EXPORTS.items()):
            if _DEV_LIB and not hasattr(lib, name):
                continue                 # an OLDER build loaded for a same-box A/B (tools/with_lib.py) may lack the newest entry points
            fn = getattr(lib, name)      # AttributeError if the ABI drifted from include/sylber_hip.h
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def use_library(path: str) -> None:
    """development only (tools/with_lib.py): load another build of the library (a reference build for a same-box A/B, or the
    experiments build with its timing kernels).  Must be called before the first load()."""
    global LIB_PATH, _DEV_LIB
    if _LIB is not None:
        raise SylberHipError("use_library() after the library was loaded")
    LIB_PATH, _DEV_LIB = os.path.abspath(path), True


def check(status: int, what: str) -> None:
    if status != 0:
        raise SylberHipError("%s failed: %s" % (what, load().sylber_last_error().decode()))
