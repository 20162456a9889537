"""ctypes binding of the C-ABI shared library (include/mtvaf_hip.h) + thin tensor-level wrappers.

The product path has NO fallback: if the library is missing or a call fails, a RuntimeError is raised.
PyTorch only supplies device memory (``tensor.data_ptr()``) and the current HIP stream.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_double, c_float, c_int, c_int64, c_long, c_size_t, c_uint64, c_void_p
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MTVAF_LIB: another build of the library (an A/B variant made by `MTVAF_LIBDIR=... MTVAF_EXTRA_FLAGS=-D... python -m mtvaf_amd.build`:
# ablation builds never overwrite the product library)
LIB_PATH = os.environ.get("MTVAF_LIB") or os.path.join(_HERE, "lib", "libmtvaf_hip.so")

_ERR = {-1: "bad shape", -2: "bad alignment", -3: "bad argument", -4: "workspace too small"}

P, I, L, F, U64, SZ = c_void_p, c_int, c_long, c_float, c_uint64, c_size_t

_SIGS = {
    "mtvaf_version": (c_int, []),
    "mtvaf_encoder_layer_fwd": (c_int, [P, P]),
    "mtvaf_encoder_layer_bwd": (c_int, [P, P, P, P, I]),
    "mtvaf_layer_struct_bytes": (SZ, [I]),
    "mtvaf_rng_set_epoch_ptr": (c_int, [P]),
    "mtvaf_rng_epoch_advance": (c_int, [P, P]),
    "mtvaf_device_cus": (c_int, []),
    "mtvaf_gemm_f32_workspace_bytes": (SZ, [I, I, I, I]),
    "mtvaf_prof_start": (c_int, [I]),
    "mtvaf_prof_stop": (c_int, [P, P, P, I]),
    "mtvaf_gemm_f32_plan": (c_int, [I, I, I, I, I, I, I, P, P]),
    "mtvaf_gemm_f32": (c_int, [I, I, P, I, P, I, P, I, I, I, I, P, I, P, I, I, I, P, SZ, I, I, P]),
    "mtvaf_gemm_f32x3": (c_int, [I, I, P, I, P, I, P, I, I, I, I, P, I, P, I, I, I, P, SZ, I, I, P]),
    "mtvaf_f32_split": (c_int, [I]),
    "mtvaf_f32x3_trace": (c_int, [P]),
    "mtvaf_gemm_f32_slabs": (c_int, [I, I, P, I, P, I, P, I, I, I, I, P, I, P, SZ, P, P]),
    "mtvaf_dropout_res_ln_fwd_slabs": (c_int, [P, I, P, P, P, P, P, P, P, P, I, I, F, c_double, U64, U64, P, P]),
    "mtvaf_dropout_res_ln_bwd_rows_slabs": (c_int, [P, P, I, P, P, P, P, P, P, P, I, I, I, c_double, U64, U64, P, P, P]),
    "mtvaf_dropout_res_ln_fwd_planes": (c_int, [P, I, P, P, P, P, P, P, P, P, I, I, F, c_double, U64, U64, P, P]),
    "mtvaf_dropout_res_ln_bwd_rows_planes": (c_int, [P, P, I, P, P, P, P, P, P, P, I, I, I, c_double, U64, U64, P, P, P]),
    "mtvaf_f32_split_planes": (c_int, [P, P, I, I, I, L, L, L, P]),
    "mtvaf_gemm_f32p": (c_int, [I, P, L, L, L, L, I, P, L, L, L, L, P, I, I, I, I, P, I, P, I, I, I, P, SZ, I, P]),
    "mtvaf_f32p_trace": (c_int, [P]),
    "mtvaf_f32p_wide": (c_int, [I]),
    "mtvaf_gemm_f32p_dw_group": (c_int, [I, P, P, P, P, P, P, P, I, P]),
    "mtvaf_gemm_f32p_dw_group_colsum": (c_int, [I, P, P, P, P, P, P, P, I, I, P, P, P, P, P, P]),
    "mtvaf_gemm_f32p_dw_group_acc": (c_int, [I, P, P, P, P, P, P, P, I, I, P, P, P, P, P, I, P]),
    "mtvaf_gemm_f32p_slabs": (c_int, [I, P, L, L, L, L, I, P, L, L, L, L, P, I, I, I, I, P, I, I, P, SZ, P, P]),
    "mtvaf_gemm_f32p_ep": (c_int, [I, P, L, L, L, L, I, P, L, L, L, L, P, I, P, P, I, I, I, P, I, P, I, I, P]),
    "mtvaf_gemm_bf16": (c_int, [I, I, P, I, P, I, P, I, I, I, I, P, I, P, I, I, I, P, SZ, I, I, P]),
    "mtvaf_prefix_attn_fwd": (c_int, [P, P, P, P, P, P, I, I, I, I, I, F, U64, U64, P]),
    "mtvaf_prefix_attn_bwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, F, U64, U64, P]),
    "mtvaf_prefix_attn_bwd_tail": (c_int, [P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, F, U64, U64, I, P]),
    "mtvaf_prefix_attn_probs": (c_int, [P, P, P, P, P, I, I, I, I, I, I, P]),
    "mtvaf_prefix_attn_mass": (c_int, [P, P, P, P, I, I, I, I, I, I, P]),
    "mtvaf_prefix_attn_varlen_fwd": (c_int, [P, P, P, P, I, P, P, I, I, I, I, I, F, U64, U64, P]),
    "mtvaf_prefix_attn_varlen_bwd": (c_int, [P, P, P, P, P, I, P, P, P, P, P, P, I, I, I, I, I, F, U64, U64, P]),
    "mtvaf_prefix_attn_varlen_fwd_planes": (c_int, [P, P, P, P, I, P, P, I, I, I, I, I, F, U64, U64, P, I, P]),
    "mtvaf_prefix_attn_varlen_bwd_planes": (c_int, [P, P, P, P, P, I, P, P, P, P, P, P, I, I, I, I, I, F, U64, U64, P, I, P]),
    "mtvaf_prefix_attn_varlen_fwd_pm": (c_int, [P, P, P, P, I, P, L, P, P, I, I, I, I, I, F, U64, U64, P, I, P]),
    "mtvaf_prefix_attn_varlen_bwd_pm": (c_int, [P, P, P, P, P, I, P, L, P, P, P, P, P, P, I, I, I, I, I, F, U64, U64, P, I, P]),
    "mtvaf_prefix_attn_bf16_varlen_fwd_pm": (c_int, [P, P, P, P, I, P, L, P, P, I, I, I, I, I, F, U64, U64, P]),
    "mtvaf_prefix_attn_bf16_varlen_bwd_pm": (c_int, [P, P, P, P, P, I, P, L, P, P, P, P, P, P, P, I, I, I, I, I, F, U64, U64, P]),
    "mtvaf_prefix_attn_bf16_varlen_fwd": (c_int, [P, P, P, P, I, P, P, I, I, I, I, I, F, U64, U64, P]),
    "mtvaf_prefix_attn_bf16_varlen_bwd": (c_int, [P, P, P, P, P, I, P, P, P, P, P, P, P, I, I, I, I, I, F, U64, U64, P]),
    "mtvaf_gather_rows": (c_int, [P, P, P, I, I, P]),
    "mtvaf_build_packing": (c_int, [P, I, I, I, I, P, P, P, P, P]),
    "mtvaf_build_packing_ordered": (c_int, [P, I, I, I, I, P, P, P, P, P]),
    "mtvaf_build_ktiles": (c_int, [P, I, I, I, I, I, P, P, P]),
    "mtvaf_gemm_f32_ktiles": (c_int, [I, I, P, I, P, I, P, I, I, I, I, P, I, P, I, I, I, P, SZ, I, I, P, P, P]),
    "mtvaf_zero_f32": (c_int, [P, L, P]),
    "mtvaf_prefix_attn_bf16_fwd": (c_int, [P, P, P, P, P, P, I, I, I, I, I, F, U64, U64, P]),
    "mtvaf_prefix_attn_bf16_bwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, F, U64, U64, P]),
    "mtvaf_prefix_attn_bf16_bwd_tail": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, F, U64, U64, I, P]),
    "mtvaf_ln_bwd_workspace_bytes": (SZ, [I, I]),
    "mtvaf_roberta_position_ids": (c_int, [P, P, I, I, I, P]),
    "mtvaf_embed_ln_fwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, I, I, I, F, c_double, U64, U64, P, P]),
    "mtvaf_embed_ln_bwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, c_double, U64,
                                   U64, P, P, SZ, P]),
    "mtvaf_dropout_res_ln_fwd": (c_int, [P, P, P, P, P, P, P, I, I, F, c_double, U64, U64, P, P]),
    "mtvaf_dropout_res_ln_bwd": (c_int, [P, P, P, P, P, P, P, P, I, P, P, P, I, I, I, c_double, U64, U64, P, SZ, P, P]),
    "mtvaf_dropout_res_ln_bwd_rows": (c_int, [P, P, P, P, P, P, P, P, I, I, I, c_double, U64, U64, P, P, P]),
    "mtvaf_dropout_res_ln_bwd_finish": (c_int, [P, I, I, P, P, P, I, P]),
    "mtvaf_colsum_workspace_bytes": (SZ, [I, I]),
    "mtvaf_colsum": (c_int, [P, I, I, I, P, I, P, SZ, P]),
    "mtvaf_dropout": (c_int, [P, P, L, c_double, U64, U64, P]),
    "mtvaf_crf_workspace_bytes": (SZ, [I, I, I]),
    "mtvaf_crf_nll_fwd": (c_int, [P, P, P, P, P, P, P, I, I, I, P, SZ, P]),
    "mtvaf_crf_nll_bwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, P, SZ, P]),
    "mtvaf_crf_viterbi": (c_int, [P, P, P, P, P, P, P, I, I, I, P]),
    "mtvaf_crf_llh_fwd": (c_int, [P, P, P, P, P, P, P, I, I, I, P, SZ, P]),
    "mtvaf_crf_llh_bwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, P, SZ, P]),
    "mtvaf_crf_marginals": (c_int, [P, P, P, P, P, P, P, I, I, I, P, SZ, P]),
    "mtvaf_split_mean": (c_int, [P, P, L, I, P]),
    "mtvaf_gate_fwd": (c_int, [P, P, L, P]),
    "mtvaf_prompt_mix_fwd": (c_int, [P, P, P, I, I, I, I, I, P]),
    "mtvaf_prompt_mix_bwd_gate": (c_int, [P, P, P, P, P, P, I, I, I, I, I, P]),
    "mtvaf_prompt_mix_bwd_enc": (c_int, [P, P, P, P, I, I, I, I, I, P]),
    "mtvaf_kl_logsoftmax_fwd": (c_int, [P, P, P, P, I, I, P]),
    "mtvaf_kl_logsoftmax_masked_fwd": (c_int, [P, P, P, P, P, I, I, P]),
    "mtvaf_kl_logsoftmax_masked_bwd": (c_int, [P, F, P, P, P, P, I, I, P]),
    "mtvaf_kl_logsoftmax_bwd": (c_int, [P, F, P, P, P, I, I, P]),
    "mtvaf_mean_l_fwd": (c_int, [P, P, L, I, I, P]),
    "mtvaf_mean_l_bwd": (c_int, [P, P, L, I, I, P]),
    "mtvaf_span_index_ints": (SZ, [I, I, I]),
    "mtvaf_span_index": (c_int, [P, P, P, P, I, I, I, P]),
    "mtvaf_span_pool_fwd": (c_int, [P, P, P, P, P, P, I, I, I, I, P]),
    "mtvaf_span_pool_bwd_workspace_bytes": (SZ, [I, I, I, I]),
    "mtvaf_span_pool_bwd": (c_int, [P, P, P, P, P, P, P, P, P, P, I, I, I, I, P, SZ, P]),
    "mtvaf_distant_ce_fwd": (c_int, [P, I, P, P, P, I, I, F, I, P]),
    "mtvaf_distant_ce_bwd": (c_int, [P, F, P, I, P, P, P, I, I, I, P]),
    "mtvaf_ce_fwd": (c_int, [P, P, P, P, I, I, P]),
    "mtvaf_ce_bwd": (c_int, [P, P, P, P, P, I, I, P]),
    "mtvaf_js_consistency_fwd": (c_int, [P, P, P, P, P, I, I, I, F, P]),
    "mtvaf_js_consistency_bwd": (c_int, [P, F, P, P, P, P, P, I, I, I, P]),
    "mtvaf_token_divergence_fwd": (c_int, [P, P, P, P, P, I, I, I, F, I, I, F, P]),
    "mtvaf_token_divergence_bwd": (c_int, [P, P, P, P, P, P, I, I, I, F, I, I, F, P]),
    "mtvaf_token_ce_fwd": (c_int, [P, P, P, P, P, P, P, I, I, L, F, F, I, I, F, P]),
    "mtvaf_token_ce_bwd": (c_int, [P, P, P, P, P, P, P, I, I, L, F, F, I, I, F, P]),
    "mtvaf_token_argmax": (c_int, [P, P, P, P, P, I, I, P]),
    "mtvaf_span_propose": (c_int, [P, I, P, P, P, P, P, P, P, I, I, I, I, F, I, I, P]),
    "mtvaf_entity_counts": (c_int, [P, I, P, P, P, P, P, P, I, I, I, I, P, P]),
    "mtvaf_span_counts": (c_int, [P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, P, P, P, P]),
    "mtvaf_crf_nbest_workspace_bytes": (SZ, [I, I, I, I]),
    "mtvaf_crf_nbest": (c_int, [P, P, P, P, P, I, P, P, P, P, I, I, I, P, SZ, P]),
    "mtvaf_crf_sample_workspace_bytes": (SZ, [I, I, I, I]),
    "mtvaf_crf_sample": (c_int, [P, P, P, P, P, I, P, U64, U64, P, P, P, P, I, I, I, P, SZ, P]),
    "mtvaf_entity_counts_rows": (c_int, [P, I, I, P, P, P, P, P, P, I, I, I, I, P, P]),
    "mtvaf_crf_entities": (c_int, [P, P, P, I, P, P, P, P, P, P, P, I, P, P, P, I, I, I, I, P]),
    "mtvaf_crf_chunk_posteriors_workspace_bytes": (SZ, [I, I, I]),
    "mtvaf_crf_chunk_posteriors": (c_int, [P, P, P, P, P, P, P, P, P, P, I, I, P, P, I, I, I, P, SZ, P]),
    "mtvaf_calibration_workspace_bytes": (SZ, [I, I, I]),
    "mtvaf_chunk_calibration": (c_int, [P, P, P, P, P, P, P, P, I, I, I, I, I, I, P, P, SZ, P]),
    "mtvaf_entity_calibration": (c_int, [P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, P, P, SZ, P]),
    "mtvaf_crf_lattice_workspace_bytes": (SZ, [I, I, I]),
    "mtvaf_crf_lattice_fwd": (c_int, [P, P, P, P, P, P, P, P, P, I, I, I, P, SZ, P]),
    "mtvaf_crf_lattice_bwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, P, SZ, P]),
    "mtvaf_crf_lattice_marginals": (c_int, [P, P, P, P, P, P, P, P, I, I, I, P, SZ, P]),
    "mtvaf_crf_lattice_viterbi": (c_int, [P, P, P, P, P, P, P, P, P, I, I, I, P]),
    "mtvaf_crf_risk_workspace_bytes": (SZ, [I, I, I]),
    "mtvaf_crf_risk_fwd": (c_int, [P, P, P, P, P, P, P, P, P, I, I, I, P, SZ, P]),
    "mtvaf_crf_risk_bwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, P, SZ, P]),
    "mtvaf_crf_path_workspace_bytes": (SZ, [I, I, I]),
    "mtvaf_crf_path_fwd": (c_int, [P, P, P, P, P, P, P, P, P, I, I, I, P, SZ, P]),
    "mtvaf_crf_path_bwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, P, SZ, P]),
    "mtvaf_mask_mul": (c_int, [P, P, P, P, I, I, I, P]),
    "mtvaf_gemm_bf16x": (c_int, [I, I, P, I, P, I, P, I, P, I, I, I, I, P, I, P, I, I, P, I, P, SZ, I, I, I, P]),
    "mtvaf_gemm_bf16x_ktiles": (c_int, [I, I, P, I, P, I, P, I, P, I, I, I, I, P, I, P, I, I, P, I, P, SZ, I, I, I, P, P, P]),
    "mtvaf_colsum_small": (c_int, [P, I, I, P, I, P]),
    "mtvaf_embed_scatter_mode": (c_int, [I]),
    "mtvaf_embed_ln_bwd_workspace_bytes": (SZ, [I, I, I, I]),
    "mtvaf_gemm_f32_dw_group": (c_int, [I, P, P, P, P, P, P, P, P, I, P, P, P, SZ, I, P]),
    "mtvaf_gemm_f32_dw_group_bias": (c_int, [I, P, P, P, P, P, P, P, P, I, P, P, P, P, SZ, I, P]),
    "mtvaf_gemm_f32_dw_group_acc": (c_int, [I, P, P, P, P, P, P, P, P, I, P, P, P, P, SZ, I, I, P]),
    "mtvaf_gemm_f32_dw_group_workspace_bytes": (SZ, [I, P, P, I, I]),
    "mtvaf_dw_group_rows": (c_int, [I]),
    "mtvaf_dw_group_wanted": (c_int, [I, I, I]),
    "mtvaf_streamk_attach": (c_int, [P, SZ, P]),
    "mtvaf_streamk_scratch_bytes": (SZ, [I]),
    "mtvaf_streamk_attached": (c_int, [P]),
    "mtvaf_gemm_bf16x_dw_group": (c_int, [I, P, P, P, P, P, P, P, P, I, P]),
    "mtvaf_gemm_bf16x_dw_group_acc": (c_int, [I, P, P, P, P, P, P, P, P, I, I, P]),
    "mtvaf_gemm_bf16x_dw_group_pieces": (c_int, [I, P, P, I, P]),
    "mtvaf_cast_bf16": (c_int, [P, I, P, I, P, I, I, I, P]),
    "mtvaf_adamw": (c_int, [P, P, P, P, L, F, c_double, c_double, F, F, F, F, F, P, I, P]),
    "mtvaf_adamw_planes": (c_int, [P, P, P, P, L, F, c_double, c_double, F, F, F, F, F, I, P, P, P, P, I, P]),
    "mtvaf_adamw_multi": (c_int, [I, P, P, P, P, P, F, c_double, c_double, F, F, F, F, F, P]),
    "mtvaf_grad_sqnorm_workspace_bytes": (SZ, [I, P]),
    "mtvaf_grad_sqnorm_multi": (c_int, [I, P, P, P, SZ, P]),
    "mtvaf_grad_clip_finalize": (c_int, [P, L, F, I, P, P, P]),
    "mtvaf_adamw_dev": (c_int, [P, P, P, P, L, F, c_double, c_double, F, F, F, F, F, P, I, P, P]),
    "mtvaf_adamw_planes_dev": (c_int, [P, P, P, P, L, F, c_double, c_double, F, F, F, F, F, I, P, P, P, P, I, P, P]),
    "mtvaf_adamw_multi_dev": (c_int, [I, P, P, P, P, P, F, c_double, c_double, F, F, F, F, F, P, P]),
    "mtvaf_adamw_ema": (c_int, [P, P, P, P, L, F, c_double, c_double, F, F, F, F, F, P, I, P, F, P, P]),
    "mtvaf_adamw_planes_ema": (c_int, [P, P, P, P, L, F, c_double, c_double, F, F, F, F, F, I, P, P, P, P, I, P, F, P, P]),
    "mtvaf_adamw_multi_ema": (c_int, [I, P, P, P, P, P, F, c_double, c_double, F, F, F, F, F, P, F, P, P]),
    "mtvaf_swap_f32_multi": (c_int, [I, P, P, P, P]),
    "mtvaf_adamw_seg": (c_int, [P, P, P, P, L, I, P, P, P, c_double, c_double, F, F, F, F, P, I, P, F, P, P]),
    "mtvaf_adamw_planes_seg": (c_int, [P, P, P, P, L, I, P, P, P, c_double, c_double, F, F, F, F, I, P, P, P, P, I, P, F, P, P]),
    "mtvaf_adamw_sched_advance": (c_int, [P, L, P, P, P]),
    "mtvaf_adamw_sched": (c_int, [P, P, P, P, L, c_double, c_double, c_double, F, F, F, P, I, P, P, P, P]),
    "mtvaf_adamw_planes_sched": (c_int, [P, P, P, P, L, c_double, c_double, c_double, F, F, F, I, P, P, P, P, I, P, P, P, P]),
    "mtvaf_adamw_multi_sched": (c_int, [I, P, P, P, P, P, c_double, c_double, c_double, F, F, F, P, P, P, P]),
    "mtvaf_adamw_seg_sched": (c_int, [P, P, P, P, L, I, P, P, P, c_double, c_double, F, F, P, I, P, P, P, P]),
    "mtvaf_adamw_planes_seg_sched": (c_int, [P, P, P, P, L, I, P, P, P, c_double, c_double, F, F, I, P, P, P, P, I, P, P, P, P]),
    "mtvaf_grad_pack_bf16": (c_int, [P, P, L, L, P]),
    "mtvaf_grad_reduce_bf16": (c_int, [P, P, I, L, F, P]),
    "mtvaf_grad_unpack_bf16": (c_int, [P, P, L, P]),
    "mtvaf_adv_workspace_bytes": (SZ, [I, I]),
    "mtvaf_adv_perturb": (c_int, [P, P, P, P, P, P, P, I, I, I, F, F, I, I, P, SZ, P]),
    "mtvaf_adv_add": (c_int, [P, P, P, L, P]),
    "mtvaf_sam_finalize": (c_int, [P, L, F, P, P, P]),
    "mtvaf_sam_perturb": (c_int, [P, P, P, L, P, P, P]),
    "mtvaf_sam_perturb_planes": (c_int, [P, P, P, L, P, I, P, P, P, P, P]),
    "mtvaf_sam_perturb_multi": (c_int, [I, P, P, P, P, P, P]),
    "mtvaf_sam_restore": (c_int, [P, P, L, P, P]),
    "mtvaf_sam_restore_planes": (c_int, [P, P, L, I, P, P, P, P, P]),
    "mtvaf_sam_restore_multi": (c_int, [I, P, P, P, P]),
    "mtvaf_word_index": (c_int, [P, P, P, P, P, P, P, P, I, I, I, P]),
    "mtvaf_word_pool_fwd": (c_int, [P, P, P, P, I, I, I, I, I, P]),
    "mtvaf_word_pool_bwd": (c_int, [P, P, P, P, P, I, I, I, I, I, P]),
    "mtvaf_layer_mix_fwd": (c_int, [P, I, P, P, P, L, I, P]),
    "mtvaf_layer_mix_dots": (c_int, [P, I, P, P, P, L, I, P, L, P, P, P, P]),
    "mtvaf_layer_mix_inject": (c_int, [P, I, I, P, P, L, I, I, P]),
    "mtvaf_uniform_fill": (c_int, [P, L, U64, U64, P]),
    "mtvaf_mlm_mask_workspace_bytes": (SZ, [I]),
    "mtvaf_mlm_mask": (c_int, [P, P, P, P, P, I, F, L, I, I, P, P, P, P, P, P, SZ, I, I, P]),
    "mtvaf_scatter_rows": (c_int, [P, P, P, I, I, I, P]),
    "mtvaf_dgelu": (c_int, [P, P, P, L, P]),
    "mtvaf_vocab_ce_workspace_bytes": (SZ, [I, I, I, I]),
    "mtvaf_vocab_ce_chunk_fwd": (c_int, [P, I, P, P, P, P, I, I, I, I, P]),
    "mtvaf_vocab_ce_finish": (c_int, [P, P, P, P, P, P, P, I, I, I, P]),
    "mtvaf_vocab_ce_chunk_bwd": (c_int, [P, I, P, P, P, P, P, P, P, I, I, I, I, I, P]),
}

class LayerStruct(ctypes.Structure):
    """mtvaf_layer_t (include/mtvaf_hip.h): one encoder layer's shapes, parameters, input and activation buffers."""
    _fields_ = ([(n, c_int) for n in ("B", "S", "P", "NH", "H", "I", "bf16")] +
                [("eps", c_float), ("p_hidden", c_double), ("p_attn", c_float)] + [("seed", c_uint64), ("offset", c_uint64)] +
                [(n, c_void_p) for n in ("wqkv", "wo", "w1", "w2", "wqkv_h", "wo_h", "w1_h", "w2_h", "bqkv", "bo", "g1", "b1",
                                         "bi1", "bi2", "g2", "b2", "x", "x_h", "pk", "pv", "addmask", "qkv", "cx", "lse", "a",
                                         "h1", "h1_h", "mean1", "rstd1", "pre", "act", "f", "h2", "h2_h", "mean2", "rstd2",
                                         "ws")] + [("ws_bytes", c_size_t), ("cu", c_void_p), ("Mv", c_int), ("Mp", c_int)] +
                [(n, c_void_p) for n in ("x_p", "cx_p", "h1_p", "act_p", "h2_p", "pmask")])


class LayerGradsStruct(ctypes.Structure):
    """mtvaf_layer_grads_t: gradient in / out, temporaries, parameter-gradient destinations, per-stream scratch."""
    _fields_ = ([(n, c_void_p) for n in ("dh", "dh1", "df", "dpre", "da", "dctx", "dqkv", "part", "partq", "partkv", "delta",
                                         "dwqkv", "dbqkv", "dwo", "dbo", "dg1", "db1", "dw1", "dbi1", "dw2", "dbi2", "dg2",
                                         "db2", "dpk", "dpv", "ws_main")] + [("ws_main_bytes", c_size_t), ("ws_side", c_void_p),
                                                                            ("ws_side_bytes", c_size_t), ("klist", c_void_p),
                                                                            ("kcnt", c_void_p), ("zero_tail", c_int),
                                                                            ("lnpart2", c_void_p), ("lnpart1", c_void_p)] +
                [(n, c_void_p) for n in ("df_p", "dpre_p", "da_p", "dqkv_p")] + [("accumulate", c_int)])


_lib = None


def lib():
    """Load (once) and return the shared library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"mtvaf_amd: HIP extension {LIB_PATH} not found -- run `python -m mtvaf_amd.build` "
                "(there is no CPU fallback for the product path)")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        if (l.mtvaf_layer_struct_bytes(0), l.mtvaf_layer_struct_bytes(1)) != (ctypes.sizeof(LayerStruct), ctypes.sizeof(LayerGradsStruct)):
            raise RuntimeError("mtvaf_amd: the ctypes mirrors of mtvaf_layer_t / mtvaf_layer_grads_t do not match the library")
        _lib = l
    return _lib


def exported_symbols():
    return sorted(_SIGS)


def _p(t: Optional[torch.Tensor]):
    """Device pointer of a tensor handed to a kernel.  A host tensor here would be dereferenced by the GPU (a memory fault that
    takes the process -- and on a shared host possibly more -- down): there is no CPU fallback, so it is an error, loudly."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"mtvaf_amd: a {t.device} tensor reached a HIP kernel -- the path has no CPU fallback; move the "
                           "model and its inputs to the GPU")
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


STREAM_OVERRIDE = None  # raw hipStream_t: set by the native executor around hooks that only enqueue library kernels


def _st():
    """hipStream_t of torch's current stream on the current device (one C call: torch.cuda.current_stream() builds a
    Stream object and costs ~8 us, which adds up over ~130 launches per step in the launch-bound configurations)."""
    if STREAM_OVERRIDE is not None:
        return STREAM_OVERRIDE
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _ck(rc: int, name: str):
    if rc != 0:
        msg = _ERR.get(rc, f"hipError {rc}" if rc > 0 else f"error {rc}")
        raise RuntimeError(f"{name} failed: {msg}")


def _f32(*ts):
    for t in ts:
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), (t.device, t.dtype, t.is_contiguous())


# -------------------------------------------------------------------------------------------------
# workspace: one growing scratch buffer per device (the library never allocates)
# -------------------------------------------------------------------------------------------------
_ws = {}


def workspace(nbytes: int, device) -> torch.Tensor:
    """Scratch for split-K slabs / column-sum partials, one buffer per (device, stream): kernels launched on a side
    stream (the weight-gradient products of the encoder backward) must not share slabs with the main stream."""
    key = (torch.device(device).index or 0, _st() if _lib is not None else 0)
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 64 << 20), dtype=torch.uint8, device=device)
        _ws[key] = buf
    return buf


PROFILE = None  # set to a list to record (key, start_event, stop_event) around every GEMM call (incl. reduce)


def prof_start(capacity: int = 4096):
    """Start the in-library launch profiler (HIP events around each main GEMM kernel, on its stream)."""
    _ck(lib().mtvaf_prof_start(capacity), "mtvaf_prof_start")


def prof_stop(capacity: int = 4096):
    """-> list of (key dict, ms).  Synchronises the recorded events."""
    n = ctypes.c_int(0)
    keys = (ctypes.c_int * (8 * capacity))()
    ms = (ctypes.c_float * capacity)()
    _ck(lib().mtvaf_prof_stop(ctypes.byref(n), keys, ms, capacity), "mtvaf_prof_stop")
    out = []
    for i in range(n.value):
        k = keys[8 * i:8 * i + 8]
        out.append((dict(cfg=k[0], la=k[1], lb=k[2], fast=k[3], M=k[4], N=k[5], K=k[6], splits=k[7]), ms[i]))
    return out


def kernel_symbol(cfg, la, lb, fast):
    """The template instantiation rocprofv3 reports for a (tile cfg, layouts, fast) launch."""
    dims = {0: (128, 128, 2, 2, 16), 1: (128, 96, 4, 1, 16), 2: (128, 288, 4, 1, 16), 3: (64, 64, 2, 2, 16),
            4: (128, 64, 4, 1, 16), 5: (128, 128, 2, 2, 32), 6: (128, 96, 4, 1, 32), 7: (128, 192, 2, 2, 16),
            8: (128, 192, 2, 2, 32), 9: (128, 96, 4, 1), 10: (128, 128, 2, 2), 11: (128, 192, 2, 2),
            12: (128, 96, 4, 1), 13: (128, 128, 2, 2), 14: (128, 64, 4, 1), 15: (128, 64, 4, 1),
            16: (64, 64, 2, 2), 17: (64, 64, 2, 2)}.get(cfg)
    b = lambda x: "true" if x else "false"
    klist, fast = bool(fast & 8), fast & 7  # (+8: the launch walked a k-tile list)
    if cfg == 1225:  # the grouped weight-gradient launch of the wave-specialised split kernel (mtvaf_gemm_f32_dw_group)
        return f"gemm_f32x3_ws_kernel<true, true, {b(klist)}, 128, true>"
    if cfg >= 1000:  # the grouped weight-gradient launch of the fp32 LDS-DMA kernel (mtvaf_gemm_f32_dw_group)
        return f"gemm_f32_dma_group_kernel<128, 96, 4, 1, 2, {b(klist)}>"
    if 400 <= cfg < 500:  # pre-split operands (csrc/gemm_f32p.hip): gemm_f32p16_kernel<ABL, TRACE, B_KM, A_KM, GROUP>
        c = cfg - 400
        if c & 32:  # the 128 x 256 tile (csrc/gemm_f32pw.hip): gemm_f32p16w_kernel<B_KM, A_KM, GROUP, ABL, TRACE>
            return f"gemm_f32p16w_kernel<{b(c & 8)}, {b(c & 4)}, {b(c & 16)}, 0, false, {6 if c & 64 else 8}>"
        return f"gemm_f32p16_kernel<0, false, {b(c & 8)}, {b(c & 4)}, {b(c & 16)}>"
    if cfg >= 300:  # gemm_bf16x_kernel<BM, BN, WM, WN, A_KM, B_KM, NSTAGE, KLIST>
        c = cfg - 300
        if c & 64:  # gemm_bf16_p256_kernel<A_KM, B_KM, SK> (+128: the in-launch-combine form, +256: a grouped launch)
            return f"gemm_bf16_p256_kernel<{b(c & 4)}, {b(c & 8)}, {b(c & 128)}>"
        t = "256, 192, 4, 2" if c & 32 else ("256, 128, 4, 2" if c & 16 else ("128, 128, 2, 2" if c & 1 else "128, 96, 4, 1"))
        return f"gemm_bf16x_kernel<{t}, {b(c & 4)}, {b(c & 8)}, {3 if c & 2 else 2}, {b(klist)}>"
    if cfg >= 200:  # split-fp32 kernels (csrc/gemm_f32x3.hip): +20 the wave-specialised kernel
        if cfg in (224, 225, 226):
            bn = {224: 64, 225: 128, 226: 96}[cfg]
            return f"gemm_f32x3_ws_kernel<{b(la)}, {b(lb)}, {b(klist)}, {bn}, false>"
        d = (64, 64, 2, 2) if cfg == 203 else ((128, 96, 4, 1) if cfg == 206 else (128, 128, 2, 2))
        return f"gemm_f32x3_kernel<{d[0]}, {d[1]}, {d[2]}, {d[3]}, {b(la)}, {b(lb)}, {b(klist)}, 32>"
    if cfg >= 100:
        d = {106: (128, 96, 4, 1), 105: (128, 128, 2, 2), 103: (64, 64, 2, 2)}[cfg]
        return f"gemm_bf16_kernel<{d[0]}, {d[1]}, {d[2]}, {d[3]}, {b(la)}, {b(lb)}, {b(fast == 2)}>"
    if cfg >= 9:
        return (f"gemm_f32_dma_kernel<{dims[0]}, {dims[1]}, {dims[2]}, {dims[3]}, {b(la)}, {b(lb)}, "
                f"{2 if cfg in (12, 13, 15, 17) else 3}, {b(klist)}>")
    return (f"gemm_f32_kernel<{dims[0]}, {dims[1]}, {dims[2]}, {dims[3]}, {dims[4]}, {b(la)}, {b(lb)}, "
            f"{b(fast >= 1)}, {b(fast == 2)}>")
TILE_NAMES = {0: "128x128x16", 1: "128x96x16", 2: "128x288x16", 3: "64x64x16", 4: "128x64x16", 5: "128x128x32",
              6: "128x96x32", 7: "128x192x16", 8: "128x192x32", 9: "128x96x32dma", 10: "128x128x32dma",
              11: "128x192x32dma", 12: "128x96x32dma2", 13: "128x128x32dma2", 14: "128x64x32dma", 15: "128x64x32dma2",
              16: "64x64x32dma", 17: "64x64x32dma2"}


def gemm_plan(M, N, K, allow_split, layout_a=0, layout_b=0, epi=0):
    c, s = ctypes.c_int(0), ctypes.c_int(0)
    _ck(lib().mtvaf_gemm_f32_plan(layout_a, layout_b, M, N, K, epi, int(allow_split), ctypes.byref(c), ctypes.byref(s)),
        "mtvaf_gemm_f32_plan")
    return c.value, s.value


KC, KM = 0, 1
EPI_NONE, EPI_GELU, EPI_TANH, EPI_DGELU, EPI_DTANH = 0, 1, 2, 3, 4
# GEMM arithmetic: "fp32" (v_mfma_f32_32x32x2_f32) or "bf16" (operands rounded to bf16 while staged, fp32
# accumulation; buffers stay fp32).  Set per call or process-wide through set_compute_dtype().
COMPUTE = "fp32"


def f32_split(on=None) -> bool:
    """fp32-mode GEMMs on the bf16 matrix pipe by three-way operand splitting (csrc/gemm_f32x3.hip: six exact bf16 partial
    products per fp32 product, fp32 accumulate; operands and results stay fp32).  on = True / False switches every
    mtvaf_gemm_f32 / _ktiles call of the process (Python orchestration and native executor alike); None queries.
    Default: ON (MTVAF_F32_SPLIT=0 in the environment keeps the fp32 MFMA pipe)."""
    return bool(lib().mtvaf_f32_split(-1 if on is None else int(bool(on))))


def f32p_wide(mask=None) -> int:
    """The pre-split GEMM's tiles (csrc/gemm_f32pw.hip, round 6): a mask of the products that may leave the 128 x 128 tile -- 1 forward
    (128 x 256, or 128 x 192 without a plane-image result), 2 dX, 4 weight gradients; a launch takes the cheapest admitted tile by the
    library's rounds x tile-time estimate; 8 = never 128 x 128 where another tile can serve (tests), 16 = never 128 x 192; True = 15,
    False = 0, None queries.  Placement only: the kernels agree bit for bit.  Default: 7."""
    if mask is True:
        mask = 15
    return int(lib().mtvaf_f32p_wide(-1 if mask is None else int(mask)))


class Planes:
    """Plane image of an fp32 matrix [rows, cols] (csrc/gemm_f32p.hip): the three bf16 planes of the split, `blocked` =
    [k-tile][plane][rows][32] (every 1-KiB request of the kernel reads contiguous memory) or natural [3][rows][cols]."""
    __slots__ = ("img", "s_plane", "s_row", "s_kt", "rows", "cols")

    def __init__(self, x: torch.Tensor, blocked: bool = True, fill: bool = True):
        rows, cols = x.shape
        self.rows, self.cols = rows, cols
        self.img = torch.empty(3 * rows * cols, dtype=torch.bfloat16, device=x.device)
        if blocked:
            self.s_plane, self.s_row, self.s_kt = rows * 64, 64, 3 * rows * 64
        else:
            self.s_plane, self.s_row, self.s_kt = rows * cols * 2, cols * 2, 64
        if fill:  # (False: an image some kernel is about to write; x only gives the shape)
            self.refresh(x)

    def refresh(self, x: torch.Tensor):
        _ck(lib().mtvaf_f32_split_planes(_p(x), _p(self.img), self.rows, self.cols, x.stride(0), self.s_plane, self.s_row, self.s_kt,
                                         _st()), "mtvaf_f32_split_planes")


def gemm_planes_ep(a: "Planes", b: "Planes", out_planes: "Planes", out=None, bias=None, epi=EPI_NONE, aux=None, colpart=None, layout_b=KC):
    """mtvaf_gemm_f32p_ep: the product of two plane images written as the (tile-blocked) plane image `out_planes` -- and as fp32 `out`
    too unless None; colpart [M / 128, N]: per-tile column sums."""
    if layout_b == KM:
        M, N, K = a.rows, b.cols, a.cols
        bs = _km_strides(b)
    else:
        M, N, K = a.rows, b.rows, a.cols
        bs = (b.s_plane, b.s_row, b.s_kt, 0)
    assert (out_planes.rows, out_planes.cols) == (M, N) and out_planes.s_row == 64, "the result image is tile-blocked"
    _ck(lib().mtvaf_gemm_f32p_ep(KC, _p(a.img), a.s_plane, a.s_row, a.s_kt, 0, layout_b, _p(b.img), bs[0], bs[1], bs[2], bs[3], _p(out),
                                 out.stride(0) if out is not None else 0, _p(out_planes.img), _p(colpart), M, N, K, _p(bias), epi, _p(aux),
                                 aux.stride(0) if aux is not None else 0, 0, _st()), "mtvaf_gemm_f32p_ep")
    return out_planes


def gemm_planes(a: Planes, b: Planes, out, bias=None, epi=EPI_NONE, aux=None, accumulate=False, splits=1, ablate=0, layout_b=KC,
                layout_a=KC):
    """out[M,N] = A[M,K] . B[N,K]^T (layout_b = KC) or A[M,K] . B[K,N] (layout_b = KM: `b` is the plane image of the [K, N]
    matrix, natural or tile-blocked) from the plane images of both operands (mtvaf_gemm_f32p)."""
    if layout_a == KM:  # weight gradients: out[M,N] = A[K,M]^T . B[K,N] (natural or tile-blocked images)
        assert layout_b == KM and a.rows == b.rows
        M, N, K = a.cols, b.cols, a.rows
        as_, bs = _km_strides(a), _km_strides(b)
    elif layout_b == KM:
        M, N, K = a.rows, b.cols, a.cols
        assert b.rows == K, "k-major B: the plane image of the [K, N] matrix"
        as_ = (a.s_plane, a.s_row, a.s_kt, 0)
        bs = _km_strides(b)
    else:
        M, N, K = a.rows, b.rows, a.cols
        as_ = (a.s_plane, a.s_row, a.s_kt, 0)
        bs = (b.s_plane, b.s_row, b.s_kt, 0)
    ws, wsb = None, 0
    if splits > 1:
        wsb = splits * M * N * 4
        ws = workspace(wsb, out.device)
    _ck(lib().mtvaf_gemm_f32p(layout_a, _p(a.img), as_[0], as_[1], as_[2], as_[3], layout_b, _p(b.img), bs[0], bs[1], bs[2], bs[3], _p(out),
                              out.stride(0), M, N, K,
                              _p(bias), epi, _p(aux), aux.stride(0) if aux is not None else 0, int(accumulate), splits, _p(ws), wsb,
                              ablate, _st()), "mtvaf_gemm_f32p")
    return out


def gemm_planes_slabs(a: Planes, b: Planes, out, ws, bias=None, accumulate=False, splits=1, layout_b=KC) -> int:
    """mtvaf_gemm_f32p_slabs: gemm_planes with a plain epilogue that leaves a split-K plan's slabs unreduced in the caller's fp32
    workspace `ws` (None: no workspace).  -> the number of slabs s: 1 = `out` holds the result (+ bias, accumulate); s > 1 = ws holds s
    slabs [M][N], neither bias nor accumulate applied, `out` untouched (the LayerNorm kernel behind the product adds them)."""
    if layout_b == KM:
        M, N, K = a.rows, b.cols, a.cols
        bs = _km_strides(b)
    else:
        M, N, K = a.rows, b.rows, a.cols
        bs = (b.s_plane, b.s_row, b.s_kt, 0)
    ns = ctypes.c_int(0)
    _ck(lib().mtvaf_gemm_f32p_slabs(KC, _p(a.img), a.s_plane, a.s_row, a.s_kt, 0, layout_b, _p(b.img), bs[0], bs[1], bs[2], bs[3], _p(out),
                                    out.stride(0), M, N, K, _p(bias), int(accumulate), splits, _p(ws),
                                    ws.numel() * ws.element_size() if ws is not None else 0, ctypes.byref(ns), _st()),
        "mtvaf_gemm_f32p_slabs")
    return ns.value


def split_planes_blocked(x: torch.Tensor, out: torch.Tensor):
    """fp32 [rows, cols] (contiguous) -> its tile-blocked plane image [cols / 32][3][rows][32] bf16 in `out` (6 rows cols bytes)."""
    rows, cols = x.shape
    _ck(lib().mtvaf_f32_split_planes(_p(x), _p(out), rows, cols, x.stride(0), rows * 64, 64, 3 * rows * 64, _st()), "mtvaf_f32_split_planes")
    return out


def _km_strides(pl: "Planes"):
    """(plane, k-row, k-tile, 128-column block) byte strides of a plane image read K-MAJOR (its rows are the reduction index)."""
    if pl.s_row == pl.cols * 2:  # natural [3][rows][cols]
        return (pl.s_plane, pl.s_row, 32 * pl.s_row, 256)
    return (pl.s_plane, 64, 32 * 64, 4 * pl.s_kt)  # tile-blocked [cols / 32][3][rows][32]: a 32-column block is pl.s_kt apart


def gemm_planes_dw_group(items, colsum=None, accumulate=False):
    """items: up to four (a: Planes of dY [K, M], b: Planes of X [K, N], out [M, N] fp32): out = dY^T . X for each, one unsplit launch
    (mtvaf_gemm_f32p_dw_group; natural or tile-blocked images).  colsum = (src fp32 [K, C], dst [C]): dst = column sums of src, as
    extra blocks of the same launch; or a list of up to eight such pairs.  accumulate: every out and every dst is ADDED to (the value the
    overwriting form stores, then one add of the old value: mtvaf_gemm_f32p_dw_group_acc)."""
    n = len(items)
    K = items[0][0].rows
    assert all(a.rows == K and b.rows == K for a, b, _ in items)
    vp = lambda ts: (ctypes.c_void_p * n)(*[_p(t) for t in ts])
    ia = lambda xs: (ctypes.c_int * n)(*xs)
    st = []
    for a, b, _ in items:
        st += list(_km_strides(a)) + list(_km_strides(b))
    if accumulate:
        jobs = [] if colsum is None else ([colsum] if isinstance(colsum, tuple) else list(colsum))
        nj = len(jobs)
        pj = lambda ts: (ctypes.c_void_p * max(nj, 1))(*[_p(t) for t in ts])
        ij = lambda xs: (ctypes.c_int * max(nj, 1))(*xs)
        _ck(lib().mtvaf_gemm_f32p_dw_group_acc(n, vp([a.img for a, _, _ in items]), vp([b.img for _, b, _ in items]),
                                               (ctypes.c_long * (8 * n))(*st), vp([o for _, _, o in items]),
                                               ia([o.stride(0) for _, _, o in items]), ia([a.cols for a, _, _ in items]),
                                               ia([b.cols for _, b, _ in items]), K, nj, pj([s_ for s_, _ in jobs]),
                                               ij([s_.shape[0] for s_, _ in jobs]), ij([s_.shape[1] for s_, _ in jobs]),
                                               ij([s_.stride(0) for s_, _ in jobs]), pj([d for _, d in jobs]), 1, _st()),
            "mtvaf_gemm_f32p_dw_group_acc")
        return
    if colsum is not None:
        jobs = [colsum] if isinstance(colsum, tuple) else list(colsum)
        nj = len(jobs)
        pj = lambda ts: (ctypes.c_void_p * nj)(*[_p(t) for t in ts])
        ij = lambda xs: (ctypes.c_int * nj)(*xs)
        _ck(lib().mtvaf_gemm_f32p_dw_group_colsum(n, vp([a.img for a, _, _ in items]), vp([b.img for _, b, _ in items]),
                                                  (ctypes.c_long * (8 * n))(*st), vp([o for _, _, o in items]),
                                                  ia([o.stride(0) for _, _, o in items]), ia([a.cols for a, _, _ in items]),
                                                  ia([b.cols for _, b, _ in items]), K, nj, pj([s_ for s_, _ in jobs]),
                                                  ij([s_.shape[0] for s_, _ in jobs]), ij([s_.shape[1] for s_, _ in jobs]),
                                                  ij([s_.stride(0) for s_, _ in jobs]), pj([d for _, d in jobs]), _st()),
            "mtvaf_gemm_f32p_dw_group_colsum")
        return
    _ck(lib().mtvaf_gemm_f32p_dw_group(n, vp([a.img for a, _, _ in items]), vp([b.img for _, b, _ in items]), (ctypes.c_long * (8 * n))(*st),
                                       vp([o for _, _, o in items]), ia([o.stride(0) for _, _, o in items]), ia([a.cols for a, _, _ in items]),
                                       ia([b.cols for _, b, _ in items]), K, _st()), "mtvaf_gemm_f32p_dw_group")


def set_compute_dtype(dtype: str):
    global COMPUTE
    if dtype not in ("fp32", "bf16"):
        raise ValueError(dtype)
    COMPUTE = dtype


def gemm(a: torch.Tensor, layout_a: int, b: torch.Tensor, layout_b: int, out: torch.Tensor, M: int, N: int, K: int,
         bias: Optional[torch.Tensor] = None, epi: int = EPI_NONE, aux: Optional[torch.Tensor] = None,
         accumulate: bool = False, allow_split: bool = False, lda: Optional[int] = None, ldb: Optional[int] = None,
         ldc: Optional[int] = None, cfg: int = -1, splits: int = -1, compute: Optional[str] = None):
    """out[M,N] = opA[M,K] . opB[K,N] (+bias, epilogue).  KC: reduction index contiguous; KM: k-major."""
    _f32(a, b, out, bias, aux)
    lda = a.stride(0) if lda is None else lda
    ldb = b.stride(0) if ldb is None else ldb
    ldc = out.stride(0) if ldc is None else ldc
    ws, wsb = None, 0
    if allow_split:
        wsb = lib().mtvaf_gemm_f32_workspace_bytes(M, N, K, 1)
        ws = workspace(wsb, out.device)
    prof = PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    mode = compute or COMPUTE
    fn = lib().mtvaf_gemm_bf16 if mode == "bf16" else (lib().mtvaf_gemm_f32x3 if mode == "fp32x3" else lib().mtvaf_gemm_f32)
    _ck(fn(layout_a, layout_b, _p(a), lda, _p(b), ldb, _p(out), ldc, M, N, K, _p(bias), epi, _p(aux),
           aux.stride(0) if aux is not None else 0, int(accumulate), int(allow_split), _p(ws), wsb, cfg, splits, _st()),
        "mtvaf_gemm")
    if prof is not None:
        e1.record()
        prof.append(((layout_a, layout_b, M, N, K, epi, int(allow_split)), e0, e1))
    return out


def gemm_ktiles(a, b, out, M, N, K, klist, kcnt, accumulate=False, cfg=-1, splits=-1):
    """out[M,N] (+)= a[K,M]^T . b[K,N] over the listed 32-row k-tiles only (a is exactly zero elsewhere): klist / kcnt int32."""
    wsb = lib().mtvaf_gemm_f32_workspace_bytes(M, N, K, 1)
    ws = workspace(wsb, out.device)
    _ck(lib().mtvaf_gemm_f32_ktiles(KM, KM, _p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, K, None,
                                    EPI_NONE, None, 0, int(accumulate), 1, _p(ws), wsb, cfg, splits, _p(klist), _p(kcnt), _st()),
        "mtvaf_gemm_f32_ktiles")
    return out


def build_ktiles(addmask, Pn, S, bk=32):
    B, T = addmask.shape
    klist = torch.empty(B * S // bk, dtype=torch.int32, device=addmask.device)
    kcnt = torch.empty(1, dtype=torch.int32, device=addmask.device)
    _ck(lib().mtvaf_build_ktiles(_p(addmask), B, T, Pn, S, bk, _p(klist), _p(kcnt), _st()), "mtvaf_build_ktiles")
    return klist, kcnt


def linear_fwd(x, w, bias, out, epi=EPI_NONE, aux=None):
    """out[M,N] = x[M,K] . w[N,K]^T + bias  (nn.Linear)."""
    M, K = x.shape
    N = w.shape[0]
    # every epilogue may follow the deterministic split-K (few output tiles, long K: e.g. the projector logits
    # [288, 48] x K = 6144, every product of a bs-4 step); the planner only splits when the tile grid underfills the chip
    return gemm(x, KC, w, KC, out, M, N, K, bias=bias, epi=epi, aux=aux, allow_split=True)


def linear_bwd_input(dy, w, dx, accumulate=False, epi=EPI_NONE, aux=None):
    """dx[M,K] (+)= dy[M,N] . w[N,K]"""
    M, N = dy.shape
    K = w.shape[1]
    return gemm(dy, KC, w, KM, dx, M, K, N, accumulate=accumulate, epi=epi, aux=aux,
                allow_split=True)


def linear_bwd_weight(dy, x, dw, accumulate=False, ktiles=None):
    """dw[N,K] (+)= dy[M,N]^T . x[M,K]   (deterministic split-K over M).  ktiles = (klist, kcnt): dy is exactly zero outside
    the listed 32-row k-tiles of the token axis (mtvaf_build_ktiles): the reduction skips the others."""
    M, N = dy.shape
    K = x.shape[1]
    if ktiles is not None and COMPUTE == "fp32":
        return gemm_ktiles(dy, x, dw, N, K, M, ktiles[0], ktiles[1], accumulate=accumulate)
    return gemm(dy, KM, x, KM, dw, N, K, M, accumulate=accumulate, allow_split=True)


def colsum(x, out, accumulate=False):
    rows, cols = x.shape
    wsb = lib().mtvaf_colsum_workspace_bytes(rows, cols)
    ws = workspace(wsb, x.device)
    _ck(lib().mtvaf_colsum(_p(x), rows, cols, x.stride(0), _p(out), int(accumulate), _p(ws), wsb, _st()), "mtvaf_colsum")
    return out


def dropout(x, out, p, seed, offset):
    _ck(lib().mtvaf_dropout(_p(x), _p(out), x.numel(), float(p), seed, offset, _st()), "mtvaf_dropout")
    return out


def embed_ln_fwd(ids, tts, pos_ids, word, pos, typ, gamma, beta, out, mean, rstd, eps, p, seed, offset, out16=None):
    B, S = ids.shape
    H = word.shape[1]
    _ck(lib().mtvaf_embed_ln_fwd(_p(ids), _p(tts), _p(pos_ids), _p(word), _p(pos), _p(typ), _p(gamma), _p(beta), _p(out),
                                 _p(mean), _p(rstd), B, S, H, float(eps), float(p), seed, offset, _p(out16), _st()),
        "mtvaf_embed_ln_fwd")


def embed_ln_bwd(dout, ids, tts, pos_ids, word, pos, typ, gamma, mean, rstd, dword, dpos, dtype, dgamma, dbeta,
                 accumulate, word_pad, pos_pad, p, seed, offset, dz_ws):
    B, S = ids.shape
    H = word.shape[1]
    wsb = lib().mtvaf_embed_ln_bwd_workspace_bytes(B * S, H, word.shape[0], pos.shape[0])
    ws = workspace(wsb, dout.device)
    _ck(lib().mtvaf_embed_ln_bwd(_p(dout), _p(ids), _p(tts), _p(pos_ids), _p(word), _p(pos), _p(typ), _p(gamma), _p(mean),
                                 _p(rstd), _p(dword), _p(dpos), _p(dtype), _p(dgamma), _p(dbeta), int(accumulate), B, S, H,
                                 word.shape[0], pos.shape[0], typ.shape[0], word_pad, pos_pad, float(p), seed, offset,
                                 _p(dz_ws), _p(ws), wsb, _st()), "mtvaf_embed_ln_bwd")


def roberta_position_ids(ids, out, pad_idx):
    B, S = ids.shape
    _ck(lib().mtvaf_roberta_position_ids(_p(ids), _p(out), B, S, pad_idx, _st()), "mtvaf_roberta_position_ids")
    return out


def dropout_res_ln_fwd(x, res, gamma, beta, out, mean, rstd, eps, p, seed, offset, out16=None):
    M, H = x.shape
    _ck(lib().mtvaf_dropout_res_ln_fwd(_p(x), _p(res), _p(gamma), _p(beta), _p(out), _p(mean), _p(rstd), M, H, float(eps),
                                       float(p), seed, offset, _p(out16), _st()), "mtvaf_dropout_res_ln_fwd")


def dropout_res_ln_bwd(dout, x, res, gamma, mean, rstd, dx, dres, dres_accumulate, dgamma, dbeta, accumulate, p, seed,
                       offset, dbias_x=None, dx16=None):
    M, H = x.shape
    wsb = lib().mtvaf_ln_bwd_workspace_bytes(M, H)
    ws = workspace(wsb, x.device)
    _ck(lib().mtvaf_dropout_res_ln_bwd(_p(dout), _p(x), _p(res), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dres),
                                       int(dres_accumulate), _p(dgamma), _p(dbeta), _p(dbias_x), int(accumulate), M, H,
                                       float(p), seed,
                                       offset, _p(ws), wsb, _p(dx16), _st()), "mtvaf_dropout_res_ln_bwd")


def prefix_attn_fwd(qkv, pk, pv, addmask, ctx, lse, B, S, Pn, NH, p, seed, offset):
    _ck(lib().mtvaf_prefix_attn_fwd(_p(qkv), _p(pk), _p(pv), _p(addmask), _p(ctx), _p(lse), B, S, Pn, NH, 64, float(p),
                                    seed, offset, _st()), "mtvaf_prefix_attn_fwd")


def prefix_attn_probs(qkv, pk, addmask, probs, prefix_mass, B, S, Pn, NH, zero_masked_queries=False):
    """probs [B,NH,S,Pn+S] (or None: prefix_mass alone) and prefix_mass [B,NH,S] (or None) <- the attention probabilities of
    qkv [B*S,3H] (Q and K thirds) over [prefix ; text] keys; every element of both is written.  zero_masked_queries: rows of
    queries whose own key is masked are zeros."""
    _f32(qkv, pk, addmask, probs, prefix_mass)
    if probs is None:
        _ck(lib().mtvaf_prefix_attn_mass(_p(qkv), _p(pk), _p(addmask), _p(prefix_mass), B, S, Pn, NH, 64,
                                         int(bool(zero_masked_queries)), _st()), "mtvaf_prefix_attn_mass")
        return
    _ck(lib().mtvaf_prefix_attn_probs(_p(qkv), _p(pk), _p(addmask), _p(probs), _p(prefix_mass), B, S, Pn, NH, 64,
                                      int(bool(zero_masked_queries)), _st()), "mtvaf_prefix_attn_probs")


def prefix_attn_bwd(dctx, qkv, pk, pv, addmask, ctx, lse, delta, dqkv, dpk, dpv, B, S, Pn, NH, p, seed, offset, zero_tail=False):
    """zero_tail: the caller vouches that dctx is exactly zero for the queries behind each sentence's last unmasked position
    (the k-tile-list contract): same bits, the query loops stop there."""
    _ck(lib().mtvaf_prefix_attn_bwd_tail(_p(dctx), _p(qkv), _p(pk), _p(pv), _p(addmask), _p(ctx), _p(lse), _p(delta), _p(dqkv),
                                         _p(dpk), _p(dpv), B, S, Pn, NH, 64, float(p), seed, offset, int(bool(zero_tail)), _st()),
        "mtvaf_prefix_attn_bwd_tail")


def prefix_attn_varlen_fwd(qkv, pk, pv, cu, pad_rows, ctx, lse, B, S, Pn, NH, p, seed, offset):
    """PACKED token rows: cu [B+1] int32 row offsets; the pad_rows rows behind the last sentence are zero-filled."""
    _ck(lib().mtvaf_prefix_attn_varlen_fwd(_p(qkv), _p(pk), _p(pv), _p(cu), int(pad_rows), _p(ctx), _p(lse), B, S, Pn, NH, 64,
                                           float(p), seed, offset, _st()), "mtvaf_prefix_attn_varlen_fwd")


def prefix_attn_varlen_bwd(dctx, qkv, pk, pv, cu, pad_rows, ctx, lse, delta, dqkv, dpk, dpv, B, S, Pn, NH, p, seed, offset):
    _ck(lib().mtvaf_prefix_attn_varlen_bwd(_p(dctx), _p(qkv), _p(pk), _p(pv), _p(cu), int(pad_rows), _p(ctx), _p(lse), _p(delta),
                                           _p(dqkv), _p(dpk), _p(dpv), B, S, Pn, NH, 64, float(p), seed, offset, _st()),
        "mtvaf_prefix_attn_varlen_bwd")


def prefix_attn_bf16_varlen_fwd(qkv16, pk16, pv16, cu, pad_rows, ctx16, lse, B, S, Pn, NH, p, seed, offset):
    _ck(lib().mtvaf_prefix_attn_bf16_varlen_fwd(_p(qkv16), _p(pk16), _p(pv16), _p(cu), int(pad_rows), _p(ctx16), _p(lse), B, S, Pn,
                                                NH, 64, float(p), seed, offset, _st()), "mtvaf_prefix_attn_bf16_varlen_fwd")


def prefix_attn_bf16_varlen_bwd(dctx16, qkv16, pk16, pv16, cu, pad_rows, ctx16, lse, dqkv16, dpk, dpv, partq, partkv, B, S, Pn, NH,
                                p, seed, offset):
    _ck(lib().mtvaf_prefix_attn_bf16_varlen_bwd(_p(dctx16), _p(qkv16), _p(pk16), _p(pv16), _p(cu), int(pad_rows), _p(ctx16),
                                                _p(lse), _p(dqkv16), _p(dpk), _p(dpv), _p(partq), _p(partkv), B, S, Pn, NH, 64,
                                                float(p), seed, offset, _st()), "mtvaf_prefix_attn_bf16_varlen_bwd")


def _pmask_len(pmask):
    if pmask is not None:
        _f32(pmask)
    return 0 if pmask is None else pmask.numel()


def prefix_attn_varlen_fwd_pm(qkv, pk, pv, cu, pad_rows, pmask, ctx, lse, B, S, Pn, NH, p, seed, offset, ctx_planes=None, rows=0):
    """prefix_attn_varlen_fwd with a per-sentence prefix-slot mask: pmask [B,P] fp32 additive (0 = slot present, -10000 = absent;
    the prefix columns of the padded layout's addmask), or None for the unmasked launch.  ctx_planes: the plane image, as the
    _planes form, or None."""
    _ck(lib().mtvaf_prefix_attn_varlen_fwd_pm(_p(qkv), _p(pk), _p(pv), _p(cu), int(pad_rows), _p(pmask), _pmask_len(pmask), _p(ctx),
                                              _p(lse), B, S, Pn, NH, 64, float(p), seed, offset, _p(ctx_planes), int(rows), _st()),
        "mtvaf_prefix_attn_varlen_fwd_pm")


def prefix_attn_varlen_bwd_pm(dctx, qkv, pk, pv, cu, pad_rows, pmask, ctx, lse, delta, dqkv, dpk, dpv, B, S, Pn, NH, p, seed, offset,
                              dqkv_planes=None, rows=0):
    _ck(lib().mtvaf_prefix_attn_varlen_bwd_pm(_p(dctx), _p(qkv), _p(pk), _p(pv), _p(cu), int(pad_rows), _p(pmask), _pmask_len(pmask),
                                              _p(ctx), _p(lse), _p(delta), _p(dqkv), _p(dpk), _p(dpv), B, S, Pn, NH, 64, float(p), seed,
                                              offset, _p(dqkv_planes), int(rows), _st()), "mtvaf_prefix_attn_varlen_bwd_pm")


def prefix_attn_bf16_varlen_fwd_pm(qkv16, pk16, pv16, cu, pad_rows, pmask, ctx16, lse, B, S, Pn, NH, p, seed, offset):
    _ck(lib().mtvaf_prefix_attn_bf16_varlen_fwd_pm(_p(qkv16), _p(pk16), _p(pv16), _p(cu), int(pad_rows), _p(pmask), _pmask_len(pmask),
                                                   _p(ctx16), _p(lse), B, S, Pn, NH, 64, float(p), seed, offset, _st()),
        "mtvaf_prefix_attn_bf16_varlen_fwd_pm")


def prefix_attn_bf16_varlen_bwd_pm(dctx16, qkv16, pk16, pv16, cu, pad_rows, pmask, ctx16, lse, dqkv16, dpk, dpv, partq, partkv, B, S,
                                   Pn, NH, p, seed, offset):
    _ck(lib().mtvaf_prefix_attn_bf16_varlen_bwd_pm(_p(dctx16), _p(qkv16), _p(pk16), _p(pv16), _p(cu), int(pad_rows), _p(pmask),
                                                   _pmask_len(pmask), _p(ctx16), _p(lse), _p(dqkv16), _p(dpk), _p(dpv), _p(partq),
                                                   _p(partkv), B, S, Pn, NH, 64, float(p), seed, offset, _st()),
        "mtvaf_prefix_attn_bf16_varlen_bwd_pm")


def prefix_attn_bf16_fwd(qkv16, pk16, pv16, addmask, ctx16, lse, B, S, Pn, NH, p, seed, offset):
    _ck(lib().mtvaf_prefix_attn_bf16_fwd(_p(qkv16), _p(pk16), _p(pv16), _p(addmask), _p(ctx16), _p(lse), B, S, Pn, NH, 64,
                                         float(p), seed, offset, _st()), "mtvaf_prefix_attn_bf16_fwd")


def prefix_attn_bf16_bwd(dctx16, qkv16, pk16, pv16, addmask, ctx16, lse, dqkv16, dpk, dpv, partq, partkv, B, S, Pn, NH, p,
                         seed, offset, zero_tail=False):
    """partq [B*ceil(S/64), H], partkv [B*ceil((Pn+S)/64), 2H]: per-block column sums of dQ and dK|dV (QKV bias gradient).
    zero_tail: as prefix_attn_bwd."""
    _ck(lib().mtvaf_prefix_attn_bf16_bwd_tail(_p(dctx16), _p(qkv16), _p(pk16), _p(pv16), _p(addmask), _p(ctx16), _p(lse),
                                              _p(dqkv16), _p(dpk), _p(dpv), _p(partq), _p(partkv), B, S, Pn, NH, 64, float(p),
                                              seed, offset, int(bool(zero_tail)), _st()), "mtvaf_prefix_attn_bf16_bwd_tail")


def crf_workspace(B, S, C, device):
    n = lib().mtvaf_crf_workspace_bytes(B, S, C)
    return torch.empty(n, dtype=torch.uint8, device=device), n


def crf_nll_fwd(em, tags, mask_u8, start, end, trans, loss, ws, wsb):
    B, S, C = em.shape
    _ck(lib().mtvaf_crf_nll_fwd(_p(em), _p(tags), _p(mask_u8), _p(start), _p(end), _p(trans), _p(loss), B, S, C, _p(ws), wsb,
                                _st()), "mtvaf_crf_nll_fwd")


def crf_nll_bwd(gout, em, tags, mask_u8, start, end, trans, dem, dstart, dend, dtrans, accumulate, ws, wsb):
    B, S, C = em.shape
    _ck(lib().mtvaf_crf_nll_bwd(_p(gout), _p(em), _p(tags), _p(mask_u8), _p(start), _p(end), _p(trans), _p(dem), _p(dstart),
                                _p(dend), _p(dtrans), int(accumulate), B, S, C, _p(ws), wsb, _st()), "mtvaf_crf_nll_bwd")


def crf_llh_fwd(em, tags, mask_u8, start, end, trans, llh, ws, wsb):
    """llh [B] = score(gold) - logZ per sentence; the workspace keeps what crf_llh_bwd reads."""
    B, S, C = em.shape
    _ck(lib().mtvaf_crf_llh_fwd(_p(em), _p(tags), _p(mask_u8), _p(start), _p(end), _p(trans), _p(llh), B, S, C, _p(ws), wsb,
                                _st()), "mtvaf_crf_llh_fwd")


def crf_llh_bwd(grad_llh, em, tags, mask_u8, start, end, trans, dem, dstart, dend, dtrans, accumulate, ws, wsb):
    """grad_llh [B]: the upstream gradient of every sentence's log-likelihood."""
    B, S, C = em.shape
    _ck(lib().mtvaf_crf_llh_bwd(_p(grad_llh), _p(em), _p(tags), _p(mask_u8), _p(start), _p(end), _p(trans), _p(dem),
                                _p(dstart), _p(dend), _p(dtrans), int(accumulate), B, S, C, _p(ws), wsb, _st()),
        "mtvaf_crf_llh_bwd")


def crf_marginals(em, mask_u8, start, end, trans, marg, logz, ws, wsb):
    """marg [B,S,C] posterior tag probabilities (zeros at masked steps); logz [B] or None."""
    B, S, C = em.shape
    _ck(lib().mtvaf_crf_marginals(_p(em), _p(mask_u8), _p(start), _p(end), _p(trans), _p(marg), _p(logz), B, S, C, _p(ws),
                                  wsb, _st()), "mtvaf_crf_marginals")


def crf_viterbi(em, mask_u8, start, end, trans, tags_out, lens_out):
    B, S, C = em.shape
    _ck(lib().mtvaf_crf_viterbi(_p(em), _p(mask_u8), _p(start), _p(end), _p(trans), _p(tags_out), _p(lens_out), B, S, C,
                                _st()), "mtvaf_crf_viterbi")


# ---- span model heads (csrc/span.hip) -----------------------------------------------------------------------------
def span_index(mask_u8, span_starts, span_ends):
    B, S = mask_u8.shape
    M = span_starts.shape[1]
    index = torch.empty(lib().mtvaf_span_index_ints(B, S, M), dtype=torch.int32, device=mask_u8.device)
    _ck(lib().mtvaf_span_index(_p(mask_u8), _p(span_starts), _p(span_ends), _p(index), B, S, M, _st()), "mtvaf_span_index")
    return index


def span_pool_fwd(seq, w_unary, b_unary, index, pooled, stats, B, S, M):
    H = seq.shape[-1]
    _ck(lib().mtvaf_span_pool_fwd(_p(seq), _p(w_unary), _p(b_unary), _p(index), _p(pooled), _p(stats), B, S, M, H, _st()),
        "mtvaf_span_pool_fwd")


def span_pool_bwd(dpooled, pooled, stats, seq, w_unary, b_unary, index, dseq, dw, db, B, S, M):
    """dseq overwritten; dw [H] and db [1] = column sums of the per-span partials (deterministic)."""
    H = seq.shape[-1]
    wsb = lib().mtvaf_span_pool_bwd_workspace_bytes(B, S, M, H)
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=seq.device)  # private: the colsum below uses the shared one
    dwp, dbp = ctypes.c_void_p(), ctypes.c_void_p()
    _ck(lib().mtvaf_span_pool_bwd(_p(dpooled), _p(pooled), _p(stats), _p(seq), _p(w_unary), _p(b_unary), _p(index), _p(dseq),
                                  ctypes.byref(dwp), ctypes.byref(dbp), B, S, M, H, _p(ws), wsb, _st()), "mtvaf_span_pool_bwd")
    off_w = (dwp.value - ws.data_ptr()) // 4
    off_b = (dbp.value - ws.data_ptr()) // 4
    NS = B * M
    colsum(ws[off_w:off_w + NS * H].view(NS, H), dw)
    colsum(ws[off_b:off_b + NS].view(NS, 1), db)


def distant_ce_fwd(logits, ld, positions, loss, row_ws, B, S, scale, accumulate):
    _ck(lib().mtvaf_distant_ce_fwd(_p(logits), ld, _p(positions), _p(loss), _p(row_ws), B, S, float(scale), int(accumulate),
                                   _st()), "mtvaf_distant_ce_fwd")


def distant_ce_bwd(gout, scale, logits, ld, positions, row_ws, dlogits, ldd, B, S):
    _ck(lib().mtvaf_distant_ce_bwd(_p(gout), float(scale), _p(logits), ld, _p(positions), _p(row_ws), _p(dlogits), ldd, B, S,
                                   _st()), "mtvaf_distant_ce_bwd")


def ce_fwd(logits, labels, loss, ws2):
    N, C = logits.shape
    _ck(lib().mtvaf_ce_fwd(_p(logits), _p(labels), _p(loss), _p(ws2), N, C, _st()), "mtvaf_ce_fwd")


def ce_bwd(gout, logits, labels, ws2, dlogits):
    N, C = logits.shape
    _ck(lib().mtvaf_ce_bwd(_p(gout), _p(logits), _p(labels), _p(ws2), _p(dlogits), N, C, _st()), "mtvaf_ce_bwd")


def js_consistency_fwd(x, y, mask_u8, loss, row_ws, scale):
    """x, y [B,M,C] fp32 contiguous, mask_u8 [B,M] or None; loss [1] written, row_ws [B] scratch."""
    _f32(x, y, loss, row_ws)
    B, M, C = x.shape
    assert y.shape == x.shape and row_ws.numel() >= B and (mask_u8 is None or (mask_u8.dtype == torch.uint8 and
           tuple(mask_u8.shape) == (B, M) and mask_u8.is_contiguous())), (x.shape, y.shape, row_ws.shape)
    _ck(lib().mtvaf_js_consistency_fwd(_p(x), _p(y), _p(mask_u8), _p(loss), _p(row_ws), B, M, C, float(scale), _st()),
        "mtvaf_js_consistency_fwd")


def js_consistency_bwd(gout, scale, x, y, mask_u8, dx, dy):
    _f32(gout, x, y, dx, dy)
    B, M, C = x.shape
    assert y.shape == x.shape == dx.shape == dy.shape and (mask_u8 is None or (mask_u8.dtype == torch.uint8 and
           tuple(mask_u8.shape) == (B, M) and mask_u8.is_contiguous())), (x.shape, y.shape, dx.shape, dy.shape)
    _ck(lib().mtvaf_js_consistency_bwd(_p(gout), float(scale), _p(x), _p(y), _p(mask_u8), _p(dx), _p(dy), B, M, C, _st()),
        "mtvaf_js_consistency_bwd")


TOKEN_DIVERGENCE_KINDS = {"sym_kl": 0, "js": 1}
TOKEN_DIVERGENCE_REDUCTIONS = {"token_mean": 0, "batch_mean": 1}


def _token_divergence_mask(mask_u8, N):
    assert mask_u8 is None or (mask_u8.dtype == torch.uint8 and mask_u8.numel() == N and mask_u8.is_contiguous()
                               and mask_u8.is_cuda), (None if mask_u8 is None else (mask_u8.dtype, tuple(mask_u8.shape)), N)


def token_divergence_fwd(x, y, mask_u8, loss, row_ws, kind, temperature, reduction, B, scale):
    """x, y [N,C] fp32 contiguous, mask_u8 [N] or None; kind / reduction are the ABI's integers (TOKEN_DIVERGENCE_*), B the
    divisor of the batch mean; loss [1] and row_ws [N] are written."""
    _f32(x, y, loss, row_ws)
    N, C = x.shape
    assert y.shape == x.shape and row_ws.numel() >= N, (x.shape, y.shape, row_ws.shape)
    _token_divergence_mask(mask_u8, N)
    _ck(lib().mtvaf_token_divergence_fwd(_p(x), _p(y), _p(mask_u8), _p(loss), _p(row_ws), N, C, int(kind), float(temperature),
                                         int(reduction), int(B), float(scale), _st()), "mtvaf_token_divergence_fwd")


def token_divergence_bwd(gout, x, y, mask_u8, dx, dy, kind, temperature, reduction, B, scale):
    _f32(gout, x, y, dx, dy)
    N, C = x.shape
    assert y.shape == x.shape == dx.shape == dy.shape, (x.shape, y.shape, dx.shape, dy.shape)
    _token_divergence_mask(mask_u8, N)
    _ck(lib().mtvaf_token_divergence_bwd(_p(gout), _p(x), _p(y), _p(mask_u8), _p(dx), _p(dy), N, C, int(kind), float(temperature),
                                         int(reduction), int(B), float(scale), _st()), "mtvaf_token_divergence_bwd")


TOKEN_CE_REDUCTIONS = {"mean": 0, "batch_mean": 1, "sum": 2}


def _token_ce_inputs(logits, labels, mask_u8, class_weight):
    _f32(logits, class_weight)
    N, C = logits.shape
    assert labels.is_cuda and labels.dtype == torch.int64 and labels.numel() == N and labels.is_contiguous(), \
        (labels.device, labels.dtype, tuple(labels.shape), N)
    assert class_weight is None or class_weight.numel() == C, (tuple(class_weight.shape), C)
    _token_divergence_mask(mask_u8, N)
    return N, C


def token_ce_fwd(logits, labels, mask_u8, class_weight, loss, row_ws, stats, ignore_index, smoothing, gamma, reduction, B, scale):
    """logits [N,C] fp32 contiguous, labels [N] int64, mask_u8 [N] or None, class_weight [C] fp32 or None; reduction is the ABI's
    integer (TOKEN_CE_REDUCTIONS), B the divisor of the batch mean; loss [1], row_ws [N] and stats [2] int32 are written."""
    _f32(loss, row_ws)
    N, C = _token_ce_inputs(logits, labels, mask_u8, class_weight)
    assert row_ws.numel() >= N and stats.is_cuda and stats.dtype == torch.int32 and stats.numel() >= 2 and stats.is_contiguous()
    _ck(lib().mtvaf_token_ce_fwd(_p(logits), _p(labels), _p(mask_u8), _p(class_weight), _p(loss), _p(row_ws), _p(stats), N, C,
                                 int(ignore_index), float(smoothing), float(gamma), int(reduction), int(B), float(scale), _st()),
        "mtvaf_token_ce_fwd")


def token_ce_bwd(gout, grows, logits, labels, mask_u8, class_weight, dlogits, ignore_index, smoothing, gamma, reduction, B, scale):
    """Exactly one of gout [1] (the gradient of the reduced loss) and grows [N] (per-row gradients of row_ws) is given."""
    _f32(gout, grows, dlogits)
    N, C = _token_ce_inputs(logits, labels, mask_u8, class_weight)
    assert dlogits.shape == logits.shape and (grows is None or grows.numel() == N), (dlogits.shape, logits.shape)
    _ck(lib().mtvaf_token_ce_bwd(_p(gout), _p(grows), _p(logits), _p(labels), _p(mask_u8), _p(class_weight), _p(dlogits), N, C,
                                 int(ignore_index), float(smoothing), float(gamma), int(reduction), int(B), float(scale), _st()),
        "mtvaf_token_ce_bwd")


def token_argmax(logits, mask_u8, allowed, tags, logp):
    """logits [N,C] fp32 contiguous, mask_u8 [N] or None, allowed [N] int64 tag sets (mtvaf_amd.constraints) or None; tags [N]
    int64 and logp [N] fp32 are written (0 on masked rows)."""
    _f32(logits, logp)
    N, C = logits.shape
    _token_divergence_mask(mask_u8, N)
    assert allowed is None or (allowed.is_cuda and allowed.dtype == torch.int64 and allowed.numel() == N and
                               allowed.is_contiguous()), (None if allowed is None else (allowed.dtype, tuple(allowed.shape)), N)
    assert tags.is_cuda and tags.dtype == torch.int64 and tags.numel() >= N and tags.is_contiguous() and logp.numel() >= N
    _ck(lib().mtvaf_token_argmax(_p(logits), _p(mask_u8), _p(allowed), _p(tags), _p(logp), N, C, _st()), "mtvaf_token_argmax")


SPAN_PROPOSE_MAX_S, SPAN_PROPOSE_MAX_N = 512, 32


def span_propose(logits, word_index, word_key=None, n_best=20, max_len=12, threshold=8.0, use_heuristics=True, nms=0):
    """Candidate spans of every sentence (csrc/span_propose.hip), one launch and no host sync.  logits [B,S,>=2] fp32, start
    and end logit of a token adjacent (any token stride: the binary_affine output or a slice of a wider tensor is read in
    place); word_index [B,S] int32 (-1 outside the word map); word_key [B,S] int32 or None (= word_index).
    -> span_starts, span_ends, label_masks [B,n_best] int64, span_scores [B,n_best] fp32, count [B] int32."""
    if logits.dim() != 3 or logits.shape[2] < 2:
        raise ValueError(f"span_propose: logits {tuple(logits.shape)}: expected [B, S, >=2]")
    B, S = logits.shape[:2]
    n_best = int(n_best)
    if not 1 <= S <= SPAN_PROPOSE_MAX_S:
        raise ValueError(f"span_propose: S={S} outside 1..{SPAN_PROPOSE_MAX_S}")
    if not 1 <= n_best <= SPAN_PROPOSE_MAX_N:
        raise ValueError(f"span_propose: n_best={n_best} outside 1..{SPAN_PROPOSE_MAX_N}")
    if nms not in (0, 1):
        raise ValueError(f"span_propose: nms={nms!r}: expected 0 (off) or 1 (shared word)")
    if B < 1 or tuple(word_index.shape) != (B, S) or (word_key is not None and tuple(word_key.shape) != (B, S)):
        raise ValueError("span_propose: word_index / word_key must be [B, S] of the logits")
    ld = logits.stride(1)
    assert logits.dtype == torch.float32 and logits.stride(2) == 1 and ld >= 2 and logits.stride(0) == S * ld, \
        (logits.dtype, logits.stride())
    for t in (word_index, word_key):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous()), (t.dtype, t.stride())
    dev = logits.device
    starts, ends, masks = (torch.empty((B, n_best), dtype=torch.int64, device=dev) for _ in range(3))
    scores = torch.empty((B, n_best), dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    _ck(lib().mtvaf_span_propose(_p(logits), ld, _p(word_index), _p(word_key), _p(starts), _p(ends), _p(masks), _p(scores),
                                 _p(count), B, S, n_best, int(max_len), float(threshold), int(bool(use_heuristics)), int(nms),
                                 _st()), "mtvaf_span_propose")
    return starts, ends, masks, scores, count


ENTITY_MAX_S, ENTITY_MAX_C = 512, 64


def entity_counts(pred, gold, mask_u8, start_tab, end_tab, type_of, gold_skip, n_types, counts):
    """Adds one batch's entity and token counts into ``counts`` (csrc/entity.hip), one launch and no host sync.  pred [B,>=S]
    int32 (``CRF.decode_packed``'s tags), gold [B,S] int64, mask_u8 [B,S] uint8; start_tab / end_tab [(C+1)^2] uint8, type_of
    [C+1] int32, gold_skip [C] uint8; counts [n_types*3+2] int64: per type predicted, gold, correct, then tokens_equal,
    tokens_kept."""
    C = gold_skip.numel()
    if gold.dim() != 2 or pred.dim() != 2:
        raise ValueError(f"entity_counts: pred {tuple(pred.shape)}, gold {tuple(gold.shape)}: expected [B, >=S] and [B, S]")
    B, S = gold.shape
    if not 1 <= S <= ENTITY_MAX_S:
        raise ValueError(f"entity_counts: S={S} outside 1..{ENTITY_MAX_S}")
    if not 1 <= C <= ENTITY_MAX_C:
        raise ValueError(f"entity_counts: C={C} outside 1..{ENTITY_MAX_C}")
    if B < 1 or pred.shape[0] != B or pred.shape[1] < S or tuple(mask_u8.shape) != (B, S):
        raise ValueError(f"entity_counts: pred {tuple(pred.shape)} / mask {tuple(mask_u8.shape)} do not fit gold [{B}, {S}]")
    if (start_tab.numel(), end_tab.numel(), type_of.numel(), counts.numel()) != ((C + 1) ** 2, (C + 1) ** 2, C + 1, n_types * 3 + 2):
        raise ValueError("entity_counts: tables / counter do not fit C and n_types")
    ldp = pred.stride(0)
    assert pred.dtype == torch.int32 and pred.stride(1) == 1 and ldp >= S, (pred.dtype, pred.stride())
    assert gold.dtype == torch.int64 and gold.is_contiguous() and mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous()
    assert start_tab.dtype == end_tab.dtype == gold_skip.dtype == torch.uint8 and type_of.dtype == torch.int32
    assert counts.dtype == torch.int64 and all(t.is_contiguous() for t in (start_tab, end_tab, type_of, gold_skip, counts))
    _ck(lib().mtvaf_entity_counts(_p(pred), ldp, _p(gold), _p(mask_u8), _p(start_tab), _p(end_tab), _p(type_of), _p(gold_skip),
                                  B, S, C, int(n_types), _p(counts), _st()), "mtvaf_entity_counts")
    return counts


def entity_counts_rows(pred, gold, mask_u8, start_tab, end_tab, type_of, gold_skip, n_types, group=1, out=None):
    """Per-row entity counts (csrc/entity.hip), one launch and no host sync: pred [R,>=S] int32, row r scored against gold /
    mask_u8 row r // group (gold [R/group,S] int64, mask_u8 [R/group,S] uint8); tables as `entity_counts`.
    -> rows int32 [R,3] = (predicted, gold, correct) chunks of each row summed over the types; ``out``: overwritten."""
    C = gold_skip.numel()
    if gold.dim() != 2 or pred.dim() != 2:
        raise ValueError(f"entity_counts_rows: pred {tuple(pred.shape)}, gold {tuple(gold.shape)}: expected [R, >=S] and [R/group, S]")
    G, S = gold.shape
    R, group = pred.shape[0], int(group)
    if not 1 <= S <= ENTITY_MAX_S:
        raise ValueError(f"entity_counts_rows: S={S} outside 1..{ENTITY_MAX_S}")
    if not 1 <= C <= ENTITY_MAX_C:
        raise ValueError(f"entity_counts_rows: C={C} outside 1..{ENTITY_MAX_C}")
    if group < 1 or R < 1 or R % group != 0 or R // group != G:
        raise ValueError(f"entity_counts_rows: {R} rows in groups of {group} do not fit {G} gold rows")
    if pred.shape[1] < S or tuple(mask_u8.shape) != (G, S):
        raise ValueError(f"entity_counts_rows: pred {tuple(pred.shape)} / mask {tuple(mask_u8.shape)} do not fit gold [{G}, {S}]")
    if (start_tab.numel(), end_tab.numel(), type_of.numel()) != ((C + 1) ** 2, (C + 1) ** 2, C + 1) or not 1 <= n_types <= C + 1:
        raise ValueError("entity_counts_rows: tables do not fit C and n_types")
    ldp = pred.stride(0)
    assert pred.dtype == torch.int32 and pred.stride(1) == 1 and ldp >= S, (pred.dtype, pred.stride())
    assert gold.dtype == torch.int64 and gold.is_contiguous() and mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous()
    assert start_tab.dtype == end_tab.dtype == gold_skip.dtype == torch.uint8 and type_of.dtype == torch.int32
    assert all(t.is_contiguous() for t in (start_tab, end_tab, type_of, gold_skip))
    if out is None:
        out = torch.empty((R, 3), dtype=torch.int32, device=pred.device)
    assert tuple(out.shape) == (R, 3) and out.dtype == torch.int32 and out.is_contiguous()
    _ck(lib().mtvaf_entity_counts_rows(_p(pred), ldp, group, _p(gold), _p(mask_u8), _p(start_tab), _p(end_tab), _p(type_of),
                                       _p(gold_skip), R, S, C, int(n_types), _p(out), _st()), "mtvaf_entity_counts_rows")
    return out


SPAN_COUNTS_MAX_S, SPAN_COUNTS_MAX_N, SPAN_COUNTS_MAX_G, SPAN_COUNTS_MIN_K, SPAN_COUNTS_MAX_K = 512, 32, 32, 2, 8


def span_counts(span_starts, span_ends, label_masks, logits, gold_starts, gold_ends, gold_class, gold_masks, word_index,
                word_key, counts, pred_class=None, matched_gold=None):
    """Adds one batch's aspect counts into ``counts`` (csrc/span_score.hip), one launch and no host sync.  span_starts /
    span_ends / label_masks [B,N] int64 (``span_propose``'s), logits [B,N,K] fp32; gold_starts / gold_ends / gold_class /
    gold_masks [B,G] int64; word_index [B,S] int32 (-1 outside the word map), word_key [B,S] int32 or None (= word_index);
    counts [3K+2] int64: per class retrieved, relevant, common, then relevant_other, sentences.  pred_class / matched_gold
    [B,N] int32 or None: written when given."""
    if logits.dim() != 3 or word_index.dim() != 2 or gold_starts.dim() != 2:
        raise ValueError(f"span_counts: logits {tuple(logits.shape)}, gold {tuple(gold_starts.shape)}, word_index "
                         f"{tuple(word_index.shape)}: expected [B, N, K], [B, G] and [B, S]")
    B, N, K = logits.shape
    G, S = gold_starts.shape[1], word_index.shape[1]
    if not 1 <= S <= SPAN_COUNTS_MAX_S:
        raise ValueError(f"span_counts: S={S} outside 1..{SPAN_COUNTS_MAX_S}")
    if not 1 <= N <= SPAN_COUNTS_MAX_N:
        raise ValueError(f"span_counts: N={N} outside 1..{SPAN_COUNTS_MAX_N}")
    if not 1 <= G <= SPAN_COUNTS_MAX_G:
        raise ValueError(f"span_counts: G={G} outside 1..{SPAN_COUNTS_MAX_G}")
    if not SPAN_COUNTS_MIN_K <= K <= SPAN_COUNTS_MAX_K:
        raise ValueError(f"span_counts: K={K} outside {SPAN_COUNTS_MIN_K}..{SPAN_COUNTS_MAX_K}")
    pred, gold = (span_starts, span_ends, label_masks), (gold_starts, gold_ends, gold_class, gold_masks)
    outs = [t for t in (pred_class, matched_gold) if t is not None]
    if B < 1 or any(tuple(t.shape) != (B, N) for t in (*pred, *outs)) or any(tuple(t.shape) != (B, G) for t in gold) or \
            tuple(word_index.shape) != (B, S) or (word_key is not None and tuple(word_key.shape) != (B, S)):
        raise ValueError(f"span_counts: spans / gold / word maps do not fit logits [{B}, {N}, {K}], G={G}, S={S}")
    if counts.numel() != 3 * K + 2:
        raise ValueError(f"span_counts: counter of {counts.numel()} elements, expected 3 * K + 2 = {3 * K + 2}")
    assert logits.dtype == torch.float32 and logits.is_contiguous(), (logits.dtype, logits.stride())
    assert all(t.dtype == torch.int64 and t.is_contiguous() for t in (*pred, *gold, counts))
    assert all(t is None or (t.dtype == torch.int32 and t.is_contiguous()) for t in (word_index, word_key, *outs))
    _ck(lib().mtvaf_span_counts(_p(span_starts), _p(span_ends), _p(label_masks), _p(logits), _p(gold_starts), _p(gold_ends),
                                _p(gold_class), _p(gold_masks), _p(word_index), _p(word_key), B, S, N, G, K, _p(counts),
                                _p(pred_class), _p(matched_gold), _st()), "mtvaf_span_counts")
    return counts


CRF_ENTITIES_MAX_E = 64


def crf_entities(em, mask_u8, tags, keep, start, end, trans, start_tab, end_tab, type_of, n_types, max_entities=32, out=None):
    """Entities of decoded tags with the CRF posterior of each decoded segment (csrc/crf_entities.hip), one launch and no host
    sync.  em [B,S,C] fp32, mask_u8 [B,S] uint8 (a prefix mask), tags [B,>=S] int32 (``CRF.decode_packed``'s), keep [B,S] uint8
    or None (= columns 1 .. L-1); start / end [C], trans [C,C] fp32; start_tab / end_tab [(C+1)^2] uint8, type_of [C+1] int32.
    -> ents [B,max_entities,3] int32 (start column, end column, type; -1 in unused slots), log_conf [B,max_entities] fp32 (0 in
    unused slots), count [B] int32 (may exceed max_entities).  ``out``: that triple, to be overwritten."""
    if em.dim() != 3 or tags.dim() != 2:
        raise ValueError(f"crf_entities: emissions {tuple(em.shape)}, tags {tuple(tags.shape)}: expected [B, S, C] and [B, >=S]")
    B, S, C = em.shape
    max_entities, n_types = int(max_entities), int(n_types)
    if not 1 <= S <= ENTITY_MAX_S:
        raise ValueError(f"crf_entities: S={S} outside 1..{ENTITY_MAX_S}")
    if not 1 <= C <= ENTITY_MAX_C:
        raise ValueError(f"crf_entities: C={C} outside 1..{ENTITY_MAX_C}")
    if not 1 <= max_entities <= CRF_ENTITIES_MAX_E:
        raise ValueError(f"crf_entities: max_entities={max_entities} outside 1..{CRF_ENTITIES_MAX_E}")
    if not 1 <= n_types <= C + 1:
        raise ValueError(f"crf_entities: n_types={n_types} outside 1..{C + 1}")
    if B < 1 or tags.shape[0] != B or tags.shape[1] < S or tuple(mask_u8.shape) != (B, S) or \
            (keep is not None and tuple(keep.shape) != (B, S)):
        raise ValueError(f"crf_entities: tags {tuple(tags.shape)} / mask {tuple(mask_u8.shape)} / keep do not fit emissions "
                         f"[{B}, {S}, {C}]")
    if (start.numel(), end.numel(), trans.numel(), start_tab.numel(), end_tab.numel(), type_of.numel()) != \
            (C, C, C * C, (C + 1) ** 2, (C + 1) ** 2, C + 1):
        raise ValueError("crf_entities: CRF parameters / tables do not fit C")
    ldt = tags.stride(0)
    if tags.stride(1) != 1 or ldt < S:
        raise ValueError(f"crf_entities: tags strides {tags.stride()}: expected unit columns and a row stride >= S")
    _f32(em, start, end, trans)
    assert tags.dtype == torch.int32 and mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous()
    assert keep is None or (keep.dtype == torch.uint8 and keep.is_contiguous())
    assert start_tab.dtype == end_tab.dtype == torch.uint8 and type_of.dtype == torch.int32
    assert all(t.is_contiguous() for t in (start_tab, end_tab, type_of))
    if out is None:
        out = (torch.empty((B, max_entities, 3), dtype=torch.int32, device=em.device),
               torch.empty((B, max_entities), dtype=torch.float32, device=em.device),
               torch.empty(B, dtype=torch.int32, device=em.device))
    ents, log_conf, count = out
    assert tuple(ents.shape) == (B, max_entities, 3) and tuple(log_conf.shape) == (B, max_entities) and count.numel() == B
    assert ents.dtype == count.dtype == torch.int32 and log_conf.dtype == torch.float32
    assert ents.is_contiguous() and log_conf.is_contiguous() and count.is_contiguous()
    _ck(lib().mtvaf_crf_entities(_p(em), _p(mask_u8), _p(tags), ldt, _p(keep), _p(start), _p(end), _p(trans), _p(start_tab),
                                 _p(end_tab), _p(type_of), n_types, _p(ents), _p(log_conf), _p(count), B, S, C, max_entities,
                                 _st()), "mtvaf_crf_entities")
    return ents, log_conf, count


CRF_NBEST_MAX_K = 8


def crf_nbest(em, mask_u8, start, end, trans, nbest, return_logprob=True, out=None):
    """The ``nbest`` best tag sequences of every sentence (csrc/crf_nbest.hip); no host sync.  em [B,S,C] fp32, mask_u8 [B,S]
    uint8 (a prefix mask with mask[:,0] == 1), start / end [C], trans [C,C] fp32.
    -> tags [B,K,S] int32 (row k the k-th best path, -1 behind the sentence), scores [B,K] fp32 (unnormalised, non-increasing),
    logprob [B,K] fp32 = score - logZ (None without ``return_logprob``: the forward recursion is then not launched), n_paths [B]
    int32 = min(K, C^len); ranks >= n_paths hold -1 / -inf / -inf.  ``out``: that quadruple, to be overwritten."""
    if em.dim() != 3:
        raise ValueError(f"crf_nbest: emissions {tuple(em.shape)}: expected [B, S, C]")
    B, S, C = em.shape
    K = int(nbest)
    if not 1 <= K <= CRF_NBEST_MAX_K:
        raise ValueError(f"crf_nbest: nbest={K} outside 1..{CRF_NBEST_MAX_K}")
    if not 1 <= S <= ENTITY_MAX_S:
        raise ValueError(f"crf_nbest: S={S} outside 1..{ENTITY_MAX_S}")
    if not 1 <= C <= ENTITY_MAX_C:
        raise ValueError(f"crf_nbest: C={C} outside 1..{ENTITY_MAX_C}")
    if B < 1 or tuple(mask_u8.shape) != (B, S):
        raise ValueError(f"crf_nbest: mask {tuple(mask_u8.shape)} does not fit emissions [{B}, {S}, {C}]")
    if (start.numel(), end.numel(), trans.numel()) != (C, C, C * C):
        raise ValueError("crf_nbest: CRF parameters do not fit C")
    _f32(em, start, end, trans)
    assert mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous()
    if out is None:
        out = (torch.empty((B, K, S), dtype=torch.int32, device=em.device),
               torch.empty((B, K), dtype=torch.float32, device=em.device),
               torch.empty((B, K), dtype=torch.float32, device=em.device) if return_logprob else None,
               torch.empty(B, dtype=torch.int32, device=em.device))
    tags, scores, logprob, n_paths = out
    assert tuple(tags.shape) == (B, K, S) and tuple(scores.shape) == (B, K) and n_paths.numel() == B
    assert tags.dtype == n_paths.dtype == torch.int32 and scores.dtype == torch.float32
    assert tags.is_contiguous() and scores.is_contiguous() and n_paths.is_contiguous()
    assert logprob is None or (tuple(logprob.shape) == (B, K) and logprob.dtype == torch.float32 and logprob.is_contiguous())
    wsb = lib().mtvaf_crf_nbest_workspace_bytes(B, S, C, K)
    ws = torch.empty(wsb, dtype=torch.uint8, device=em.device)
    _ck(lib().mtvaf_crf_nbest(_p(em), _p(mask_u8), _p(start), _p(end), _p(trans), K, _p(tags), _p(scores), _p(logprob),
                              _p(n_paths), B, S, C, _p(ws), wsb, _st()), "mtvaf_crf_nbest")
    return tags, scores, logprob, n_paths


CRF_SAMPLE_MAX_K = 64


def crf_sample(em, mask_u8, start, end, trans, n_samples, uniforms=None, seed=0, offset=0, return_logprob=True,
               return_uniforms=False, out=None):
    """``n_samples`` tag sequences of every sentence drawn from the posterior (csrc/crf_sample.hip); no host sync.  em [B,S,C]
    fp32, mask_u8 [B,S] uint8 (a prefix mask with mask[:,0] == 1), start / end [C], trans [C,C] fp32.  ``uniforms`` [B,K,S] fp32
    in [0,1): the uniform of every draw; None: Philox keyed by (seed, offset).
    -> tags [B,K,S] int32 (-1 behind the sentence), scores [B,K] fp32 (unnormalised), logprob [B,K] fp32 = score - logZ (None
    without ``return_logprob``), uniforms_out [B,K,S] fp32 (the uniforms used, 0 behind the sentence; None without
    ``return_uniforms``).  ``out``: that quadruple, to be overwritten."""
    if em.dim() != 3:
        raise ValueError(f"crf_sample: emissions {tuple(em.shape)}: expected [B, S, C]")
    B, S, C = em.shape
    K = int(n_samples)
    if not 1 <= K <= CRF_SAMPLE_MAX_K:
        raise ValueError(f"crf_sample: n_samples={K} outside 1..{CRF_SAMPLE_MAX_K}")
    if not 1 <= S <= ENTITY_MAX_S:
        raise ValueError(f"crf_sample: S={S} outside 1..{ENTITY_MAX_S}")
    if not 1 <= C <= ENTITY_MAX_C:
        raise ValueError(f"crf_sample: C={C} outside 1..{ENTITY_MAX_C}")
    if B < 1 or tuple(mask_u8.shape) != (B, S):
        raise ValueError(f"crf_sample: mask {tuple(mask_u8.shape)} does not fit emissions [{B}, {S}, {C}]")
    if (start.numel(), end.numel(), trans.numel()) != (C, C, C * C):
        raise ValueError("crf_sample: CRF parameters do not fit C")
    if uniforms is not None and tuple(uniforms.shape) != (B, K, S):
        raise ValueError(f"crf_sample: uniforms {tuple(uniforms.shape)}: expected [{B}, {K}, {S}]")
    _f32(em, start, end, trans, uniforms)
    assert mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous()
    if out is None:
        out = (torch.empty((B, K, S), dtype=torch.int32, device=em.device),
               torch.empty((B, K), dtype=torch.float32, device=em.device),
               torch.empty((B, K), dtype=torch.float32, device=em.device) if return_logprob else None,
               torch.empty((B, K, S), dtype=torch.float32, device=em.device) if return_uniforms else None)
    tags, scores, logprob, uout = out
    assert tuple(tags.shape) == (B, K, S) and tuple(scores.shape) == (B, K)
    assert tags.dtype == torch.int32 and tags.is_contiguous()
    _f32(scores, logprob, uout)
    assert logprob is None or tuple(logprob.shape) == (B, K)
    assert uout is None or tuple(uout.shape) == (B, K, S)
    wsb = lib().mtvaf_crf_sample_workspace_bytes(B, S, C, K)
    ws = torch.empty(wsb, dtype=torch.uint8, device=em.device)
    _ck(lib().mtvaf_crf_sample(_p(em), _p(mask_u8), _p(start), _p(end), _p(trans), K, _p(uniforms), int(seed), int(offset),
                               _p(tags), _p(scores), _p(logprob), _p(uout), B, S, C, _p(ws), wsb, _st()), "mtvaf_crf_sample")
    return tags, scores, logprob, uout


# ---- per-token tag constraints (csrc/crf_lattice.hip) -------------------------------------------------------------
CRF_LATTICE_MAX_S = 512
CRF_LATTICE_MAX_C = 64


def _crf_chain_shape(em, who):
    """The [B,S,C] / C / S / B checks every chain entry point starts with (csrc/crf_chain.h: bad_shape)."""
    if em.dim() != 3:
        raise ValueError(f"{who}: emissions {tuple(em.shape)}: expected [B, S, C]")
    B, S, C = em.shape
    if not 1 <= C <= CRF_LATTICE_MAX_C:
        raise ValueError(f"{who}: C={C} outside 1..{CRF_LATTICE_MAX_C}")
    if not 1 <= S <= CRF_LATTICE_MAX_S:
        raise ValueError(f"{who}: S={S} outside 1..{CRF_LATTICE_MAX_S}")
    if B < 1:
        raise ValueError(f"{who}: empty batch")
    return B, S, C


def _crf_workspace(bytes_fn, B, S, C, device):
    """(uint8 workspace on ``device``, its size in bytes) for a ``mtvaf_crf_*_workspace_bytes(B, S, C)``."""
    n = bytes_fn(B, S, C)
    return torch.empty(n, dtype=torch.uint8, device=device), n


def crf_lattice_check(em, allowed, mask_u8=None, who="crf_lattice"):
    """Argument checks shared by the lattice entry points (host-side: shapes and dtypes only, nothing is read).  em [B,S,C]
    fp32, allowed [B,S] int64 (bit j of a word = tag j allowed; 0 = no constraint), mask_u8 [B,S] uint8."""
    B, S, C = _crf_chain_shape(em, who)
    if not isinstance(allowed, torch.Tensor) or allowed.dtype != torch.int64:
        raise ValueError(f"{who}: allowed must be an int64 tensor of tag-set words, got "
                         f"{getattr(allowed, 'dtype', type(allowed).__name__)}")
    if tuple(allowed.shape) != (B, S):
        raise ValueError(f"{who}: allowed {tuple(allowed.shape)} does not fit emissions [{B}, {S}, {C}]")
    if mask_u8 is not None and tuple(mask_u8.shape) != (B, S):
        raise ValueError(f"{who}: mask {tuple(mask_u8.shape)} does not fit emissions [{B}, {S}, {C}]")
    return B, S, C


def crf_lattice_workspace(B, S, C, device):
    return _crf_workspace(lib().mtvaf_crf_lattice_workspace_bytes, B, S, C, device)


def crf_lattice_fwd(em, allowed, mask_u8, start, end, trans, pllh, logz_a, logz, ws, wsb):
    """pllh [B] = logZ_A - logZ; logz_a / logz [B] or None; the workspace keeps what crf_lattice_bwd reads."""
    B, S, C = crf_lattice_check(em, allowed, mask_u8, "crf_lattice_fwd")
    _ck(lib().mtvaf_crf_lattice_fwd(_p(em), _p(allowed), _p(mask_u8), _p(start), _p(end), _p(trans), _p(pllh), _p(logz_a),
                                    _p(logz), B, S, C, _p(ws), wsb, _st()), "mtvaf_crf_lattice_fwd")


def crf_lattice_bwd(grad, em, allowed, mask_u8, start, end, trans, dem, dstart, dend, dtrans, accumulate, ws, wsb):
    """grad [B]: the upstream gradient of every sentence's pllh."""
    B, S, C = crf_lattice_check(em, allowed, mask_u8, "crf_lattice_bwd")
    _ck(lib().mtvaf_crf_lattice_bwd(_p(grad), _p(em), _p(allowed), _p(mask_u8), _p(start), _p(end), _p(trans), _p(dem),
                                    _p(dstart), _p(dend), _p(dtrans), int(accumulate), B, S, C, _p(ws), wsb, _st()),
        "mtvaf_crf_lattice_bwd")


def crf_lattice_marginals(em, allowed, mask_u8, start, end, trans, marg, logz_a, ws, wsb):
    """marg [B,S,C] posteriors under the constraint (zeros at disallowed tags and masked columns); logz_a [B] or None."""
    B, S, C = crf_lattice_check(em, allowed, mask_u8, "crf_lattice_marginals")
    _ck(lib().mtvaf_crf_lattice_marginals(_p(em), _p(allowed), _p(mask_u8), _p(start), _p(end), _p(trans), _p(marg),
                                          _p(logz_a), B, S, C, _p(ws), wsb, _st()), "mtvaf_crf_lattice_marginals")


def crf_lattice_viterbi(em, allowed, mask_u8, start, end, trans, tags_out, lens_out, score_out=None):
    """tags_out [B,S] int32 the best allowed path (-1 behind the sentence), lens_out [B] int32, score_out [B] fp32 or None."""
    B, S, C = crf_lattice_check(em, allowed, mask_u8, "crf_lattice_viterbi")
    _ck(lib().mtvaf_crf_lattice_viterbi(_p(em), _p(allowed), _p(mask_u8), _p(start), _p(end), _p(trans), _p(tags_out),
                                        _p(lens_out), _p(score_out), B, S, C, _st()), "mtvaf_crf_lattice_viterbi")


# ---- expected cost under the posterior (csrc/crf_risk.hip) ----------------------------------------------------------
def crf_risk_check(em, cost=None, mask_u8=None, who="crf_risk"):
    """Argument checks shared by the risk entry points (host-side: shapes, dtypes and devices only, nothing is read).  em
    [B,S,C] fp32 on the GPU, cost (None: a call without one) floating-point [B,S,C] on the same device, mask_u8 [B,S] uint8."""
    B, S, C = _crf_chain_shape(em, who)
    if cost is not None:
        if not isinstance(cost, torch.Tensor) or not cost.dtype.is_floating_point:
            raise ValueError(f"{who}: cost must be a floating-point tensor, got {getattr(cost, 'dtype', type(cost).__name__)}")
        if tuple(cost.shape) != (B, S, C):
            raise ValueError(f"{who}: cost {tuple(cost.shape)} does not fit emissions [{B}, {S}, {C}]")
    if mask_u8 is not None and tuple(mask_u8.shape) != (B, S):
        raise ValueError(f"{who}: mask {tuple(mask_u8.shape)} does not fit emissions [{B}, {S}, {C}]")
    if not em.is_cuda or (cost is not None and not cost.is_cuda):
        raise RuntimeError(f"{who}: emissions on {em.device}" + ("" if cost is None else f", cost on {cost.device}") +
                           ": the CRF kernels run on the GPU and there is no CPU fallback")
    if cost is not None and cost.device != em.device:
        raise ValueError(f"{who}: cost on {cost.device}, emissions on {em.device}")
    return B, S, C


def crf_risk_workspace(B, S, C, device):
    return _crf_workspace(lib().mtvaf_crf_risk_workspace_bytes, B, S, C, device)


def crf_risk_fwd(em, cost, mask_u8, start, end, trans, risk, logz, marg, ws, wsb):
    """risk [B] = the expected cost; logz [B] / marg [B,S,C] or None; the workspace keeps what crf_risk_bwd reads."""
    B, S, C = crf_risk_check(em, cost, mask_u8, "crf_risk_fwd")
    _f32(em, cost, start, end, trans, risk)
    assert mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous()
    assert marg is None or (tuple(marg.shape) == (B, S, C) and marg.dtype == torch.float32 and marg.is_contiguous())
    _ck(lib().mtvaf_crf_risk_fwd(_p(em), _p(cost), _p(mask_u8), _p(start), _p(end), _p(trans), _p(risk), _p(logz), _p(marg),
                                 B, S, C, _p(ws), wsb, _st()), "mtvaf_crf_risk_fwd")


def crf_risk_bwd(grad, em, cost, mask_u8, start, end, trans, dem, dcost, dstart, dend, dtrans, accumulate, ws, wsb):
    """grad [B]: the upstream gradient of every sentence's risk; dcost [B,S,C] or None."""
    B, S, C = crf_risk_check(em, cost, mask_u8, "crf_risk_bwd")
    _f32(grad, em, cost, start, end, trans, dem, dstart, dend, dtrans)
    assert mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous() and grad.numel() == B
    assert tuple(dem.shape) == (B, S, C) and dem.is_contiguous()
    assert dcost is None or (tuple(dcost.shape) == (B, S, C) and dcost.dtype == torch.float32 and dcost.is_contiguous())
    _ck(lib().mtvaf_crf_risk_bwd(_p(grad), _p(em), _p(cost), _p(mask_u8), _p(start), _p(end), _p(trans), _p(dem), _p(dcost),
                                 _p(dstart), _p(dend), _p(dtrans), int(accumulate), B, S, C, _p(ws), wsb, _st()),
        "mtvaf_crf_risk_bwd")


# ---- expected path cost with edge terms (csrc/crf_path.hip) ---------------------------------------------------------
def crf_path_check(em, cost=None, ecost=None, mask_u8=None, who="crf_path"):
    """`crf_risk_check` plus the edge cost: None or a floating-point [C,C] tensor on the emissions' device."""
    if ecost is not None and em.dim() == 3:
        C = em.shape[2]
        if not isinstance(ecost, torch.Tensor) or not ecost.dtype.is_floating_point:
            raise ValueError(f"{who}: edge_cost must be a floating-point tensor, got "
                             f"{getattr(ecost, 'dtype', type(ecost).__name__)}")
        if tuple(ecost.shape) != (C, C):
            raise ValueError(f"{who}: edge_cost {tuple(ecost.shape)} does not fit [{C}, {C}]")
        if ecost.device != em.device:
            raise ValueError(f"{who}: edge_cost on {ecost.device}, emissions on {em.device}")
    return crf_risk_check(em, cost, mask_u8, who)


def crf_path_workspace(B, S, C, device):
    return _crf_workspace(lib().mtvaf_crf_path_workspace_bytes, B, S, C, device)


def crf_path_fwd(em, cost, ecost, mask_u8, start, end, trans, risk, logz, ws, wsb):
    """risk [B] = the expected path cost (cost [B,S,C] / ecost [C,C] or None = zeros); logz [B] or None; the workspace keeps
    what crf_path_bwd reads."""
    B, S, C = crf_path_check(em, cost, ecost, mask_u8, "crf_path_fwd")
    _f32(em, cost, ecost, start, end, trans, risk, logz)
    assert mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous() and risk.numel() == B
    _ck(lib().mtvaf_crf_path_fwd(_p(em), _p(cost), _p(ecost), _p(mask_u8), _p(start), _p(end), _p(trans), _p(risk), _p(logz),
                                 B, S, C, _p(ws), wsb, _st()), "mtvaf_crf_path_fwd")


def crf_path_bwd(grad, gz, em, cost, ecost, mask_u8, start, end, trans, dem, dcost, decost, dstart, dend, dtrans, accumulate,
                 ws, wsb):
    """grad [B] / gz [B] or None: the upstream gradients of every sentence's risk and logZ; dcost [B,S,C] / decost [C,C] or
    None.  cost and ecost are those of the crf_path_fwd call that filled the workspace."""
    B, S, C = crf_path_check(em, cost, ecost, mask_u8, "crf_path_bwd")
    _f32(grad, gz, em, cost, ecost, start, end, trans, dem, dcost, decost, dstart, dend, dtrans)
    assert mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous() and grad.numel() == B
    assert gz is None or gz.numel() == B
    assert tuple(dem.shape) == (B, S, C) and (dcost is None or tuple(dcost.shape) == (B, S, C))
    assert decost is None or tuple(decost.shape) == (C, C)
    _ck(lib().mtvaf_crf_path_bwd(_p(grad), _p(gz), _p(em), _p(cost), _p(ecost), _p(mask_u8), _p(start), _p(end), _p(trans),
                                 _p(dem), _p(dcost), _p(decost), _p(dstart), _p(dend), _p(dtrans), int(accumulate), B, S, C,
                                 _p(ws), wsb, _st()), "mtvaf_crf_path_bwd")


CRF_CHUNKS_MAX_W = 16
CRF_CHUNKS_MAX_TYPES = 64


def crf_chunk_posteriors(em, allowed, mask_u8, keep, start, end, trans, start_tab, end_tab, type_of, n_types, max_width=8,
                         out=None):
    """Chunk-event log posteriors of every span of kept columns and every type (csrc/crf_chunks.hip), one launch and no host
    sync.  em [B,S,C] fp32, allowed [B,S] int64 set words or None (no constraint), mask_u8 [B,S] uint8 (a prefix mask), keep
    [B,S] uint8 or None (= columns 1 .. L-1); the CRF parameters and the scheme tables as `crf_entities` takes them.
    -> log_post [B,S,max_width,n_types] fp32 (start column, width in kept columns, type; -inf where the event is impossible or
    undefined), logz_a [B] fp32.  ``out``: that pair, to be overwritten."""
    if em.dim() != 3:
        raise ValueError(f"crf_chunk_posteriors: emissions {tuple(em.shape)}: expected [B, S, C]")
    B, S, C = em.shape
    W, n_types = int(max_width), int(n_types)
    if not 1 <= S <= CRF_LATTICE_MAX_S:
        raise ValueError(f"crf_chunk_posteriors: S={S} outside 1..{CRF_LATTICE_MAX_S}")
    if not 1 <= C <= CRF_LATTICE_MAX_C:
        raise ValueError(f"crf_chunk_posteriors: C={C} outside 1..{CRF_LATTICE_MAX_C}")
    if not 1 <= W <= CRF_CHUNKS_MAX_W:
        raise ValueError(f"crf_chunk_posteriors: max_width={W} outside 1..{CRF_CHUNKS_MAX_W}")
    if not 1 <= n_types <= CRF_CHUNKS_MAX_TYPES:
        raise ValueError(f"crf_chunk_posteriors: n_types={n_types} outside 1..{CRF_CHUNKS_MAX_TYPES}")
    if B < 1 or tuple(mask_u8.shape) != (B, S) or (keep is not None and tuple(keep.shape) != (B, S)) or \
            (allowed is not None and tuple(allowed.shape) != (B, S)):
        raise ValueError(f"crf_chunk_posteriors: mask {tuple(mask_u8.shape)} / keep / allowed do not fit emissions [{B}, {S}, {C}]")
    if (start.numel(), end.numel(), trans.numel(), start_tab.numel(), end_tab.numel(), type_of.numel()) != \
            (C, C, C * C, (C + 1) ** 2, (C + 1) ** 2, C + 1):
        raise ValueError("crf_chunk_posteriors: CRF parameters / tables do not fit C")
    if allowed is not None and allowed.dtype != torch.int64:
        raise ValueError(f"crf_chunk_posteriors: allowed must be an int64 tensor of tag-set words, got {allowed.dtype}")
    _f32(em, start, end, trans)
    assert mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous()
    assert keep is None or (keep.dtype == torch.uint8 and keep.is_contiguous())
    assert allowed is None or allowed.is_contiguous()
    assert start_tab.dtype == end_tab.dtype == torch.uint8 and type_of.dtype == torch.int32
    assert all(t.is_contiguous() for t in (start_tab, end_tab, type_of))
    if out is None:
        out = (torch.empty((B, S, W, n_types), dtype=torch.float32, device=em.device),
               torch.empty(B, dtype=torch.float32, device=em.device))
    log_post, logz_a = out
    assert tuple(log_post.shape) == (B, S, W, n_types) and logz_a.numel() == B
    _f32(log_post, logz_a)
    wsb = lib().mtvaf_crf_chunk_posteriors_workspace_bytes(B, S, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=em.device)
    _ck(lib().mtvaf_crf_chunk_posteriors(_p(em), _p(allowed), _p(mask_u8), _p(keep), _p(start), _p(end), _p(trans),
                                         _p(start_tab), _p(end_tab), _p(type_of), n_types, W, _p(log_post), _p(logz_a), B, S,
                                         C, _p(ws), wsb, _st()), "mtvaf_crf_chunk_posteriors")
    return log_post, logz_a


CALIBRATION_MAX_S, CALIBRATION_MAX_C, CALIBRATION_MAX_T, CALIBRATION_MAX_W, CALIBRATION_MAX_E, CALIBRATION_MAX_BINS = \
    512, 64, 64, 16, 64, 64


def calibration_words(n_types, n_bins):
    """8-byte words of the counter block of `chunk_calibration` / `entity_calibration` (include/mtvaf_hip.h): n [T,NB], hit
    [T,NB], gold [T], gold_reachable [T] as int64, sum_p [T,NB], sum_sq [T,NB] as float64, sentences as int64."""
    return 4 * n_types * n_bins + 2 * n_types + 1


def _calibration_common(name, gold, mask_u8, keep, start_tab, end_tab, type_of, edges, n_types, counter):
    """The checks both calibration entries share -> (B, S, C, n_bins)"""
    if gold.dim() != 2:
        raise ValueError(f"{name}: gold {tuple(gold.shape)}: expected [B, S]")
    B, S = gold.shape
    C, NB = type_of.numel() - 1, edges.numel() - 1
    if not 1 <= S <= CALIBRATION_MAX_S:
        raise ValueError(f"{name}: S={S} outside 1..{CALIBRATION_MAX_S}")
    if not 1 <= C <= CALIBRATION_MAX_C:
        raise ValueError(f"{name}: C={C} outside 1..{CALIBRATION_MAX_C}")
    if not 1 <= n_types <= CALIBRATION_MAX_T:
        raise ValueError(f"{name}: n_types={n_types} outside 1..{CALIBRATION_MAX_T}")
    if not 1 <= NB <= CALIBRATION_MAX_BINS:
        raise ValueError(f"{name}: {NB} bins outside 1..{CALIBRATION_MAX_BINS}")
    if B < 1 or tuple(mask_u8.shape) != (B, S) or (keep is not None and tuple(keep.shape) != (B, S)):
        raise ValueError(f"{name}: mask {tuple(mask_u8.shape)} / keep do not fit gold [{B}, {S}]")
    if (start_tab.numel(), end_tab.numel()) != ((C + 1) ** 2, (C + 1) ** 2) or counter.numel() != calibration_words(n_types, NB):
        raise ValueError(f"{name}: tables / counter block do not fit C, n_types and the bins")
    assert gold.dtype == torch.int64 and gold.is_contiguous() and mask_u8.dtype == torch.uint8 and mask_u8.is_contiguous()
    assert keep is None or (keep.dtype == torch.uint8 and keep.is_contiguous())
    assert start_tab.dtype == end_tab.dtype == torch.uint8 and type_of.dtype == torch.int32 and edges.dtype == torch.float32
    assert counter.dtype == torch.int64 and all(t.is_contiguous() for t in (start_tab, end_tab, type_of, edges, counter))
    return B, S, C, NB


def chunk_calibration(log_post, gold, mask_u8, keep, start_tab, end_tab, type_of, edges, counter):
    """Adds the calibration counts of one batch's chunk events into ``counter`` (csrc/calibration.hip), two launches and no host
    sync.  log_post [B,S,W,T] fp32 (`crf_chunk_posteriors`'), gold [B,S] int64, mask_u8 [B,S] uint8 (a prefix mask), keep [B,S]
    uint8 or None (= columns 1 .. L-1); start_tab / end_tab [(C+1)^2] uint8, type_of [C+1] int32; edges [NB+1] fp32 ascending
    log-probability bin edges; counter [`calibration_words`(T, NB)] int64 words (the two sums are float64 bit patterns)."""
    if log_post.dim() != 4:
        raise ValueError(f"chunk_calibration: log_post {tuple(log_post.shape)}: expected [B, S, W, T]")
    W, T = int(log_post.shape[2]), int(log_post.shape[3])
    if not 1 <= W <= CALIBRATION_MAX_W:
        raise ValueError(f"chunk_calibration: max_width={W} outside 1..{CALIBRATION_MAX_W}")
    B, S, C, NB = _calibration_common("chunk_calibration", gold, mask_u8, keep, start_tab, end_tab, type_of, edges, T, counter)
    if tuple(log_post.shape[:2]) != (B, S):
        raise ValueError(f"chunk_calibration: log_post {tuple(log_post.shape)} does not fit gold [{B}, {S}]")
    _f32(log_post)
    wsb = lib().mtvaf_calibration_workspace_bytes(B, T, NB)
    ws = torch.empty(wsb, dtype=torch.uint8, device=log_post.device)
    _ck(lib().mtvaf_chunk_calibration(_p(log_post), _p(gold), _p(mask_u8), _p(keep), _p(start_tab), _p(end_tab), _p(type_of),
                                      _p(edges), B, S, C, T, W, NB, _p(counter), _p(ws), wsb, _st()), "mtvaf_chunk_calibration")
    return counter


def entity_calibration(ents, log_conf, gold, mask_u8, keep, start_tab, end_tab, type_of, edges, n_types, counter):
    """Adds the calibration counts of one batch's listed entities into ``counter`` (csrc/calibration.hip), two launches and no
    host sync.  ents [B,E,3] int32 (start column, end column, type; -1 in unused slots) and log_conf [B,E] fp32 as `crf_entities`
    returns them; the other arguments as `chunk_calibration`."""
    if ents.dim() != 3 or ents.shape[2] != 3 or tuple(log_conf.shape) != tuple(ents.shape[:2]):
        raise ValueError(f"entity_calibration: ents {tuple(ents.shape)}, log_conf {tuple(log_conf.shape)}: expected [B, E, 3] "
                         "and [B, E]")
    E, n_types = int(ents.shape[1]), int(n_types)
    if not 1 <= E <= CALIBRATION_MAX_E:
        raise ValueError(f"entity_calibration: max_entities={E} outside 1..{CALIBRATION_MAX_E}")
    B, S, C, NB = _calibration_common("entity_calibration", gold, mask_u8, keep, start_tab, end_tab, type_of, edges, n_types,
                                      counter)
    if ents.shape[0] != B:
        raise ValueError(f"entity_calibration: ents {tuple(ents.shape)} do not fit gold [{B}, {S}]")
    _f32(log_conf)
    assert ents.dtype == torch.int32 and ents.is_contiguous()
    wsb = lib().mtvaf_calibration_workspace_bytes(B, n_types, NB)
    ws = torch.empty(wsb, dtype=torch.uint8, device=ents.device)
    _ck(lib().mtvaf_entity_calibration(_p(ents), _p(log_conf), _p(gold), _p(mask_u8), _p(keep), _p(start_tab), _p(end_tab),
                                       _p(type_of), _p(edges), B, S, C, n_types, E, NB, _p(counter), _p(ws), wsb, _st()),
        "mtvaf_entity_calibration")
    return counter


def mask_mul(x, row_keep, col_keep, out):
    B, S, H = x.shape
    _ck(lib().mtvaf_mask_mul(_p(x), _p(row_keep), _p(col_keep), _p(out), B, S, H, _st()), "mtvaf_mask_mul")
    return out


# ---- bf16-operand GEMM (csrc/gemm_bf16x.hip) ----------------------------------------------------------------------
def cast_bf16(x, out=None, out_t=None):
    """x [R,C] fp32 -> out [R,C] bf16 and / or out_t [C,R] bf16 (either may be None)."""
    R, C = x.shape
    _ck(lib().mtvaf_cast_bf16(_p(x), x.stride(0), _p(out), out.stride(0) if out is not None else 0, _p(out_t),
                              out_t.stride(0) if out_t is not None else 0, R, C, _st()), "mtvaf_cast_bf16")


def gemm_bf16x(a, layout_a, b, layout_b, M, N, K, out32=None, out16=None, bias=None, epi=EPI_NONE, aux16=None,
               accumulate=False, colpart=None, allow_split=False, tile=0, splits=-1, stages=0, ktiles=None):
    """out[M,N] = opA[M,K] . opB[K,N], bf16 operands, fp32 accumulation.  KC: a is [M,K] / b is [N,K]; KM: a is [K,M] /
    b is [K,N] (the same row-major tensors read in their other role).  out32 fp32 and / or out16 bf16; aux16: bf16
    pre-activation (written by EPI_GELU, read by EPI_DGELU); colpart [M/128, N] fp32 per-tile column sums of the result."""
    ws, wsb = None, 0
    if allow_split:
        wsb = 8 * M * N * 4
        ws = workspace(wsb, a.device)
    if ktiles is not None:  # (a, KM) is exactly zero outside the listed 64-row k-tiles (mtvaf_build_ktiles, bk = 64)
        _ck(lib().mtvaf_gemm_bf16x_ktiles(layout_a, layout_b, _p(a), a.stride(0), _p(b), b.stride(0), _p(out32),
                                          out32.stride(0) if out32 is not None else 0, _p(out16),
                                          out16.stride(0) if out16 is not None else 0, M, N, K, _p(bias), epi, _p(aux16),
                                          aux16.stride(0) if aux16 is not None else 0, int(accumulate), _p(colpart),
                                          int(allow_split), _p(ws), wsb, tile, splits, stages, _p(ktiles[0]), _p(ktiles[1]),
                                          _st()), "mtvaf_gemm_bf16x_ktiles")
        return
    _ck(lib().mtvaf_gemm_bf16x(layout_a, layout_b, _p(a), a.stride(0), _p(b), b.stride(0), _p(out32),
                               out32.stride(0) if out32 is not None else 0, _p(out16),
                               out16.stride(0) if out16 is not None else 0, M, N, K, _p(bias), epi, _p(aux16),
                               aux16.stride(0) if aux16 is not None else 0, int(accumulate), _p(colpart), int(allow_split),
                               _p(ws), wsb, tile, splits, stages, _st()), "mtvaf_gemm_bf16x")


_sk_scratch = {}


def streamk_ensure(device) -> bool:
    """Attach (once per device and stream) the scratch of the stream-K launches of the 256x256 bf16 kernel to the CURRENT
    stream: 4 KiB of flag words + one 256-KiB slab per CU, zero-initialised, owned here.  False: the library serves no more
    streams and keeps to its tile-per-block / split-K launches on this one."""
    key = (torch.device(device).index or 0, _st())
    if key not in _sk_scratch:
        nbytes = int(lib().mtvaf_streamk_scratch_bytes(256))
        # zero-filled ON the stream it is attached to: every launch that uses it is ordered behind the fill (no host sync --
        # this may run inside a HIP-graph capture, where the fill simply becomes the graph's first node)
        buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        if lib().mtvaf_streamk_attach(_p(buf), nbytes, key[1]) != 0:  # (the library serves 8 streams)
            _sk_scratch[key] = None
        else:
            _sk_scratch[key] = buf
    return _sk_scratch[key] is not None


def streamk_detach_all():
    for (_, st), buf in list(_sk_scratch.items()):
        if buf is not None:
            _ck(lib().mtvaf_streamk_attach(None, 0, st), "mtvaf_streamk_attach")
    _sk_scratch.clear()
    _sk_poll.clear()


def streamk_error(device) -> int:
    """The error word of the current stream's scratch (non-zero: a bounded wait inside a stream-K launch ran out)."""
    buf = _sk_scratch.get((torch.device(device).index or 0, _st()))
    return 0 if buf is None else int(buf[4092:4096].view(torch.int32).item())


def streamk_errors() -> int:
    """Sum of the error words of every attached scratch (all streams); synchronises.  Non-zero: some finisher's bounded wait
    ran out and its tile is wrong -- never observed; bench.py and the tests assert it."""
    torch.cuda.synchronize()
    return sum(int(buf[4092:4096].view(torch.int32).item()) for buf in _sk_scratch.values() if buf is not None)


_sk_poll = {}


def streamk_poll():
    """Asynchronous check of the stream-K error words, for once-per-step callers (the encoder backward in bf16 mode): raises if
    the copy enqueued by the PREVIOUS call has landed non-zero, then enqueues a fresh 4-byte copy of every attached scratch's
    error word to pinned memory on the current stream.  No host synchronisation: a timed-out wait (wrong weight gradients in
    that launch) surfaces one step later instead of never; the header is re-zeroed so that later launches do not read the
    stale flags the failed launch left behind.  Inside a HIP-graph capture it does nothing (pinned allocations and host
    reads would invalidate the capture; bench.py and the graph tests call streamk_errors() instead)."""
    if torch.cuda.is_current_stream_capturing():
        return
    for key, buf in _sk_scratch.items():
        if buf is None:
            continue
        ent = _sk_poll.get(key)
        if ent is not None:
            host, ev = ent
            if ev.query() and int(host.item()) != 0:
                buf[:4096].zero_()
                host.zero_()
                raise RuntimeError("a stream-K launch of the bf16 GEMM timed out waiting for a contribution: the weight gradients of "
                                   "that step are wrong (mtvaf_amd.hip.streamk_poll); flags and error word were reset")
        else:
            host = torch.zeros(1, dtype=torch.int32).pin_memory()
            ev = torch.cuda.Event()
            _sk_poll[key] = (host, ev)
        host, ev = _sk_poll[key]
        host.copy_(buf[4092:4096].view(torch.int32), non_blocking=True)
        ev.record()


def dw_group_rows(rows: int = -1) -> int:
    """fp32 mode: layers of at most this many token rows send their four weight-gradient products as one grouped launch
    (csrc/executor.hip: mtvaf_dw_group_rows; default 1024, MTVAF_DW_GROUP_ROWS).  rows >= 0 sets it."""
    return lib().mtvaf_dw_group_rows(rows)


def dw_group_wanted(rows: int, H: int, I: int) -> bool:
    """fp32 mode: does a layer of `rows` token rows send its four weight gradients as one grouped launch?  (The rule of
    csrc/executor.hip: few-token layers on the fp32 pipe's grouped ring; under the split arithmetic also longer ones, unsplit,
    on the split kernel's GROUP form.)"""
    return bool(lib().mtvaf_dw_group_wanted(rows, H, I))


def gemm_f32_dw_group(items, K, ktiles=None, splits=-1, dbias=None, accumulate=False):
    """items: up to four (a [K,M] fp32, b [K,N] fp32, out [M,N] fp32): out = a^T . b for each, ONE launch (the 128x96 LDS-DMA
    kernel, or -- split arithmetic, K > 1024, whole 128x128 tiles -- the GROUP form of the wave-specialised split kernel) + one
    ordered slab reduction per product when the reduction is split.  dbias: list of len(items) tensors / None -- dbias[i] [M]
    <- column sums of a over its K rows (the bias gradient that goes with the weight gradient).  accumulate: out and dbias are ADDED to
    (mtvaf_gemm_f32_dw_group_acc: the same plan, the old value added last)."""
    n = len(items)
    vp = lambda ts: (ctypes.c_void_p * n)(*[_p(t) for t in ts])
    ia = lambda xs: (ctypes.c_int * n)(*xs)
    As, Bs, Cs = [i[0] for i in items], [i[1] for i in items], [i[2] for i in items]
    Ms, Ns = ia([t.shape[1] for t in As]), ia([t.shape[1] for t in Bs])
    wsb = int(lib().mtvaf_gemm_f32_dw_group_workspace_bytes(n, Ms, Ns, K, splits))  # the library's own plan, as the executor's call
    if dbias is not None:
        wsb = max(wsb, max(int(lib().mtvaf_colsum_workspace_bytes(K, t.shape[1])) for t in As))
    ws = workspace(max(wsb, 16), As[0].device)
    kl, kc = (ktiles if ktiles is not None else (None, None))
    if accumulate:
        if dbias is not None:
            assert len(dbias) == n
            _f32(*[t for t in dbias if t is not None])
        _ck(lib().mtvaf_gemm_f32_dw_group_acc(n, vp(As), ia([t.stride(0) for t in As]), vp(Bs), ia([t.stride(0) for t in Bs]), vp(Cs),
                                              ia([t.stride(0) for t in Cs]), Ms, Ns, K, _p(kl), _p(kc), vp(dbias) if dbias is not None else None,
                                              _p(ws), ws.numel(), splits, 1, _st()), "mtvaf_gemm_f32_dw_group_acc")
    elif dbias is None:
        _ck(lib().mtvaf_gemm_f32_dw_group(n, vp(As), ia([t.stride(0) for t in As]), vp(Bs), ia([t.stride(0) for t in Bs]), vp(Cs),
                                          ia([t.stride(0) for t in Cs]), Ms, Ns,
                                          K, _p(kl), _p(kc), _p(ws), ws.numel(), splits, _st()), "mtvaf_gemm_f32_dw_group")
    else:
        assert len(dbias) == n
        _f32(*[t for t in dbias if t is not None])
        _ck(lib().mtvaf_gemm_f32_dw_group_bias(n, vp(As), ia([t.stride(0) for t in As]), vp(Bs), ia([t.stride(0) for t in Bs]), vp(Cs),
                                               ia([t.stride(0) for t in Cs]), Ms, Ns, K, _p(kl), _p(kc), vp(dbias), _p(ws), ws.numel(),
                                               splits, _st()), "mtvaf_gemm_f32_dw_group_bias")


def gemm_bf16x_dw_group(items, K, accumulate=False):
    """items: up to four (a [K,M] bf16, b [K,N] bf16, out [M,N] fp32): out = a^T . b for each, ONE stream-K launch."""
    n = len(items)
    vp = lambda ts: (ctypes.c_void_p * n)(*[_p(t) for t in ts])
    ia = lambda xs: (ctypes.c_int * n)(*xs)
    As, Bs, Cs = [i[0] for i in items], [i[1] for i in items], [i[2] for i in items]
    streamk_ensure(As[0].device)
    if accumulate:  # (out += a^T . b: the block that finishes a tile adds the old value last)
        _ck(lib().mtvaf_gemm_bf16x_dw_group_acc(n, vp(As), ia([t.stride(0) for t in As]), vp(Bs), ia([t.stride(0) for t in Bs]), vp(Cs),
                                                ia([t.stride(0) for t in Cs]), ia([t.shape[1] for t in As]), ia([t.shape[1] for t in Bs]),
                                                K, 1, _st()), "mtvaf_gemm_bf16x_dw_group_acc")
        return
    _ck(lib().mtvaf_gemm_bf16x_dw_group(n, vp(As), ia([t.stride(0) for t in As]), vp(Bs), ia([t.stride(0) for t in Bs]), vp(Cs),
                                        ia([t.stride(0) for t in Cs]), ia([t.shape[1] for t in As]), ia([t.shape[1] for t in Bs]),
                                        K, _st()), "mtvaf_gemm_bf16x_dw_group")


def gemm_bf16x_dw_group_pieces(shapes, K, device=None) -> int:
    """shapes: the (M, N) of up to four products over K token rows -> the pieces every tile's reduction is cut into by
    gemm_bf16x_dw_group on the current stream (1: whole tiles; > 1: tiles are shared between blocks; 0: the launch would be refused)."""
    n = len(shapes)
    ia = lambda xs: (ctypes.c_int * n)(*xs)
    if device is not None:
        streamk_ensure(device)
    return int(lib().mtvaf_gemm_bf16x_dw_group_pieces(n, ia([m for m, _ in shapes]), ia([c for _, c in shapes]), K, _st()))


def colsum_small(part, out, accumulate=False):
    rows, cols = part.shape
    _ck(lib().mtvaf_colsum_small(_p(part), rows, cols, _p(out), int(accumulate), _st()), "mtvaf_colsum_small")
    return out


# ---- optimizer / gradient wire format (csrc/optim.hip, csrc/gradnorm.hip) -------------------------------------------
def _clip_ptr(clip):
    """Device state of a gradient norm: 4 floats, {norm, coef, finite, 0} of grad_clip_finalize for the *_dev update kernels or
    {norm, scale, finite, 0} of sam_finalize for the perturb kernels."""
    assert clip.is_cuda and clip.dtype == torch.float32 and clip.numel() >= 4 and clip.is_contiguous(), (clip.device, clip.dtype, clip.shape)
    return clip.data_ptr()


def _ema_arg(ema, like):
    """Device pointer of the average an *_ema update keeps: fp32, contiguous, as long as the parameter."""
    assert ema.is_cuda and ema.dtype == torch.float32 and ema.is_contiguous() and ema.numel() == like.numel(), (ema.device, ema.dtype,
                                                                                                                  ema.shape, like.shape)
    return ema.data_ptr()


def _opt(t, fn=_p, *a):
    return None if t is None else fn(t, *a)


# The pieces every update's argument list is made of, in the order of the C ABI: the flat buffers, then the hyper-parameters of a
# uniform launch (_uniform_args) or the segment table of a segmented one (_seg_table) -- with the host's bias corrections in front
# of grad_scale when `step` is given, without them on the device's schedule --, then what the form adds (_mat_args, the shadow,
# max_blocks) and its optional pointers.
def _flat_args(p, g, m, v, check=True):
    if check:
        _f32(p, g, m, v)
    return _p(p), _p(g), _p(m), _p(v), p.numel()


def _ptr_array(ts, fn=_p):
    return (ctypes.c_void_p * len(ts))(*[fn(t) for t in ts])


def _multi_args(ps, gs, ms, vs):
    return len(ps), _ptr_array(ps), _ptr_array(gs), _ptr_array(ms), _ptr_array(vs), (ctypes.c_long * len(ps))(*[t.numel() for t in ps])


def _bias_corrections(beta1, beta2, step):
    """(1 - beta1^t, sqrt(1 - beta2^t)) of the 1-based step t, in Python doubles: the C ABI rounds each to float once."""
    return 1.0 - beta1 ** step, (1.0 - beta2 ** step) ** 0.5


def _uniform_args(lr, beta1, beta2, eps, weight_decay, grad_scale, step=None):
    bc = () if step is None else _bias_corrections(beta1, beta2, step)
    return (float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), *bc, float(grad_scale))


def _seg_table(segments, beta1, beta2, eps, grad_scale, lr_type, step=None):
    """segments = [(end element, lr, weight_decay), ...] in buffer order; the lr column as `lr_type` (float: this step's lr; double:
    the BASE lr of the device's schedule)."""
    k = len(segments)
    bc = () if step is None else _bias_corrections(beta1, beta2, step)
    return (k, (ctypes.c_long * k)(*[int(s[0]) for s in segments]), (lr_type * k)(*[float(s[1]) for s in segments]),
            (ctypes.c_float * k)(*[float(s[2]) for s in segments]), float(beta1), float(beta2), float(eps), *bc, float(grad_scale))


def _mat_args(mats):
    n = len(mats)
    return (n, (ctypes.c_long * n)(*[s[0] for s in mats]), (ctypes.c_int * n)(*[s[1] for s in mats]),
            (ctypes.c_int * n)(*[s[2] for s in mats]), (ctypes.c_void_p * n)(*[_p(s[3]) for s in mats]))


def _uniform_update(name, args, ema_arg, ema_omd, clip):
    """The three entry points of a uniform update on host scalars: `name`, `name`_dev (clip state) and `name`_ema (the average; the
    clip state optional)."""
    if ema_arg is not None:
        name, args = name + "_ema", (*args, ema_arg, float(ema_omd), _opt(clip, _clip_ptr))
    elif clip is not None:
        name, args = name + "_dev", (*args, _clip_ptr(clip))
    _ck(getattr(lib(), name)(*args, _st()), name)


def adamw_planes(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, segs, grad_scale=1.0, max_blocks=0, clip=None, ema=None,
                 ema_omd=0.0):
    """adamw over a flat buffer that also rewrites the plane images of the matrices inside it: segs = [(begin element, rows, cols,
    image uint8 tensor), ...] (at most four).  clip, ema, ema_omd: see adamw."""
    _uniform_update("mtvaf_adamw_planes", (*_flat_args(p, g, m, v), *_uniform_args(lr, beta1, beta2, eps, weight_decay, grad_scale, step),
                                           *_mat_args(segs), int(max_blocks)), _opt(ema, _ema_arg, p), ema_omd, clip)


def adamw(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, p_bf16=None, max_blocks=0, clip=None, ema=None,
          ema_omd=0.0):
    """In-place AdamW update of one flat fp32 tensor (torch.optim.AdamW semantics); `step` is the 1-based step count;
    max_blocks > 0: a background update on that many blocks (runs under MFMA-bound kernels without starving them).
    clip: the device state written by grad_clip_finalize -- the gradient is scaled by grad_scale * coef on the device, and a
    state whose `finite` is 0 makes the launch write nothing.
    ema: an fp32 tensor as long as p that the same launch averages the new parameter into, ema += ema_omd * (p_new - ema) with
    ema_omd = 1 - decay (1: ema becomes p_new exactly); None: the launch without it."""
    _uniform_update("mtvaf_adamw", (*_flat_args(p, g, m, v, check=False),
                                    *_uniform_args(lr, beta1, beta2, eps, weight_decay, grad_scale, step), _p(p_bf16), int(max_blocks)),
                    _opt(ema, _ema_arg, p), ema_omd, clip)


def _ema_array(ema, ps):
    assert ema is None or len(ema) == len(ps)
    return None if ema is None else (ctypes.c_void_p * len(ps))(*[_ema_arg(e, t) for e, t in zip(ema, ps)])


def adamw_multi(ps, gs, ms, vs, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, clip=None, ema=None, ema_omd=0.0):
    """One launch per 48 tensors of a parameter group sharing hyper-parameters and step count.  clip: see adamw; ema: a list of
    averages parallel to ps (one ema_omd for all of them), None: without."""
    if len(ps) == 0:
        return
    _uniform_update("mtvaf_adamw_multi", (*_multi_args(ps, gs, ms, vs), *_uniform_args(lr, beta1, beta2, eps, weight_decay, grad_scale, step)),
                    _ema_array(ema, ps), ema_omd, clip)


def adamw_seg(p, g, m, v, segments, beta1, beta2, eps, step, grad_scale=1.0, p_bf16=None, max_blocks=0, clip=None, ema=None, ema_omd=0.0):
    """adamw with lr and weight decay per segment of the flat buffer: segments = [(end element, lr, weight_decay), ...], at most 16,
    ends strictly increasing, the last one p.numel(), every other one a multiple of 4.  One launch; each element gets the bits
    adamw gives it on its segment alone.  p_bf16, max_blocks, clip, ema, ema_omd: see adamw (all optional, one entry point)."""
    _ck(lib().mtvaf_adamw_seg(*_flat_args(p, g, m, v), *_seg_table(segments, beta1, beta2, eps, grad_scale, ctypes.c_float, step),
                              _p(p_bf16), int(max_blocks), _opt(ema, _ema_arg, p), float(ema_omd), _opt(clip, _clip_ptr), _st()),
        "mtvaf_adamw_seg")


def adamw_planes_seg(p, g, m, v, segments, beta1, beta2, eps, step, mats, grad_scale=1.0, max_blocks=0, clip=None, ema=None,
                     ema_omd=0.0):
    """adamw_seg that also rewrites the plane images of the matrices inside the buffer: mats = [(begin element, rows, cols, image
    uint8 tensor), ...] (at most four, as adamw_planes' segs; a matrix may lie across segment ends)."""
    _ck(lib().mtvaf_adamw_planes_seg(*_flat_args(p, g, m, v), *_seg_table(segments, beta1, beta2, eps, grad_scale, ctypes.c_float, step),
                                     *_mat_args(mats), int(max_blocks), _opt(ema, _ema_arg, p), float(ema_omd), _opt(clip, _clip_ptr),
                                     _st()), "mtvaf_adamw_planes_seg")


# ---- the schedule on the device: the *_sched updates read lr factor, bias corrections and 1 - decay from `current` -------------------
SCHED_ROW_BYTES = 24      # {double lr_factor; float bc1, bc2_sqrt, ema_omd; int32 pad}
SCHED_CURRENT_BYTES = 32  # {double lr_factor; float bc1, bc2_sqrt, ema_omd; int32 overrun; int64 step}


def _sched_ptr(current):
    """The 32-byte block mtvaf_adamw_sched_advance writes: four int64 on the device."""
    assert current.is_cuda and current.dtype == torch.int64 and current.numel() == 4 and current.is_contiguous(), \
        (current.device, current.dtype, current.shape)
    return current.data_ptr()


def adamw_sched_advance(table, counter, current):
    """counter (device int64, one element) += 1 and the table's row for that step -> current.  table: uint8 on the device, 24 bytes
    per step (optim.schedule_table); past its end current's overrun word is set and every *_sched update writes nothing."""
    assert table.is_cuda and table.dtype == torch.uint8 and table.is_contiguous() and table.numel() % SCHED_ROW_BYTES == 0 \
        and table.numel() > 0, (table.device, table.dtype, table.shape)
    assert counter.is_cuda and counter.dtype == torch.int64 and counter.numel() == 1, (counter.device, counter.dtype, counter.shape)
    _ck(lib().mtvaf_adamw_sched_advance(table.data_ptr(), table.numel() // SCHED_ROW_BYTES, counter.data_ptr(), _sched_ptr(current),
                                        _st()), "mtvaf_adamw_sched_advance")


def _sched_update(name, args, ema_arg, clip, current):
    """Every *_sched entry point ends alike: the average, the clip state (both optional), the schedule block, the stream."""
    _ck(getattr(lib(), name)(*args, ema_arg, _opt(clip, _clip_ptr), _sched_ptr(current), _st()), name)


def adamw_sched(p, g, m, v, base_lr, beta1, beta2, eps, weight_decay, current, grad_scale=1.0, p_bf16=None, max_blocks=0, clip=None,
                ema=None):
    """adamw whose lr is float(base_lr * current.lr_factor) and whose bias corrections and 1 - decay come from `current`: no argument
    changes from step to step.  p_bf16, max_blocks, clip, ema: see adamw."""
    _sched_update("mtvaf_adamw_sched", (*_flat_args(p, g, m, v, check=False),
                                        *_uniform_args(base_lr, beta1, beta2, eps, weight_decay, grad_scale), _p(p_bf16), int(max_blocks)),
                  _opt(ema, _ema_arg, p), clip, current)


def adamw_planes_sched(p, g, m, v, base_lr, beta1, beta2, eps, weight_decay, current, mats, grad_scale=1.0, max_blocks=0, clip=None,
                       ema=None):
    """adamw_planes on the device's schedule (adamw_sched); mats as adamw_planes' segs."""
    _sched_update("mtvaf_adamw_planes_sched", (*_flat_args(p, g, m, v), *_uniform_args(base_lr, beta1, beta2, eps, weight_decay, grad_scale),
                                               *_mat_args(mats), int(max_blocks)), _opt(ema, _ema_arg, p), clip, current)


def adamw_multi_sched(ps, gs, ms, vs, base_lr, beta1, beta2, eps, weight_decay, current, grad_scale=1.0, clip=None, ema=None):
    """adamw_multi on the device's schedule (adamw_sched): any number of tensors, 48 per launch; ema: a list parallel to ps, or None."""
    if len(ps) == 0:
        return
    _sched_update("mtvaf_adamw_multi_sched", (*_multi_args(ps, gs, ms, vs), *_uniform_args(base_lr, beta1, beta2, eps, weight_decay, grad_scale)),
                  _ema_array(ema, ps), clip, current)


def adamw_seg_sched(p, g, m, v, segments, beta1, beta2, eps, current, grad_scale=1.0, p_bf16=None, max_blocks=0, clip=None, ema=None):
    """adamw_seg on the device's schedule: segments = [(end element, base lr, weight_decay), ...]."""
    _sched_update("mtvaf_adamw_seg_sched", (*_flat_args(p, g, m, v), *_seg_table(segments, beta1, beta2, eps, grad_scale, ctypes.c_double),
                                            _p(p_bf16), int(max_blocks)), _opt(ema, _ema_arg, p), clip, current)


def adamw_planes_seg_sched(p, g, m, v, segments, beta1, beta2, eps, current, mats, grad_scale=1.0, max_blocks=0, clip=None, ema=None):
    """adamw_planes_seg on the device's schedule."""
    _sched_update("mtvaf_adamw_planes_seg_sched", (*_flat_args(p, g, m, v), *_seg_table(segments, beta1, beta2, eps, grad_scale, ctypes.c_double),
                                                   *_mat_args(mats), int(max_blocks)), _opt(ema, _ema_arg, p), clip, current)


def swap_f32(a_list, b_list):
    """a_list[i] <-> b_list[i], bit for bit, for fp32 tensors of equal length pair by pair (48 pairs per launch)."""
    k = len(a_list)
    assert len(b_list) == k
    if k == 0:
        return
    for a, b in zip(a_list, b_list):
        assert a.is_cuda and b.is_cuda and a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() \
            and a.numel() == b.numel(), (a.device, b.device, a.dtype, b.dtype, a.shape, b.shape)
    _ck(lib().mtvaf_swap_f32_multi(k, (ctypes.c_void_p * k)(*[t.data_ptr() for t in a_list]),
                                   (ctypes.c_void_p * k)(*[t.data_ptr() for t in b_list]),
                                   (ctypes.c_long * k)(*[t.numel() for t in a_list]), _st()), "mtvaf_swap_f32_multi")


def grad_sqnorm_slots(gs) -> int:
    """Number of partial sums (doubles) grad_sqnorm writes for these tensors: one per chunk of 65536 elements."""
    k = len(gs)
    return int(lib().mtvaf_grad_sqnorm_workspace_bytes(k, (ctypes.c_long * k)(*[t.numel() for t in gs]))) // 8


def grad_sqnorm(gs, partials=None):
    """Sums of squares of the fp32 tensors gs (contiguous; 4-byte aligned views are fine), in double, one per chunk of 65536
    elements, tensor after tensor -> the float64 tensor of partial sums (`partials`, or a new one of grad_sqnorm_slots(gs))."""
    k = len(gs)
    for t in gs:
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() > 0, (t.device, t.dtype, t.shape)
    ns = (ctypes.c_long * k)(*[t.numel() for t in gs])
    slots = int(lib().mtvaf_grad_sqnorm_workspace_bytes(k, ns)) // 8
    if partials is None:
        partials = torch.empty(slots, dtype=torch.float64, device=gs[0].device if k else "cuda")
    assert partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous()
    _ck(lib().mtvaf_grad_sqnorm_multi(k, (ctypes.c_void_p * k)(*[t.data_ptr() for t in gs]), ns, _p(partials),
                                      partials.numel() * 8, _st()), "mtvaf_grad_sqnorm_multi")
    return partials[:slots]


def grad_clip_finalize(partials, max_norm, state, skipped=None, skip_nonfinite=True):
    """state (4 floats on the device) <- {norm, coef, finite, 0} from the partial sums of grad_sqnorm, added in index order:
    coef = min(1, max_norm / (norm + 1e-6)), or 1 for max_norm <= 0; a non-finite norm under skip_nonfinite gives coef = 0,
    finite = 0 and adds 1 to `skipped` (device int32)."""
    assert partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous()
    assert skipped is None or (skipped.is_cuda and skipped.dtype == torch.int32)
    _ck(lib().mtvaf_grad_clip_finalize(_p(partials), partials.numel(), float(max_norm), int(bool(skip_nonfinite)), _clip_ptr(state),
                                       _p(skipped), _st()), "mtvaf_grad_clip_finalize")
    return state


def grad_pack_bf16(src, dst, n, npad):
    _ck(lib().mtvaf_grad_pack_bf16(_p(src), _p(dst), n, npad, _st()), "mtvaf_grad_pack_bf16")


def grad_reduce_bf16(recv, out, world, chunk, scale):
    _ck(lib().mtvaf_grad_reduce_bf16(_p(recv), _p(out), world, chunk, scale, _st()), "mtvaf_grad_reduce_bf16")


def grad_unpack_bf16(src, dst, n):
    _ck(lib().mtvaf_grad_unpack_bf16(_p(src), _p(dst), n, _st()), "mtvaf_grad_unpack_bf16")


# ---- adversarial perturbation of the embedding output (csrc/adversarial.hip) ----------------------------------------
ADV_NORMS = {"l2": 0, "linf": 1}          # MTVAF_ADV_NORM_*
ADV_SCOPES = {"sentence": 0, "token": 1}  # MTVAF_ADV_SCOPE_*
ADV_MAX_S, ADV_MAX_H = 512, 1024


def adv_mask(mask):
    """[B,S] mask of any dtype -> the contiguous u8 form the kernels read (non-zero = live)."""
    if mask.dtype == torch.uint8 and mask.is_contiguous():
        return mask
    return mask.ne(0).contiguous().view(torch.uint8)


def adv_perturb(g, mask, eps, step=0.0, norm="l2", scope="sentence", delta_in=None, x=None, delta_out=None, out=None, stats=None):
    """One FGM (delta_in None) / PGD step on the gradient g [B,S,H] at the embedding output (include/mtvaf_hip.h,
    mtvaf_adv_perturb): -> (delta_out [B,S,H], out = x + delta_out or None, stats [B,2] = |g|, |delta_out| per sentence).
    mask [B,S], non-zero = live, any dtype; ``out`` is made when x is given.  No host sync; the launches go to the current stream.
    delta_out may be delta_in."""
    _f32(g, delta_in, x, delta_out, out, stats)
    if g.dim() != 3:
        raise ValueError(f"adv_perturb: g {tuple(g.shape)}: expected [B, S, H]")
    B, S, H = g.shape
    if norm not in ADV_NORMS or scope not in ADV_SCOPES:
        raise ValueError(f"adv_perturb: norm {norm!r} / scope {scope!r}: expected one of {sorted(ADV_NORMS)} / {sorted(ADV_SCOPES)}")
    m8 = adv_mask(mask)
    if tuple(m8.shape) != (B, S):
        raise ValueError(f"adv_perturb: mask {tuple(mask.shape)} does not match g {tuple(g.shape)}")
    for name, t in (("delta_in", delta_in), ("x", x), ("delta_out", delta_out), ("out", out)):
        if t is not None and t.shape != g.shape:
            raise ValueError(f"adv_perturb: {name} {tuple(t.shape)} does not match g {tuple(g.shape)}")
    if delta_out is None:
        delta_out = torch.empty_like(g)
    if out is not None and x is None:
        raise ValueError("adv_perturb: out = x + delta_out needs x")
    if x is not None and out is None:
        out = torch.empty_like(g)
    if stats is None:
        stats = torch.empty(B, 2, dtype=torch.float32, device=g.device)
    assert tuple(stats.shape) == (B, 2), stats.shape
    nbytes = int(lib().mtvaf_adv_workspace_bytes(B, S))
    ws = workspace(nbytes, g.device)
    _ck(lib().mtvaf_adv_perturb(_p(g), _p(delta_in), _p(x), _p(m8), _p(delta_out), _p(out), _p(stats), B, S, H,
                                float(eps), float(step), ADV_NORMS[norm], ADV_SCOPES[scope], _p(ws), ws.numel(), _st()),
        "mtvaf_adv_perturb")
    return delta_out, out, stats


def adv_add(x, delta, out=None):
    """out = x + delta (fp32, same shape, contiguous): the forward of the embedding tap."""
    _f32(x, delta, out)
    assert x.shape == delta.shape, (x.shape, delta.shape)
    if out is None:
        out = torch.empty_like(x)
    _ck(lib().mtvaf_adv_add(_p(x), _p(delta), _p(out), x.numel(), _st()), "mtvaf_adv_add")
    return out


# ---- sharpness-aware minimisation: the ascent step in weight space (csrc/optim.hip, csrc/gradnorm.hip) --------------
def _sam_same(p, *others):
    _f32(p, *others)
    for t in others:
        assert t is None or t.numel() == p.numel(), (p.shape, t.shape)


def sam_finalize(partials, rho, state, skipped=None):
    """state (4 floats on the device) <- {norm, scale, finite, 0} from the partial sums of grad_sqnorm, added in index order:
    scale = float(rho / (norm + 1e-12)) with the quotient in double; a norm that fp32 cannot hold gives scale = 0, finite = 0 and
    adds 1 to `skipped` (device int32)."""
    assert partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous()
    assert skipped is None or (skipped.is_cuda and skipped.dtype == torch.int32)
    _ck(lib().mtvaf_sam_finalize(_p(partials), partials.numel(), float(rho), _clip_ptr(state), _p(skipped), _st()),
        "mtvaf_sam_finalize")
    return state


def sam_perturb(p, g, backup, state, p_bf16=None):
    """backup = p; p = fmaf(scale, g, p) over one flat fp32 tensor, scale read from the device state of sam_finalize (finite == 0: p
    keeps its bits, backup is written all the same).  p_bf16: the bf16 shadow of p, written from the new p in the same pass."""
    _sam_same(p, g, backup)
    _ck(lib().mtvaf_sam_perturb(_p(p), _p(g), _p(backup), p.numel(), _clip_ptr(state), _p(p_bf16), _st()), "mtvaf_sam_perturb")


def sam_perturb_planes(p, g, backup, state, segs):
    """sam_perturb over a flat buffer that also rewrites the plane images of the matrices inside it: segs as adamw_planes'."""
    _sam_same(p, g, backup)
    _ck(lib().mtvaf_sam_perturb_planes(_p(p), _p(g), _p(backup), p.numel(), _clip_ptr(state), *_mat_args(segs), _st()),
        "mtvaf_sam_perturb_planes")


def sam_perturb_multi(ps, gs, backups, state):
    """sam_perturb over lists of tensors: one launch per 48."""
    k = len(ps)
    assert len(gs) == k and len(backups) == k
    if k == 0:
        return
    for t in zip(ps, gs, backups):
        _sam_same(*t)
    _ck(lib().mtvaf_sam_perturb_multi(k, _ptr_array(ps), _ptr_array(gs), _ptr_array(backups), (ctypes.c_long * k)(*[t.numel() for t in ps]),
                                      _clip_ptr(state), _st()), "mtvaf_sam_perturb_multi")


def sam_restore(p, backup, p_bf16=None):
    """p = backup, bit for bit; p_bf16: the bf16 shadow of p, rewritten from the restored values."""
    _sam_same(p, backup)
    _ck(lib().mtvaf_sam_restore(_p(p), _p(backup), p.numel(), _p(p_bf16), _st()), "mtvaf_sam_restore")


def sam_restore_planes(p, backup, segs):
    """sam_restore over a flat buffer that also rewrites the plane images of the matrices inside it: segs as adamw_planes'."""
    _sam_same(p, backup)
    _ck(lib().mtvaf_sam_restore_planes(_p(p), _p(backup), p.numel(), *_mat_args(segs), _st()), "mtvaf_sam_restore_planes")


def sam_restore_multi(ps, backups):
    """sam_restore over lists of tensors: one launch per 48 (no image is rewritten)."""
    k = len(ps)
    assert len(backups) == k
    if k == 0:
        return
    for t in zip(ps, backups):
        _sam_same(*t)
    _ck(lib().mtvaf_sam_restore_multi(k, _ptr_array(ps), _ptr_array(backups), (ctypes.c_long * k)(*[t.numel() for t in ps]), _st()),
        "mtvaf_sam_restore_multi")


# ---- word-level tagging head: the word axis, piece-to-word pooling and its backward (csrc/wordpool.hip) -------------
WORD_POOL_MODES = {"first": 0, "last": 1, "mean": 2}  # MTVAF_WORD_POOL_*
WORD_MAX_S = 512


def _word_out(t, shape, dtype, device, name):
    """An output the caller may bring (tests pre-fill it): checked, or allocated."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor of shape {tuple(shape)} on the device, got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")
    return t


def _word_i32(t, shape, name):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name}: expected a contiguous int32 tensor of shape {tuple(shape)} on the device, got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")
    return t


def word_index(attention_mask, token_to_word, max_words=None, out=None):
    """The word axis of a batch (include/mtvaf_hip.h, mtvaf_word_index): attention_mask [B,S], a prefix mask of any dtype
    (non-zero = live); token_to_word [B,S] int32, -1 outside the map.  -> dict of col_start, col_len [B,W] int32, col_of_token
    [B,S] int32, word_mask [B,W] uint8, word_id [B,W] int32, n_cols [B] int32, with W = max_words or S.  ``out``: a dict holding
    any of those tensors to write into.  No host sync; the launch goes to the current stream."""
    if attention_mask.dim() != 2:
        raise ValueError(f"word_index: attention_mask {tuple(attention_mask.shape)}: expected [B, S]")
    B, S = attention_mask.shape
    W = S if max_words is None else int(max_words)
    if W < 1:
        raise ValueError(f"word_index: max_words {max_words}: expected a width >= 1")
    m8 = adv_mask(attention_mask)
    _word_i32(token_to_word, (B, S), "word_index: token_to_word")
    out = dict(out or {})
    dev = m8.device
    res = {}
    for name, shape, dtype in (("col_start", (B, W), torch.int32), ("col_len", (B, W), torch.int32),
                               ("col_of_token", (B, S), torch.int32), ("word_mask", (B, W), torch.uint8),
                               ("word_id", (B, W), torch.int32), ("n_cols", (B,), torch.int32)):
        res[name] = _word_out(out.pop(name, None), shape, dtype, dev, f"word_index: {name}")
    if out:
        raise ValueError(f"word_index: unknown outputs {sorted(out)}")
    _ck(lib().mtvaf_word_index(_p(m8), _p(token_to_word), _p(res["col_start"]), _p(res["col_len"]), _p(res["col_of_token"]),
                               _p(res["word_mask"]), _p(res["word_id"]), _p(res["n_cols"]), B, S, W, _st()), "mtvaf_word_index")
    return res


def _word_mode(mode, who):
    if mode not in WORD_POOL_MODES:
        raise ValueError(f"{who}: mode {mode!r}: expected one of {sorted(WORD_POOL_MODES)}")
    return WORD_POOL_MODES[mode]


def _word_rows(t, name):
    """[B,N,H] fp32 on the device whose rows lie one behind the other (a view that starts off a 16-byte boundary is fine: the
    kernels then take their scalar path)."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous fp32 [B, N, H] tensor on the device, got {t.dtype} {tuple(t.shape)} on "
                         f"{t.device}")
    return t


def word_pool_fwd(x, col_start, col_len, mode="first", out=None):
    """y [B,W,H] = the pieces of every column of x [B,S,H] pooled (first | last | mean; mtvaf_word_pool_fwd); dead columns are
    exact zeros.  col_start / col_len [B,W] int32 from word_index."""
    _word_rows(x, "word_pool_fwd: x")
    B, S, H = x.shape
    if col_start.dim() != 2 or col_start.shape[0] != B:
        raise ValueError(f"word_pool_fwd: col_start {tuple(col_start.shape)} does not match x {tuple(x.shape)}")
    W = col_start.shape[1]
    _word_i32(col_start, (B, W), "word_pool_fwd: col_start")
    _word_i32(col_len, (B, W), "word_pool_fwd: col_len")
    m = _word_mode(mode, "word_pool_fwd")
    out = _word_out(out, (B, W, H), torch.float32, x.device, "word_pool_fwd: out")
    _ck(lib().mtvaf_word_pool_fwd(_p(x), _p(col_start), _p(col_len), _p(out), B, S, W, H, m, _st()), "mtvaf_word_pool_fwd")
    return out


def word_pool_bwd(dy, col_start, col_len, col_of_token, mode="first", out=None):
    """dx [B,S,H] from dy [B,W,H]: every token row gathers its column's dy (mtvaf_word_pool_bwd); masked tokens, tokens of
    dropped columns and unselected pieces get exact zeros."""
    _word_rows(dy, "word_pool_bwd: dy")
    B, W, H = dy.shape
    if col_of_token.dim() != 2 or col_of_token.shape[0] != B:
        raise ValueError(f"word_pool_bwd: col_of_token {tuple(col_of_token.shape)} does not match dy {tuple(dy.shape)}")
    S = col_of_token.shape[1]
    _word_i32(col_start, (B, W), "word_pool_bwd: col_start")
    _word_i32(col_len, (B, W), "word_pool_bwd: col_len")
    _word_i32(col_of_token, (B, S), "word_pool_bwd: col_of_token")
    m = _word_mode(mode, "word_pool_bwd")
    out = _word_out(out, (B, S, H), torch.float32, dy.device, "word_pool_bwd: out")
    _ck(lib().mtvaf_word_pool_bwd(_p(dy), _p(col_start), _p(col_len), _p(col_of_token), _p(out), B, S, W, H, m, _st()),
        "mtvaf_word_pool_bwd")
    return out


# ---- layer mix: a learned weighted sum of hidden states, its parameter gradients and the injection (csrc/layermix.hip) ---------
LAYER_MIX_MAX_K = 32                  # MTVAF_LAYER_MIX_MAX_K
LAYER_MIX_WORKSPACE_BYTES = 262144    # MTVAF_LAYER_MIX_WORKSPACE_BYTES


def _mix_states(states, who):
    """The K states as the host array of device pointers the entry points take -> (array, K, rows, H)."""
    K = len(states)
    if not 1 <= K <= LAYER_MIX_MAX_K:
        raise ValueError(f"{who}: {K} states: expected 1 .. {LAYER_MIX_MAX_K}")
    shape = tuple(states[0].shape)
    for t in states:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape and t.dim() >= 2):
            raise ValueError(f"{who}: every state must be a contiguous fp32 [..., H] tensor of one shape on the device, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
    H = shape[-1]
    return (ctypes.c_void_p * K)(*[t.data_ptr() for t in states]), K, states[0].numel() // H, H


def _mix_vec(t, n, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
        raise ValueError(f"{name}: expected {n} contiguous fp32 value(s) on the device, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def layer_mix_fwd(states, scalars, gamma, out=None):
    """y = gamma * sum_j softmax(scalars)_j * states[j] (mtvaf_layer_mix_fwd): states a list of K fp32 tensors of one shape
    [..., H], H % 4 == 0; scalars [K] and gamma [1] on the device (no host read)."""
    arr, K, rows, H = _mix_states(states, "layer_mix_fwd")
    _mix_vec(scalars, K, "layer_mix_fwd: scalars")
    _mix_vec(gamma, 1, "layer_mix_fwd: gamma")
    out = _word_out(out, states[0].shape, torch.float32, states[0].device, "layer_mix_fwd: out")
    _ck(lib().mtvaf_layer_mix_fwd(arr, K, _p(scalars), _p(gamma), _p(out), rows, H, _st()), "mtvaf_layer_mix_fwd")
    return out


def layer_mix_dots(states, dy, scalars, gamma, rows=None):
    """-> (dscalars [K], dgamma [1], coef [K]) of the mix for the upstream gradient dy (mtvaf_layer_mix_dots); coef[j] = gamma * s_j
    is what `layer_mix_inject` multiplies dy by.  rows: take only the leading rows of every tensor (a packed image's live rows)."""
    arr, K, all_rows, H = _mix_states(states, "layer_mix_dots")
    rows = all_rows if rows is None else int(rows)
    if not (dy.is_cuda and dy.dtype == torch.float32 and dy.is_contiguous() and dy.numel() == states[0].numel()) or not 1 <= rows <= all_rows:
        raise ValueError(f"layer_mix_dots: dy {dy.dtype} {tuple(dy.shape)} / rows {rows} do not match the states {tuple(states[0].shape)}")
    _mix_vec(scalars, K, "layer_mix_dots: scalars")
    _mix_vec(gamma, 1, "layer_mix_dots: gamma")
    dev = dy.device
    ws = torch.empty(LAYER_MIX_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
    dscalars, dgamma, coef = (torch.empty(n, dtype=torch.float32, device=dev) for n in (K, 1, K))
    _ck(lib().mtvaf_layer_mix_dots(arr, K, _p(dy), _p(scalars), _p(gamma), rows, H, _p(ws), ws.numel(), _p(dscalars), _p(dgamma),
                                   _p(coef), _st()), "mtvaf_layer_mix_dots")
    return dscalars, dgamma, coef


def layer_mix_inject(coef, j, dy, dh=None):
    """dh = fmaf(coef[j], dy, dh) in place, or a new dh = coef[j] * dy where none exists yet (mtvaf_layer_mix_inject)."""
    if not (dy.is_cuda and dy.dtype == torch.float32 and dy.is_contiguous() and dy.dim() >= 2):
        raise ValueError(f"layer_mix_inject: dy {dy.dtype} {tuple(dy.shape)} on {dy.device}: expected contiguous fp32 [..., H] on the device")
    K = coef.numel()
    _mix_vec(coef, K, "layer_mix_inject: coef")
    H = dy.shape[-1]
    acc = dh is not None
    dh = _word_out(dh, dy.shape, torch.float32, dy.device, "layer_mix_inject: dh")
    _ck(lib().mtvaf_layer_mix_inject(_p(coef), int(j), K, _p(dy), _p(dh), dy.numel() // H, H, int(acc), _st()), "mtvaf_layer_mix_inject")
    return dh


# -------------------------------------------------------------------------------------------------
# masked-LM head (csrc/mlm.hip)
# -------------------------------------------------------------------------------------------------
VOCAB_CE_REDUCTIONS = {"mean": 0, "sum": 1}
MLM_MAX_SPECIAL = 8


def _i32(t, n, what):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= n):
        raise ValueError(f"{what}: {t.dtype} {tuple(t.shape)} on {t.device}: expected contiguous int32 [>= {n}] on the device")


def uniform_fill(out, seed, offset):
    """out (fp32, contiguous, device): uniforms in [0, 1) from the dropout generator at (seed, offset)."""
    _f32(out)
    _ck(lib().mtvaf_uniform_fill(_p(out), out.numel(), seed, offset, _st()), "mtvaf_uniform_fill")
    return out


def mlm_mask(input_ids, live_u8, special_u8, uniforms, special_ids, probability, mask_token_id, vocab_size, capacity):
    """mtvaf_mlm_mask on [B,S] int64 ids, u8 masks and [B,S,3] fp32 uniforms (all contiguous, on the device).
    -> ids_out [B,S] int64, positions [capacity] int32, labels [capacity] int64, count [1] int32, stats [3] int32."""
    B, S = input_ids.shape
    dev = input_ids.device
    for t, dt, n, what in ((input_ids, torch.int64, B * S, "input_ids"), (live_u8, torch.uint8, B * S, "attention mask"),
                           (special_u8, torch.uint8, B * S, "special_mask"), (uniforms, torch.float32, 3 * B * S, "uniforms")):
        if t is not None and not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == n):
            raise ValueError(f"mlm_mask: {what} {t.dtype} {tuple(t.shape)} on {t.device}: expected contiguous {dt} with {n} elements "
                             "on the device")
    special_ids = [int(i) for i in special_ids]
    if len(special_ids) > MLM_MAX_SPECIAL:
        raise ValueError(f"mlm_mask: {len(special_ids)} special ids (at most {MLM_MAX_SPECIAL}; use special_mask for more)")
    if not 1 <= int(capacity) <= B * S:
        raise ValueError(f"mlm_mask: capacity {capacity} outside 1 .. {B * S}")
    sp = (c_int64 * MLM_MAX_SPECIAL)(*special_ids)
    ids_out = torch.empty_like(input_ids)
    positions = torch.empty(capacity, dtype=torch.int32, device=dev)
    labels = torch.empty(capacity, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    stats = torch.empty(3, dtype=torch.int32, device=dev)
    wsb = lib().mtvaf_mlm_mask_workspace_bytes(B)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _ck(lib().mtvaf_mlm_mask(_p(input_ids), _p(live_u8), _p(special_u8), _p(uniforms), sp, len(special_ids), float(probability),
                             int(mask_token_id), int(vocab_size), int(capacity), _p(ids_out), _p(positions), _p(labels), _p(count),
                             _p(stats), _p(ws), wsb, B, S, _st()), "mtvaf_mlm_mask")
    return ids_out, positions, labels, count, stats


def gather_rows(src, rowmap, out):
    """out[r] = src[rowmap[r]] (zeros where rowmap[r] < 0); src [rows_src,H], out [rows,H] fp32, rowmap int32 [rows]."""
    _f32(src, out)
    _i32(rowmap, out.shape[0], "gather_rows: rowmap")
    _ck(lib().mtvaf_gather_rows(_p(src), _p(rowmap), _p(out), out.shape[0], out.shape[1], _st()), "mtvaf_gather_rows")
    return out


def scatter_rows(d, rowmap, dsrc):
    """dsrc = 0, then dsrc[rowmap[r]] = d[r] for the rows with rowmap[r] >= 0 (distinct): the backward of gather_rows."""
    _f32(d, dsrc)
    _i32(rowmap, d.shape[0], "scatter_rows: rowmap")
    _ck(lib().mtvaf_scatter_rows(_p(d), _p(rowmap), _p(dsrc), d.shape[0], dsrc.shape[0], d.shape[1], _st()), "mtvaf_scatter_rows")
    return dsrc


def dgelu(dy, pre, out):
    """out = dy * gelu_erf'(pre), elementwise (contiguous fp32 of one shape)."""
    _f32(dy, pre, out)
    assert dy.shape == pre.shape == out.shape, (dy.shape, pre.shape, out.shape)
    _ck(lib().mtvaf_dgelu(_p(dy), _p(pre), _p(out), dy.numel(), _st()), "mtvaf_dgelu")
    return out


def vocab_ce_workspace_bytes(R, H, V, chunk):
    return int(lib().mtvaf_vocab_ce_workspace_bytes(int(R), int(H), int(V), int(chunk)))


def _vocab_ce_inputs(logits, bias, labels, count, V, v0, v1):
    _f32(logits, bias)
    R = logits.shape[0]
    assert logits.shape[1] == v1 - v0 and 0 <= v0 < v1 <= V and (bias is None or bias.numel() == V), (tuple(logits.shape), v0, v1, V)
    assert labels.is_cuda and labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == R, (labels.dtype, R)
    _i32(count, 1, "vocab_ce: count")
    return R


def vocab_ce_chunk_fwd(logits, bias, labels, count, state, V, v0, v1):
    """Folds the logits chunk [R, v1 - v0] (+ bias[v0:v1]) into state (fp32 [4 R]); the chunk with v0 == 0 starts it."""
    R = _vocab_ce_inputs(logits, bias, labels, count, V, v0, v1)
    _f32(state)
    assert state.numel() >= 4 * R
    _ck(lib().mtvaf_vocab_ce_chunk_fwd(_p(logits), logits.stride(0), _p(bias), _p(labels), _p(count), _p(state), R, V, v0, v1, _st()),
        "mtvaf_vocab_ce_chunk_fwd")


def vocab_ce_finish(state, labels, count, loss, loss_row, lse_row, stats, V, reduction):
    R = labels.numel()
    _f32(state, loss, loss_row, lse_row)
    _i32(count, 1, "vocab_ce: count")
    _i32(stats, 3, "vocab_ce: stats")
    assert state.numel() >= 4 * R and loss_row.numel() >= R and lse_row.numel() >= R
    _ck(lib().mtvaf_vocab_ce_finish(_p(state), _p(labels), _p(count), _p(loss), _p(loss_row), _p(lse_row), _p(stats), R, V,
                                    int(reduction), _st()), "mtvaf_vocab_ce_finish")


def vocab_ce_chunk_bwd(logits, bias, labels, count, lse_row, gout, grows, stats, V, v0, v1, reduction):
    """In place: the chunk becomes its gradient.  Exactly one of gout [1] and grows [R] is given."""
    R = _vocab_ce_inputs(logits, bias, labels, count, V, v0, v1)
    _f32(lse_row, gout, grows)
    _i32(stats, 3, "vocab_ce: stats")
    assert lse_row.numel() >= R and (grows is None or grows.numel() == R)
    _ck(lib().mtvaf_vocab_ce_chunk_bwd(_p(logits), logits.stride(0), _p(bias), _p(labels), _p(count), _p(lse_row), _p(gout), _p(grows),
                                       _p(stats), R, V, v0, v1, int(reduction), _st()), "mtvaf_vocab_ce_chunk_bwd")
