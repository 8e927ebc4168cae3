"""ctypes binding of ``libskrec_hip.so`` (C ABI declared in ``include/skrec_hip.h``).

This is the only way the host mirror reaches the hot path: there is no CPU fallback.  If the
library is missing, or no gfx950 device is visible when a kernel is needed, the call raises.
PyTorch is used for device memory and streams only: tensors go in as ``data_ptr()`` and the
current stream as ``cuda_stream``.
"""
import ctypes as C
import os

import numpy as np

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # scikit-recommender_amd/
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libskrec_hip.so")
CSRC_DIR = os.path.join(_PKG_ROOT, "csrc")

vp, i32, i64, u32, u64, f32, sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_size_t

# name -> (restype, argtypes); every symbol include/skrec_hip.h declares
SIGNATURES = {
    "skr_abi_version": (i32, []),
    "skr_last_error": (C.c_char_p, []),
    "skr_device_count": (i32, []),
    "skr_device_summary": (i32, [C.c_char_p, sz]),
    "skr_csr_max_row_len": (i32, [vp, i32, C.POINTER(i32), vp]),
    "skr_sampler_create": (i32, [u32, C.POINTER(vp)]),
    "skr_sampler_destroy": (i32, [vp]),
    "skr_sampler_get_state": (i32, [vp, vp, C.POINTER(i32)]),
    "skr_sampler_set_state": (i32, [vp, vp, i32]),
    "skr_sampler_draws": (i32, [vp, C.POINTER(u64)]),
    "skr_sampler_last_epoch": (i32, [vp, C.POINTER(i64)]),
    "skr_sampler_words": (i32, [vp, i64, vp, vp]),
    "skr_sampler_slab_stats": (i32, [vp, C.POINTER(i64)]),
    "skr_mt_jump_host": (i32, [vp, i32, i64, vp, C.POINTER(i32)]),
    "skr_randint_choice": (i32, [vp, i32, i32, i32, vp, vp, i32, vp, vp]),
    "skr_sample_epoch_exact": (i32, [vp, i32, i32, vp, vp, i64, i32, vp, vp]),
    "skr_sample_epoch_exact_counts": (i32, [vp, i32, i32, vp, vp, i64, vp, i64, vp, vp]),
    "skr_csr_row_stats": (i32, [vp, i32, C.POINTER(i64), vp]),
    "skr_sample_epoch_exact_stats": (i32, [vp, i32, i32, vp, vp, i64, i32, vp, C.POINTER(i64), vp]),
    "skr_sample_epoch_fast": (i32, [u64, u64, i64, i32, i32, vp, vp, i64, i32, vp, vp]),
    "skr_adam_block_mark": (i32, [vp, i64, i64, i32, vp, i32, vp, i64, vp]),
    "skr_adam_block_cold": (i32, [vp, vp, vp, i64, f32, f32, f32, f32, i64, i32, vp, i32, vp]),
    "skr_adam_block_hot": (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, i64, i64, vp, i64, i64, i32, vp, vp]),
    "skr_adam_block_cold_rest": (i32, [vp, vp, vp, i64, f32, f32, f32, f32, i64, i32, vp, i32, vp, i32, vp]),
    "skr_cold_rest_census": (i32, [C.POINTER(u64), i32]),
    "skr_adam_step_tf": (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, i64, i32, vp, vp]),
    "skr_adam_block_cold_tf": (i32, [vp, vp, vp, i64, f32, f32, f32, f32, i64, i32, vp, i32, vp]),
    "skr_adam_block_hot_tf": (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, i64, i64, vp, i64, i64, i32, vp, vp]),
    "skr_adam_step_wd": (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i64, i32, vp, vp]),
    "skr_adam_block_cold_wd": (i32, [vp, vp, vp, i64, f32, f32, f32, f32, f32, i64, i32, vp, i32, vp]),
    "skr_adam_block_hot_wd": (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i64, i64, vp, i64, i64, i32, vp, vp]),
    "skr_bpr_fused_plan": (i32, [vp, vp, vp, i32, i32, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp]),
    "skr_bpr_fused_step": (i32, [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, i32, i64, i64, i64, f32, f32, f32, f32, i64, i32, i32,
                                 f32, vp, vp]),
    "skr_bpr_fused_block": (i32, [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, i32, i64, i64, i64, f32, f32, f32, f32, i64, i32, f32, vp,
                                  i64, vp, vp, vp, vp, i32, vp]),
    "skr_bpr_fused_plan2": (i32, [vp, vp, vp, i32, i32, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, i32, vp]),
    "skr_bpr_fused_pre": (i32, [vp, vp, vp, i64, vp, i64, vp, vp, vp, f32, f32, f32, f32, i64, i32, vp, i32, vp]),
    "skr_bpr_fused_step2": (i32, [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, i32, i64, i64, i64, f32, f32, f32, f32, i64, i32, i32,
                                  f32, vp, vp, vp]),
    "skr_bpr_fused_block2": (i32, [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, i32, i64, i64, i64, f32, f32, f32, f32, i64, i32, f32, vp,
                                   i64, vp, vp, vp, vp, i32, vp, vp]),
    "skr_bpr_fused_end": (i32, [vp, vp, vp, i64, vp, i64, vp, vp, vp, f32, f32, f32, f32, i64, i32, vp, i32, i32, vp]),
    "skr_bpr_fused_loss_part_floats": (i64, [i32, i32]),
    "skr_bpr_fused_step3": (i32, [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, i32, i64, i64, i64, f32, f32, f32, f32, i64, i32, i32,
                                  f32, vp, vp, vp, vp]),
    "skr_bpr_fused_end3": (i32, [vp, vp, vp, i64, vp, i64, vp, vp, vp, f32, f32, f32, f32, i64, i32, vp, i32, i32, vp, vp, i64, i32,
                                 vp]),
    "skr_bpr_fused_block3": (i32, [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, i32, i64, i64, i64, f32, f32, f32, f32, i64, i32, f32, vp,
                                   i64, vp, vp, vp, vp, i32, vp, vp, vp]),
    "skr_host_permutation": (i32, [vp, C.POINTER(i32), i64, vp]),
    "skr_shuffle_gather": (i32, [vp, u64, i64, i64, i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(vp), vp]),
    "skr_shuffle_permutation": (i32, [u64, i64, i64, vp, vp]),
    "skr_shuffle_permutation_host": (i32, [u64, i64, i64, vp]),
    "skr_cold_pass_census": (i32, [C.POINTER(u64), i32]),
    "skr_selftest_cold_math": (i32, [u64, C.POINTER(u64), vp]),
    "skr_fused_census": (i32, [C.POINTER(u64), i32, i32]),
    "skr_selftest_grad_math": (i32, [u64, f32, f32, f32, f32, i64, i32, i32, i32, C.POINTER(u64), vp]),
    "skr_selftest_step_chain": (i32, [u64, f32, f32, f32, f32, i64, i32, i32, i32, i32, C.POINTER(u64), vp]),
    "skr_pack_grad_rows": (i32, [vp, i32, vp, vp, i32, vp, vp]),
    "skr_unpack_grad_rows": (i32, [vp, i32, i32, vp, vp, i32, vp, vp, vp]),
    "skr_unpack_grad_rows_sorted": (i32, [vp, i32, i32, vp, vp, i32, vp, vp, vp]),
    "skr_gru_cell_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
    "skr_gru_cell_bwd": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "skr_gru_cell_bwd_scatter": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp,
                                       vp]),
    "skr_session_loss": (i32, [vp, i32, i32, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, vp]),
    "skr_session_loss_sharded": (i32, [vp, i32, i32, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, i32, i32, vp]),
    "skr_session_loss_grads": (i32, [vp, i32, i32, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, i32, i32, f32, vp, vp, vp, vp, vp]),
    "skr_session_out_grads": (i32, [vp, vp, i32, i32, vp, i32, vp, vp, f32, vp, vp, vp, vp, vp]),
    "skr_pop_sample": (i32, [vp, i32, vp, u64, i64, vp, vp]),
    "skr_scatter_add_rows": (i32, [vp, vp, i32, i32, vp, f32, vp, vp, vp, vp]),
    "skr_eval_scores": (i32, [vp, i32, i32, i64, vp, vp, C.POINTER(i32), i32, i32, vp, vp, vp, vp]),
    "skr_eval_fused_workspace": (sz, [i32, i32]),
    "skr_eval_fused_rejected": (i32, [vp, vp]),
    "skr_eval_fused_topk": (i32, [vp, vp, i32, vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, sz, vp]),
    "skr_mask_train": (i32, [vp, i32, i32, i64, vp, vp, vp, vp]),
    "skr_score_matrix": (i32, [vp, vp, i32, vp, vp, i32, i32, vp, i64, vp]),
    "skr_rank_metrics": (i32, [vp, i32, i32, vp, vp, vp, C.POINTER(i32), i32, vp, vp, vp]),
    "skr_bpr_step": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "skr_bpr_step_sharded": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, vp]),
    "skr_bpr_step_spread": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "skr_bpr_step_dim": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp, i32, vp, vp, f32, vp]),
    "skr_csr_spmm_strided": (i32, [i32, vp, vp, vp, vp, i32, i32, i64, vp, vp, vp, f32, vp]),
    "skr_adam_step": (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, i64, i32, vp, vp]),
    "skr_csr_spmm": (i32, [i32, vp, vp, vp, vp, i32, i64, vp, vp, vp, f32, vp]),
    "skr_spmm_plan_create": (i32, [i32, i32, vp, vp, vp, i64, i32, C.POINTER(vp), vp]),
    "skr_spmm_plan_run": (i32, [vp, vp, i32, vp, vp, vp, f32, vp]),
    "skr_spmm_plan_run_masked": (i32, [vp, vp, i32, vp, vp, vp, f32, vp, vp, vp]),
    "skr_spmm_plan_run_ex": (i32, [vp, vp, i32, vp, vp, vp, vp]),
    "skr_clear_marked_rows": (i32, [vp, i64, i64, vp, i32, vp]),
    "skr_layer_refine_bwd_masked": (i32, [vp, vp, vp, vp, i64, i32, vp, vp, vp, i32, vp]),
    "skr_mark_ids": (i32, [vp, i64, i64, vp, vp]),
    "skr_csr_scatter_marked_rows": (i32, [i32, vp, vp, vp, vp, vp, i32, vp, vp]),
    "skr_spmm_plan_info": (i32, [vp, C.POINTER(i64)]),
    "skr_spmm_plan_destroy": (i32, [vp]),
    "skr_layer_refine_fwd": (i32, [vp, vp, i64, i32, vp, vp, vp, vp]),
    "skr_layer_refine_bwd": (i32, [vp, vp, vp, vp, i64, i32, vp, vp, vp]),
    "skr_gather_rows": (i32, [vp, vp, i64, i32, vp, vp]),
    "skr_scatter_rows": (i32, [vp, vp, i64, i32, vp, vp]),
    "skr_sum_blocks": (i32, [vp, i32, i64, vp, vp]),
    "skr_axpy": (i32, [f32, vp, vp, i64, vp]),
    "skr_scale_copy": (i32, [f32, vp, vp, i64, vp]),
    "skr_scale": (i32, [f32, vp, i64, vp]),
    "skr_fpmc_step": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, i32, vp]),
    "skr_transrec_step": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp, i32, vp]),
    "skr_seq_scores": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, vp, i64, vp]),
    "skr_hgn_step": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32,
                           vp]),
    "skr_hgn_queries": (i32, [vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp, vp]),
    "skr_multvae_workspace": (sz, [i32, i32]),
    "skr_multvae_step": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, vp, vp, u64, u64, vp, vp, vp, vp, vp, sz,
                               vp, vp]),
    "skr_multvae_step_timed": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, vp, vp, u64, u64, vp, vp, vp, vp, vp,
                                     sz, vp, vp, vp]),
    "skr_multvae_queries": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "skr_multvae_draws": (i32, [vp, vp, vp, i32, i32, i32, f32, u64, u64, vp, vp, vp, vp]),
    "skr_cdae_workspace": (sz, [i32, i64]),
    "skr_cdae_step": (i32, [vp] * 14 + [i32, i64, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, sz, vp, vp]),
    "skr_cdae_step_timed": (i32, [vp] * 14 + [i32, i64, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp]),
    "skr_cdae_queries": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
    "skr_cdae_draws": (i32, [vp, vp, vp, vp, i64, i32, f32, u64, u64, vp, vp]),
    "skr_lightgcl_cl_workspace": (sz, [i32, i32]),
    "skr_lightgcl_cl": (i32, [vp, i32, vp, i32, f32, f32, vp, vp, vp, vp, sz, vp]),
    "skr_lightgcl_workspace": (sz, [i32, i32, i32]),
    "skr_lightgcl_step": (i32, [vp, vp]),
    "skr_lightgcl_step_timed": (i32, [vp, vp, vp]),
    "skr_dens_workspace": (sz, [i32, i32]),
    "skr_dens_step": (i32, [vp, vp]),
    "skr_dens_step_timed": (i32, [vp, vp, vp]),
    "skr_spmm_plan_run_dropped": (i32, [vp, vp, i32, vp, vp, f32, vp]),
    "skr_selfcf_keeps": (i32, [vp, i64, vp, vp, f32, u64, u64, vp, vp, vp, vp, vp]),
    "skr_selfcf_workspace": (sz, [i32, i32]),
    "skr_selfcf_step": (i32, [vp, vp]),
    "skr_selfcf_step_timed": (i32, [vp, vp, vp]),
    "skr_selfcf_queries": (i32, [vp, vp, i32, i32, vp, vp, vp, vp]),
    "skr_bm3_project": (i32, [vp, i32, i32, i32, vp, vp, i32, vp, vp]),
    "skr_bm3_draws": (i32, [vp, i32, i32, f32, u64, u64, vp, vp]),
    "skr_bm3_workspace": (sz, [i32]),
    "skr_bm3_step": (i32, [vp, vp]),
    "skr_bm3_step_timed": (i32, [vp, vp, vp]),
    "skr_bm3_queries": (i32, [vp, vp, i32, i32, vp, vp, vp]),
    "skr_knn_workspace": (sz, [i32, i32]),
    "skr_knn_topk": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
    "skr_freedom_keys": (i32, [vp, i64, u64, u64, vp, vp]),
    "skr_freedom_select_workspace": (sz, [i64]),
    "skr_freedom_select": (i32, [vp, i64, i64, vp, vp, sz, vp]),
    "skr_freedom_pruned_workspace": (sz, [i32, i32, i64]),
    "skr_freedom_pruned_csr": (i32, [i32, i32, i64] + [vp] * 14 + [sz, vp]),
    "skr_freedom_workspace": (sz, [i32]),
    "skr_freedom_step": (i32, [vp, vp]),
    "skr_freedom_step_timed": (i32, [vp, vp, vp]),
    "skr_mgcn_project": (i32, [vp, i32, i32, i32, vp, vp, vp]),
    "skr_mgcn_row_block": (i32, [i32]),
    "skr_mgcn_project_bwd_workspace": (sz, [i32, i32]),
    "skr_mgcn_project_bwd": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    "skr_mgcn_purify": (i32, [vp, vp, vp, i32, i32, vp, vp, vp]),
    "skr_mgcn_purify_bwd_workspace": (sz, [i32]),
    "skr_mgcn_purify_bwd": (i32, [vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, sz, vp]),
    "skr_mgcn_fuse": (i32, [vp, vp, vp, vp, vp, vp, i64, i32, vp, vp, vp]),
    "skr_mgcn_workspace": (sz, [i32, i32, i32]),
    "skr_mgcn_step": (i32, [vp, vp]),
    "skr_mgcn_step_timed": (i32, [vp, vp, vp]),
    "skr_lattice_graph_workspace": (sz, [i32]),
    "skr_lattice_graph": (i32, [i32, i32, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "skr_lattice_sddmm": (i32, [i32, i32, vp, vp, vp, i64, vp, i64, i32, vp, i32, vp, vp]),
    "skr_lattice_graph_bwd_workspace": (sz, [i32, i64]),
    "skr_lattice_graph_bwd": (i32, [i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp, sz, vp]),
    "skr_lattice_add_normalized": (i32, [vp, i64, vp, vp]),
    "skr_lattice_workspace": (sz, [i32, i32]),
    "skr_lattice_step": (i32, [vp, vp]),
    "skr_lattice_step_timed": (i32, [vp, vp, vp]),
    "skr_slmrec_project_bwd_w": (i32, [vp, vp, i32, i32, i32, vp, vp, sz, vp]),
    "skr_slmrec_fuse": (i32, [vp, vp, vp, vp, i64, i32, vp, vp]),
    "skr_slmrec_workspace": (sz, [i32, i32, i32]),
    "skr_slmrec_step": (i32, [vp, vp]),
    "skr_slmrec_step_timed": (i32, [vp, vp, vp]),
    "skr_caser_workspace": (sz, [i32, i32, i32, i32]),
    "skr_caser_step": (i32, [vp] * 9 + [i32] * 10 + [f32, vp, vp, u64, u64, vp, vp, vp, vp, vp, vp, sz, vp, i32, vp]),
    "skr_caser_step_timed": (i32, [vp] * 9 + [i32] * 10 + [f32, vp, vp, u64, u64, vp, vp, vp, vp, vp, vp, sz, vp, i32, vp, vp]),
    "skr_caser_queries": (i32, [vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp, vp]),
    "skr_sasrec_workspace": (i64, [i32, i32, i32, i32]),
    "skr_sasrec_step": (i32, [vp] * 6 + [i32] * 6 + [f32, vp, vp, u64, u64, vp, vp, vp, vp, sz, vp, i32, vp]),
    "skr_sasrec_step_timed": (i32, [vp] * 6 + [i32] * 6 + [f32, vp, vp, u64, u64, vp, vp, vp, vp, sz, vp, i32, vp, vp]),
    "skr_sasrec_queries": (i32, [vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
}


class SpmmEpilogue(C.Structure):
    """skr_spmm_epilogue (include/skrec_hip.h): what happens to a finished row of a propagation"""
    _fields_ = [("mode", C.c_int32), ("accum_init", C.c_int32), ("addend", vp), ("Y", vp), ("accum", vp), ("accum_base", vp),
                ("accum_scale", C.c_float), ("ld", C.c_int32), ("E", vp), ("w", vp), ("Z", vp), ("rawY", vp), ("dE", vp), ("accum_mask", vp), ("addend_mask", vp)]


EPI_PLAIN, EPI_REFINE_FWD, EPI_REFINE_BWD = 0, 1, 2


class LightGCLStepArgs(C.Structure):
    """skr_lightgcl_step_args (include/skrec_hip.h): the tables, the batch and the scratch of one LightGCL step"""
    _fields_ = [("plan_a", vp), ("plan_at", vp), ("n_users", C.c_int32), ("n_items", C.c_int32), ("dim", C.c_int32),
                ("n_layers", C.c_int32), ("q", C.c_int32), ("n", C.c_int32), ("E0", vp), ("fac_us", vp), ("fac_vs", vp),
                ("fac_ut", vp), ("fac_vt", vp), ("uids", vp), ("pos", vp), ("neg", vp), ("inv_temp", C.c_float),
                ("lambda1", C.c_float), ("lambda2", C.c_float), ("sum", vp), ("below", vp), ("ping", vp * 2), ("gsum", vp),
                ("addend", vp), ("grad", vp), ("loss", vp), ("work", vp), ("work_bytes", C.c_size_t)]


class DensStepArgs(C.Structure):
    """skr_dens_step_args (include/skrec_hip.h): the parameters, the batch, the hop tables and the scratch of one DENS step"""
    _fields_ = [("plan_a", vp), ("plan_at", vp), ("n_users", C.c_int32), ("n_items", C.c_int32), ("dim", C.c_int32),
                ("n_hops", C.c_int32), ("n_negs", C.c_int32), ("n", C.c_int32), ("params", vp), ("uids", vp), ("pos", vp),
                ("cand", vp), ("sel_in", vp), ("sel_out", vp), ("w", C.c_float), ("gamma", C.c_float), ("l2", C.c_float),
                ("hop", vp * 3), ("G", vp * 4), ("ping", vp), ("grad", vp), ("loss", vp), ("work", vp), ("work_bytes", C.c_size_t)]


class SelfCFStepArgs(C.Structure):
    """skr_selfcf_step_args (include/skrec_hip.h): the parameters, the batch, the keep flags and the scratch of one SelfCF step"""
    _fields_ = [("plan_a", vp), ("plan_at", vp), ("n_users", C.c_int32), ("n_items", C.c_int32), ("dim", C.c_int32),
                ("n_layers", C.c_int32), ("n", C.c_int32), ("params", vp), ("users", vp), ("items", vp), ("keep_fu", vp),
                ("keep_fi", vp), ("keep_bu", vp), ("keep_bi", vp), ("edge_scale", C.c_float), ("ku", vp), ("ki", vp),
                ("dropout", C.c_float), ("reg", C.c_float), ("seed", C.c_uint64), ("step", C.c_uint64), ("M", vp), ("ping", vp * 2),
                ("G", vp), ("grad", vp), ("loss", vp), ("work", vp), ("work_bytes", C.c_size_t)]


class BM3StepArgs(C.Structure):
    """skr_bm3_step_args (include/skrec_hip.h): the parameters, the feature blocks (image, text), the batch, the keep flags and
    the scratch of one BM3 step"""
    _fields_ = [("plan_a", vp), ("plan_at", vp), ("n_users", C.c_int32), ("n_items", C.c_int32), ("dim", C.c_int32),
                ("n_layers", C.c_int32), ("n", C.c_int32), ("feat_dim", C.c_int32 * 2), ("feat_ld", C.c_int32 * 2), ("params", vp),
                ("trs", vp * 2), ("feat", vp * 2), ("users", vp), ("items", vp), ("clear_items", vp), ("n_clear", C.c_int32),
                ("keep", vp * 4), ("dropout", C.c_float), ("reg", C.c_float), ("cl_weight", C.c_float), ("seed", C.c_uint64),
                ("step", C.c_uint64), ("M", vp), ("ping", vp * 2), ("G", vp), ("grad", vp), ("trs_grad", vp * 2), ("feat_grad", vp * 2),
                ("loss", vp), ("work", vp), ("work_bytes", C.c_size_t)]


class FreedomStepArgs(C.Structure):
    """skr_freedom_step_args (include/skrec_hip.h): the plans of both graphs, the parameters, the feature blocks (image, text),
    the batch and the scratch of one FREEDOM step"""
    _fields_ = [("plan_a", vp), ("plan_at", vp), ("plan_s", vp), ("plan_st", vp), ("n_users", C.c_int32), ("n_items", C.c_int32),
                ("dim", C.c_int32), ("n_ui_layers", C.c_int32), ("n_mm_layers", C.c_int32), ("n", C.c_int32),
                ("feat_dim", C.c_int32 * 2), ("feat_ld", C.c_int32 * 2), ("params", vp), ("trs", vp * 2), ("feat", vp * 2),
                ("users", vp), ("pos", vp), ("neg", vp), ("clear_items", vp), ("n_clear", C.c_int32), ("reg", C.c_float), ("M", vp),
                ("ping", vp * 2), ("G", vp), ("grad", vp), ("trs_grad", vp * 2), ("feat_grad", vp * 2), ("loss", vp), ("work", vp),
                ("work_bytes", C.c_size_t)]


class MGCNStepArgs(C.Structure):
    """skr_mgcn_step_args (include/skrec_hip.h): the plans of the three graphs, the parameter blocks, the batch, the forward's
    tables and the scratch of one MGCN step"""
    _fields_ = [("plan_a", vp), ("plan_at", vp), ("plan_s", vp * 2), ("plan_st", vp * 2), ("n_users", C.c_int32), ("n_items", C.c_int32),
                ("dim", C.c_int32), ("n_ui_layers", C.c_int32), ("n_layers", C.c_int32), ("n", C.c_int32), ("feat_dim", C.c_int32 * 2),
                ("feat_ld", C.c_int32 * 2), ("params", vp), ("trs", vp * 2), ("feat", vp * 2), ("gate", vp * 2), ("query", vp),
                ("prefer", vp * 2), ("users", vp), ("pos", vp), ("neg", vp), ("reg", C.c_float), ("cl_loss", C.c_float), ("F", vp * 2),
                ("gate_out", vp * 2), ("Z", vp * 2), ("M", vp), ("G", vp * 3), ("ping", vp * 2), ("grad", vp), ("trs_grad", vp * 2),
                ("feat_grad", vp * 2), ("gate_grad", vp * 2), ("query_grad", vp), ("prefer_grad", vp * 2), ("loss", vp), ("work", vp),
                ("work_bytes", C.c_size_t)]


class LatticeStepArgs(C.Structure):
    """skr_lattice_step_args (include/skrec_hip.h): the plans of the square adjacency and of the item graph, the parameters, the
    batch, the layer tables and the scratch of one LATTICE step"""
    _fields_ = [("plan_p", vp), ("plan_pt", vp), ("plan_s", vp), ("plan_st", vp), ("n_users", C.c_int32), ("n_items", C.c_int32),
                ("dim", C.c_int32), ("n_ui_layers", C.c_int32), ("n_layers", C.c_int32), ("cf_model", C.c_int32), ("n", C.c_int32),
                ("reg", C.c_float), ("params", vp), ("users", vp), ("pos", vp), ("neg", vp), ("M", vp), ("ping", vp * 2), ("G", vp),
                ("DH", vp), ("H", vp), ("grad", vp), ("g_out", vp), ("s_rowptr", vp), ("s_col", vp), ("loss", vp), ("work", vp),
                ("work_bytes", C.c_size_t)]


class SLMRecStepArgs(C.Structure):
    """skr_slmrec_step_args (include/skrec_hip.h): the plans of the user-item graph, the parameter blocks, the constant feature
    tables, the batch, the forward's tables and the scratch of one SLMRec step"""
    _fields_ = [("plan_a", vp), ("plan_at", vp), ("n_users", C.c_int32), ("n_items", C.c_int32), ("dim", C.c_int32), ("n_layers", C.c_int32),
                ("n", C.c_int32), ("feat_dim", C.c_int32 * 2), ("feat_ld", C.c_int32 * 2), ("temp", C.c_float), ("ssl_temp", C.c_float),
                ("ssl_alpha", C.c_float), ("params", vp), ("dense", vp * 2), ("feat", vp * 2), ("fusion_user", vp), ("fusion_item", vp),
                ("chain", vp * 5), ("users", vp), ("pos", vp), ("D", vp * 2), ("M", vp * 3), ("G", vp * 3), ("ping", vp * 2), ("dD", vp),
                ("grad", vp), ("dense_grad", vp * 2), ("fusion_user_grad", vp), ("fusion_item_grad", vp), ("chain_grad", vp * 5),
                ("loss", vp), ("work", vp), ("work_bytes", C.c_size_t)]


SKR_MAX_TOPK = 128            # skr_eval_fused_topk
SKR_MAX_TOPK_SCORES = 512     # skr_eval_scores, skr_rank_metrics
SKR_LOSS_SLOTS = 32      # skr_bpr_step_spread: pairs of loss words per batch
SKR_TRANSREC_MAX_BLOCKS = 1024   # skr_transrec_step: d_work holds this many rows of dim floats
SKR_SEQ_FPMC, SKR_SEQ_TRANSREC = 0, 1     # skr_seq_scores modes
SKR_HGN_MAX_L, SKR_HGN_MAX_T, SKR_HGN_MAX_BLOCKS = 32, 16, 256   # skr_hgn_step limits; d_work holds MAX_BLOCKS partials
SKR_MULTVAE_MAX_BATCH = 1024   # skr_multvae_step: users of a batch
SKR_CDAE_MAX_BATCH = 1024      # skr_cdae_step: users of a batch
SKR_CDAE_IDENTITY, SKR_CDAE_SIGMOID, SKR_CDAE_LAUNCHES = 0, 1, 3
SKR_LIGHTGCL_MAX_QUERIES, SKR_LIGHTGCL_MAX_Q, SKR_LIGHTGCL_GROUPS = 4096, 16, 8   # skr_lightgcl_cl / _step limits
SKR_DENS_MAX_BATCH, SKR_DENS_MAX_NEGS, SKR_DENS_MAX_HOPS, SKR_DENS_GROUPS = 2048, 16, 3, 6   # skr_dens_step limits
SKR_SELFCF_MAX_BATCH, SKR_SELFCF_MAX_LAYERS, SKR_SELFCF_GROUPS = 2048, 4, 4   # skr_selfcf_step limits
SKR_SELFCF_PRED_FLOATS = 64 * 64 + 64    # the predictor's block of the flat parameter buffer: W [64 out][64 in], then b [64]
SKR_BM3_MAX_BATCH, SKR_BM3_MAX_LAYERS, SKR_BM3_MAX_FEAT, SKR_BM3_GROUPS = 2048, 4, 4096, 7   # skr_bm3_step limits
SKR_BM3_PRED_FLOATS = 64 * 64 + 64       # the predictor's block of BM3's parameter buffer
SKR_BM3_DRAW_USER, SKR_BM3_DRAW_ITEM, SKR_BM3_DRAW_TEXT, SKR_BM3_DRAW_IMAGE = 0, 1, 2, 3   # the tables of the target draws
SKR_FREEDOM_MAX_BATCH, SKR_FREEDOM_MAX_LAYERS, SKR_FREEDOM_MAX_FEAT, SKR_FREEDOM_GROUPS = 2048, 4, 4096, 7   # skr_freedom_step limits
SKR_FREEDOM_MAX_NNZ = 2 ** 31 - 1         # skr_freedom_keys / _select / _pruned_csr: entries of the train matrix
SKR_KNN_MAX_K = 32                       # skr_knn_topk: neighbours per row
SKR_MGCN_MAX_BATCH, SKR_MGCN_MAX_LAYERS, SKR_MGCN_MAX_FEAT, SKR_MGCN_GROUPS = 2048, 4, 4096, 8   # skr_mgcn_step limits
SKR_MGCN_GATE_FLOATS, SKR_MGCN_QUERY_FLOATS = 64 * 64 + 64, 64 * 64 + 64 + 64   # a gate block; query_common's W | b | q
SKR_LATTICE_MAX_BATCH, SKR_LATTICE_MAX_LAYERS, SKR_LATTICE_GROUPS = 2048, 4, 7   # skr_lattice_step limits
SKR_LATTICE_CF_LIGHTGCN, SKR_LATTICE_CF_MF = 0, 1                               # skr_lattice_step_args.cf_model
SKR_SLMREC_MAX_BATCH, SKR_SLMREC_MAX_LAYERS, SKR_SLMREC_MAX_FEAT, SKR_SLMREC_GROUPS = 2048, 4, 4096, 8   # skr_slmrec_step limits
SKR_SLMREC_GATE_FLOATS, SKR_SLMREC_FUSION_FLOATS = 64 * 64 + 64, 64 * 192 + 64   # a chain layer's block; a fusion layer's W [64][192] | b
SKR_DENS_GATE_FLOATS = 64 * 64 + 64     # one gate block of the flat parameter buffer: W [64 out][64 in], then b [64]
SKR_CASER_MAX_L, SKR_CASER_MAX_T, SKR_CASER_MAX_NV, SKR_CASER_MAX_NH, SKR_CASER_MAX_BATCH = 8, 16, 8, 32, 2048   # skr_caser_step limits
SKR_CASER_LAUNCHES = 10                  # skr_caser_step_timed: launch groups
SKR_SASREC_MAX_HIDDEN, SKR_SASREC_MAX_LEN, SKR_SASREC_MAX_BLOCKS, SKR_SASREC_MAX_HEADS, SKR_SASREC_MAX_BATCH = 64, 64, 4, 8, 2048
SKR_SASREC_BLOCK_ROWS, SKR_SASREC_LAUNCHES = 329, 6   # rows of 64 floats per block of the shared parameters; launch groups


def sasrec_shared_floats(blocks):
    """SKR_SASREC_SHARED_FLOATS(blocks): floats of SASRec's shared parameters (include/skrec_hip.h names the rows)"""
    return 64 * (SKR_SASREC_BLOCK_ROWS * int(blocks) + 2)


def sasrec_keep_bytes(hidden, max_len, blocks, heads):
    """SKR_SASREC_KEEP_BYTES: keep flags per sequence -- input | per block: attention [heads][T][T] | ffn 1 | ffn 2"""
    d, T = int(hidden), int(max_len)
    return T * d + int(blocks) * (int(heads) * T * T + 2 * T * d)


def hgn_gate_floats(L):
    """SKR_HGN_GATE_FLOATS(L): floats of HGN's shared gate parameters (and of one partial of their gradient)"""
    return 2 * 64 * 64 + 3 * 64 + 64 * int(L)


def caser_rows(L, nh):
    """SKR_CASER_ROWS(L, nh): 64-float rows of Caser's horizontal filters, ordered (h, k, r)"""
    return int(nh) * int(L) * (int(L) + 1) // 2


def caser_fp(L, nv, nh):
    """SKR_CASER_FP(L, nv, nh): the row stride of Caser's fc1.weight, its nv 64 + nh L columns rounded up to 64"""
    return 64 * ((int(nv) * 64 + int(nh) * int(L) + 63) // 64)


def caser_shared_floats(L, nv, nh):
    """SKR_CASER_SHARED_FLOATS(L, nv, nh): floats of Caser's shared parameters (include/skrec_hip.h names the parts)"""
    return 128 + 64 * caser_rows(L, nh) + 64 * ((int(L) * int(nh) + 63) // 64) + 64 * caser_fp(L, nv, nh) + 64


class HipError(RuntimeError):
    pass


_lib = None


def build(force=False):
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    import subprocess
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-C", CSRC_DIR, "-j4"], check=True)
    return LIB_PATH


def lib():
    """Load the shared library (no GPU needed for loading / symbol checks)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           f"(there is no CPU fallback for the hot path)")
        # torch first: it ships its own libamdhip64; if this library pulled in /opt/rocm's copy before torch
        # loaded, the process would hold two HIP runtimes and torch.cuda would report no device afterwards
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here = the .so and the header disagree
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().skr_last_error()
        raise (ValueError if rc == -1 else HipError)(msg.decode() if msg else f"libskrec_hip error {rc}")


def require_gpu():
    import torch
    if not torch.cuda.is_available() or lib().skr_device_count() == 0:
        raise HipError("no MI355X / HIP device is visible: the skrec hot path runs on the GPU only")
    return torch.device("cuda", torch.cuda.current_device())


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """device (or host) address of a torch tensor / numpy array / None"""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    assert t.is_contiguous(), "tensor must be contiguous"
    return t.data_ptr()


def score_matrix(user_table, users, item_table, bias):
    """predict() helper: dense [len(users), n_items] fp32 scores on the device (skr_score_matrix)"""
    import torch
    dev = user_table.device
    du = torch.as_tensor(np.asarray(users, dtype=np.int32)).to(dev)
    n_items = int(item_table.shape[0])
    out = torch.empty((du.numel(), n_items), dtype=torch.float32, device=dev)
    check(lib().skr_score_matrix(ptr(user_table), ptr(du), du.numel(), ptr(item_table), ptr(bias), n_items,
                                 int(item_table.shape[1]), ptr(out), n_items, stream()))
    return out


def host_permutation(n):
    """np.random.permutation(n) of numpy's GLOBAL legacy generator, as int32, computed natively (skr_host_permutation):
    same values, same generator state afterwards; the GIL is released while it runs"""
    kind, key, pos, has_gauss, cached = np.random.get_state()
    if kind != "MT19937":
        return np.random.permutation(n).astype(np.int32)
    key = np.ascontiguousarray(key, dtype=np.uint32).copy()
    cpos = i32(int(pos))
    out = np.empty(int(n), dtype=np.int32)
    check(lib().skr_host_permutation(key.ctypes.data, C.byref(cpos), int(n), out.ctypes.data))
    np.random.set_state((kind, key, int(cpos.value), has_gauss, cached))
    return out


def shuffle_gather(columns, perm=None, seed=0, n_out=None):
    """One launch for all columns (skr_shuffle_gather): row r of every result = row perm[r] of the column, or row
    pi_seed(r) when ``perm`` is None.  ``columns``: contiguous 4-byte-element device tensors [n] or [n, w]."""
    import torch
    n = int(columns[0].shape[0])
    n_out = n if n_out is None else int(n_out)
    if perm is not None:      # the kernel reads int32 indices and trusts them
        assert perm.dtype == torch.int32 and perm.is_contiguous() and perm.numel() >= n_out, \
            "shuffle_gather: perm must be a contiguous int32 tensor with at least n_out entries"
    outs = []
    for s in range(0, len(columns), 4):
        cols = columns[s:s + 4]
        for c in cols:
            assert c.is_contiguous() and c.element_size() == 4 and c.shape[0] == n
        res = [torch.empty((n_out,) + tuple(c.shape[1:]), dtype=c.dtype, device=c.device) for c in cols]
        k = len(cols)
        check(lib().skr_shuffle_gather(ptr(perm), int(seed), n, n_out, k, (vp * k)(*[c.data_ptr() for c in cols]),
                                       (i32 * k)(*[max(1, c.numel() // max(n, 1)) for c in cols]),
                                       (vp * k)(*[r.data_ptr() for r in res]), stream()))
        outs.extend(res)
    return outs


def metric_array(ids):
    return (i32 * len(ids))(*[int(x) for x in ids])
