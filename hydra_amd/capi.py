"""ctypes binding of the C ABI in include/hgibbs.h (libhgibbs.so, HIP/gfx950).

This is plumbing only: every compute entry point lives in the shared library.
There is no CPU fallback -- if the library is missing or no gfx950 device is
visible the calls raise.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhgibbs.so")

# every symbol include/hgibbs.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "hgibbs_last_error", "hgibbs_version", "hgibbs_create", "hgibbs_destroy", "hgibbs_comm_unique_id",
    "hgibbs_comm_init", "hgibbs_comm_init_external", "hgibbs_p2p_export", "hgibbs_p2p_import", "hgibbs_load_bed", "hgibbs_synth_bed", "hgibbs_dims", "hgibbs_get_bed",
    "hgibbs_marker_stats", "hgibbs_set_residual", "hgibbs_get_residual", "hgibbs_reduce_eps", "hgibbs_add_scalar",
    "hgibbs_update_marker", "hgibbs_dot_marker", "hgibbs_set_covariates", "hgibbs_cov_dot", "hgibbs_cov_update",
    "hydra_chain_set_covariates", "hydra_chain_gamma", "hgibbs_set_components", "hydra_chain_restore",
    "hydra_rng_to_boost_words", "hydra_rng_from_boost_words", "hydra_rng_shuffle", "hgibbs_set_model", "hgibbs_set_beta", "hgibbs_get_beta",
    "hgibbs_beta_sqnorm", "hgibbs_sweep", "hgibbs_set_option", "hgibbs_walker_search", "hgibbs_last_sweep_stats", "hgibbs_stream_ceiling", "hgibbs_debug_times", "hgibbs_resident_trace", "hydra_chain_create",
    "hydra_chain_destroy", "hydra_chain_iterate", "hydra_chain_state", "hydra_chain_csv_line", "hydra_chain_order",
    "hydra_chain_last_nnz", "hgibbs_score", "hgibbs_last_score_ms", "hgibbs_ld", "hgibbs_last_ld_ms",
    "hgibbs_ld_scores", "hgibbs_last_ld_scores_ms",
    "hgibbs_ld_mask", "hgibbs_last_ld_mask_ms", "hgibbs_ld_greedy", "hgibbs_ld_clump",
    "hgibbs_ss_begin", "hgibbs_ss_sweep", "hgibbs_ss_state", "hgibbs_ss_band_get", "hgibbs_ss_end", "hgibbs_last_ss_ms", "hgibbs_ss_sweep_host",
    "hgibbs_ss_partition", "hgibbs_ss_sweep_streams", "hgibbs_ss_sweep_streams_host", "hydra_ss_chain_set_streams", "hydra_ss_chain_streams",
    "hydra_ss_chain_create", "hydra_ss_chain_create_host", "hydra_ss_chain_destroy", "hydra_ss_chain_iterate", "hydra_ss_chain_state",
    "hydra_ss_chain_effects", "hydra_ss_chain_last_nnz", "hydra_ss_chain_order", "hydra_ss_chain_csv_line",
    "hgibbs_ss_replicas", "hgibbs_ss_sweep_replicas", "hgibbs_ss_replica_sums", "hgibbs_ss_replica_get", "hgibbs_ss_replica_set_beta", "hgibbs_mcmc_diag",
    "hgibbs_ss_post_begin", "hgibbs_ss_post_add", "hgibbs_ss_post_get", "hgibbs_ss_post_raw", "hgibbs_ss_post_end", "hgibbs_last_ss_post_ms",
    "hgibbs_cs_begin", "hgibbs_cs_add_flags", "hgibbs_ss_cs_add", "hgibbs_cs_counts", "hgibbs_cs_history", "hgibbs_cs_sets", "hgibbs_cs_end", "hgibbs_last_cs_ms",
    "hgibbs_cs_select",
    "hydra_ss_multi_create", "hydra_ss_multi_destroy", "hydra_ss_multi_iterate", "hydra_ss_multi_state", "hydra_ss_multi_effects", "hydra_ss_multi_streams",
    "hydra_ss_multi_last_nnz", "hydra_ss_multi_csv_line",
    "hgibbs_marker_dots", "hgibbs_last_marker_dots_ms", "hgibbs_marker_class_sums", "hgibbs_last_marker_class_sums_ms", "hgibbs_logit_null",
    "hgibbs_set_gram", "hgibbs_last_set_gram_ms", "hgibbs_set_tests",
    "hgibbs_spa_roots", "hgibbs_last_spa_ms", "hgibbs_spa_pvalue",
    "hgibbs_firth_fit", "hgibbs_last_firth_ms", "hgibbs_firth_stats",
    "hgibbs_king", "hgibbs_king_pairs", "hgibbs_king_pairs_get", "hgibbs_last_king_ms",
    "hgibbs_roh", "hgibbs_roh_get", "hgibbs_last_roh_ms",
    "hgibbs_pair_tables", "hgibbs_last_pair_tables_ms", "hgibbs_epi_scan", "hgibbs_epi_scan_get", "hgibbs_last_epi_ms", "hgibbs_epi_test",
    "hgibbs_pca", "hgibbs_last_pca_ms", "hgibbs_region_var", "hgibbs_last_region_var_ms",
    "hgibbs_grm", "hgibbs_grm_info", "hgibbs_last_grm_ms",
    "hgibbs_grm_rowsums", "hgibbs_last_grm_rowsums_ms", "hgibbs_he_fit",
    "hgibbs_reml_solve", "hgibbs_reml_eval", "hgibbs_reml", "hgibbs_reml_next", "hgibbs_reml_finish", "hgibbs_last_reml_ms",
    "hgibbs_row_sums", "hgibbs_last_row_sums_ms", "hgibbs_hwe_exact",
    "hgibbs_sparse_begin", "hgibbs_sparse_put", "hgibbs_sparse_end", "hgibbs_sparse_counts", "hgibbs_sparse_get", "hgibbs_last_sparse_ms",
    # BayesW
    "hgibbs_grand_seed", "hgibbs_grand_next", "hgibbs_ars_sample", "hgibbs_w_init", "hgibbs_w_marker_stats", "hgibbs_w_set_model",
    "hgibbs_w_reduce", "hgibbs_w_refresh_vi", "hgibbs_w_get_vi", "hgibbs_w_marker_sums", "hgibbs_w_sweep", "hgibbs_w_last_sweep_stats", "hgibbs_w_ars_device_probe",
    "hgibbs_w_get_beta", "hgibbs_w_set_beta", "hydraw_chain_create", "hydraw_chain_destroy", "hydraw_chain_set_covariates",
    "hydraw_chain_reseed_ars", "hydraw_chain_iterate", "hydraw_chain_state", "hydraw_chain_gamma", "hydraw_chain_order",
    "hydraw_chain_last_nnz", "hydraw_chain_csv_line", "hydraw_chain_restore",
]


class RngState(C.Structure):
    _fields_ = [("x", C.c_uint32 * 624), ("idx", C.c_uint32)]


class SweepStats(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("nnz_updates", C.c_uint64), ("device_ms", C.c_double),
                ("kernel_ms_avg", C.c_double), ("carried_columns", C.c_uint64), ("working_launches", C.c_uint64),
                ("accepted_markers", C.c_uint64), ("streamed_columns", C.c_uint64), ("tiles_per_workgroup_min", C.c_uint32),
                ("tiles_per_workgroup_max", C.c_uint32), ("engine", C.c_uint32), ("walker", C.c_uint32), ("eps_sum_drift", C.c_double),
                ("rounds", C.c_uint64), ("events", C.c_uint64), ("advances", C.c_uint64), ("chunks", C.c_uint64), ("refolds", C.c_uint64), ("pivots", C.c_uint64), ("predicted", C.c_uint64), ("shader_mhz", C.c_double),
                ("ticks", C.c_uint64 * 16), ("refill", C.c_uint32), ("turned_down", C.c_uint32)]


class PcaReport(C.Structure):
    _fields_ = [("iters_run", C.c_int32), ("m_used", C.c_uint32), ("ritz_change", C.c_double), ("resid", C.c_double * 32)]


class SpaRoot(C.Structure):
    """hgibbs_spa_root: index 0 is the tail at +|s|, index 1 the tail at -|s|"""
    _fields_ = [("t", C.c_double * 2), ("K", C.c_double * 2), ("K2", C.c_double * 2), ("k2_0", C.c_double), ("s_lo", C.c_double),
                ("s_hi", C.c_double), ("iters", C.c_int32 * 2), ("flags", C.c_uint32), ("reserved_", C.c_uint32)]


class SetResult(C.Structure):
    """hgibbs_set_result"""
    _fields_ = [("q", C.c_double), ("p_skat", C.c_double), ("t_burden", C.c_double), ("p_burden", C.c_double), ("lam_sum", C.c_double),
                ("lam_max", C.c_double), ("neig", C.c_int32), ("skat_ok", C.c_int32)]


class FirthRec(C.Structure):
    """hgibbs_firth_rec: flags bit 0 converged, bit 1 degenerate"""
    _fields_ = [("beta", C.c_double), ("K", C.c_double), ("K2", C.c_double), ("g", C.c_double), ("k2_0", C.c_double),
                ("iters", C.c_int32), ("flags", C.c_uint32)]


class EpiResult(C.Structure):
    """hgibbs_epi_result"""
    _fields_ = [("ksa", C.c_double), ("lr", C.c_double), ("df", C.c_int), ("iters", C.c_int), ("converged", C.c_int), ("p", C.c_double)]


class RohParams(C.Structure):
    """hgibbs_roh_params"""
    _fields_ = [("window", C.c_uint32), ("window_het", C.c_uint32), ("window_missing", C.c_uint32), ("need", C.c_uint32 * 65),
                ("min_snps", C.c_uint32), ("min_bp", C.c_int64), ("dens_bp", C.c_int64), ("gap_bp", C.c_int64), ("max_het", C.c_uint32)]


# hgibbs_roh_seg as a numpy record
ROH_SEG = np.dtype([(k, np.uint32) for k in ("row", "first", "last", "nsnp", "nhet", "nmiss")])


def roh_need(threshold, window):
    """need[0 .. 64] of hgibbs_roh_params: need[n] = the smallest integer c with float(c) / float(n) >= threshold, n = 1 .. window"""
    need = [0] * 65
    for n in range(1, int(window) + 1):
        c = 1
        while float(c) / float(n) < threshold:
            c += 1
        need[n] = c
    return need


class HeForm(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("intercept", "slope", "h2", "intercept_se", "slope_se", "h2_se", "intercept_se_jk", "slope_se_jk",
                                         "h2_se_jk", "intercept_p", "slope_p", "intercept_p_jk", "slope_p_jk")]


class HeResult(C.Structure):
    _fields_ = [("n_used", C.c_uint32), ("n_left_out", C.c_uint32), ("pairs", C.c_uint64), ("vp", C.c_double), ("cp", HeForm), ("sd", HeForm)]


class RemlEstimate(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("logdelta", "delta", "vg", "ve", "vp", "h2", "se_vg", "se_ve", "se_vp", "se_h2", "se_mc", "se_logdelta_mc")]


class RemlOpts(C.Structure):
    _fields_ = [("trials", C.c_int), ("h2_start", C.c_double), ("cg_tol", C.c_double), ("cg_iters", C.c_int), ("x_tol", C.c_double),
                ("max_steps", C.c_int), ("seed", C.c_uint64)]


class RemlResult(C.Structure):
    _fields_ = [("status", C.c_int), ("steps", C.c_int), ("x", C.c_double * 32), ("f", C.c_double * 32), ("cg_iters", C.c_int * 32),
                ("sums_prev", C.c_double * 96), ("sums_last", C.c_double * 96), ("ai3", C.c_double * 3), ("ai_cg_iters", C.c_int),
                ("est", RemlEstimate), ("n", C.c_uint32), ("m_used", C.c_uint32), ("q", C.c_int), ("trials", C.c_int),
                ("products_ms", C.c_double), ("algebra_ms", C.c_double)]


REML_CONTINUE, REML_CONVERGED, REML_AT_BOUND = 0, 1, 2
REML_STATUS = {REML_CONTINUE: "CONTINUE", REML_CONVERGED: "CONVERGED", REML_AT_BOUND: "AT_BOUND"}


class SparseList(C.Structure):
    _fields_ = [("start", C.POINTER(C.c_uint64)), ("len", C.POINTER(C.c_uint64)), ("idx", C.POINTER(C.c_uint32)),
                ("idx_base", C.c_uint64), ("idx_count", C.c_uint64)]


class RestartState(C.Structure):
    _fields_ = [("iteration", C.c_uint32), ("sigmaE", C.c_double), ("mu", C.c_double),
                ("sigmaG", C.POINTER(C.c_double)), ("estPi", C.POINTER(C.c_double)), ("beta", C.POINTER(C.c_double)),
                ("components", C.POINTER(C.c_int32)), ("eps", C.POINTER(C.c_double)), ("order", C.POINTER(C.c_int32)),
                ("gamma", C.POINTER(C.c_double)), ("xI", C.POINTER(C.c_int32)), ("rng", RngState)]


class GrandState(C.Structure):
    _fields_ = [("r", C.c_int32 * 31), ("f", C.c_int32), ("b", C.c_int32)]


class WSweepStats(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("nnz_updates", C.c_uint64), ("ars_draws", C.c_uint64), ("ars_evals", C.c_uint64),
                ("device_ms", C.c_double), ("sums_kernel_ms", C.c_double)]


class WModelDesc(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("shuffle", C.c_int32), ("G", C.c_int32), ("K", C.c_int32),
                ("groups", C.POINTER(C.c_int32)), ("mS", C.POINTER(C.c_double)), ("quad_points", C.c_int32)]


class WRestartState(C.Structure):
    _fields_ = [("iteration", C.c_uint32), ("mu", C.c_double), ("alpha", C.c_double), ("sigmaG", C.POINTER(C.c_double)),
                ("pi", C.POINTER(C.c_double)), ("beta", C.POINTER(C.c_double)), ("components", C.POINTER(C.c_int32)),
                ("eps", C.POINTER(C.c_double)), ("order", C.POINTER(C.c_int32)), ("gamma", C.POINTER(C.c_double)),
                ("xI", C.POINTER(C.c_int32)), ("rng", RngState), ("ars_seed", C.c_uint32)]


LOGDENS_FN = C.CFUNCTYPE(C.c_double, C.c_double, C.c_void_p)


class ModelDesc(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("shuffle", C.c_int32), ("G", C.c_int32), ("K", C.c_int32),
                ("groups", C.POINTER(C.c_int32)), ("mS", C.POINTER(C.c_double))]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int)


C_U32P = C.POINTER(C.c_uint32)
C_U64P = C.POINTER(C.c_uint64)


class HgError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("HGIBBS_LIB", LIB_PATH)  # A/B runs of two builds of the same ABI
    if not os.path.exists(path):
        raise HgError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(there is no CPU fallback)" % path)
    L = C.CDLL(path)
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    u8p, u64p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.hgibbs_last_error.restype = C.c_char_p
    L.hgibbs_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.hgibbs_destroy.argtypes = [vp]
    L.hgibbs_comm_unique_id.argtypes = [C.c_void_p]
    L.hgibbs_comm_init.argtypes = [vp, C.c_int, C.c_int, C.c_void_p]
    L.hgibbs_comm_init_external.argtypes = [vp, C.c_int, C.c_int, ALLREDUCE_FN, C.c_void_p]
    L.hgibbs_p2p_export.argtypes = [vp, C.c_void_p]
    L.hgibbs_p2p_import.argtypes = [vp, C.c_void_p]
    L.hgibbs_load_bed.argtypes = [vp, u8p, C.c_uint64, C.c_uint32, C.c_uint32, u8p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.hgibbs_synth_bed.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_double]
    L.hgibbs_dims.argtypes = [vp, u32p, u32p, u32p, u32p]
    L.hgibbs_get_bed.argtypes = [vp, C.c_uint32, C.c_uint32, u8p, C.c_uint64]
    L.hgibbs_marker_stats.argtypes = [vp, dp, dp, u64p, u64p, u64p]
    L.hgibbs_set_residual.argtypes = [vp, dp]
    L.hgibbs_get_residual.argtypes = [vp, dp]
    L.hgibbs_reduce_eps.argtypes = [vp, dp, dp]
    L.hgibbs_add_scalar.argtypes = [vp, C.c_double]
    L.hgibbs_update_marker.argtypes = [vp, C.c_uint32, C.c_double]
    L.hgibbs_dot_marker.argtypes = [vp, C.c_uint32, dp]
    L.hgibbs_set_covariates.argtypes = [vp, dp, C.c_int]
    L.hgibbs_cov_dot.argtypes = [vp, C.c_int, C.c_double, dp]
    L.hgibbs_cov_update.argtypes = [vp, C.c_int, C.c_double]
    L.hydra_chain_set_covariates.argtypes = [vp, dp, C.c_int]
    L.hydra_chain_gamma.argtypes = [vp, dp, ip]
    L.hgibbs_set_components.argtypes = [vp, ip]
    L.hydra_chain_restore.argtypes = [vp, C.POINTER(RestartState)]
    L.hydra_rng_to_boost_words.argtypes = [C.POINTER(RngState), u32p]
    L.hydra_rng_from_boost_words.argtypes = [u32p, C.POINTER(RngState)]
    L.hydra_rng_shuffle.argtypes = [C.POINTER(RngState), ip, C.c_uint32]
    L.hgibbs_set_model.argtypes = [vp, C.c_int, C.c_int, ip, dp, dp]
    L.hgibbs_set_beta.argtypes = [vp, dp]
    L.hgibbs_get_beta.argtypes = [vp, dp, ip, dp]
    L.hgibbs_beta_sqnorm.argtypes = [vp, dp]
    L.hgibbs_sweep.argtypes = [vp, ip, C.c_double, dp, dp, u8p, C.POINTER(RngState), ip, u64p]
    L.hgibbs_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.hgibbs_walker_search.argtypes = [u64p, C.c_uint32, C.c_uint32, u32p, C.c_uint32]
    L.hgibbs_last_sweep_stats.argtypes = [vp, C.POINTER(SweepStats)]
    L.hgibbs_stream_ceiling.argtypes = [vp, C.c_uint64, C.c_int, dp]
    L.hgibbs_debug_times.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.hgibbs_resident_trace.argtypes = [vp, C.POINTER(C.c_uint64), C.c_uint64]
    L.hydra_chain_create.argtypes = [vp, C.POINTER(ModelDesc), dp, C.POINTER(vp)]
    L.hydra_chain_destroy.argtypes = [vp]
    L.hydra_chain_iterate.argtypes = [vp]
    L.hydra_chain_state.argtypes = [vp, dp, dp, dp, dp, ip, ip, C.POINTER(RngState)]
    L.hydra_chain_csv_line.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_size_t]
    L.hydra_chain_order.argtypes = [vp]
    L.hydra_chain_order.restype = ip
    L.hydra_chain_last_nnz.argtypes = [vp]
    gp = C.POINTER(GrandState)
    L.hgibbs_grand_seed.argtypes = [gp, C.c_uint32]
    L.hgibbs_grand_seed.restype = None
    L.hgibbs_grand_next.argtypes = [gp]
    L.hgibbs_grand_next.restype = C.c_int32
    L.hgibbs_ars_sample.argtypes = [dp, C.c_double, C.c_double, LOGDENS_FN, C.c_void_p, gp, dp, ip]
    L.hgibbs_w_init.argtypes = [vp, ip]
    L.hgibbs_w_marker_stats.argtypes = [vp, dp, dp, dp]
    L.hgibbs_w_set_model.argtypes = [vp, C.c_int, C.c_int, ip, dp, C.c_int]
    L.hgibbs_w_reduce.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, dp]
    L.hgibbs_w_refresh_vi.argtypes = [vp, C.c_double]
    L.hgibbs_w_get_vi.argtypes = [vp, dp, dp]
    L.hgibbs_w_marker_sums.argtypes = [vp, C.c_uint32, C.c_double, C.c_double, dp, dp, dp]
    L.hgibbs_w_sweep.argtypes = [vp, ip, C.c_double, dp, dp, C.c_double, C.POINTER(RngState), gp, ip, dp, u64p]
    L.hgibbs_w_last_sweep_stats.argtypes = [vp, C.POINTER(WSweepStats)]
    L.hgibbs_w_ars_device_probe.argtypes = [vp, dp, C.c_double, C.c_double, C.c_uint32, C.c_uint32, dp, dp, dp]
    L.hgibbs_w_get_beta.argtypes = [vp, dp, ip]
    L.hgibbs_w_set_beta.argtypes = [vp, dp, ip]
    L.hydraw_chain_create.argtypes = [vp, C.POINTER(WModelDesc), dp, ip, C.POINTER(vp)]
    L.hydraw_chain_destroy.argtypes = [vp]
    L.hydraw_chain_set_covariates.argtypes = [vp, dp, C.c_int]
    L.hydraw_chain_reseed_ars.argtypes = [vp, C.c_uint32]
    L.hydraw_chain_iterate.argtypes = [vp]
    L.hydraw_chain_state.argtypes = [vp, dp, dp, dp, dp, ip, ip, C.POINTER(RngState), gp]
    L.hydraw_chain_gamma.argtypes = [vp, dp, ip]
    L.hydraw_chain_order.argtypes = [vp]
    L.hydraw_chain_order.restype = C.POINTER(C.c_int32)
    L.hydraw_chain_last_nnz.argtypes = [vp]
    L.hydraw_chain_last_nnz.restype = C.c_uint64
    L.hydraw_chain_csv_line.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_size_t]
    L.hydraw_chain_restore.argtypes = [vp, C.POINTER(WRestartState)]
    L.hydra_chain_last_nnz.restype = C.c_uint64
    L.hgibbs_score.argtypes = [vp, C.c_int, dp, dp, dp]
    L.hgibbs_last_score_ms.argtypes = [vp, dp]
    L.hgibbs_ld.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, dp, C.POINTER(C.c_int64)]
    L.hgibbs_last_ld_ms.argtypes = [vp, dp]
    L.hgibbs_ld_scores.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint64), C.c_int, dp]
    L.hgibbs_last_ld_scores_ms.argtypes = [vp, dp, dp]
    L.hgibbs_ld_mask.argtypes = [vp, C.c_uint32, u32p, C.c_double, u64p, u64p, u64p]
    L.hgibbs_last_ld_mask_ms.argtypes = [vp, dp, dp]
    L.hgibbs_ld_greedy.argtypes = [C.c_uint32, C.c_uint32, u64p, u64p, u32p, C.c_uint32, u8p, ip]
    L.hgibbs_ld_clump.argtypes = [vp, C.c_uint32, u32p, C.c_double, u32p, C.c_uint32, u8p, ip, u64p]
    rp = C.POINTER(RngState)
    L.hgibbs_ss_begin.argtypes = [vp, C.c_double, C.c_uint32, u32p, dp]
    L.hgibbs_ss_sweep.argtypes = [vp, ip, C.c_double, dp, dp, u8p, rp, ip, u64p]
    L.hgibbs_ss_state.argtypes = [vp, dp, dp, dp]
    L.hgibbs_ss_band_get.argtypes = [vp, C.c_uint32, C.c_uint32, dp]
    L.hgibbs_ss_end.argtypes = [vp]
    L.hgibbs_last_ss_ms.argtypes = [vp, dp, dp]
    L.hgibbs_ss_sweep_host.argtypes = [C.c_uint32, C.c_double, C.c_uint32, u32p, dp, dp, dp, ip, dp, C.c_int, C.c_int, ip, dp, dp, ip, C.c_double, dp, dp,
                                       u8p, rp, ip, u64p]
    L.hgibbs_ss_partition.argtypes = [C.c_uint32, u32p, C.c_uint32, u32p, u32p]
    L.hgibbs_ss_sweep_streams.argtypes = [vp, ip, C.c_double, dp, dp, u8p, C.c_uint32, u32p, rp, ip, u64p]
    L.hgibbs_ss_sweep_streams_host.argtypes = [C.c_uint32, C.c_double, C.c_uint32, u32p, dp, dp, dp, ip, dp, C.c_int, C.c_int, ip, dp, dp, ip, C.c_double, dp,
                                               dp, u8p, C.c_uint32, u32p, rp, ip, u64p]
    L.hydra_ss_chain_set_streams.argtypes = [vp, C.c_uint32]
    L.hydra_ss_chain_streams.argtypes = [vp, u32p, u32p, rp]
    L.hydra_ss_chain_create.argtypes = [vp, C.POINTER(ModelDesc), C.c_double, C.c_uint32, u32p, dp, u8p, C.POINTER(vp)]
    L.hydra_ss_chain_create_host.argtypes = [C.c_uint32, C.POINTER(ModelDesc), C.c_double, C.c_uint32, u32p, dp, dp, u8p, C.POINTER(vp)]
    L.hydra_ss_chain_destroy.argtypes = [vp]
    L.hydra_ss_chain_iterate.argtypes = [vp]
    L.hydra_ss_chain_state.argtypes = [vp, dp, dp, dp, dp, ip, ip, rp]
    L.hydra_ss_chain_effects.argtypes = [vp, dp, ip, dp, dp]
    L.hydra_ss_chain_last_nnz.argtypes = [vp]
    L.hydra_ss_chain_last_nnz.restype = C.c_uint64
    L.hydra_ss_chain_order.argtypes = [vp]
    L.hydra_ss_chain_order.restype = ip
    L.hydra_ss_chain_csv_line.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_size_t]
    L.hgibbs_ss_replicas.argtypes = [vp, C.c_uint32]
    L.hgibbs_ss_sweep_replicas.argtypes = [vp, C.c_uint32, ip, dp, dp, dp, u8p, C.c_uint32, u32p, rp, ip, u64p]
    L.hgibbs_ss_replica_sums.argtypes = [vp, dp, dp, dp]
    L.hgibbs_ss_replica_get.argtypes = [vp, C.c_uint32, dp, ip, dp, dp]
    L.hgibbs_ss_replica_set_beta.argtypes = [vp, C.c_uint32, dp]
    L.hgibbs_mcmc_diag.argtypes = [C.c_uint32, C.c_uint32, dp, dp, dp, dp, dp]
    L.hgibbs_ss_post_begin.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.hgibbs_ss_post_add.argtypes = [vp]
    L.hgibbs_ss_post_get.argtypes = [vp, dp, dp, dp, u32p, dp]
    L.hgibbs_ss_post_raw.argtypes = [vp, C.c_uint32, C.c_uint32, dp, dp]
    L.hgibbs_ss_post_end.argtypes = [vp]
    L.hgibbs_last_ss_post_ms.argtypes = [vp, dp, dp]
    L.hgibbs_cs_begin.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.hgibbs_cs_add_flags.argtypes = [vp, u8p]
    L.hgibbs_ss_cs_add.argtypes = [vp, C.c_uint32]
    L.hgibbs_cs_counts.argtypes = [vp, u32p]
    L.hgibbs_cs_history.argtypes = [vp, u64p]
    L.hgibbs_cs_sets.argtypes = [vp, C.c_uint32, u64p, u64p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, u32p, u32p, u64p, u32p, u32p]
    L.hgibbs_cs_end.argtypes = [vp]
    L.hgibbs_last_cs_ms.argtypes = [vp, dp, dp, dp]
    L.hgibbs_cs_select.argtypes = [C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p, u32p, u32p, C.c_uint32, C.c_uint32, u32p, u32p]
    L.hydra_ss_multi_create.argtypes = [vp, C.POINTER(ModelDesc), C.c_uint32, u32p, C.c_double, C.c_uint32, u32p, dp, u8p, C.c_uint32, C.POINTER(vp)]
    L.hydra_ss_multi_destroy.argtypes = [vp]
    L.hydra_ss_multi_iterate.argtypes = [vp]
    L.hydra_ss_multi_state.argtypes = [vp, C.c_uint32, dp, dp, dp, dp, ip, ip, rp]
    L.hydra_ss_multi_effects.argtypes = [vp, C.c_uint32, dp, ip, dp, dp]
    L.hydra_ss_multi_streams.argtypes = [vp, u32p, u32p, rp]
    L.hydra_ss_multi_last_nnz.argtypes = [vp, C.c_uint32]
    L.hydra_ss_multi_last_nnz.restype = C.c_uint64
    L.hydra_ss_multi_csv_line.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]
    L.hgibbs_marker_dots.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, dp, dp, dp]
    L.hgibbs_last_marker_dots_ms.argtypes = [vp, dp]
    L.hgibbs_marker_class_sums.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, dp, dp]
    L.hgibbs_last_marker_class_sums_ms.argtypes = [vp, dp]
    L.hgibbs_set_gram.argtypes = [vp, C.c_uint32, C_U64P, C_U32P, dp, dp, dp]
    L.hgibbs_last_set_gram_ms.argtypes = [vp, dp]
    L.hgibbs_set_tests.argtypes = [C.c_uint32, dp, dp, dp, C.POINTER(SetResult)]
    L.hgibbs_logit_null.argtypes = [C.c_uint32, C.c_int, dp, dp, dp, dp, dp, dp, C.POINTER(C.c_int)]
    L.hgibbs_spa_roots.argtypes = [vp, C.c_uint32, C_U32P, C.c_int, dp, dp, dp, dp, dp, C.POINTER(SpaRoot)]
    L.hgibbs_last_spa_ms.argtypes = [vp, dp]
    L.hgibbs_spa_pvalue.argtypes = [C.c_double, C.POINTER(SpaRoot), dp, dp, dp, C.POINTER(C.c_int)]
    L.hgibbs_firth_fit.argtypes = [vp, C.c_uint32, C_U32P, C.c_int, dp, dp, dp, dp, dp, C.POINTER(FirthRec)]
    L.hgibbs_last_firth_ms.argtypes = [vp, dp]
    L.hgibbs_firth_stats.argtypes = [C.c_double, C.POINTER(FirthRec), dp, dp, dp, C.POINTER(C.c_int)]
    L.hgibbs_king.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]
    L.hgibbs_king_pairs.argtypes = [vp, C.c_double, C.POINTER(C.c_uint64)]
    L.hgibbs_king_pairs_get.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), dp]
    L.hgibbs_last_king_ms.argtypes = [vp, dp]
    L.hgibbs_roh.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(RohParams), C.POINTER(C.c_uint64)]
    L.hgibbs_roh_get.argtypes = [vp, C.c_void_p]
    L.hgibbs_last_roh_ms.argtypes = [vp, dp]
    L.hgibbs_pair_tables.argtypes = [vp, C.c_uint32, C_U32P, C.c_uint32, C_U32P, u8p, C.POINTER(C.c_int32)]
    L.hgibbs_last_pair_tables_ms.argtypes = [vp, dp]
    L.hgibbs_epi_scan.argtypes = [vp, C.c_uint32, C_U32P, C.c_uint32, C_U32P, u8p, C.c_double, C.POINTER(C.c_uint64)]
    L.hgibbs_epi_scan_get.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), dp]
    L.hgibbs_last_epi_ms.argtypes = [vp, dp, dp]
    L.hgibbs_epi_test.argtypes = [C.POINTER(C.c_int32), C.POINTER(EpiResult)]
    L.hgibbs_pca.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, dp, C.c_uint64, dp, dp, dp, C.POINTER(PcaReport)]
    L.hgibbs_last_pca_ms.argtypes = [vp, dp]
    L.hgibbs_region_var.argtypes = [vp, C.c_int, dp, dp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), dp, dp]
    L.hgibbs_last_region_var_ms.argtypes = [vp, dp]
    L.hgibbs_grm.argtypes = [vp, C.c_uint32, C.c_uint32, dp, C.POINTER(C.c_int32)]
    L.hgibbs_grm_info.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
    L.hgibbs_last_grm_ms.argtypes = [vp, dp]
    L.hgibbs_grm_rowsums.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, u32p]
    L.hgibbs_last_grm_rowsums_ms.argtypes = [vp, dp, dp]
    L.hgibbs_he_fit.argtypes = [C.c_uint32, dp, dp, dp, dp, dp, u32p, C.POINTER(HeResult)]
    ip = C.POINTER(C.c_int)
    L.hgibbs_reml_solve.argtypes = [vp, C.c_int, C.c_int, dp, C.c_double, C.c_double, C.c_int, dp, dp, ip, dp]
    L.hgibbs_reml_eval.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.c_uint64, C.c_double, C.c_double, C.c_int, dp, ip]
    L.hgibbs_reml.argtypes = [vp, C.POINTER(RemlOpts), C.c_int, dp, dp, C.POINTER(RemlResult), dp]
    L.hgibbs_reml_next.argtypes = [C.c_int, dp, dp, C.c_double, C.c_double, C.c_int, dp, ip]
    L.hgibbs_reml_finish.argtypes = [C.c_int, C.c_uint32, C.c_int, dp, dp, dp, dp, C.POINTER(RemlEstimate)]
    L.hgibbs_last_reml_ms.argtypes = [vp, dp, dp]
    L.hgibbs_row_sums.argtypes = [vp, C.c_int, dp, dp]
    L.hgibbs_last_row_sums_ms.argtypes = [vp, dp]
    sl = C.POINTER(SparseList)
    L.hgibbs_sparse_begin.argtypes = [vp, C.c_uint32, C.c_uint32, u8p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.hgibbs_sparse_put.argtypes = [vp, C.c_uint32, C.c_uint32, sl, sl, sl]
    L.hgibbs_sparse_end.argtypes = [vp]
    L.hgibbs_sparse_counts.argtypes = [vp, C.c_uint32, C.c_uint32, u64p, u64p, u64p]
    L.hgibbs_sparse_get.argtypes = [vp, C.c_uint32, C.c_uint32, u32p, u32p, u32p]
    L.hgibbs_last_sparse_ms.argtypes = [vp, dp, dp]
    L.hgibbs_hwe_exact.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, dp]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise HgError(lib().hgibbs_last_error().decode(errors="replace"))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def rng_shuffle(rng, v):
    """hydra_rng_shuffle: the chain's marker shuffle on a caller's RngState and contiguous int32 array, both in place."""
    if v.dtype != np.int32 or not v.flags.c_contiguous:
        raise ValueError("rng_shuffle: a contiguous int32 array is required")
    check(lib().hydra_rng_shuffle(C.byref(rng), _ip(v), v.size))


def _order_and_leaders(M, order, may_lead):
    od = np.ascontiguousarray(order, dtype=np.uint32).reshape(-1)
    ml = None
    if may_lead is not None:
        ml = np.ascontiguousarray(may_lead, dtype=np.uint8)
        if ml.shape != (M,):
            raise ValueError("may_lead must be (%d,)" % M)
    return od, ml


def ld_greedy(M, W, fwd, bwd, order, may_lead=None):
    """hgibbs_ld_greedy (host only): the greedy selection on two masks in Device.ld_mask's layout, (M, wpr) uint64 each.  order: the
    participating markers in descending priority; may_lead (M,) bytes or None for "all may".  Returns owner (M,) int32: the leader
    that claimed the marker (itself for a leader), -1 for a marker nobody claimed or that does not participate."""
    wpr = (int(W) + 63) // 64
    fwd = np.ascontiguousarray(fwd, dtype=np.uint64)
    bwd = np.ascontiguousarray(bwd, dtype=np.uint64)
    if 1 <= W <= 4096 and (fwd.shape != (M, wpr) or bwd.shape != (M, wpr)):
        raise ValueError("fwd and bwd must be (%d, %d)" % (M, wpr))
    od, ml = _order_and_leaders(M, order, may_lead)
    owner = np.full(max(int(M), 1), -1, dtype=np.int32)
    check(lib().hgibbs_ld_greedy(M, W, _u64(fwd), _u64(bwd), od.ctypes.data_as(C_U32P), od.size, _u8(ml) if ml is not None else None, _ip(owner)))
    return owner[:M]


def _u32(a):
    return a.ctypes.data_as(C_U32P)


def cs_select(M, leads, lead_cnt, status, size, pep, members, max_size, min_pep):
    """hgibbs_cs_select (host only): the walk over Device.cs_sets' candidates by descending lead_cnt, ties by ascending lead; one is
    accepted iff its status is 0, its pep >= min_pep and none of its members belongs to a set accepted before.  members is
    (nlead, max_size) uint32.  Returns the accepted candidates' positions in the order taken (uint32)."""
    leads, lead_cnt, status, size, pep = (np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in (leads, lead_cnt, status, size, pep))
    n = leads.size
    members = np.ascontiguousarray(members, dtype=np.uint32)
    for a in (lead_cnt, status, size, pep):
        if a.size != n:
            raise ValueError("lead_cnt, status, size and pep must have one entry per lead")
    if 1 <= max_size <= 256 and members.size != n * max_size:
        raise ValueError("members must be (%d, %d)" % (n, max_size))
    taken = np.zeros(max(n, 1), dtype=np.uint32)
    nt = C.c_uint32(0)
    check(lib().hgibbs_cs_select(M, n, _u32(leads), _u32(lead_cnt), _u32(status), _u32(size), _u32(pep), _u32(members), int(max_size) & 0xffffffff,
                                 int(min_pep) & 0xffffffff, _u32(taken), C.byref(nt)))
    return taken[:nt.value].copy()


def ss_ahead(M, W, ahead=None):
    """The window of the summary-statistics engines as they take it: (M,) uint32, min(W, M - 1 - j) where none is given."""
    if ahead is None:
        return np.minimum(W, M - 1 - np.arange(M)).astype(np.uint32)
    return np.ascontiguousarray(ahead, dtype=np.uint32)


def ss_sweep_host(n_eff, W, ahead, band, c, beta, components, acum, groups, cVa, cVaI, order, sigmaE, sigmaG, estPi, adaV, rng):
    """hgibbs_ss_sweep_host (host only): one sweep of the summary-statistics step on host arrays.  band (M, W) float64; c, beta, acum
    float64 and components int32 of M entries are the state, updated in place (contiguous arrays of those types are required); cVa and
    cVaI (G, K); rng: RngState, updated in place.  Returns (cass[G, K], nnz_updates)."""
    for a, t in ((c, np.float64), (beta, np.float64), (acum, np.float64), (components, np.int32)):
        if a.dtype != t or not a.flags.c_contiguous:
            raise ValueError("ss_sweep_host: the state must be contiguous float64 / int32 arrays (they are updated in place)")
    M = c.shape[0]
    band = np.ascontiguousarray(band, dtype=np.float64)
    cVa = np.ascontiguousarray(cVa, dtype=np.float64)
    cVaI = np.ascontiguousarray(cVaI, dtype=np.float64)
    G, K = cVa.shape
    ah = ss_ahead(M, W, ahead)
    groups = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
    order = np.ascontiguousarray(order, dtype=np.int32)
    sigmaG = np.ascontiguousarray(sigmaG, dtype=np.float64)
    estPi = np.ascontiguousarray(estPi, dtype=np.float64)
    adaV = np.ascontiguousarray(adaV, dtype=np.uint8)
    cass = np.zeros((G, K), dtype=np.int32)
    nnz = C.c_uint64()
    check(lib().hgibbs_ss_sweep_host(M, float(n_eff), W, ah.ctypes.data_as(C_U32P), _dp(band), _dp(c), _dp(beta), _ip(components), _dp(acum), G, K,
                                     _ip(groups) if groups is not None else None, _dp(cVa), _dp(cVaI), _ip(order), float(sigmaE), _dp(sigmaG),
                                     _dp(estPi), _u8(adaV), C.byref(rng), _ip(cass), C.byref(nnz)))
    return cass, nnz.value


def ss_partition(ahead, S_max):
    """hgibbs_ss_partition (host only): the bounds of at most S_max intervals of whole LD blocks, (S + 1,) uint32 from 0 to M."""
    ah = np.ascontiguousarray(ahead, dtype=np.uint32)
    bounds = np.zeros(max(int(S_max), 0) + 1 if 0 <= int(S_max) <= 1024 else 1, dtype=np.uint32)
    S = C.c_uint32()
    check(lib().hgibbs_ss_partition(ah.shape[0], ah.ctypes.data_as(C_U32P), int(S_max) & 0xffffffff, bounds.ctypes.data_as(C_U32P), C.byref(S)))
    return bounds[:S.value + 1].copy()


class _RngArray:
    """A list of RngState as the contiguous array the streams' calls take; `back()` copies the states into the list's items again."""

    def __init__(self, rngs):
        self.rngs = list(rngs)
        self.arr = (RngState * max(len(self.rngs), 1))()
        for a, r in zip(self.arr, self.rngs):
            C.memmove(C.byref(a), C.byref(r), C.sizeof(RngState))

    def back(self):
        for a, r in zip(self.arr, self.rngs):
            C.memmove(C.byref(r), C.byref(a), C.sizeof(RngState))


def mcmc_diag(x):
    """hgibbs_mcmc_diag (host only): x (R, T), chain-major.  Returns (mean, sd, rhat, ess): split-R^ and the effective sample size of
    the 2 R half-chains; rhat and ess are NaN where no half-chain moves."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("mcmc_diag: x must be (R, T)")
    out = [C.c_double() for _ in range(4)]
    check(lib().hgibbs_mcmc_diag(x.shape[0], x.shape[1], _dp(x), *[C.byref(o) for o in out]))
    return tuple(o.value for o in out)


def ss_sweep_streams_host(n_eff, W, ahead, band, c, beta, components, acum, groups, cVa, cVaI, order, sigmaE, sigmaG, estPi, adaV, bounds, rngs, S=None):
    """hgibbs_ss_sweep_streams_host (host only): ss_sweep_host with the intervals `bounds` (S + 1) of independent LD blocks, swept one
    after the other, interval s with rngs[s] (a list of RngState, updated in place).  Returns (cass[G, K], nnz_updates)."""
    for a, t in ((c, np.float64), (beta, np.float64), (acum, np.float64), (components, np.int32)):
        if a.dtype != t or not a.flags.c_contiguous:
            raise ValueError("ss_sweep_streams_host: the state must be contiguous float64 / int32 arrays (they are updated in place)")
    M = c.shape[0]
    band = np.ascontiguousarray(band, dtype=np.float64)
    cVa = np.ascontiguousarray(cVa, dtype=np.float64)
    cVaI = np.ascontiguousarray(cVaI, dtype=np.float64)
    G, K = cVa.shape
    ah = ss_ahead(M, W, ahead)
    groups = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
    order = np.ascontiguousarray(order, dtype=np.int32)
    sigmaG = np.ascontiguousarray(sigmaG, dtype=np.float64)
    estPi = np.ascontiguousarray(estPi, dtype=np.float64)
    adaV = np.ascontiguousarray(adaV, dtype=np.uint8)
    bounds = np.ascontiguousarray(bounds, dtype=np.uint32)
    S = bounds.shape[0] - 1 if S is None else S
    ra = _RngArray(rngs)
    cass = np.zeros((G, K), dtype=np.int32)
    nnz = C.c_uint64()
    check(lib().hgibbs_ss_sweep_streams_host(M, float(n_eff), W, ah.ctypes.data_as(C_U32P), _dp(band), _dp(c), _dp(beta), _ip(components), _dp(acum), G, K,
                                             _ip(groups) if groups is not None else None, _dp(cVa), _dp(cVaI), _ip(order), float(sigmaE), _dp(sigmaG),
                                             _dp(estPi), _u8(adaV), S, bounds.ctypes.data_as(C_U32P), ra.arr, _ip(cass), C.byref(nnz)))
    ra.back()
    return cass, nnz.value


def he_fit(y, ay, ayy, a1, a2, partners):
    """hgibbs_he_fit (host only): Haseman-Elston regression from the row sums of Device.grm_rowsums for Y = [y, y * y] (ay = A y,
    ayy = A (y o y)).  Returns a dict: n_used, n_left_out, pairs, vp, and under "cp" and "sd" a dict of intercept, slope, h2, their OLS
    and jackknife SEs (…_se, …_se_jk) and the P values of intercept and slope (…_p, …_p_jk)."""
    v = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (y, ay, ayy, a1, a2)]
    pt = np.ascontiguousarray(partners, dtype=np.uint32).reshape(-1)
    n = v[0].size
    if any(x.size != n for x in v) or pt.size != n:
        raise ValueError("he_fit: y, ay, ayy, a1, a2 and partners must have one length")
    res = HeResult()
    check(lib().hgibbs_he_fit(n, *[_dp(x) for x in v], pt.ctypes.data_as(C_U32P), C.byref(res)))
    out = {k: getattr(res, k) for k in ("n_used", "n_left_out", "pairs", "vp")}
    for form in ("cp", "sd"):
        out[form] = {k: getattr(getattr(res, form), k) for k, _ in HeForm._fields_}
    return out


def reml_next(x, f, h2_start=0.25, x_tol=0.01, max_steps=12):
    """hgibbs_reml_next (host only): the root rule of --reml on x = log delta from the points evaluated so far.  Returns (x_next,
    status): REML_CONTINUE to evaluate x_next, REML_CONVERGED or REML_AT_BOUND when x[-1] is the estimate.  A flat f or max_steps
    evaluations without a root raise."""
    xs = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    fs = np.ascontiguousarray(f, dtype=np.float64).reshape(-1)
    if xs.size != fs.size:
        raise ValueError("reml_next: x and f must have one length")
    xn, st = C.c_double(), C.c_int()
    check(lib().hgibbs_reml_next(xs.size, _dp(xs), _dp(fs), float(h2_start), float(x_tol), int(max_steps), C.byref(xn), C.byref(st)))
    return xn.value, st.value


def reml_finish(n, q, x2, sums_prev, sums_last, ai3=None):
    """hgibbs_reml_finish (host only): the estimate at x2[1] from the sums ((T + 1, 3)) of the last two evaluations and, with ai3 =
    (a'z1, a'z2, v'z2), the standard errors of the average-information matrix.  Returns a dict of hgibbs_reml_estimate's fields."""
    sp = np.ascontiguousarray(sums_prev, dtype=np.float64).reshape(-1)
    sl = np.ascontiguousarray(sums_last, dtype=np.float64).reshape(-1)
    if sp.size != sl.size or sp.size % 3 or sp.size < 6:
        raise ValueError("reml_finish: the sums must be (T + 1, 3) each")
    xx = np.ascontiguousarray(x2, dtype=np.float64).reshape(2)
    ai = np.ascontiguousarray(ai3, dtype=np.float64).reshape(3) if ai3 is not None else None
    est = RemlEstimate()
    check(lib().hgibbs_reml_finish(sp.size // 3 - 1, int(n), int(q), _dp(xx), _dp(sp), _dp(sl), _dp(ai) if ai is not None else None, C.byref(est)))
    return {k: getattr(est, k) for k, _ in RemlEstimate._fields_}


def hwe_exact(n_het, n_hom_a, n_hom_b):
    """hgibbs_hwe_exact (host only): the P value of the exact test of Hardy-Weinberg proportions (Wigginton, Cutler & Abecasis 2005)
    for the genotype counts; NaN without genotypes."""
    p = C.c_double()
    check(lib().hgibbs_hwe_exact(int(n_het), int(n_hom_a), int(n_hom_b), C.byref(p)))
    return p.value


def logit_null(Z, y):
    """hgibbs_logit_null (host only): the maximum-likelihood logistic fit of y in {0, 1} on the columns of Z (n, q), first column ones.
    Returns a dict: coef (q,), mu (n,), w = mu (1 - mu) (n,), chol (q, q) the lower Cholesky factor of Z'WZ, iters."""
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim != 2:
        raise ValueError("logit_null: Z must be (n, q)")
    n, q = Z.shape
    y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if y.size != n:
        raise ValueError("logit_null: y must have Z's %d rows" % n)
    Zc = np.ascontiguousarray(Z.T)  # column-major
    coef, mu, w, chol = np.zeros(max(q, 1)), np.zeros(max(n, 1)), np.zeros(max(n, 1)), np.zeros((max(q, 1), max(q, 1)))
    it = C.c_int(0)
    check(lib().hgibbs_logit_null(n, q, _dp(Zc), _dp(y), _dp(coef), _dp(mu), _dp(w), _dp(chol), C.byref(it)))
    return {"coef": coef[:q], "mu": mu[:n], "w": w[:n], "chol": np.ascontiguousarray(chol[:q, :q].T), "iters": it.value}


def spa_pvalue(s, root):
    """hgibbs_spa_pvalue (host only): the saddlepoint p-value of the score s from a SpaRoot of Device.spa_roots.  Returns
    (p_upper, p_lower, p, valid); p is NaN and valid False unless both tails are valid."""
    up, dn, p, ok = C.c_double(), C.c_double(), C.c_double(), C.c_int()
    check(lib().hgibbs_spa_pvalue(float(s), C.byref(root), C.byref(up), C.byref(dn), C.byref(p), C.byref(ok)))
    return up.value, dn.value, p.value, bool(ok.value)


def set_tests(U, Phi, a):
    """hgibbs_set_tests (host only): burden and SKAT statistics of one marker set from its scores U (m,), their covariance Phi (m, m)
    and the weights a (m,).  Returns a SetResult."""
    U = np.ascontiguousarray(U, dtype=np.float64).reshape(-1)
    m = U.size
    Phi = np.ascontiguousarray(Phi, dtype=np.float64)
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    if Phi.shape != (m, m) or a.size != m:
        raise ValueError("set_tests: Phi must be (%d, %d) and a (%d,)" % (m, m, m))
    r = SetResult()
    check(lib().hgibbs_set_tests(m, _dp(U), _dp(Phi), _dp(a), C.byref(r)))
    return r


def epi_test(table):
    """hgibbs_epi_test (host only): BOOST's interaction test of one 2 x 3 x 3 table, table[k, i, j] (or its 18 counts in that order).
    Returns an EpiResult: ksa, lr, df, iters, converged, p."""
    t = np.ascontiguousarray(table, dtype=np.int32).reshape(-1)
    if t.size != 18:
        raise ValueError("epi_test: the table has 18 counts")
    r = EpiResult()
    check(lib().hgibbs_epi_test(_ip(t), C.byref(r)))
    return r


def firth_stats(s, rec):
    """hgibbs_firth_stats (host only): the statistics of the score s from a FirthRec of Device.firth_fit.  Returns (lrt, se, p, valid);
    the three numbers are NaN and valid False where the fit does not stand (the caller keeps the score test)."""
    lrt, se, p, ok = C.c_double(), C.c_double(), C.c_double(), C.c_int()
    check(lib().hgibbs_firth_stats(float(s), C.byref(rec), C.byref(lrt), C.byref(se), C.byref(p), C.byref(ok)))
    return lrt.value, se.value, p.value, bool(ok.value)


class Device:
    """One GPU's share of the problem (hgibbs_t)."""

    def __init__(self, device_id=0):
        self.L = lib()
        self.h = C.c_void_p()
        check(self.L.hgibbs_create(device_id, C.byref(self.h)))
        self.M = self.n_local = self.n_global = self.row_begin = 0
        self.G = self.K = 0

    def close(self):
        if self.h:
            self.L.hgibbs_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- distributed --
    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        check(lib().hgibbs_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, nranks, rank, uid):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid) if uid else None
        check(self.L.hgibbs_comm_init(self.h, nranks, rank, buf))

    def comm_init_external(self, nranks, rank, allreduce):
        """allreduce(numpy_array) must sum the array in place over all ranks."""
        def cb(user, buf, count, dtype):
            try:
                ty = C.c_double if dtype == 0 else C.c_uint64
                arr = np.ctypeslib.as_array(C.cast(buf, C.POINTER(ty)), shape=(count,))
                allreduce(arr)
                return 0
            except Exception:  # pragma: no cover - reported through the return code
                import traceback
                traceback.print_exc()
                return 1
        self._cb = ALLREDUCE_FN(cb)  # keep alive
        check(self.L.hgibbs_comm_init_external(self.h, nranks, rank, self._cb, None))

    def p2p_export(self):
        buf = (C.c_uint8 * 64)()
        check(self.L.hgibbs_p2p_export(self.h, buf))
        return bytes(buf)

    def p2p_import(self, handles):
        blob = b"".join(handles)
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        check(self.L.hgibbs_p2p_import(self.h, buf))

    # -- data --
    def _dims(self):
        a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(self.L.hgibbs_dims(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        self.n_global, self.n_local, self.M, self.row_begin = a.value, b.value, c.value, d.value

    def load_bed(self, bed, n_total, keep=None, row_begin=0, row_end=None, n_global=None):
        bed = np.ascontiguousarray(bed, dtype=np.uint8)
        M, stride = bed.shape
        kept = int(np.count_nonzero(keep)) if keep is not None else n_total
        if row_end is None:
            row_end = kept
        if n_global is None:
            n_global = kept
        kp = _u8(np.ascontiguousarray(keep, dtype=np.uint8)) if keep is not None else None
        check(self.L.hgibbs_load_bed(self.h, _u8(bed), stride, n_total, M, kp, row_begin, row_end, n_global))
        self._dims()

    def synth_bed(self, n_global, M, seed=42, missing_rate=0.0, row_begin=0, row_end=None):
        if row_end is None:
            row_end = n_global
        check(self.L.hgibbs_synth_bed(self.h, n_global, M, row_begin, row_end, seed, missing_rate))
        self._dims()

    def get_bed(self, m0=0, mcount=None):
        if mcount is None:
            mcount = self.M - m0
        out = np.zeros((mcount, (self.n_local + 3) // 4), dtype=np.uint8)
        check(self.L.hgibbs_get_bed(self.h, m0, mcount, _u8(out), out.shape[1]))
        return out

    # -- hydra's sparse representation: three index lists per marker (genotype 1, genotype 2, missing call) --
    def sparse_begin(self, n_total, M, keep=None, row_begin=0, row_end=None, n_global=None):
        kept = int(np.count_nonzero(keep)) if keep is not None else n_total
        if row_end is None:
            row_end = kept
        if n_global is None:
            n_global = kept
        kp = _u8(np.ascontiguousarray(keep, dtype=np.uint8)) if keep is not None else None
        check(self.L.hgibbs_sparse_begin(self.h, n_total, M, kp, row_begin, row_end, n_global))

    def sparse_put(self, m0, lists):
        """lists: three (start, len, idx, idx_base) for genotype 1, genotype 2 and missing calls; start and len hold one entry per
        marker of the slab, start as absolute positions, idx the piece of the index list that starts at idx_base."""
        hold, args, count = [], [], None
        for start, ln, idx, base in lists:
            start = np.ascontiguousarray(start, dtype=np.uint64)
            ln = np.ascontiguousarray(ln, dtype=np.uint64)
            idx = np.ascontiguousarray(idx, dtype=np.uint32)
            if count is None:
                count = start.shape[0]
            if start.shape[0] != count or ln.shape[0] != count:
                raise ValueError("start and len must hold one entry per marker of the slab")
            hold.append((start, ln, idx))
            args.append(SparseList(_u64(start), _u64(ln), idx.ctypes.data_as(C_U32P), int(base), idx.shape[0]))
        check(self.L.hgibbs_sparse_put(self.h, m0, count, C.byref(args[0]), C.byref(args[1]), C.byref(args[2])))

    def sparse_end(self):
        check(self.L.hgibbs_sparse_end(self.h))
        self._dims()

    def sparse_counts(self, m0=0, count=None):
        if count is None:
            count = self.M - m0
        n1, n2, nm = (np.zeros(count, dtype=np.uint64) for _ in range(3))
        check(self.L.hgibbs_sparse_counts(self.h, m0, count, _u64(n1), _u64(n2), _u64(nm)))
        return n1, n2, nm

    def sparse_get(self, m0=0, count=None, want=(True, True, True)):
        """The three concatenated index lists of markers [m0, m0 + count); a list not wanted comes back as None."""
        if count is None:
            count = self.M - m0
        cnt = self.sparse_counts(m0, count)
        out = [np.zeros(int(c.sum()), dtype=np.uint32) if w else None for c, w in zip(cnt, want)]
        check(self.L.hgibbs_sparse_get(self.h, m0, count, *[o.ctypes.data_as(C_U32P) if o is not None else None for o in out]))
        return out

    def last_sparse_ms(self):
        a, b = C.c_double(), C.c_double()
        check(self.L.hgibbs_last_sparse_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def marker_stats(self):
        M = self.M
        mave, mstd = np.zeros(M), np.zeros(M)
        n1, n2, nm = (np.zeros(M, dtype=np.uint64) for _ in range(3))
        check(self.L.hgibbs_marker_stats(self.h, _dp(mave), _dp(mstd), _u64(n1), _u64(n2), _u64(nm)))
        return mave, mstd, n1, n2, nm

    def set_residual(self, eps):
        eps = np.ascontiguousarray(eps, dtype=np.float64)
        assert eps.shape[0] == self.n_local
        check(self.L.hgibbs_set_residual(self.h, _dp(eps)))

    def get_residual(self):
        out = np.zeros(self.n_local)
        check(self.L.hgibbs_get_residual(self.h, _dp(out)))
        return out

    def reduce_eps(self):
        s, q = C.c_double(), C.c_double()
        check(self.L.hgibbs_reduce_eps(self.h, C.byref(s), C.byref(q)))
        return s.value, q.value

    def add_scalar(self, c):
        check(self.L.hgibbs_add_scalar(self.h, c))

    def set_covariates(self, X):
        """X (n_local, C) replaces the covariates on the handle; None takes them off (hgibbs_set_covariates(NULL, 0))."""
        if X is None:
            check(self.L.hgibbs_set_covariates(self.h, None, 0))
            return
        X = np.ascontiguousarray(X, dtype=np.float64)
        assert X.shape[0] == self.n_local
        check(self.L.hgibbs_set_covariates(self.h, _dp(X), X.shape[1]))

    def cov_dot(self, c, gamma_old):
        """sum_k X[k, c] * (eps_k + gamma_old * X[k, c]) over all ranks (hgibbs_cov_dot)."""
        v = C.c_double()
        check(self.L.hgibbs_cov_dot(self.h, c, gamma_old, C.byref(v)))
        return v.value

    def cov_update(self, c, dgamma):
        """eps_k = eps_k + dgamma * X[k, c] (hgibbs_cov_update)."""
        check(self.L.hgibbs_cov_update(self.h, c, dgamma))

    def w_ars_device_probe(self, dens9, beta_old, safe_limit, seed, ndraws):
        """hgibbs_w_ars_device_probe: `ndraws` adaptive-rejection draws of an effect on one device lane from the density with the nine
        parameters dens9.  Returns (microseconds per draw, density evaluations per draw, the last draw)."""
        d = np.ascontiguousarray(dens9, dtype=np.float64).reshape(-1)
        if d.size != 9:
            raise ValueError("w_ars_device_probe: dens9 has nine numbers")
        us, ev, last = C.c_double(), C.c_double(), C.c_double()
        check(self.L.hgibbs_w_ars_device_probe(self.h, _dp(d), beta_old, safe_limit, seed, ndraws, C.byref(us), C.byref(ev), C.byref(last)))
        return us.value, ev.value, last.value

    def update_marker(self, marker, dbeta):
        check(self.L.hgibbs_update_marker(self.h, marker, dbeta))

    def dot_marker(self, marker):
        v = C.c_double()
        check(self.L.hgibbs_dot_marker(self.h, marker, C.byref(v)))
        return v.value

    def set_model(self, groups, cVa, cVaI):
        cVa = np.ascontiguousarray(cVa, dtype=np.float64)
        cVaI = np.ascontiguousarray(cVaI, dtype=np.float64)
        G, K = cVa.shape
        g = _ip(np.ascontiguousarray(groups, dtype=np.int32)) if groups is not None else None
        check(self.L.hgibbs_set_model(self.h, G, K, g, _dp(cVa), _dp(cVaI)))
        self.G, self.K = G, K

    def set_beta(self, beta):
        beta = np.ascontiguousarray(beta, dtype=np.float64)
        check(self.L.hgibbs_set_beta(self.h, _dp(beta)))

    def get_beta(self):
        beta, comp, acum = np.zeros(self.M), np.zeros(self.M, dtype=np.int32), np.zeros(self.M)
        check(self.L.hgibbs_get_beta(self.h, _dp(beta), _ip(comp), _dp(acum)))
        return beta, comp, acum

    def beta_sqnorm(self):
        out = np.zeros(self.G)
        check(self.L.hgibbs_beta_sqnorm(self.h, _dp(out)))
        return out

    def stream_ceiling(self, nbytes=2 << 30, reps=10):
        out = C.c_double()
        check(self.L.hgibbs_stream_ceiling(self.h, nbytes, reps, C.byref(out)))
        return out.value

    def set_option(self, name, value):
        check(self.L.hgibbs_set_option(self.h, name.encode(), int(value)))

    def score(self, a, o):
        """(S, M) weights a, o -> (n_local, S): sum_j [g_ij not missing] (a_sj g_ij + o_sj) (hgibbs_score)."""
        a = np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64)
        o = np.ascontiguousarray(np.atleast_2d(o), dtype=np.float64)
        if a.shape != o.shape or a.shape[1] != self.M:
            raise ValueError("a and o must both be (S, %d)" % self.M)
        out = np.zeros((self.n_local, a.shape[0]))
        check(self.L.hgibbs_score(self.h, a.shape[0], _dp(a), _dp(o), _dp(out)))
        return out

    def last_score_ms(self):
        v = C.c_double()
        check(self.L.hgibbs_last_score_ms(self.h, C.byref(v)))
        return v.value

    def row_sums(self, tab):
        """(T, M, 4) tables -> (n_local, T): sum_j tab[t, j, code_ij], code 3 = missing call (hgibbs_row_sums)."""
        tab = np.ascontiguousarray(tab, dtype=np.float64)
        if tab.ndim != 3 or tab.shape[1:] != (self.M, 4):
            raise ValueError("tab must be (T, %d, 4)" % self.M)
        out = np.zeros((self.n_local, tab.shape[0]))
        check(self.L.hgibbs_row_sums(self.h, tab.shape[0], _dp(tab), _dp(out)))
        return out

    def last_row_sums_ms(self):
        v = C.c_double()
        check(self.L.hgibbs_last_row_sums_ms(self.h, C.byref(v)))
        return v.value

    def region_var(self, a, o, sets):
        """(S, M) weights a, o and a list of marker index arrays (each strictly increasing) -> (mean, var), both (nsets, S): mean and
        ddof = 1 variance over the rows of sum_{j in set} [g_ij not missing] (a_sj g_ij + o_sj) (hgibbs_region_var)."""
        a = np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64)
        o = np.ascontiguousarray(np.atleast_2d(o), dtype=np.float64)
        if a.shape != o.shape or a.shape[1] != self.M:
            raise ValueError("a and o must both be (S, %d)" % self.M)
        sets = [np.asarray(r, dtype=np.int64).ravel() for r in sets]
        for r in sets:
            if r.size and (r.min() < 0 or r.max() > 0xFFFFFFFF):
                raise ValueError("a marker index does not fit in 32 bits")
        off = np.zeros(len(sets) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([r.size for r in sets], dtype=np.uint64)
        idx = np.ascontiguousarray(np.concatenate(sets) if sets else np.zeros(0), dtype=np.uint32)
        if idx.size == 0:
            idx = np.zeros(1, dtype=np.uint32)  # (a pointer to pass; off says that nothing is read)
        mean = np.zeros((len(sets), a.shape[0]))
        var = np.zeros((len(sets), a.shape[0]))
        check(self.L.hgibbs_region_var(self.h, a.shape[0], _dp(a), _dp(o), len(sets), off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       idx.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(mean), _dp(var)))
        return mean, var

    def last_region_var_ms(self):
        v = C.c_double()
        check(self.L.hgibbs_last_region_var_ms(self.h, C.byref(v)))
        return v.value

    def ld(self, W, m0=0, count=None, r=True, sums=True):
        """Windowed LD (hgibbs_ld): r (count, W) with r[j - m0, d - 1] = x_j'x_{j+d} / (N - 1), and sums (count, W, 4) int64
        G, Bjq, Bqj, D; either may be turned off (None returned)."""
        if count is None:
            count = self.M - m0
        rr = np.zeros((count, W)) if r else None
        ss = np.zeros((count, W, 4), dtype=np.int64) if sums else None
        check(self.L.hgibbs_ld(self.h, m0, count, W, _dp(rr) if r else None,
                               ss.ctypes.data_as(C.POINTER(C.c_int64)) if sums else None))
        return rr, ss

    def last_ld_ms(self):
        v = C.c_double()
        check(self.L.hgibbs_last_ld_ms(self.h, C.byref(v)))
        return v.value

    def ld_scores(self, W, ahead=None, annot=None, C=None, adjust=True):
        """LD scores (hgibbs_ld_scores): (M, C) float64 with l2[j, c] = a_jc + sum over the pairs of j's window of a_qc t_jq.  ahead (M,)
        uint32: pair (j, q), j < q, is in the window iff q - j <= ahead[j] (None: min(W, M - 1 - j)); annot (M,) uint64: bit c says the
        marker is in annotation c (None: one column with every marker); C defaults to 1 without annot and to the highest bit used + 1
        with it; adjust: t = r^2 - (1 - r^2) / (N - 2), else r^2."""
        ah = an = None
        if ahead is not None:
            ah = np.ascontiguousarray(ahead, dtype=np.uint32)
            if ah.shape != (self.M,):
                raise ValueError("ahead must be (%d,)" % self.M)
        if annot is not None:
            an = np.ascontiguousarray(annot, dtype=np.uint64)
            if an.shape != (self.M,):
                raise ValueError("annot must be (%d,)" % self.M)
        if C is None:
            C = 1 if an is None else max(1, int(np.bitwise_or.reduce(an)).bit_length())
        out = np.zeros((self.M, max(int(C), 0)))
        check(self.L.hgibbs_ld_scores(self.h, W, ah.ctypes.data_as(C_U32P) if ah is not None else None, C,
                                      an.ctypes.data_as(C_U64P) if an is not None else None, 1 if adjust else 0, _dp(out)))
        return out

    def last_ld_scores_ms(self):
        """(products ms, reduce ms) of the last ld_scores()"""
        a, b = C.c_double(), C.c_double()
        check(self.L.hgibbs_last_ld_scores_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def _ahead(self, ahead):
        if ahead is None:
            return None
        ah = np.ascontiguousarray(ahead, dtype=np.uint32)
        if ah.shape != (self.M,):
            raise ValueError("ahead must be (%d,)" % self.M)
        return ah

    def ld_mask(self, W, t, ahead=None, backward=True):
        """LD masks (hgibbs_ld_mask): fwd, bwd (M, wpr) uint64, wpr = (W + 63) // 64, and the number of passing pairs.  Bit (d - 1) % 64 of
        fwd[j, (d - 1) // 64] says that pair (j, j + d) is in the window (d <= ahead[j]; None: min(W, M - 1 - j)) and has r * r >= t with
        hgibbs_ld's r; bwd[q] holds the same bit for pair (q - d, q).  backward=False: bwd is not computed (None returned)."""
        ah = self._ahead(ahead)
        wpr = (max(int(W), 1) + 63) // 64
        fwd = np.zeros((self.M, wpr), dtype=np.uint64)
        bwd = np.zeros((self.M, wpr), dtype=np.uint64) if backward else None
        n = C.c_uint64(0)
        check(self.L.hgibbs_ld_mask(self.h, W, ah.ctypes.data_as(C_U32P) if ah is not None else None, t, _u64(fwd),
                                    _u64(bwd) if backward else None, C.byref(n)))
        return fwd, bwd, n.value

    def ld_clump(self, W, t, order, may_lead=None, ahead=None):
        """hgibbs_ld_clump: ld_mask, then ld_greedy on its masks.  Returns owner (M,) int32 and the number of passing pairs."""
        ah = self._ahead(ahead)
        od, ml = _order_and_leaders(self.M, order, may_lead)
        owner = np.full(self.M, -1, dtype=np.int32)
        n = C.c_uint64(0)
        check(self.L.hgibbs_ld_clump(self.h, W, ah.ctypes.data_as(C_U32P) if ah is not None else None, t, od.ctypes.data_as(C_U32P), od.size,
                                     _u8(ml) if ml is not None else None, _ip(owner), C.byref(n)))
        return owner, n.value

    def last_ld_mask_ms(self):
        """(products ms, reduce ms) of the last ld_mask() or ld_clump()"""
        a, b = C.c_double(), C.c_double()
        check(self.L.hgibbs_last_ld_mask_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def marker_dots(self, U, m0=0, count=None, raw=False):
        """x_j'u_k for markers j in [m0, m0 + count) against the rows u_k of U (K, n_local) (hgibbs_marker_dots): out (count, K),
        and with raw=True also (count, K, 2) the sums P = sum_called g u, Q = sum_called u, each rounded once."""
        U = np.ascontiguousarray(np.atleast_2d(U), dtype=np.float64)
        if U.shape[1] != self.n_local:
            raise ValueError("U must be (K, %d)" % self.n_local)
        if count is None:
            count = self.M - m0
        K = U.shape[0]
        out = np.zeros((count, K))
        rr = np.zeros((count, K, 2)) if raw else None
        check(self.L.hgibbs_marker_dots(self.h, m0, count, K, _dp(U), _dp(out), _dp(rr) if raw else None))
        return (out, rr) if raw else out

    def last_marker_dots_ms(self):
        v = C.c_double()
        check(self.L.hgibbs_last_marker_dots_ms(self.h, C.byref(v)))
        return v.value

    def marker_class_sums(self, U, m0=0, count=None):
        """Sums of the rows u_k of U (K, n_local) over the individuals of each genotype code, for markers j in [m0, m0 + count)
        (hgibbs_marker_class_sums): out (count, K, 4), codes 0, 1, 2 copies of A1 and 3 a missing call, each rounded once."""
        U = np.ascontiguousarray(np.atleast_2d(U), dtype=np.float64)
        if U.shape[1] != self.n_local:
            raise ValueError("U must be (K, %d)" % self.n_local)
        if count is None:
            count = self.M - m0
        K = U.shape[0]
        out = np.zeros((count, K, 4))
        check(self.L.hgibbs_marker_class_sums(self.h, m0, count, K, _dp(U), _dp(out)))
        return out

    def last_marker_class_sums_ms(self):
        v = C.c_double()
        check(self.L.hgibbs_last_marker_class_sums_ms(self.h, C.byref(v)))
        return v.value

    def set_gram(self, sets, w, raw=False):
        """Row-weighted Gram matrices of marker sets (hgibbs_set_gram): sets is a list of index lists, w (n_local,) the non-negative
        row weights.  Returns a list of (m_s, m_s) arrays sum_i w_i x_ia x_ib, and with raw=True also a list of (m_s, m_s, 3) arrays
        GG, GC, CC, each rounded once.  Option sgram_split: ranges of individuals split over workgroups (0 = automatic)."""
        lists = [np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in sets]
        off = np.zeros(len(lists) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([x.size for x in lists], dtype=np.uint64)
        idx = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), dtype=np.uint32)
        if idx.size == 0:
            idx = np.zeros(1, dtype=np.uint32)
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        if w.size != self.n_local:
            raise ValueError("w must be (%d,)" % self.n_local)
        E = int(sum(int(x.size) ** 2 for x in lists))
        out = np.zeros(max(E, 1))
        rr = np.zeros(max(E, 1) * 3) if raw else None
        check(self.L.hgibbs_set_gram(self.h, len(lists), off.ctypes.data_as(C_U64P), idx.ctypes.data_as(C_U32P), _dp(w), _dp(out),
                                     _dp(rr) if raw else None))
        outs, raws, b = [], [], 0
        for x in lists:
            m = int(x.size)
            outs.append(out[b:b + m * m].reshape(m, m).copy())
            if raw:
                raws.append(rr[3 * b:3 * (b + m * m)].reshape(m, m, 3).copy())
            b += m * m
        return (outs, raws) if raw else outs

    def last_set_gram_ms(self):
        v = C.c_double()
        check(self.L.hgibbs_last_set_gram_ms(self.h, C.byref(v)))
        return v.value

    def _null_list(self, fn, rec, markers, Z, mu, B, xv, s):
        """The arguments that spa_roots and firth_fit share, checked and marshalled for `fn`; returns its nm records of type `rec`."""
        markers = np.ascontiguousarray(markers, dtype=np.uint32).reshape(-1)
        nm = markers.size
        Z = np.asarray(Z, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[0] != self.n_local:
            raise ValueError("Z must be (%d, q)" % self.n_local)
        q = Z.shape[1]
        Zc = np.ascontiguousarray(Z.T)  # column-major
        mu = np.ascontiguousarray(mu, dtype=np.float64).reshape(-1)
        B = np.ascontiguousarray(B, dtype=np.float64).reshape(-1)
        xv = np.ascontiguousarray(xv, dtype=np.float64).reshape(-1)
        s = np.ascontiguousarray(s, dtype=np.float64).reshape(-1)
        if mu.size != self.n_local or B.size != nm * q or xv.size != nm * 4 or s.size != nm:
            raise ValueError("mu must be (%d,), B (%d, %d), xv (%d, 4), s (%d,)" % (self.n_local, nm, q, nm, nm))
        out = (rec * max(nm, 1))()
        check(fn(self.h, nm, markers.ctypes.data_as(C_U32P), q, _dp(Zc), _dp(mu), _dp(B), _dp(xv), _dp(s), out))
        return out

    def spa_roots(self, markers, Z, mu, B, xv, s):
        """The saddlepoints of the logistic score test for a list of markers (hgibbs_spa_roots): Z (n_local, q) and mu (n_local,) of
        the null model, B (nm, q), xv (nm, 4) and s (nm,) per entry.  Returns a ctypes array of nm SpaRoot."""
        return self._null_list(self.L.hgibbs_spa_roots, SpaRoot, markers, Z, mu, B, xv, s)

    def last_spa_ms(self):
        v = C.c_double()
        check(self.L.hgibbs_last_spa_ms(self.h, C.byref(v)))
        return v.value

    def firth_fit(self, markers, Z, mu, B, xv, s):
        """Firth's penalised fit of the score test's one-parameter model for a list of markers (hgibbs_firth_fit): the arguments of
        spa_roots.  Returns a ctypes array of nm FirthRec.  Option firth_piece: entries per piece of the list (0 = automatic)."""
        return self._null_list(self.L.hgibbs_firth_fit, FirthRec, markers, Z, mu, B, xv, s)

    def last_firth_ms(self):
        v = C.c_double()
        check(self.L.hgibbs_last_firth_ms(self.h, C.byref(v)))
        return v.value

    def king(self, a0=0, acount=None, b0=0, bcount=None):
        """KING counts of rows [a0, a0 + acount) x [b0, b0 + bcount) (hgibbs_king): int32 (acount, bcount, 5) with NSNP, HET_a,
        HET_b, HETHET, IBS0."""
        if acount is None:
            acount = self.n_local - a0
        if bcount is None:
            bcount = self.n_local - b0
        out = np.zeros((acount, bcount, 5), dtype=np.int32)
        check(self.L.hgibbs_king(self.h, a0, acount, b0, bcount, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def king_pairs(self, cutoff):
        """Every pair a < b with KINSHIP >= cutoff (hgibbs_king_pairs, then hgibbs_king_pairs_get), sorted by (a, b): ab uint32 (P, 2),
        counts int32 (P, 5), kin float64 (P,)."""
        n = C.c_uint64()
        check(self.L.hgibbs_king_pairs(self.h, float(cutoff), C.byref(n)))
        P = n.value
        ab = np.zeros((P, 2), dtype=np.uint32)
        cnt = np.zeros((P, 5), dtype=np.int32)
        kin = np.zeros(P)
        check(self.L.hgibbs_king_pairs_get(self.h, ab.ctypes.data_as(C.POINTER(C.c_uint32)), cnt.ctypes.data_as(C.POINTER(C.c_int32)), _dp(kin)))
        return ab, cnt, kin

    def last_king_ms(self):
        v = C.c_double()
        check(self.L.hgibbs_last_king_ms(self.h, C.byref(v)))
        return v.value

    def roh(self, run_off, idx, bp, window=50, window_het=1, window_missing=5, threshold=0.05, min_snps=100, min_bp=1000000, dens_bp=50000,
            gap_bp=1000000, max_het=None, need=None):
        """Runs of homozygosity of every row (hgibbs_roh, then hgibbs_roh_get): run r is the entries run_off[r] .. run_off[r + 1] - 1 of
        idx (markers) and bp.  Returns a record array (ROH_SEG: row, first, last, nsnp, nhet, nmiss) sorted by (row, first); first and
        last are positions in idx.  need: the table itself (65 entries) in place of the one roh_need makes of threshold."""
        run_off = np.ascontiguousarray(run_off, dtype=np.uint32)
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        bp = np.ascontiguousarray(bp, dtype=np.int64)
        if run_off.ndim != 1 or run_off.size < 1 or idx.shape != bp.shape or idx.ndim != 1 or idx.size < int(run_off[-1]):
            raise ValueError("run_off needs nruns + 1 entries, idx and bp run_off[-1] each")
        p = RohParams()
        p.window, p.window_het, p.window_missing, p.min_snps = int(window), int(window_het), int(window_missing), int(min_snps)
        p.min_bp, p.dens_bp, p.gap_bp = int(min_bp), int(dens_bp), int(gap_bp)
        p.max_het = 0xFFFFFFFF if max_het is None else int(max_het)
        if need is None:
            need = roh_need(threshold, window) if 1 <= int(window) <= 64 else [0] * 65
        p.need[:] = [int(v) for v in need]
        n = C.c_uint64()
        check(self.L.hgibbs_roh(self.h, run_off.size - 1, run_off.ctypes.data_as(C.POINTER(C.c_uint32)), idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                bp.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(p), C.byref(n)))
        segs = np.zeros(n.value, dtype=ROH_SEG)
        check(self.L.hgibbs_roh_get(self.h, segs.ctypes.data_as(C.c_void_p)))
        return segs

    def last_roh_ms(self):
        v = C.c_double()
        check(self.L.hgibbs_last_roh_ms(self.h, C.byref(v)))
        return v.value

    def _cls(self, cls):
        if cls is None:
            return None
        cls = np.ascontiguousarray(cls, dtype=np.uint8).reshape(-1)
        if cls.size != self.n_local:
            raise ValueError("cls must be (%d,)" % self.n_local)
        return cls

    def pair_tables(self, idxA, idxB, cls=None):
        """The 3 x 3 tables of stored codes of every pair of a marker of idxA with one of idxB, per class of rows
        (hgibbs_pair_tables): int32 (na, nb, 2, 3, 3), [a, b, k, i, j] = rows of class k with code i at idxA[a] and code j at idxB[b];
        cls (n_local,) of 0 / 1, None = every row class 0.  Option ptab_split: ranges of individuals split over workgroups."""
        A = np.ascontiguousarray(idxA, dtype=np.uint32).reshape(-1)
        B = np.ascontiguousarray(idxB, dtype=np.uint32).reshape(-1)
        cls = self._cls(cls)
        out = np.zeros((A.size, B.size, 2, 3, 3), dtype=np.int32)
        pad = np.zeros(1, dtype=np.uint32)  # (an empty list still needs an address: the call refuses it by name)
        check(self.L.hgibbs_pair_tables(self.h, A.size, (A if A.size else pad).ctypes.data_as(C_U32P), B.size, (B if B.size else pad).ctypes.data_as(C_U32P),
                                        _u8(cls) if cls is not None else None, _ip(out) if out.size else _ip(np.zeros(1, dtype=np.int32))))
        return out

    def last_pair_tables_ms(self):
        v = C.c_double()
        check(self.L.hgibbs_last_pair_tables_ms(self.h, C.byref(v)))
        return v.value

    def epi_scan(self, idxA, idxB, cls, threshold):
        """BOOST's screen on the device (hgibbs_epi_scan, then hgibbs_epi_scan_get): every pair of a marker of idxA with one of idxB
        (idxB None: the pairs a < b of idxA) whose Kirkwood bound reaches threshold (less the rounding slack), sorted by (a, b).  Returns
        ab uint32 (P, 2) the positions in the lists, tables int32 (P, 2, 3, 3), ksa float64 (P,) the device's values."""
        A = np.ascontiguousarray(idxA, dtype=np.uint32).reshape(-1)
        B = None if idxB is None else np.ascontiguousarray(idxB, dtype=np.uint32).reshape(-1)
        cls = self._cls(cls)
        pad = np.zeros(1, dtype=np.uint32)
        n = C.c_uint64()
        check(self.L.hgibbs_epi_scan(self.h, A.size, (A if A.size else pad).ctypes.data_as(C_U32P), 0 if B is None else B.size,
                                     None if B is None else (B if B.size else pad).ctypes.data_as(C_U32P), _u8(cls) if cls is not None else None,
                                     float(threshold), C.byref(n)))
        P = n.value
        ab = np.zeros((P, 2), dtype=np.uint32)
        tab = np.zeros((P, 2, 3, 3), dtype=np.int32)
        ksa = np.zeros(P)
        check(self.L.hgibbs_epi_scan_get(self.h, ab.ctypes.data_as(C.POINTER(C.c_uint32)), _ip(tab), _dp(ksa)))
        return ab, tab, ksa

    def last_epi_ms(self):
        """(products ms, screen ms) of the last epi_scan"""
        a, b = C.c_double(), C.c_double()
        check(self.L.hgibbs_last_epi_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def grm(self, a0=0, acount=None):
        """S = X X' and NSNP of rows [a0, a0 + acount), each with its columns 0 .. a (hgibbs_grm): packed 1-D arrays in GCTA's order,
        float64 S and int32 nsnp; the GCTA entry is S / nsnp."""
        if acount is None:
            acount = self.n_local - a0
        n = sum(a + 1 for a in range(a0, a0 + acount))
        S = np.zeros(n)
        nsnp = np.zeros(n, dtype=np.int32)
        check(self.L.hgibbs_grm(self.h, a0, acount, _dp(S), nsnp.ctypes.data_as(C.POINTER(C.c_int32))))
        return S, nsnp

    def grm_info(self):
        """(M_used, E) of the last grm()"""
        m, e = C.c_uint32(), C.c_int32()
        check(self.L.hgibbs_grm_info(self.h, C.byref(m), C.byref(e)))
        return m.value, e.value

    def last_grm_ms(self):
        v = C.c_double()
        check(self.L.hgibbs_last_grm_ms(self.h, C.byref(v)))
        return v.value

    def grm_rowsums(self, Y):
        """Row sums of the relationship matrix over each row's partners (hgibbs_grm_rowsums): Y (P, n_local) or (n_local,).  Returns
        ay (n_local, P) = A Y', a1 and a2 (n_local,) = the sums of A and of A^2, diag (n_local,) and partners (n_local,) uint32."""
        Y = np.ascontiguousarray(np.atleast_2d(np.asarray(Y, dtype=np.float64)))
        P, n = Y.shape[0], self.n_local
        if Y.ndim != 2 or (P and n and Y.shape[1] != n):
            raise ValueError("Y must be (P, %d)" % n)
        ay = np.zeros((n, P))
        a1, a2, diag = np.zeros(n), np.zeros(n), np.zeros(n)
        partners = np.zeros(n, dtype=np.uint32)
        check(self.L.hgibbs_grm_rowsums(self.h, P, _dp(Y), _dp(ay), _dp(a1), _dp(a2), _dp(diag), partners.ctypes.data_as(C_U32P)))
        return ay, a1, a2, diag, partners

    def last_grm_rowsums_ms(self):
        """(products ms, reduce ms) of the last grm_rowsums()"""
        a, b = C.c_double(), C.c_double()
        check(self.L.hgibbs_last_grm_rowsums_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def pca(self, K, L=None, iters=20, tol=1e-10, Q0=None, seed=1, loadings=False):
        """The top K principal components of the loaded rows (hgibbs_pca): eigenvalues (K,), PCs (K, n_local), loadings (K, M) or None,
        and the report as a dict (iters_run, m_used, ritz_change, resid (K,)).  L is the panel width (default: the smallest multiple
        of 8 that is >= K + 8, at most 32); Q0 (L, n_local) replaces the seeded start panel."""
        if L is None:
            L = min(32, (K + 8 + 7) // 8 * 8)
        q = None
        if Q0 is not None:
            q = np.ascontiguousarray(Q0, dtype=np.float64)
            if q.shape != (L, self.n_local):
                raise ValueError("Q0 must be (%d, %d)" % (L, self.n_local))
        kk = max(int(K), 0)
        val = np.zeros(kk)
        pcs = np.zeros((kk, self.n_local))
        ld = np.zeros((kk, self.M)) if loadings else None
        rep = PcaReport()
        check(self.L.hgibbs_pca(self.h, int(K), int(L), int(iters), float(tol), _dp(q) if q is not None else None, int(seed) & (2 ** 64 - 1),
                                _dp(val), _dp(pcs), _dp(ld) if loadings else None, C.byref(rep)))
        return val, pcs, ld, {"iters_run": rep.iters_run, "m_used": rep.m_used, "ritz_change": rep.ritz_change,
                              "resid": np.array(rep.resid[:kk], dtype=np.float64)}

    def _reml_z(self, Z):
        """the design (n_local, q), the column of ones included, as the q x n_local the library takes"""
        z = np.asarray(Z, dtype=np.float64)
        if z.ndim != 2 or z.shape[0] != self.n_local:
            raise ValueError("Z must be (%d, q)" % self.n_local)
        return np.ascontiguousarray(z.T)

    def reml_solve(self, B, Z, delta, tol=1e-5, max_iters=200):
        """hgibbs_reml_solve: V[k] = H(delta)^-1 P_c B[k] for the K rows of B (K, n_local) by conjugate gradients, H = P_c A P_c +
        delta I with A = X X'/M_used and P_c the projection off the columns of Z (n_local, q).  Returns V (K, n_local), the iterations
        (K,) and the recurrence's relative residuals (K,)."""
        b = np.ascontiguousarray(B, dtype=np.float64)
        if b.ndim != 2 or b.shape[1] != self.n_local:
            raise ValueError("B must be (K, %d)" % self.n_local)
        z = self._reml_z(Z)
        K = b.shape[0]
        V = np.zeros((K, self.n_local))
        iters = np.zeros(max(K, 1), dtype=np.intc)
        rel = np.zeros(max(K, 1))
        check(self.L.hgibbs_reml_solve(self.h, K, z.shape[0], _dp(z), float(delta), float(tol), int(max_iters), _dp(b), _dp(V),
                                       iters.ctypes.data_as(C.POINTER(C.c_int)), _dp(rel)))
        return V, iters[:K].astype(np.int64), rel[:K]

    def reml_eval(self, y, Z, delta, trials=15, seed=1, tol=1e-5, max_iters=200):
        """hgibbs_reml_eval: the sums (trials + 1, 3) of vAv, vv, vb at delta from `trials` sign probes and y, and the largest
        iteration count of the solve."""
        z = self._reml_z(Z)
        yy = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        if yy.size != self.n_local:
            raise ValueError("y must have %d entries" % self.n_local)
        T = int(trials)
        sums = np.zeros((max(T, 0) + 1, 3))
        it = C.c_int()
        check(self.L.hgibbs_reml_eval(self.h, T, z.shape[0], _dp(z), _dp(yy), int(seed) & (2 ** 64 - 1), float(delta), float(tol), int(max_iters),
                                      _dp(sums), C.byref(it)))
        return sums, it.value

    def reml(self, y, Z, trials=15, h2_start=0.25, cg_tol=1e-5, cg_iters=200, x_tol=0.01, max_steps=12, seed=1, blup=False):
        """hgibbs_reml: the REML estimate of h2 of the loaded rows without the relationship matrix.  Returns a dict: status (a
        REML_* value), steps, the trace x, f, cg_iters (steps,), sums_prev and sums_last (trials + 1, 3), ai3, ai_cg_iters, the
        estimate's fields (logdelta, delta, vg, ve, vp, h2, se_*), n, m_used, q, trials, products_ms, algebra_ms, and blup (M,) or None."""
        z = self._reml_z(Z)
        yy = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        if yy.size != self.n_local:
            raise ValueError("y must have %d entries" % self.n_local)
        opt = RemlOpts(int(trials), float(h2_start), float(cg_tol), int(cg_iters), float(x_tol), int(max_steps), int(seed) & (2 ** 64 - 1))
        res = RemlResult()
        bl = np.zeros(self.M) if blup else None
        check(self.L.hgibbs_reml(self.h, C.byref(opt), z.shape[0], _dp(z), _dp(yy), C.byref(res), _dp(bl) if blup else None))
        k, T1 = res.steps, res.trials + 1
        out = {"status": res.status, "steps": k, "x": np.array(res.x[:k]), "f": np.array(res.f[:k]), "cg_iters": np.array(res.cg_iters[:k], dtype=np.int64),
               "sums_prev": np.array(res.sums_prev[:3 * T1]).reshape(T1, 3), "sums_last": np.array(res.sums_last[:3 * T1]).reshape(T1, 3),
               "ai3": np.array(res.ai3[:3]), "ai_cg_iters": res.ai_cg_iters, "n": res.n, "m_used": res.m_used, "q": res.q, "trials": res.trials,
               "products_ms": res.products_ms, "algebra_ms": res.algebra_ms, "blup": bl}
        out.update({k2: getattr(res.est, k2) for k2, _ in RemlEstimate._fields_})
        return out

    def last_reml_ms(self):
        """(products ms, algebra ms) of the last reml_solve() / reml_eval() / reml()"""
        a, b = C.c_double(), C.c_double()
        check(self.L.hgibbs_last_reml_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_pca_ms(self):
        """Device ms of the last pca(): whole call, X'Q products, X T products, panel algebra of the iterations."""
        v = (C.c_double * 4)()
        check(self.L.hgibbs_last_pca_ms(self.h, v))
        return [v[i] for i in range(4)]

    def debug_times(self):
        """The 48 stage-timestamp words of the sweep kernel's debug build (option debug_timing; 100 MHz ticks, accumulated
        over the launches since the last call, which clears them); layout in hg_sweep.hip.h (sweep_draw_phase)."""
        t = (C.c_uint64 * 48)()
        check(self.L.hgibbs_debug_times(self.h, t))
        return [int(x) for x in t]

    def sweep(self, order, sigmaE, sigmaG, estPi, adaV, rng):
        """rng: RngState, updated in place.  Returns (cass[G,K], nnz_updates)."""
        order = np.ascontiguousarray(order, dtype=np.int32)
        sigmaG = np.ascontiguousarray(sigmaG, dtype=np.float64)
        estPi = np.ascontiguousarray(estPi, dtype=np.float64)
        adaV = np.ascontiguousarray(adaV, dtype=np.uint8)
        cass = np.zeros((self.G, self.K), dtype=np.int32)
        nnz = C.c_uint64()
        check(self.L.hgibbs_sweep(self.h, _ip(order), float(sigmaE), _dp(sigmaG), _dp(estPi), _u8(adaV), C.byref(rng),
                                  _ip(cass), C.byref(nnz)))
        return cass, nnz.value

    def ss_begin(self, n_eff, W, xty, ahead=None):
        """hgibbs_ss_begin: the band of the loaded panel on the device, c = xty, every effect 0.  ahead (M,) or None."""
        xty = np.ascontiguousarray(xty, dtype=np.float64)
        if xty.shape != (self.M,):
            raise ValueError("ss_begin: xty must have M entries")
        ah = None if ahead is None else np.ascontiguousarray(ahead, dtype=np.uint32)
        if ah is not None and ah.shape != (self.M,):
            raise ValueError("ss_begin: ahead must have M entries")
        check(self.L.hgibbs_ss_begin(self.h, float(n_eff), W, ah.ctypes.data_as(C_U32P) if ah is not None else None, _dp(xty)))
        self.ss_W = W

    def ss_sweep(self, order, sigmaE, sigmaG, estPi, adaV, rng):
        """hgibbs_ss_sweep; rng: RngState, updated in place.  Returns (cass[G,K], nnz_updates)."""
        order = np.ascontiguousarray(order, dtype=np.int32)
        sigmaG = np.ascontiguousarray(sigmaG, dtype=np.float64)
        estPi = np.ascontiguousarray(estPi, dtype=np.float64)
        adaV = np.ascontiguousarray(adaV, dtype=np.uint8)
        if order.shape != (self.M,) or adaV.shape != (self.M,):
            raise ValueError("ss_sweep: order and adaV must have M entries")
        cass = np.zeros((self.G, self.K), dtype=np.int32)
        nnz = C.c_uint64()
        check(self.L.hgibbs_ss_sweep(self.h, _ip(order), float(sigmaE), _dp(sigmaG), _dp(estPi), _u8(adaV), C.byref(rng), _ip(cass), C.byref(nnz)))
        return cass, nnz.value

    def ss_sweep_streams(self, order, sigmaE, sigmaG, estPi, adaV, bounds, rngs, S=None):
        """hgibbs_ss_sweep_streams: ss_sweep with one workgroup per interval of `bounds` (S + 1); rngs: a list of S RngState, updated in
        place.  Returns (cass[G,K], nnz_updates)."""
        order = np.ascontiguousarray(order, dtype=np.int32)
        sigmaG = np.ascontiguousarray(sigmaG, dtype=np.float64)
        estPi = np.ascontiguousarray(estPi, dtype=np.float64)
        adaV = np.ascontiguousarray(adaV, dtype=np.uint8)
        bounds = np.ascontiguousarray(bounds, dtype=np.uint32)
        if order.shape != (self.M,) or adaV.shape != (self.M,):
            raise ValueError("ss_sweep_streams: order and adaV must have M entries")
        S = bounds.shape[0] - 1 if S is None else S
        ra = _RngArray(rngs)
        cass = np.zeros((self.G, self.K), dtype=np.int32)
        nnz = C.c_uint64()
        check(self.L.hgibbs_ss_sweep_streams(self.h, _ip(order), float(sigmaE), _dp(sigmaG), _dp(estPi), _u8(adaV), S, bounds.ctypes.data_as(C_U32P),
                                             ra.arr, _ip(cass), C.byref(nnz)))
        ra.back()
        return cass, nnz.value

    def ss_state(self):
        """hgibbs_ss_state: (c, sum beta_j b_j, sum beta_j c_j)."""
        c = np.zeros(self.M)
        sb, sc = C.c_double(), C.c_double()
        check(self.L.hgibbs_ss_state(self.h, _dp(c), C.byref(sb), C.byref(sc)))
        return c, sb.value, sc.value

    def ss_band(self, m0=0, count=None):
        """hgibbs_ss_band_get: (count, W) float64, out[j - m0, d - 1] = (n_eff - 1) r(j, j + d), 0 outside the window."""
        count = self.M - m0 if count is None else count
        out = np.zeros((count, self.ss_W))
        check(self.L.hgibbs_ss_band_get(self.h, m0, count, _dp(out)))
        return out

    def ss_replicas(self, R):
        """hgibbs_ss_replicas: R chains' state beside the handle's own, c = xty and every effect 0."""
        check(self.L.hgibbs_ss_replicas(self.h, int(R) & 0xffffffff))

    def ss_sweep_replicas(self, orders, sigmaE, sigmaG, estPi, adaV, rngs, bounds=None, R=None, S=None):
        """hgibbs_ss_sweep_replicas: one launch for R replicas x S intervals.  orders (R, M); sigmaE (R,); sigmaG (R, G); estPi
        (R, G, K); adaV (M,) for every replica or (R, M); bounds (S + 1) or None for the single stream; rngs: a list of R lists of S
        RngState (or R RngState for the single stream), updated in place.  Returns (cass[R, G, K], nnz[R])."""
        orders = np.ascontiguousarray(orders, dtype=np.int32)
        R = orders.shape[0] if R is None else R
        n = max(R, 1)
        sigmaE = np.ascontiguousarray(sigmaE, dtype=np.float64)
        sigmaG = np.ascontiguousarray(sigmaG, dtype=np.float64)
        estPi = np.ascontiguousarray(estPi, dtype=np.float64)
        adaV = np.ascontiguousarray(adaV, dtype=np.uint8)
        if adaV.ndim == 1:
            adaV = np.ascontiguousarray(np.broadcast_to(adaV, (orders.shape[0], adaV.shape[0])))
        if orders.ndim != 2 or orders.shape[1] != self.M or adaV.shape != orders.shape:
            raise ValueError("ss_sweep_replicas: orders must be (R, M), adaV (M,) or (R, M)")
        # (an R the library refuses before it reads anything goes through as it is: the refusal is the library's)
        if 1 <= R <= 64 and (sigmaE.size < R or sigmaG.size < R * self.G or estPi.size < R * self.G * self.K or orders.shape[0] < R):
            raise ValueError("ss_sweep_replicas: sigmaE, sigmaG, estPi and orders must hold R replicas")
        bounds = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.uint32)
        S = (1 if bounds is None else bounds.shape[0] - 1) if S is None else S
        flat = [r for row in rngs for r in (row if isinstance(row, (list, tuple)) else [row])]
        if 1 <= R <= 64 and 1 <= S <= 1024 and len(flat) < R * S:
            raise ValueError("ss_sweep_replicas: rngs must hold R x S generators")
        ra = _RngArray(flat)
        cass = np.zeros((n, self.G, self.K), dtype=np.int32)
        nnz = np.zeros(n, dtype=np.uint64)
        check(self.L.hgibbs_ss_sweep_replicas(self.h, R, _ip(orders), _dp(sigmaE), _dp(sigmaG), _dp(estPi), _u8(adaV), S,
                                              bounds.ctypes.data_as(C_U32P) if bounds is not None else None, ra.arr, _ip(cass),
                                              nnz.ctypes.data_as(C.POINTER(C.c_uint64))))
        ra.back()
        return cass, nnz

    def ss_replica_sums(self, R):
        """hgibbs_ss_replica_sums: (sb[R], sc[R], bsq[R, G]) of the R allocated replicas."""
        sb, sc, bsq = np.zeros(R), np.zeros(R), np.zeros((R, self.G))
        check(self.L.hgibbs_ss_replica_sums(self.h, _dp(sb), _dp(sc), _dp(bsq)))
        return sb, sc, bsq

    def ss_replica_get(self, r):
        """hgibbs_ss_replica_get: (beta, components, acum, c) of replica r."""
        beta, acum, c = np.zeros(self.M), np.zeros(self.M), np.zeros(self.M)
        comp = np.zeros(self.M, dtype=np.int32)
        check(self.L.hgibbs_ss_replica_get(self.h, int(r) & 0xffffffff, _dp(beta), _ip(comp), _dp(acum), _dp(c)))
        return beta, comp, acum, c

    def ss_replica_set_beta(self, r, beta):
        """hgibbs_ss_replica_set_beta: replica r's effects alone (c stays as it is)."""
        beta = np.ascontiguousarray(beta, dtype=np.float64)
        if beta.shape != (self.M,):
            raise ValueError("ss_replica_set_beta: beta must have M entries")
        check(self.L.hgibbs_ss_replica_set_beta(self.h, int(r) & 0xffffffff, _dp(beta)))

    def ss_post_begin(self, R, T):
        """hgibbs_ss_post_begin: per-marker accumulators over T planned records of the R allocated replicas (R = 0: the handle's own chain)."""
        check(self.L.hgibbs_ss_post_begin(self.h, int(R) & 0xffffffff, int(T) & 0xffffffff))

    def ss_post_add(self):
        """hgibbs_ss_post_add: folds the chains' effects and components as they stand into the accumulators (one record)."""
        check(self.L.hgibbs_ss_post_add(self.h))

    def ss_post_get(self):
        """hgibbs_ss_post_get, after the last planned record: (mean[M], sd[M], pip[M], cnt[K, M] uint32, rhat[M])."""
        mean, sd, pip, rhat = np.zeros(self.M), np.zeros(self.M), np.zeros(self.M), np.zeros(self.M)
        cnt = np.zeros((self.K, self.M), dtype=np.uint32)
        check(self.L.hgibbs_ss_post_get(self.h, _dp(mean), _dp(sd), _dp(pip), cnt.ctypes.data_as(C_U32P), _dp(rhat)))
        return mean, sd, pip, cnt, rhat

    def ss_post_raw(self, r, half):
        """hgibbs_ss_post_raw: the Welford pair (mean[M], m2[M]) of half `half` of chain r; r = the number of chains, half = 0: the pooled pair."""
        hmean, hm2 = np.zeros(self.M), np.zeros(self.M)
        check(self.L.hgibbs_ss_post_raw(self.h, int(r) & 0xffffffff, int(half) & 0xffffffff, _dp(hmean), _dp(hm2)))
        return hmean, hm2

    def ss_post_end(self):
        check(self.L.hgibbs_ss_post_end(self.h))

    def last_ss_post_ms(self):
        """(add_ms, final_ms): device time of every ss_post_add since ss_post_begin (their sum) and of ss_post_get's kernel."""
        a, b = C.c_double(), C.c_double()
        check(self.L.hgibbs_last_ss_post_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def cs_begin(self, C_, T):
        """hgibbs_cs_begin: the inclusion history of C_ chains x T planned records, one bit per marker and record, zeroed."""
        check(self.L.hgibbs_cs_begin(self.h, int(C_) & 0xffffffff, int(T) & 0xffffffff))
        self._cs_shape = (int(C_), int(T))

    def cs_add_flags(self, flags):
        """hgibbs_cs_add_flags: one record of every chain from flags (C, M) bytes, non-zero = in the model."""
        C_ = self._cs_shape[0]
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        if fl.size != C_ * self.M:
            raise ValueError("flags must be (%d, %d)" % (C_, self.M))
        check(self.L.hgibbs_cs_add_flags(self.h, _u8(fl)))

    def ss_cs_add(self, R):
        """hgibbs_ss_cs_add: one record of every chain from the ss chains' components as they stand (R = 0: the handle's own chain)."""
        check(self.L.hgibbs_ss_cs_add(self.h, int(R) & 0xffffffff))

    def cs_counts(self):
        """hgibbs_cs_counts: cnt (M,) uint32, the records added so far in which the marker is in the model."""
        cnt = np.zeros(self.M, dtype=np.uint32)
        check(self.L.hgibbs_cs_counts(self.h, _u32(cnt)))
        return cnt

    def cs_history(self):
        """hgibbs_cs_history: the words (NW, M) uint64, NW = (C T + 63) // 64; bit q % 64 of word [q // 64, j] is marker j in record q."""
        C_, T = self._cs_shape
        out = np.zeros(((C_ * T + 63) // 64, self.M), dtype=np.uint64)
        check(self.L.hgibbs_cs_history(self.h, _u64(out)))
        return out

    def cs_sets(self, W, fwd, bwd, leads, need, max_size):
        """hgibbs_cs_sets: the candidate set of every lead on masks in ld_mask's layout.  Returns status, size (nlead,) uint32, sum
        (nlead,) uint64, pep (nlead,) uint32 and members (nlead, max_size) uint32 (0xFFFFFFFF in the unused slots)."""
        wpr = (max(int(W), 1) + 63) // 64
        fwd = np.ascontiguousarray(fwd, dtype=np.uint64)
        bwd = np.ascontiguousarray(bwd, dtype=np.uint64)
        if 1 <= W <= 4096 and (fwd.shape != (self.M, wpr) or bwd.shape != (self.M, wpr)):
            raise ValueError("fwd and bwd must be (%d, %d)" % (self.M, wpr))
        ld = np.ascontiguousarray(leads, dtype=np.uint32).reshape(-1)
        n, ms = ld.size, max_size if 1 <= max_size <= 256 else 1
        status, size, pep = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        total = np.zeros(max(n, 1), dtype=np.uint64)
        members = np.zeros((max(n, 1), ms), dtype=np.uint32)
        check(self.L.hgibbs_cs_sets(self.h, W, _u64(fwd), _u64(bwd), n, _u32(ld), int(need) & 0xffffffff, int(max_size) & 0xffffffff, _u32(status), _u32(size),
                                    _u64(total), _u32(pep), _u32(members)))
        return status[:n], size[:n], total[:n], pep[:n], members[:n]

    def cs_end(self):
        check(self.L.hgibbs_cs_end(self.h))

    def last_cs_ms(self):
        """(add_ms, counts_ms, sets_ms): device time of every add since cs_begin (their sum), of the last counts kernel, of the last sets kernel."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(self.L.hgibbs_last_cs_ms(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def ss_end(self):
        check(self.L.hgibbs_ss_end(self.h))

    def last_ss_ms(self):
        """(band_ms, sweep_ms): device time of ss_begin's band and of the last ss_sweep's kernel."""
        a, b = C.c_double(), C.c_double()
        check(self.L.hgibbs_last_ss_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def resident_trace(self):
        out = np.zeros((10, 4096), dtype=np.uint64)
        check(self.L.hgibbs_resident_trace(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size))
        return out

    def sweep_stats(self):
        s = SweepStats()
        check(self.L.hgibbs_last_sweep_stats(self.h, C.byref(s)))
        return {"launches": s.launches, "nnz_updates": s.nnz_updates, "device_ms": s.device_ms,
                "kernel_ms_avg": s.kernel_ms_avg, "carried_columns": s.carried_columns, "working_launches": s.working_launches,
                "accepted_markers": s.accepted_markers, "streamed_columns": s.streamed_columns,
                "tiles_per_workgroup_min": s.tiles_per_workgroup_min, "tiles_per_workgroup_max": s.tiles_per_workgroup_max,
                "engine": s.engine, "walker": s.walker, "refill": s.refill, "eps_sum_drift": s.eps_sum_drift, "rounds": s.rounds, "events": s.events,
                "advances": s.advances, "chunks": s.chunks, "refolds": s.refolds, "pivots": s.pivots, "predicted": s.predicted, "turned_down": s.turned_down, "shader_mhz": s.shader_mhz, "ticks": list(s.ticks)}


class Chain:
    """hydra_chain_t: the runMpiGibbs body on top of a loaded Device."""

    def __init__(self, dev, y, mS=None, groups=None, seed=1222, shuffle=1):
        self.dev = dev
        self.L = dev.L
        if mS is None:
            mS = np.array([[0.0, 0.0001, 0.001, 0.01]])
        self.mS = np.ascontiguousarray(mS, dtype=np.float64)
        self.G, self.K = self.mS.shape
        self.groups = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
        y = np.ascontiguousarray(y, dtype=np.float64)
        assert y.shape[0] == dev.n_global
        d = ModelDesc(seed, shuffle, self.G, self.K, _ip(self.groups) if self.groups is not None else None, _dp(self.mS))
        self.h = C.c_void_p()
        check(self.L.hydra_chain_create(dev.h, C.byref(d), _dp(y), C.byref(self.h)))
        dev.G, dev.K = self.G, self.K

    def __del__(self):
        try:
            if self.h:
                self.L.hydra_chain_destroy(self.h)
        except Exception:
            pass

    def set_covariates(self, X):
        X = np.ascontiguousarray(X, dtype=np.float64)
        assert X.shape[0] == self.dev.n_global
        self.C = X.shape[1]
        check(self.L.hydra_chain_set_covariates(self.h, _dp(X), self.C))

    def gamma(self):
        g, xi = np.zeros(self.C), np.zeros(self.C, dtype=np.int32)
        check(self.L.hydra_chain_gamma(self.h, _dp(g), _ip(xi)))
        return g, xi

    def iterate(self):
        check(self.L.hydra_chain_iterate(self.h))

    def state(self):
        G, K = self.G, self.K
        sE, mu = C.c_double(), C.c_double()
        sG, pi = np.zeros(G), np.zeros((G, K))
        m0, cass = np.zeros(G, dtype=np.int32), np.zeros((G, K), dtype=np.int32)
        rng = RngState()
        check(self.L.hydra_chain_state(self.h, C.byref(sE), C.byref(mu), _dp(sG), _dp(pi), _ip(m0), _ip(cass), C.byref(rng)))
        return {"sigmaE": sE.value, "mu": mu.value, "sigmaG": sG, "estPi": pi, "m0": m0, "cass": cass,
                "rng_x": np.array(rng.x, dtype=np.uint32), "rng_idx": int(rng.idx)}

    def order(self):
        return np.ctypeslib.as_array(self.L.hydra_chain_order(self.h), shape=(self.dev.M,)).copy()

    def rng_words(self):
        """dist.rng in Boost's stream form (what hydra's .rng.<rank> holds)."""
        rng = RngState()
        check(self.L.hydra_chain_state(self.h, None, None, None, None, None, None, C.byref(rng)))
        out = np.zeros(624, dtype=np.uint32)
        check(self.L.hydra_rng_to_boost_words(C.byref(rng), out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def restore(self, iteration, sigmaE, mu, sigmaG, estPi, beta, components, eps, order, rng_words, gamma=None, xI=None):
        """init_from_restart: eps = this rank's rows; the chain continues at iteration + 1."""
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        keep = [f64(sigmaG), f64(estPi), f64(beta), i32(components), f64(eps), i32(order)]
        st = RestartState()
        st.iteration, st.sigmaE, st.mu = iteration, sigmaE, mu
        st.sigmaG, st.estPi, st.beta = _dp(keep[0]), _dp(keep[1]), _dp(keep[2])
        st.components, st.eps, st.order = _ip(keep[3]), _dp(keep[4]), _ip(keep[5])
        if gamma is not None:
            keep += [f64(gamma), i32(xI)]
            st.gamma, st.xI = _dp(keep[6]), _ip(keep[7])
        w = np.ascontiguousarray(rng_words, dtype=np.uint32)
        check(self.L.hydra_rng_from_boost_words(w.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(st.rng)))
        check(self.L.hydra_chain_restore(self.h, C.byref(st)))

    def last_nnz(self):
        return int(self.L.hydra_chain_last_nnz(self.h))

    def csv_line(self, it):
        buf = C.create_string_buffer(50000)
        n = self.L.hydra_chain_csv_line(self.h, it, buf, 50000)
        return buf.raw[:n].decode()


class SsChain:
    """hydra_ss_chain_t: hydra_chain's iteration from summary statistics.  dev: a Device that holds the panel (the device engine), or
    None with `band` (M, W) for the host engine, which needs no device."""

    def __init__(self, dev, n_eff, W, xty, ahead=None, band=None, use=None, mS=None, groups=None, seed=1222, shuffle=1, streams=None):
        self.dev = dev
        self.L = lib()
        if mS is None:
            mS = np.array([[0.0, 0.0001, 0.001, 0.01]])
        self.mS = np.ascontiguousarray(mS, dtype=np.float64)
        self.G, self.K = self.mS.shape
        self.groups = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
        xty = np.ascontiguousarray(xty, dtype=np.float64)
        self.M = xty.shape[0]
        use = None if use is None else np.ascontiguousarray(use, dtype=np.uint8)
        d = ModelDesc(seed, shuffle, self.G, self.K, _ip(self.groups) if self.groups is not None else None, _dp(self.mS))
        self.h = C.c_void_p()
        if dev is not None:
            assert self.M == dev.M
            ah = None if ahead is None else np.ascontiguousarray(ahead, dtype=np.uint32)
            check(self.L.hydra_ss_chain_create(dev.h, C.byref(d), float(n_eff), W, ah.ctypes.data_as(C_U32P) if ah is not None else None, _dp(xty),
                                               _u8(use) if use is not None else None, C.byref(self.h)))
            dev.G, dev.K, dev.ss_W = self.G, self.K, W
        else:
            band = np.ascontiguousarray(band, dtype=np.float64)
            assert band.shape == (self.M, W)
            ah = ss_ahead(self.M, W, ahead)
            check(self.L.hydra_ss_chain_create_host(self.M, C.byref(d), float(n_eff), W, ah.ctypes.data_as(C_U32P), _dp(band), _dp(xty),
                                                    _u8(use) if use is not None else None, C.byref(self.h)))
        if streams is not None:
            self.set_streams(streams)

    def set_streams(self, S_max):
        """hydra_ss_chain_set_streams: independent LD blocks in at most S_max parallel streams; before the first iteration only."""
        check(self.L.hydra_ss_chain_set_streams(self.h, int(S_max) & 0xffffffff))

    def streams(self):
        """hydra_ss_chain_streams: (bounds (S + 1,) uint32, [RngState] * S); (empty, []) for the single stream."""
        S = C.c_uint32()
        check(self.L.hydra_ss_chain_streams(self.h, C.byref(S), None, None))
        if S.value == 0:
            return np.zeros(0, dtype=np.uint32), []
        bounds = np.zeros(S.value + 1, dtype=np.uint32)
        ra = _RngArray([RngState() for _ in range(S.value)])
        check(self.L.hydra_ss_chain_streams(self.h, None, bounds.ctypes.data_as(C_U32P), ra.arr))
        ra.back()
        return bounds, ra.rngs

    def __del__(self):
        try:
            if self.h:
                self.L.hydra_ss_chain_destroy(self.h)
        except Exception:
            pass

    def iterate(self):
        check(self.L.hydra_ss_chain_iterate(self.h))

    def state(self):
        G, K = self.G, self.K
        sE, mu = C.c_double(), C.c_double()
        sG, pi = np.zeros(G), np.zeros((G, K))
        m0, cass = np.zeros(G, dtype=np.int32), np.zeros((G, K), dtype=np.int32)
        rng = RngState()
        check(self.L.hydra_ss_chain_state(self.h, C.byref(sE), C.byref(mu), _dp(sG), _dp(pi), _ip(m0), _ip(cass), C.byref(rng)))
        return {"sigmaE": sE.value, "mu": mu.value, "sigmaG": sG, "estPi": pi, "m0": m0, "cass": cass,
                "rng_x": np.array(rng.x, dtype=np.uint32), "rng_idx": int(rng.idx)}

    def effects(self):
        """(beta, components, acum, c)"""
        beta, acum, c = np.zeros(self.M), np.zeros(self.M), np.zeros(self.M)
        comp = np.zeros(self.M, dtype=np.int32)
        check(self.L.hydra_ss_chain_effects(self.h, _dp(beta), _ip(comp), _dp(acum), _dp(c)))
        return beta, comp, acum, c

    def order(self):
        return np.ctypeslib.as_array(self.L.hydra_ss_chain_order(self.h), shape=(self.M,)).copy()

    def last_nnz(self):
        return int(self.L.hydra_ss_chain_last_nnz(self.h))

    def csv_line(self, it):
        buf = C.create_string_buffer(50000)
        n = self.L.hydra_ss_chain_csv_line(self.h, it, buf, 50000)
        return buf.raw[:n].decode()


class SsMultiChain:
    """hydra_ss_multi_t: R chains from `seeds` on the one band of `dev`, one sweep launch per iteration; chain r is the SsChain with
    seed = seeds[r] (and the same streams) bit for bit."""

    def __init__(self, dev, n_eff, W, xty, seeds, ahead=None, use=None, mS=None, groups=None, shuffle=1, streams=None):
        self.dev = dev
        self.L = lib()
        if mS is None:
            mS = np.array([[0.0, 0.0001, 0.001, 0.01]])
        self.mS = np.ascontiguousarray(mS, dtype=np.float64)
        self.G, self.K = self.mS.shape
        self.groups = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
        xty = np.ascontiguousarray(xty, dtype=np.float64)
        self.M = xty.shape[0]
        assert self.M == dev.M
        use = None if use is None else np.ascontiguousarray(use, dtype=np.uint8)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        self.R = seeds.shape[0]
        ah = None if ahead is None else np.ascontiguousarray(ahead, dtype=np.uint32)
        d = ModelDesc(0, shuffle, self.G, self.K, _ip(self.groups) if self.groups is not None else None, _dp(self.mS))
        self.h = C.c_void_p()
        check(self.L.hydra_ss_multi_create(dev.h, C.byref(d), self.R, seeds.ctypes.data_as(C_U32P), float(n_eff), W,
                                           ah.ctypes.data_as(C_U32P) if ah is not None else None, _dp(xty), _u8(use) if use is not None else None,
                                           0 if streams is None else int(streams) & 0xffffffff, C.byref(self.h)))
        dev.G, dev.K, dev.ss_W = self.G, self.K, W

    def __del__(self):
        try:
            if self.h:
                self.L.hydra_ss_multi_destroy(self.h)
        except Exception:
            pass

    def iterate(self):
        check(self.L.hydra_ss_multi_iterate(self.h))

    def state(self, r):
        G, K = self.G, self.K
        sE, mu = C.c_double(), C.c_double()
        sG, pi = np.zeros(G), np.zeros((G, K))
        m0, cass = np.zeros(G, dtype=np.int32), np.zeros((G, K), dtype=np.int32)
        rng = RngState()
        check(self.L.hydra_ss_multi_state(self.h, r, C.byref(sE), C.byref(mu), _dp(sG), _dp(pi), _ip(m0), _ip(cass), C.byref(rng)))
        return {"sigmaE": sE.value, "mu": mu.value, "sigmaG": sG, "estPi": pi, "m0": m0, "cass": cass,
                "rng_x": np.array(rng.x, dtype=np.uint32), "rng_idx": int(rng.idx)}

    def effects(self, r):
        """(beta, components, acum, c) of chain r"""
        beta, acum, c = np.zeros(self.M), np.zeros(self.M), np.zeros(self.M)
        comp = np.zeros(self.M, dtype=np.int32)
        check(self.L.hydra_ss_multi_effects(self.h, r, _dp(beta), _ip(comp), _dp(acum), _dp(c)))
        return beta, comp, acum, c

    def streams(self):
        """(bounds (S + 1,) uint32, R lists of S RngState); (empty, []) for the single stream."""
        S = C.c_uint32()
        check(self.L.hydra_ss_multi_streams(self.h, C.byref(S), None, None))
        if S.value == 0:
            return np.zeros(0, dtype=np.uint32), []
        bounds = np.zeros(S.value + 1, dtype=np.uint32)
        ra = _RngArray([RngState() for _ in range(self.R * S.value)])
        check(self.L.hydra_ss_multi_streams(self.h, None, bounds.ctypes.data_as(C_U32P), ra.arr))
        ra.back()
        return bounds, [ra.rngs[r * S.value:(r + 1) * S.value] for r in range(self.R)]

    def last_nnz(self, r):
        return int(self.L.hydra_ss_multi_last_nnz(self.h, r))

    def csv_line(self, r, it):
        buf = C.create_string_buffer(50000)
        n = self.L.hydra_ss_multi_csv_line(self.h, r, it, buf, 50000)
        return buf.raw[:n].decode()


def ars_sample(logdens, xinit, xl, xr, grand):
    """One ARS draw from exp(logdens) on [xl, xr] (host code; no GPU involved). Returns (err, x, neval)."""
    L = lib()
    cb = LOGDENS_FN(lambda x, _d: logdens(x))
    xi = np.ascontiguousarray(xinit, dtype=np.float64)
    out, ne = C.c_double(0.0), C.c_int(0)
    err = L.hgibbs_ars_sample(_dp(xi), xl, xr, cb, None, C.byref(grand), C.byref(out), C.byref(ne))
    return err, out.value, ne.value


class BwOps:
    """BayesW operators of a loaded Device (hgibbs_w_*)."""

    def __init__(self, dev, failure):
        self.dev, self.L = dev, dev.L
        self.fail = np.ascontiguousarray(failure, dtype=np.int32)
        assert self.fail.shape[0] == dev.n_global
        check(self.L.hgibbs_w_init(dev.h, _ip(self.fail)))

    def marker_stats(self):
        M = self.dev.M
        a, b, c = np.zeros(M), np.zeros(M), np.zeros(M)
        check(self.L.hgibbs_w_marker_stats(self.dev.h, _dp(a), _dp(b), _dp(c)))
        return a, b, c

    def set_model(self, mS, groups=None, quad=9):
        mS = np.ascontiguousarray(mS, dtype=np.float64)
        self.G, self.K = mS.shape
        g = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
        check(self.L.hgibbs_w_set_model(self.dev.h, self.G, self.K, _ip(g) if g is not None else None, _dp(mS), quad))

    def reduce(self, kind, col=0, p0=0.0, p1=0.0, p2=0.0):
        out = C.c_double()
        check(self.L.hgibbs_w_reduce(self.dev.h, kind, col, p0, p1, p2, C.byref(out)))
        return out.value

    def refresh_vi(self, alpha):
        check(self.L.hgibbs_w_refresh_vi(self.dev.h, alpha))

    def get_vi(self):
        v, s = np.zeros(self.dev.n_local), C.c_double()
        check(self.L.hgibbs_w_get_vi(self.dev.h, _dp(v), C.byref(s)))
        return v, s.value

    def marker_sums(self, marker, beta_old, alpha):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(self.L.hgibbs_w_marker_sums(self.dev.h, marker, beta_old, alpha, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def get_beta(self):
        b, c = np.zeros(self.dev.M), np.zeros(self.dev.M, dtype=np.int32)
        check(self.L.hgibbs_w_get_beta(self.dev.h, _dp(b), _ip(c)))
        return b, c

    def sweep_stats(self):
        st = WSweepStats()
        check(self.L.hgibbs_w_last_sweep_stats(self.dev.h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}


class BwChain:
    """hydraw_chain_t: the runMpiGibbs_bW body on top of a loaded Device."""

    def __init__(self, dev, y, failure, mS=None, groups=None, seed=1222, shuffle=1, quad=9):
        self.dev, self.L = dev, dev.L
        if mS is None:
            mS = np.array([[0.0, 0.001, 0.01]])
        self.mS = np.ascontiguousarray(mS, dtype=np.float64)
        self.G, self.K = self.mS.shape
        self.groups = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
        y = np.ascontiguousarray(y, dtype=np.float64)
        self.fail = np.ascontiguousarray(failure, dtype=np.int32)
        assert y.shape[0] == dev.n_global and self.fail.shape[0] == dev.n_global
        d = WModelDesc(seed, shuffle, self.G, self.K, _ip(self.groups) if self.groups is not None else None, _dp(self.mS), quad)
        self.h = C.c_void_p()
        self.C = 0
        check(self.L.hydraw_chain_create(dev.h, C.byref(d), _dp(y), _ip(self.fail), C.byref(self.h)))

    def __del__(self):
        try:
            if self.h:
                self.L.hydraw_chain_destroy(self.h)
        except Exception:
            pass

    def set_covariates(self, X):
        X = np.ascontiguousarray(X, dtype=np.float64)
        self.C = X.shape[1]
        check(self.L.hydraw_chain_set_covariates(self.h, _dp(X), self.C))

    def reseed_ars(self, seed):
        check(self.L.hydraw_chain_reseed_ars(self.h, seed))

    def rng_words(self):
        st = self.state()
        rng = RngState()
        rng.x[:] = list(st["rng_x"])
        rng.idx = st["rng_idx"]
        out = np.zeros(624, dtype=np.uint32)
        check(self.L.hydra_rng_to_boost_words(C.byref(rng), out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def restore(self, iteration, mu, alpha, sigmaG, pi, beta, components, eps, order, rng_words, ars_seed, gamma=None, xI=None):
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        keep = [f64(sigmaG), f64(pi), f64(beta), i32(components), f64(eps), i32(order)]
        st = WRestartState()
        st.iteration, st.mu, st.alpha, st.ars_seed = iteration, mu, alpha, ars_seed
        st.sigmaG, st.pi, st.beta = _dp(keep[0]), _dp(keep[1]), _dp(keep[2])
        st.components, st.eps, st.order = _ip(keep[3]), _dp(keep[4]), _ip(keep[5])
        if gamma is not None:
            keep += [f64(gamma), i32(xI)]
            st.gamma, st.xI = _dp(keep[6]), _ip(keep[7])
        w = np.ascontiguousarray(rng_words, dtype=np.uint32)
        check(self.L.hydra_rng_from_boost_words(w.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(st.rng)))
        check(self.L.hydraw_chain_restore(self.h, C.byref(st)))

    def iterate(self):
        check(self.L.hydraw_chain_iterate(self.h))

    def state(self):
        G, K = self.G, self.K
        mu, alpha = C.c_double(), C.c_double()
        sG, pi = np.zeros(G), np.zeros((G, K))
        m0, cass = np.zeros(G, dtype=np.int32), np.zeros((G, K), dtype=np.int32)
        rng, gr = RngState(), GrandState()
        check(self.L.hydraw_chain_state(self.h, C.byref(mu), C.byref(alpha), _dp(sG), _dp(pi), _ip(m0), _ip(cass), C.byref(rng), C.byref(gr)))
        return {"mu": mu.value, "alpha": alpha.value, "sigmaG": sG, "pi": pi, "m0": m0, "cass": cass,
                "rng_x": np.array(rng.x, dtype=np.uint32), "rng_idx": int(rng.idx), "grand": gr}

    def gamma(self):
        g, xi = np.zeros(self.C), np.zeros(self.C, dtype=np.int32)
        check(self.L.hydraw_chain_gamma(self.h, _dp(g), _ip(xi)))
        return g, xi

    def beta(self):
        b, c = np.zeros(self.dev.M), np.zeros(self.dev.M, dtype=np.int32)
        check(self.L.hgibbs_w_get_beta(self.dev.h, _dp(b), _ip(c)))
        return b, c

    def order(self):
        return np.ctypeslib.as_array(self.L.hydraw_chain_order(self.h), shape=(self.dev.M,)).copy()

    def last_nnz(self):
        return int(self.L.hydraw_chain_last_nnz(self.h))

    def sweep_stats(self):
        st = WSweepStats()
        check(self.L.hgibbs_w_last_sweep_stats(self.dev.h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def csv_line(self, it):
        buf = C.create_string_buffer(50000)
        n = self.L.hydraw_chain_csv_line(self.h, it, buf, 50000)
        return buf.raw[:n].decode()
