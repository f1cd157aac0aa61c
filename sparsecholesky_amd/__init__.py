"""MI355X-native supernodal sparse Cholesky -- Python mirror of the reference API.

The compute lives in ``libsparsecholesky_amd.so`` (host symbolic analysis in C++,
numeric factorization in hand-written HIP for gfx950), reached through its C ABI
(``include/sparsecholesky.h``) with ctypes.  This module mirrors the reference's
C++ API (evanwporter/SparseCholesky ``include/chol.hpp``) so tests read like the
reference's own gtests:

=========================  ===========================================
reference (chol.hpp)       here
=========================  ===========================================
csc_matrix<T, S>   :134    :class:`csc_matrix`
SChol              :99     :class:`SChol`
triplet_to_csc_matrix :308 :func:`triplet_to_csc_matrix`
etree              :377    :func:`etree`
post_order         :466    :func:`post_order`
col_count          :567    :func:`col_count`
ereach             :725    :func:`ereach`
chol               :750    :func:`chol`   (GPU numeric path)
schol              :874    :func:`schol`
chol_sn            :1407   :func:`chol_sn` (same GPU path; the reference's is broken)
csc_to_dense       :1448   :func:`csc_to_dense`
compute_levels     src/chol.cpp:7     :func:`compute_levels`
compute_supernodes src/chol.cpp:42    :func:`compute_supernodes`
atree              src/chol.cpp:102   :func:`atree`
load_matrix_market_to_csc  mtx_reader.hpp:17  :func:`load_matrix_market_to_csc`
=========================  ===========================================

There is no CPU fallback: :func:`chol` raises if the HIP library or a GPU is
missing.
"""
from __future__ import annotations

import ctypes as C
import enum
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

__all__ = [
    "sym", "csc_matrix", "SChol", "Expected", "lib", "LibraryError",
    "triplet_to_csc_matrix", "build_csc_matrix_from_pattern", "load_matrix_market_to_csc",
    "etree", "post_order", "col_count", "ereach", "schol", "chol", "chol_sn",
    "csc_to_dense", "compute_levels", "compute_supernodes", "atree", "laplacian3d",
    "Symbolic", "Numeric", "Options",
    "SC_OP_SOLVE_A", "SC_OP_SOLVE_L", "SC_OP_SOLVE_LT", "SC_OP_MUL_L", "SC_OP_MUL_LT", "SC_OP_PERM", "SC_OP_PERM_T",
    "RefineOptions", "RefineInfo", "SC_RESIDUAL_FP64", "SC_RESIDUAL_DD",
    "SC_REFINE_CONVERGED", "SC_REFINE_STALLED", "SC_REFINE_MAXITER", "SC_REFINE_DIVERGED",
    "PcgOptions", "PcgInfo", "SC_PCG_CONVERGED", "SC_PCG_MAXITER", "SC_PCG_BREAKDOWN",
    "EigsOptions", "EigsInfo", "SC_EIGS_CONVERGED", "SC_EIGS_MAXBLOCKS", "SC_EIGS_EXHAUSTED",
    "NormalEquations", "LstsqInfo",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsparsecholesky_amd.so")

SC_OK = 0
# enum sc_factor_op: what Numeric.apply / sc_apply_* compute from the factor P A P^T = L L^T
SC_OP_SOLVE_A, SC_OP_SOLVE_L, SC_OP_SOLVE_LT, SC_OP_MUL_L, SC_OP_MUL_LT, SC_OP_PERM, SC_OP_PERM_T = range(7)
# residual accumulation of Numeric.residual / solve_refined, and the states a refined column ends in
SC_RESIDUAL_FP64, SC_RESIDUAL_DD = 0, 1
SC_REFINE_CONVERGED, SC_REFINE_STALLED, SC_REFINE_MAXITER, SC_REFINE_DIVERGED = range(4)
# the states a column of Numeric.solve_pcg ends in
SC_PCG_CONVERGED, SC_PCG_MAXITER, SC_PCG_BREAKDOWN = range(3)
# the states an eigenpair of Numeric.eigsh ends in
SC_EIGS_CONVERGED, SC_EIGS_MAXBLOCKS, SC_EIGS_EXHAUSTED = range(3)
_RESIDUAL_MODES = {"fp64": SC_RESIDUAL_FP64, "dd": SC_RESIDUAL_DD}
_STATUS = {
    -1: "invalid argument", -2: "host allocation failed", -3: "HIP runtime error",
    -4: "device allocation failed", -5: "call out of order", -6: "communication error",
    -7: "not implemented", -8: "matrix is not symmetric", -9: "file could not be opened",
}


class LibraryError(RuntimeError):
    pass


class Options(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("relax", C.c_int32), ("nrelax", C.c_int32 * 3), ("zrelax", C.c_double * 3),
        ("small_front_max", C.c_int32), ("panel_nb", C.c_int32), ("panel_nb_outer", C.c_int32),
        ("use_graph", C.c_int32), ("relax_wmax", C.c_int32), ("syrk_tile", C.c_int32),
        ("lookahead", C.c_int32), ("inner_order", C.c_int32),
        ("asm_tile_min_m", C.c_int32), ("dist_split", C.c_int32), ("dist_cbb", C.c_int32),
        ("ordering", C.c_int32), ("dist_early", C.c_int32), ("dist_panel", C.c_int32),
        ("cb_gather", C.c_int32),
        ("dist_slab_block", C.c_int32), ("trsm_split_wg", C.c_int32),
        ("syrk_lean_kmax", C.c_int32), ("cb_tail_split", C.c_int32), ("tiny_dense", C.c_int32),
        ("dist_asm", C.c_int32),
        ("dist_pieces", C.c_int32), ("dist_local_pieces", C.c_int32), ("panel_prefactor", C.c_int32),
    ]


class RefineOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("max_iter", C.c_int32), ("residual", C.c_int32),
                ("rho_max", C.c_double)]


class RefineInfo(C.Structure):
    _fields_ = [("iters", C.c_int32), ("state", C.c_int32), ("berr_norm", C.c_double),
                ("berr_comp", C.c_double), ("dx_ratio", C.c_double)]


class PcgOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("max_iter", C.c_int32), ("use_x0", C.c_int32), ("tol", C.c_double)]


class PcgInfo(C.Structure):
    _fields_ = [("iters", C.c_int32), ("state", C.c_int32), ("relres", C.c_double), ("relres_true", C.c_double),
                ("berr_norm", C.c_double), ("berr_comp", C.c_double)]


class EigsOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("max_blocks", C.c_int32), ("use_x0", C.c_int32), ("seed", C.c_uint64),
                ("tol", C.c_double), ("sigma", C.c_double)]


class EigsInfo(C.Structure):
    _fields_ = [("state", C.c_int32), ("blocks", C.c_int32), ("est", C.c_double), ("resid", C.c_double)]


class LstsqInfo(C.Structure):
    _fields_ = [("iters", C.c_int32), ("state", C.c_int32), ("grad_norm", C.c_double),
                ("resid_norm", C.c_double), ("dx_ratio", C.c_double)]


class SymbolicStats(C.Structure):
    _fields_ = [
        ("n", C.c_int64), ("nnz_A", C.c_int64), ("nnz_L", C.c_int64), ("flops", C.c_double),
        ("etree_depth", C.c_int64), ("n_fundamental", C.c_int64), ("n_supernodes", C.c_int64),
        ("n_levels", C.c_int64), ("max_front_m", C.c_int64), ("max_front_w", C.c_int64),
        ("panel_entries", C.c_int64), ("cb_entries", C.c_int64), ("flops_executed", C.c_double),
        ("flops_syrk_w256", C.c_double), ("n_small_fronts", C.c_int64), ("n_large_fronts", C.c_int64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_P = C.c_void_p
_I64 = C.c_int64
_I32 = C.c_int32
_D = C.c_double

# (name, restype, argtypes)
_SIGS = [
    ("sc_version", _I32, []),
    ("sc_status_string", C.c_char_p, [_I64]),
    ("sc_last_error", C.c_char_p, []),
    ("sc_default_options", None, [C.POINTER(Options)]),
    ("sc_analyze", _I64, [_I64, _P, _P, C.POINTER(Options), C.POINTER(_P)]),
    ("sc_symbolic_get_stats", _I64, [_P, C.POINTER(SymbolicStats)]),
    ("sc_nnz_L", _I64, [_P]),
    ("sc_flops", _D, [_P]),
    ("sc_symbolic_pattern", _I64, [_P, _P, _P]),
    ("sc_symbolic_etree", _I64, [_P, _P, _P]),
    ("sc_symbolic_supernodes", _I64, [_P, _P, _P, _P, _P]),
    ("sc_symbolic_perm", _I64, [_P, _P]),
    ("sc_free_symbolic", None, [_P]),
    ("sc_numeric_create", _I64, [_P, _I32, C.POINTER(_P)]),
    ("sc_factor", _I64, [_P, _P]),
    ("sc_factor_device", _I64, [_P, _P, _I32]),
    ("sc_numeric_status", _I64, [_P]),
    ("sc_export_L", _I64, [_P, _P, _P, _P]),
    ("sc_export_L_cols", _I64, [_P, _I64, _I64, _P, _P, _P]),
    ("sc_numeric_stream", _P, [_P]),
    ("sc_numeric_set_profile", _I64, [_P, _I32]),
    ("sc_numeric_timing", _I64, [_P, _P, _I32]),
    ("sc_numeric_level_times", _I64, [_P, _P, _I32]),
    ("sc_numeric_launch_trace", _I64, [_P, _P, _P, _P, _P, _P, _I64]),
    ("sc_numeric_syrk_stats", _I64, [_P, _I32, C.POINTER(_D), C.POINTER(_D), C.POINTER(_I64)]),
    ("sc_numeric_syrk_bytes", _I64, [_P, _I32, C.POINTER(_D)]),
    ("sc_numeric_launch_times", _I64, [_P, _P, _P, _P, _P, _P, _I64]),
    ("sc_free_numeric", None, [_P]),
    ("sc_solve_host", _I64, [_P, _P, _P]),
    ("sc_solve_device", _I64, [_P, _P, _P]),
    ("sc_solve_device_multi", _I64, [_P, _I32, _P, _I64, _P, _I64]),
    ("sc_solve_host_multi", _I64, [_P, _I32, _P, _I64, _P, _I64]),
    ("sc_apply_device", _I64, [_P, _I32, _P, _P]),
    ("sc_apply_host", _I64, [_P, _I32, _P, _P]),
    ("sc_apply_device_multi", _I64, [_P, _I32, _I32, _P, _I64, _P, _I64]),
    ("sc_apply_host_multi", _I64, [_P, _I32, _I32, _P, _I64, _P, _I64]),
    ("sc_logdet", _I64, [_P, _P]),
    ("sc_selinv", _I64, [_P]),
    ("sc_selinv_diag_host", _I64, [_P, _P]),
    ("sc_selinv_diag_device", _I64, [_P, _P]),
    ("sc_selinv_export", _I64, [_P, _P, _P, _P]),
    ("sc_selinv_flops", _I64, [_P, C.POINTER(_D)]),
    ("sc_updown_check", _I64, [_P, _I32, _P, _P, _P, _P]),
    ("sc_updown_host", _I64, [_P, _I32, _I32, _P, _P, _P]),
    ("sc_analyze_schur", _I64, [_I64, _P, _P, C.POINTER(Options), _I32, _P, C.POINTER(_P)]),
    ("sc_symbolic_schur", _I64, [_P, _P]),
    ("sc_schur_factor_device", _I64, [_P, _P, _I64]),
    ("sc_schur_factor_host", _I64, [_P, _P, _I64]),
    ("sc_schur_matrix_device", _I64, [_P, _P, _I64]),
    ("sc_schur_matrix_host", _I64, [_P, _P, _I64]),
    ("sc_schur_condense_device_multi", _I64, [_P, _I32, _P, _I64, _P, _I64]),
    ("sc_schur_condense_host_multi", _I64, [_P, _I32, _P, _I64, _P, _I64]),
    ("sc_schur_expand_device_multi", _I64, [_P, _I32, _P, _I64, _P, _I64, _P, _I64]),
    ("sc_schur_expand_host_multi", _I64, [_P, _I32, _P, _I64, _P, _I64, _P, _I64]),
    ("sc_default_refine_options", None, [C.POINTER(RefineOptions)]),
    ("sc_spmv_structure", _I64, [_P, _P, _P, _P]),
    ("sc_spmv_host_multi", _I64, [_P, _I32, _P, _P, _I64, _P, _I64]),
    ("sc_spmv_device_multi", _I64, [_P, _I32, _P, _P, _I64, _P, _I64]),
    ("sc_residual_host_multi", _I64, [_P, _I32, _I32, _P, _P, _I64, _P, _I64, _P, _I64, _P, _P]),
    ("sc_residual_device_multi", _I64, [_P, _I32, _I32, _P, _P, _I64, _P, _I64, _P, _I64, _P, _P]),
    ("sc_solve_refine_host_multi", _I64, [_P, C.POINTER(RefineOptions), _I32, _P, _P, _I64, _P, _I64, _P]),
    ("sc_solve_refine_device_multi", _I64, [_P, C.POINTER(RefineOptions), _I32, _P, _P, _I64, _P, _I64, _P]),
    ("sc_default_pcg_options", None, [C.POINTER(PcgOptions)]),
    ("sc_solve_pcg_host_multi", _I64, [_P, C.POINTER(PcgOptions), _I32, _P, _P, _I64, _P, _I64, _P]),
    ("sc_solve_pcg_device_multi", _I64, [_P, C.POINTER(PcgOptions), _I32, _P, _P, _I64, _P, _I64, _P]),
    ("sc_default_eigs_options", None, [C.POINTER(EigsOptions)]),
    ("sc_eigs_host", _I64, [_P, C.POINTER(EigsOptions), _I32, _P, _P, _I64, _P, _P, _I64, _P]),
    ("sc_eigs_device", _I64, [_P, C.POINTER(EigsOptions), _I32, _P, _P, _I64, _P, _P, _I64, _P]),
    ("sc_value_entries", _I64, [_P, _P, _P, _P]),
    ("sc_pattern_outer_host", _I64, [_P, _D, _I32, _P, _I64, _P, _I64, _D, _P]),
    ("sc_pattern_outer_device", _I64, [_P, _D, _I32, _P, _I64, _P, _I64, _D, _P]),
    ("sc_pattern_dot_host", _I64, [_P, _P, _P, C.POINTER(_D)]),
    ("sc_pattern_dot_device", _I64, [_P, _P, _P, C.POINTER(_D)]),
    ("sc_logdet_grad_host", _I64, [_P, _P]),
    ("sc_logdet_grad_device", _I64, [_P, _P]),
    ("sc_solve_grad_host", _I64, [_P, _I32, _P, _I64, _P, _I64, _P, _I64, _P]),
    ("sc_solve_grad_device", _I64, [_P, _I32, _P, _I64, _P, _I64, _P, _I64, _P]),
    ("sc_normal_create", _I64, [_I64, _I64, _P, _P, _P, _P, _I32, C.POINTER(_P)]),
    ("sc_normal_free", None, [_P]),
    ("sc_normal_pattern", _I64, [_P, _P, _P]),
    ("sc_normal_terms", _I64, [_P]),
    ("sc_normal_term_lists", _I64, [_P, _P, _P, _P, _P, _P]),
    ("sc_normal_rows", _I64, [_P, _P, _P, _P]),
    ("sc_normal_memory", _I64, [_P, _P, _I32]),
    ("sc_normal_constants", _I64, [_P, _I32]),
    ("sc_normal_values_host", _I64, [_P, _P, _P, _P, _P, _D, _P]),
    ("sc_normal_values_device", _I64, [_P, _P, _P, _P, _P, _D, _P]),
    ("sc_normal_factor_host", _I64, [_P, _P, _P, _P, _P, _P, _D]),
    ("sc_normal_factor_device", _I64, [_P, _P, _P, _P, _P, _P, _D]),
    ("sc_normal_values_ptr", _P, [_P]),
    ("sc_normal_mul_host_multi", _I64, [_P, _I32, _P, _P, _I64, _P, _I64]),
    ("sc_normal_mul_device_multi", _I64, [_P, _I32, _P, _P, _I64, _P, _I64]),
    ("sc_normal_mult_host_multi", _I64, [_P, _I32, _P, _P, _P, _I64, _P, _I64]),
    ("sc_normal_mult_device_multi", _I64, [_P, _I32, _P, _P, _P, _I64, _P, _I64]),
    ("sc_normal_lstsq_host_multi", _I64, [_P, _P, C.POINTER(RefineOptions), _I32, _P, _P, _P, _I64, _P, _I64, _P]),
    ("sc_normal_lstsq_device_multi", _I64, [_P, _P, C.POINTER(RefineOptions), _I32, _P, _P, _P, _I64, _P, _I64, _P]),
    ("sc_etree", _I64, [_I64, _P, _P, _P]),
    ("sc_post_order", _I64, [_I64, _P, _P]),
    ("sc_col_count", _I64, [_I64, _P, _P, _P, _P, _P]),
    ("sc_ereach", _I64, [_I64, _P, _P, _P, _I64, _P, _P, _P, _P]),
    ("sc_compute_levels", _I64, [_I64, _P, _P]),
    ("sc_compute_supernodes", _I64, [_I64, _P, _P, _P, _P]),
    ("sc_atree", _I64, [_I64, _P, _P, _P, _P, _I64, _P]),
    ("sc_triplet_to_csc", _I64, [_I64, _I64, _P, _P, _P, _P, _P, _P]),
    ("sc_read_mtx", _I64, [C.c_char_p, C.POINTER(_I64), _P, _P, _P]),
    ("sc_laplacian3d", _I64, [_I64, _I32, _P, _P, _P, _P]),
    ("sc_dist_unique_id", _I64, [_P]),
    ("sc_dist_owner_map", _I64, [_P, _I32, _P, _P]),
    ("sc_numeric_create_dist", _I64, [_P, _I32, _I32, _I32, _P, C.POINTER(_P)]),
    ("sc_dist_schedule", _I64, [_P, _I32, _I32, _P, _P, _P, _P, _I64]),
    ("sc_dist_plan_info", _I64, [_P, _I32, _P, _P, _P, C.POINTER(_I64)]),
    ("sc_dist_steps", _I64, [_P, _I32, _P, _P, _P, _P, _P, _I64]),
    ("sc_numeric_create_dist_host", _I64, [_P, _I32, _I32, _I32, C.c_void_p, _P, C.POINTER(_P)]),
    ("sc_numeric_create_dist_dry", _I64, [_P, _I32, _I32, _I32, C.POINTER(_P)]),
    ("sc_numeric_create_dist_emulated", _I64, [_P, _I32, _I32, _I32, C.POINTER(_P)]),
    ("sc_numeric_memory", _I64, [_P, _P, _I32]),
    ("sc_memory_plan", _I64, [_P, _I32, _P, _P, _P]),
    ("sc_memory_plan_check", _I64, [_P, _I32]),
    ("sc_debug_syrk", _I64, [_P, _I32, _P, _I32, _I32, _I32, _I32]),
    ("sc_debug_syrk_ex", _I64, [_P, _I32, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32]),
    ("sc_debug_panel", _I64, [_P, _I32, _I32, _I32, _I32, C.POINTER(_I32)]),
    ("sc_debug_updown_block", _I64, [_P, _I32, _I32, _I32, _P, _I32, C.POINTER(_I32)]),
    ("sc_debug_schur_llt", _I64, [_P, _I32, _I64, _P, _I64]),
    ("sc_debug_solve_step", _I64, [_P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P]),
    ("sc_debug_solve_gather", _I64, [_I32, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
    ("sc_debug_spmv", _I64, [_I32, _I32, _P, _P, _P, _I64, _P, _I32, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _P]),
    ("sc_debug_normal_form", _I64, [_I64, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, _P, _P, _P, _D, _P]),
    ("sc_debug_normal_mul", _I64, [_I32, _I64, _I64, _P, _P, _P, _I64, _P, _I32, _P, _I64, _P, _I64, _P, _I64]),
    ("sc_debug_normal_mult", _I64, [_I64, _I64, _P, _P, _P, _P, _I32, _P, _I64, _P, _I64]),
    ("sc_debug_normal_pair", _I64, [_I64, _I64, _P, _P, _P, _P, _P, _P, _P, _I32, _P, _I64, _P, _I64, _P, _P, _I64, _P, _P,
                                    _I64]),
    ("sc_debug_pcg_vec", _I64, [_I32, _I32, _I32, C.c_uint32, _P, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _P]),
    ("sc_debug_eigs_gram", _I64, [_I32, _I32, _I32, _P, _I64, _I64, _P, _I64, _P]),
    ("sc_debug_eigs_update", _I64, [_I32, _I32, _I32, _I32, _D, _P, _I64, _P, _I64, _P, _I64, _I64, _P]),
    ("sc_debug_eigs_dense", _I64, [_I32, _I32, _P, _P]),
    ("sc_debug_bench", _I64, [_I32, _I32, _I32, _I32, _I32, C.POINTER(_D)]),
    ("sc_device_count", _I64, []),
    ("sc_debug_chain_stamps", _I64, [_P, _I32, _P, _I64]),
    ("sc_debug_time_factor", _I64, [_P, C.c_void_p, _I32, C.POINTER(_D)]),
    ("sc_debug_solve_eager", _I64, [_P, _I32]),
    ("sc_debug_selinv_times", _I64, [_P, _I32, _P]),
    ("sc_debug_selinv_cols", _I64, [_P, _I64, _I64, _P, _P, _P]),
    ("sc_debug_selinv_step", _I64, [_P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    ("sc_debug_selinv_push", _I64, [_I32, _I32, _P, _P, _I32, _P, _P]),
    ("sc_debug_extend_add", _I64, [_I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _I32, _I32, _I32,
                                   C.POINTER(_I32)]),
    ("sc_debug_hwid", _I64, [_I32, _I32, _I32, _P]),
    ("sc_debug_contention", _I64, [_I32, _I32, _I32, _I32, _I32, _I32, _P]),
    ("sc_debug_schedule_digest", _I64, [_P, _I32, _I32, _I32, _P, _I64]),
    ("sc_debug_schedule_syrk", _I64, [_P, _I32, _I32, _I32, _P, _I64]),
    ("sc_debug_numeric_digest", _I64, [_P, _P, _I64]),
]

# decoded call kinds of a schedule entry, in the order of the digest's counters
CALL_KINDS = ("front_small", "chain", "tiny_tree", "tiny_dense", "asm_cols", "asm_tiled", "asm_tiled_lim", "potrf",
              "trsm_fused", "trsm_pre", "trsm_partial", "syrk_panel", "syrk_cb", "comm", "record", "wait")
_DIGEST_COUNTERS = ("tail_split", "pf", "comm_steps", "events", "msgs", "gsegs")


def _digest_dict(call, what):
    n = len(CALL_KINDS) + len(_DIGEST_COUNTERS) + 1
    v = np.zeros(n, dtype=np.int64)
    assert _check(call(_ptr(v), n), what) == n
    d = {"hash": "%016x" % (int(v[0]) & (2 ** 64 - 1)), "calls": dict(zip(CALL_KINDS, v[1:].tolist()))}
    d.update(zip(_DIGEST_COUNTERS, v[1 + len(CALL_KINDS):].tolist()))
    return d

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load the product library (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LibraryError(
                f"{LIB_PATH} missing: build it with `make -C sparsecholesky_amd/csrc` "
                "(or __graft_entry__.build())")
        # torch (when present) bundles its own libamdhip64.so.7; loading it first
        # lets this library bind to the same HIP runtime (same soname) so device
        # pointers and streams are shared instead of two runtimes fighting over
        # the device.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, res, args in _SIGS:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def exported_symbols():
    return [name for name, _, _ in _SIGS]


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(rc: int, what: str):
    if rc < 0:
        msg = lib().sc_last_error()
        raise LibraryError(f"{what}: {_STATUS.get(rc, rc)}" + (f" ({msg.decode()})" if msg else ""))
    return rc


# --------------------------------------------------------------------------
# storage types (chol.hpp:26-299)
# --------------------------------------------------------------------------
class sym(enum.Enum):
    none = 0
    upper = 1
    lower = 2


@dataclass
class csc_matrix:
    """CSC matrix with int64 column pointers (chol.hpp:134 csc_matrix<T,S>)."""
    n_rows: int
    n_cols: int
    p: np.ndarray
    i: np.ndarray
    x: np.ndarray
    S: sym = sym.upper

    def rows(self):
        return self.n_rows

    def cols(self):
        return self.n_cols

    def size(self):
        return self.n_cols

    def capacity(self):
        return int(self.p[-1]) if len(self.p) else 0

    def find_index(self, i: int, j: int) -> int:
        a, b = int(self.p[j]), int(self.p[j + 1])
        k = a + int(np.searchsorted(self.i[a:b], i))
        return k if k < b and self.i[k] == i else -1

    def __getitem__(self, ij):
        i, j = ij
        if self.S == sym.upper and j < i:
            i, j = j, i
        elif self.S == sym.lower and i < j:
            i, j = j, i
        k = self.find_index(i, j)
        return 0.0 if k < 0 else float(self.x[k])

    def transpose(self) -> "csc_matrix":
        n = self.n_cols
        cols = np.repeat(np.arange(n, dtype=np.int32), np.diff(self.p).astype(np.int64))
        order = np.lexsort((cols, self.i))
        tp = np.zeros(self.n_rows + 1, dtype=np.int64)
        np.add.at(tp, self.i.astype(np.int64) + 1, 1)
        tp = np.cumsum(tp)
        St = {sym.upper: sym.lower, sym.lower: sym.upper, sym.none: sym.none}[self.S]
        return csc_matrix(self.n_cols, self.n_rows, tp, cols[order].astype(np.int32),
                          self.x[order].copy(), St)


@dataclass
class SChol:
    """Symbolic factor: pattern of L plus the etree (chol.hpp:99-132)."""
    p: np.ndarray
    i: np.ndarray
    parent: np.ndarray

    def size(self):
        return len(self.p) - 1

    def capacity(self):
        return int(self.p[-1])

    def __getitem__(self, ij):
        i, j = ij
        if i < j:
            i, j = j, i
        a, b = int(self.p[j]), int(self.p[j + 1])
        k = a + int(np.searchsorted(self.i[a:b], i))
        return bool(k < b and self.i[k] == i)


@dataclass
class Expected:
    """std::expected<csc_matrix, std::string> (chol.hpp:750)."""
    _value: Optional[csc_matrix] = None
    _error: Optional[str] = None
    status: int = 0

    def has_value(self):
        return self._value is not None

    def __bool__(self):
        return self.has_value()

    def value(self) -> csc_matrix:
        if self._value is None:
            raise RuntimeError(self._error)
        return self._value

    def error(self) -> str:
        return self._error


# --------------------------------------------------------------------------
# input construction (chol.hpp:308-435, mtx_reader.hpp)
# --------------------------------------------------------------------------
def triplet_to_csc_matrix(ti, tj, tx, n: int) -> csc_matrix:
    ti = np.ascontiguousarray(ti, dtype=np.int32)
    tj = np.ascontiguousarray(tj, dtype=np.int32)
    tx = np.ascontiguousarray(tx, dtype=np.float64)
    assert len(ti) == len(tj) == len(tx)
    Ap = np.zeros(n + 1, dtype=np.int64)
    nnz = _check(lib().sc_triplet_to_csc(n, len(ti), _ptr(ti), _ptr(tj), _ptr(tx), _ptr(Ap), None, None),
                 "triplet_to_csc")
    Ai = np.zeros(max(nnz, 1), dtype=np.int32)
    Ax = np.zeros(max(nnz, 1), dtype=np.float64)
    _check(lib().sc_triplet_to_csc(n, len(ti), _ptr(ti), _ptr(tj), _ptr(tx), _ptr(Ap), _ptr(Ai), _ptr(Ax)),
           "triplet_to_csc")
    return csc_matrix(n, n, Ap, Ai[:nnz], Ax[:nnz], sym.upper)


def build_csc_matrix_from_pattern(pattern) -> csc_matrix:
    """chol.hpp:412-435: every listed (row, col) becomes an upper entry of value 1."""
    ti, tj = [], []
    for r, cols in enumerate(pattern):
        for c in cols:
            a, b = (r, c) if r <= c else (c, r)
            ti.append(a)
            tj.append(b)
    return triplet_to_csc_matrix(ti, tj, np.ones(len(ti)), len(pattern))


def load_matrix_market_to_csc(path: str) -> csc_matrix:
    n = C.c_int64(0)
    nnz = _check(lib().sc_read_mtx(path.encode(), C.byref(n), None, None, None), "read_mtx")
    Ap = np.zeros(n.value + 1, dtype=np.int64)
    Ai = np.zeros(max(nnz, 1), dtype=np.int32)
    Ax = np.zeros(max(nnz, 1), dtype=np.float64)
    _check(lib().sc_read_mtx(path.encode(), C.byref(n), _ptr(Ap), _ptr(Ai), _ptr(Ax)), "read_mtx")
    return csc_matrix(n.value, n.value, Ap, Ai[:nnz], Ax[:nnz], sym.upper)


def laplacian3d(k: int, nd: bool = True, with_perm: bool = False):
    """7-point Laplacian on a k^3 grid in geometric nested-dissection order."""
    nnz = _check(lib().sc_laplacian3d(k, 1 if nd else 0, None, None, None, None), "laplacian3d")
    n = k ** 3
    Ap = np.zeros(n + 1, dtype=np.int64)
    Ai = np.zeros(nnz, dtype=np.int32)
    Ax = np.zeros(nnz, dtype=np.float64)
    perm = np.zeros(n, dtype=np.int32)
    _check(lib().sc_laplacian3d(k, 1 if nd else 0, _ptr(Ap), _ptr(Ai), _ptr(Ax), _ptr(perm)), "laplacian3d")
    A = csc_matrix(n, n, Ap, Ai, Ax, sym.upper)
    return (A, perm) if with_perm else A


# --------------------------------------------------------------------------
# symbolic helpers (chol.hpp:371-739, src/chol.cpp)
# --------------------------------------------------------------------------
def etree(A: csc_matrix) -> np.ndarray:
    parent = np.zeros(A.size(), dtype=np.int32)
    _check(lib().sc_etree(A.size(), _ptr(A.p), _ptr(A.i), _ptr(parent)), "etree")
    return parent


def post_order(parent: np.ndarray) -> np.ndarray:
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    post = np.zeros(len(parent), dtype=np.int32)
    _check(lib().sc_post_order(len(parent), _ptr(parent), _ptr(post)), "post_order")
    return post


def col_count(A: csc_matrix, parent, post) -> np.ndarray:
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    post = np.ascontiguousarray(post, dtype=np.int32)
    cc = np.zeros(A.size(), dtype=np.int64)
    _check(lib().sc_col_count(A.size(), _ptr(A.p), _ptr(A.i), _ptr(parent), _ptr(post), _ptr(cc)), "col_count")
    return cc


def ereach(A: csc_matrix, k: int, parent, s: np.ndarray, w: np.ndarray, x: Optional[np.ndarray] = None) -> int:
    """Fills s[top:] with the reach of row k; w is the caller's mark array (chol.hpp:725,737)."""
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    assert s.dtype == np.int32 and w.dtype == np.int32
    return _check(lib().sc_ereach(A.size(), _ptr(A.p), _ptr(A.i), _ptr(A.x) if x is not None else None, k,
                                  _ptr(parent), _ptr(s), _ptr(w), _ptr(x)), "ereach")


def compute_levels(parent) -> list:
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    lev = np.zeros(len(parent), dtype=np.int32)
    nl = _check(lib().sc_compute_levels(len(parent), _ptr(parent), _ptr(lev)), "compute_levels")
    return [list(np.nonzero(lev == l)[0]) for l in range(nl)]


def compute_supernodes(S: "SChol"):
    """Returns (sn_id, supernodes) as src/chol.cpp:42-100."""
    n = S.size()
    sn_id = np.zeros(n, dtype=np.int32)
    sup = np.zeros(n + 1, dtype=np.int64)
    ns = _check(lib().sc_compute_supernodes(n, _ptr(np.ascontiguousarray(S.parent, dtype=np.int32)),
                                            _ptr(S.p), _ptr(sn_id), _ptr(sup)), "compute_supernodes")
    return sn_id, sup[:ns + 1]


def atree(S: "SChol", sn_id, supernodes) -> np.ndarray:
    ns = len(supernodes) - 1
    sp = np.zeros(ns, dtype=np.int32)
    _check(lib().sc_atree(S.size(), _ptr(S.p), _ptr(S.i), _ptr(np.ascontiguousarray(sn_id, dtype=np.int32)),
                          _ptr(np.ascontiguousarray(supernodes, dtype=np.int64)), ns, _ptr(sp)), "atree")
    return sp


def permute_symmetric(A: csc_matrix, perm: np.ndarray) -> csc_matrix:
    """P A P^T as upper CSC (perm[new] = old); entries below the diagonal of A are
    ignored as the reference does, duplicates are summed."""
    n = A.size()
    ip = np.empty(n, dtype=np.int64)
    ip[np.asarray(perm, dtype=np.int64)] = np.arange(n)
    col = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.p))
    keep = A.i <= col
    a, b = ip[A.i[keep]], ip[col[keep]]
    return triplet_to_csc_matrix(np.minimum(a, b).astype(np.int32), np.maximum(a, b).astype(np.int32),
                                 A.x[keep], n)


def csc_to_dense(A: csc_matrix) -> np.ndarray:
    """chol.hpp:1448-1479 (returns a 2-D array; the reference returns column-major flat)."""
    D = np.zeros((A.rows(), A.cols()))
    cols = np.repeat(np.arange(A.cols()), np.diff(A.p).astype(np.int64))
    D[A.i, cols] = A.x
    if A.S != sym.none:
        D[cols, A.i] = A.x
    return D


# --------------------------------------------------------------------------
# analysis / numeric handles
# --------------------------------------------------------------------------
def default_options(**kw) -> Options:
    o = Options()
    lib().sc_default_options(C.byref(o))
    for k, v in kw.items():
        if k in ("nrelax", "zrelax"):
            for t, vv in enumerate(v):
                getattr(o, k)[t] = vv
        else:
            setattr(o, k, v)
    return o


def _updown_W(W, n: int):
    """(Wp, Wi, Wx, k) of an update matrix: a (Wp, Wi, Wx) triple as it is, a dense (n, k)
    array by its nonzeros."""
    if isinstance(W, tuple):
        Wp, Wi, Wx = W
        Wp = np.ascontiguousarray(Wp, dtype=np.int64)
        Wi = np.ascontiguousarray(Wi, dtype=np.int32)
        Wx = np.ascontiguousarray(Wx, dtype=np.float64)
        if len(Wp) < 1 or len(Wi) != len(Wx) or len(Wi) < int(Wp[-1]):
            raise ValueError("updown: (Wp, Wi, Wx) is not a CSC triple")
        return Wp, Wi, Wx, len(Wp) - 1
    D = np.asarray(W, dtype=np.float64)
    if D.ndim == 1:
        D = D[:, None]
    if D.ndim != 2 or D.shape[0] != n:
        raise ValueError(f"updown: W has shape {D.shape}, the matrix {n} rows")
    cols, rows = np.nonzero(D.T)
    Wp = np.zeros(D.shape[1] + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=D.shape[1]), out=Wp[1:])
    return Wp, rows.astype(np.int32), np.ascontiguousarray(D.T[cols, rows]), D.shape[1]


class Symbolic:
    """Host symbolic analysis (schol + supernodal plan).  ``schur=idx``: a Schur analysis
    (sc_analyze_schur) that orders the distinct rows ``idx`` last, in the given order, for
    :meth:`Numeric.schur_complement` and the partial solves."""

    def __init__(self, A: csc_matrix, options: Optional[Options] = None, schur=None, **kw):
        self.A = A
        self.opt = options if options is not None else default_options(**kw)
        h = C.c_void_p()
        if schur is None:
            _check(lib().sc_analyze(A.size(), _ptr(A.p), _ptr(A.i), C.byref(self.opt), C.byref(h)), "analyze")
        else:
            idx = np.ascontiguousarray(schur, dtype=np.int32).reshape(-1)
            _check(lib().sc_analyze_schur(A.size(), _ptr(A.p), _ptr(A.i), C.byref(self.opt), len(idx),
                                          _ptr(idx) if len(idx) else None, C.byref(h)), "analyze_schur")
        self.h = h
        self.n = A.size()

    def schur_indices(self) -> np.ndarray:
        """The index set of a Schur analysis in the caller's order (empty for a plain one)."""
        ns = _check(lib().sc_symbolic_schur(self.h, None), "schur_indices")
        idx = np.zeros(max(ns, 1), dtype=np.int32)
        _check(lib().sc_symbolic_schur(self.h, _ptr(idx)), "schur_indices")
        return idx[:ns]

    def spmv_structure(self) -> tuple:
        """The full symmetric A the analysis saw (entries with row > column ignored, of
        duplicates the last one, mirrored), by rows in A's own numbering: (rp, ci, sp) with
        ascending columns ci per row and sp the index of each value in the value array
        (sc_spmv_structure).  Host only."""
        rp = np.zeros(self.n + 1, dtype=np.int64)
        nz = _check(lib().sc_spmv_structure(self.h, _ptr(rp), None, None), "spmv_structure")
        ci = np.zeros(max(nz, 1), dtype=np.int32)
        sp = np.zeros(max(nz, 1), dtype=np.int64)
        assert _check(lib().sc_spmv_structure(self.h, _ptr(rp), _ptr(ci), _ptr(sp)), "spmv_structure") == nz
        return rp, ci[:nz], sp[:nz]

    def value_entries(self) -> tuple:
        """(rows, cols, effective), one entry per slot of the value array: the slot's row and
        column as given, and whether the analysis uses it (row <= column, of duplicates the
        last one -- the slots :meth:`spmv_structure`'s sp names).  Gradients are zero on the
        other slots (sc_value_entries).  Host only."""
        nnz = _check(lib().sc_value_entries(self.h, None, None, None), "value_entries")
        rows = np.zeros(max(nnz, 1), dtype=np.int32)
        cols = np.zeros(max(nnz, 1), dtype=np.int32)
        eff = np.zeros(max(nnz, 1), dtype=np.int32)
        assert _check(lib().sc_value_entries(self.h, _ptr(rows), _ptr(cols), _ptr(eff)), "value_entries") == nnz
        return rows[:nnz], cols[:nnz], eff[:nnz].astype(bool)

    def stats(self) -> dict:
        st = SymbolicStats()
        _check(lib().sc_symbolic_get_stats(self.h, C.byref(st)), "stats")
        return st.as_dict()

    @property
    def nnz_L(self) -> int:
        return int(lib().sc_nnz_L(self.h))

    @property
    def flops(self) -> float:
        return float(lib().sc_flops(self.h))

    def selinv_flops(self) -> float:
        """Dense flops of the selected inversion's sweep (C ABI sc_selinv_flops)."""
        v = C.c_double()
        _check(lib().sc_selinv_flops(self.h, C.byref(v)), "selinv_flops")
        return v.value

    def pattern(self):
        Lp = np.zeros(self.n + 1, dtype=np.int64)
        Li = np.zeros(max(self.nnz_L, 1), dtype=np.int32)
        _check(lib().sc_symbolic_pattern(self.h, _ptr(Lp), _ptr(Li)), "pattern")
        return Lp, Li[: self.nnz_L]

    def perm(self) -> np.ndarray:
        """Ordering in effect, perm[new] = old (identity unless ordering=SC_ORDER_ND)."""
        p = np.zeros(max(self.n, 1), dtype=np.int32)
        _check(lib().sc_symbolic_perm(self.h, _ptr(p)), "perm")
        return p[: self.n]

    def etree(self):
        parent = np.zeros(self.n, dtype=np.int32)
        post = np.zeros(self.n, dtype=np.int32)
        _check(lib().sc_symbolic_etree(self.h, _ptr(parent), _ptr(post)), "etree")
        return parent, post

    def supernodes(self):
        """dict(start, m, w, parent, level) of the device supernode partition (postorder numbering)."""
        ns = self.stats()["n_supernodes"]
        st = np.zeros(ns + 1, dtype=np.int32)
        m = np.zeros(max(ns, 1), dtype=np.int32)
        par = np.zeros(max(ns, 1), dtype=np.int32)
        lev = np.zeros(max(ns, 1), dtype=np.int32)
        _check(lib().sc_symbolic_supernodes(self.h, _ptr(st), _ptr(m), _ptr(par), _ptr(lev)), "supernodes")
        return dict(start=st, m=m[:ns], w=np.diff(st), parent=par[:ns], level=lev[:ns])

    def updown_check(self, W) -> tuple:
        """Admissibility of W for :meth:`Numeric.update` / :meth:`Numeric.downdate`, on the host
        alone: ``(first_col, path)`` with ``first_col[c]`` the first row of column c in the order
        of P A P^T (-1: empty column) and ``path`` a dict of what one sweep touches:
        ``supernodes``, ``blocks`` (64-column block steps) and ``panel_entries`` (sum of m w).
        W as for :meth:`Numeric.updown`.  Raises :class:`LibraryError` naming the column and
        the row when a column is not admissible."""
        Wp, Wi, _, k = _updown_W(W, self.n)
        first = np.zeros(max(k, 1), dtype=np.int32)
        path = np.zeros(3, dtype=np.int64)
        _check(lib().sc_updown_check(self.h, k, _ptr(Wp), _ptr(Wi), _ptr(first), _ptr(path)), "updown_check")
        return first[:k], dict(supernodes=int(path[0]), blocks=int(path[1]), panel_entries=int(path[2]))

    def owner_map(self, nranks: int):
        ns = self.stats()["n_supernodes"]
        own = np.zeros(max(ns, 1), dtype=np.int32)
        work = np.zeros(nranks, dtype=np.float64)
        _check(lib().sc_dist_owner_map(self.h, nranks, _ptr(own), _ptr(work)), "owner_map")
        return own[:ns], work

    def dist_plan_info(self, nranks: int) -> dict:
        """Multi-GPU plan summary: rank-group size per supernode, CB ranks of split fronts,
        slab ranks of distributed panels, comm steps and total messages."""
        ns = self.stats()["n_supernodes"]
        g = np.zeros(max(ns, 1), dtype=np.int32)
        cbr = np.zeros(max(ns, 1), dtype=np.int32)
        slr = np.zeros(max(ns, 1), dtype=np.int32)
        nst = C.c_int64()
        nmsg = _check(lib().sc_dist_plan_info(self.h, nranks, _ptr(g), _ptr(cbr), _ptr(slr), C.byref(nst)),
                      "dist_plan_info")
        return dict(gsize=g[:ns], split_cb_ranks=cbr[:ns], slab_ranks=slr[:ns], n_steps=nst.value, n_msgs=nmsg)

    def memory_plan(self, nranks: int = 1) -> dict:
        """Device memory plan without a device: per rank the panel arena (L), the
        interval-planned work arena (contribution blocks) and its lower bound, bytes."""
        pb, wb, lb = (np.zeros(nranks, dtype=np.int64) for _ in range(3))
        _check(lib().sc_memory_plan(self.h, nranks, _ptr(pb), _ptr(wb), _ptr(lb)), "memory_plan")
        return dict(panel=pb, work=wb, work_lower_bound=lb)

    def schedule_digest(self, nranks: int = 1, rank: int = 0, emulate: int = 0) -> dict:
        """Digest of the launch schedule a :class:`Numeric` of this analysis would build, computed
        on the host (no GPU): ``hash`` (hex) over every decoded launch and every uploaded task
        array, ``calls`` per kind (:data:`CALL_KINDS`) and the counters.  ``emulate``: 0 one real
        rank, 1 every rank in this process (``virtual=True``), 2 the same with ``rccl_self=True``."""
        return _digest_dict(lambda out, n: lib().sc_debug_schedule_digest(self.h, nranks, rank, emulate, out, n),
                            "schedule_digest")

    def syrk_launches(self, nranks: int = 1, rank: int = 0, emulate: int = 0):
        """The SYRK launches of the schedule :meth:`schedule_digest` plans (same arguments), in
        schedule order: one dict per launch with ``kind`` ("panel" or "cb"), ``bt``, ``lean``,
        ``epi``, ``pf``, ``tail``, ``tiles`` and ``gather`` (any task gathers its children)."""
        n = _check(lib().sc_debug_schedule_syrk(self.h, nranks, rank, emulate, None, 0), "syrk_launches")
        v = np.zeros(max(n, 1), dtype=np.int64)
        assert _check(lib().sc_debug_schedule_syrk(self.h, nranks, rank, emulate, _ptr(v), n), "syrk_launches") == n
        keys = ("kind", "bt", "lean", "epi", "pf", "tail", "tiles", "gather")
        out = [dict(zip(keys, row)) for row in v[:n].reshape(-1, 8).tolist()]
        for d in out:
            d["kind"] = "cb" if d["kind"] else "panel"
        return out

    def dist_steps(self, nranks: int) -> dict:
        """The plan's comm steps in order: kind (0 INIT, 1 SLAB, 2 DELIVER), level, front,
        slab / column group k and slab piece p."""
        n = _check(lib().sc_dist_steps(self.h, nranks, None, None, None, None, None, 0), "dist_steps")
        k, l, f, sk, sp = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(5))
        _check(lib().sc_dist_steps(self.h, nranks, _ptr(k), _ptr(l), _ptr(f), _ptr(sk), _ptr(sp), n), "dist_steps")
        return dict(kind=k[:n], level=l[:n], front=f[:n], k=sk[:n], p=sp[:n])

    def dist_schedule(self, nranks: int, rank: int):
        """This rank's messages in posting order: (comm step, peer, bytes, is_send)."""
        cnt = _check(lib().sc_dist_schedule(self.h, nranks, rank, None, None, None, None, 0), "dist_schedule")
        lev = np.zeros(max(cnt, 1), dtype=np.int32)
        peer = np.zeros(max(cnt, 1), dtype=np.int32)
        nb = np.zeros(max(cnt, 1), dtype=np.int64)
        snd = np.zeros(max(cnt, 1), dtype=np.int32)
        _check(lib().sc_dist_schedule(self.h, nranks, rank, _ptr(lev), _ptr(peer), _ptr(nb), _ptr(snd), cnt),
               "dist_schedule")
        return lev[:cnt], peer[:cnt], nb[:cnt], snd[:cnt]

    def __del__(self):
        h = getattr(self, "h", None)
        if h and _lib is not None:
            _lib.sc_free_symbolic(h)
            self.h = None


class Numeric:
    """Device factorization handle (pools + level schedule on one HIP device)."""

    def __init__(self, symb: Symbolic, device: int = -1, rank: int = 0, nranks: int = 1,
                 uid: Optional[bytes] = None, virtual: bool = False, transport=None, rccl_self: bool = False):
        """nranks > 1 with ``uid`` (from :func:`dist_unique_id` on rank 0): this process is
        ``rank`` of a subtree-partitioned multi-GPU factorization over RCCL.  ``virtual=True``
        runs all ``nranks`` ranks in this one process, each with its own memory; every
        message of the plan moves between them (device copies, or with ``rccl_self=True``
        RCCL send/receive to self on a 1-rank communicator).  ``transport`` (e.g.
        :class:`GlooHostTransport`): the multi-process protocol with every transfer staged
        through host memory instead of RCCL (tests; ranks may share a GPU)."""
        self.symb = symb
        self.rank, self.nranks = rank, nranks
        self.transport = transport
        h = C.c_void_p()
        if transport == "dry":
            _check(lib().sc_numeric_create_dist_dry(symb.h, device, rank, nranks, C.byref(h)),
                   "numeric_create_dist_dry")
        elif transport is not None:
            _check(lib().sc_numeric_create_dist_host(symb.h, device, rank, nranks, C.cast(transport.fn, C.c_void_p),
                                                     None, C.byref(h)), "numeric_create_dist_host")
        elif virtual:
            _check(lib().sc_numeric_create_dist_emulated(symb.h, device, nranks, 1 if rccl_self else 0, C.byref(h)),
                   "numeric_create_dist_emulated")
        elif nranks > 1:
            assert uid is not None and len(uid) == 128
            idbuf = C.create_string_buffer(uid, 128)
            _check(lib().sc_numeric_create_dist(symb.h, device, rank, nranks, idbuf, C.byref(h)),
                   "numeric_create_dist")
        else:
            _check(lib().sc_numeric_create(symb.h, device, C.byref(h)), "numeric_create")
        self.h = h

    def factor(self, Ax: np.ndarray) -> int:
        Ax = np.ascontiguousarray(Ax, dtype=np.float64)
        return _check(lib().sc_factor(self.h, _ptr(Ax)), "factor")

    def factor_device(self, d_Ax_ptr: int, sync: bool = True) -> int:
        return _check(lib().sc_factor_device(self.h, C.c_void_p(d_Ax_ptr), 1 if sync else 0), "factor_device")

    def status(self) -> int:
        return _check(lib().sc_numeric_status(self.h), "status")

    def set_profile(self, on=True):
        """True/1: HIP events around every launch (eager); 2: timestamp kernels around the
        CB SYRK launches only (compatible with hipGraph replay); False/0: off."""
        _check(lib().sc_numeric_set_profile(self.h, int(on)), "set_profile")

    def timing(self) -> np.ndarray:
        t = np.zeros(8)
        _check(lib().sc_numeric_timing(self.h, _ptr(t), 8), "timing")
        return t

    def level_times(self) -> np.ndarray:
        nl = self.symb.stats()["n_levels"]
        t = np.zeros(max(nl, 1))
        _check(lib().sc_numeric_level_times(self.h, _ptr(t), nl), "level_times")
        return t[:nl]

    def launch_trace(self) -> dict:
        n = _check(lib().sc_numeric_launch_trace(self.h, None, None, None, None, None, 0), "launch_trace")
        k, l, st = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(3))
        ms, fl = np.zeros(max(n, 1)), np.zeros(max(n, 1))
        _check(lib().sc_numeric_launch_trace(self.h, _ptr(k), _ptr(l), _ptr(st), _ptr(ms), _ptr(fl), n), "trace")
        return dict(kind=k[:n], level=l[:n], stream=st[:n], ms=ms[:n], flops=fl[:n])

    def syrk_stats(self, wmin: int = 256):
        fl, ms, nl = C.c_double(), C.c_double(), C.c_int64()
        _check(lib().sc_numeric_syrk_stats(self.h, wmin, C.byref(fl), C.byref(ms), C.byref(nl)), "syrk_stats")
        return fl.value, ms.value, nl.value

    def launch_times(self) -> dict:
        """Per launch of the last profiled factorization: start / end ms (from the first
        main-stream launch), kind, comm step index (-1 if not a comm launch)."""
        n = _check(lib().sc_numeric_launch_times(self.h, None, None, None, None, None, 0), "launch_times")
        t0, t1 = np.zeros(max(n, 1)), np.zeros(max(n, 1))
        k, st, sm = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(3))
        _check(lib().sc_numeric_launch_times(self.h, _ptr(t0), _ptr(t1), _ptr(k), _ptr(st), _ptr(sm), n),
               "launch_times")
        return dict(t0=t0[:n], t1=t1[:n], kind=k[:n], step=st[:n], stream=sm[:n])

    def syrk_bytes(self, wmin: int = 256) -> float:
        """Algorithmic HBM bytes of the launches syrk_stats(wmin) selects (C ABI
        sc_numeric_syrk_bytes)."""
        b = C.c_double()
        _check(lib().sc_numeric_syrk_bytes(self.h, wmin, C.byref(b)), "syrk_bytes")
        return b.value

    def memory(self) -> dict:
        """Device memory held, bytes: total, panel arenas, work arenas, work lower bound."""
        v = np.zeros(4, dtype=np.int64)
        _check(lib().sc_numeric_memory(self.h, _ptr(v), 4), "memory")
        return dict(total=int(v[0]), panel=int(v[1]), work=int(v[2]), work_lower_bound=int(v[3]))

    def schedule_digest(self) -> dict:
        """The digest (:meth:`Symbolic.schedule_digest`) of this handle's schedule, hashed at
        creation from what was uploaded."""
        return _digest_dict(lambda out, n: lib().sc_debug_numeric_digest(self.h, out, n), "numeric_digest")

    @property
    def stream(self) -> int:
        return lib().sc_numeric_stream(self.h) or 0

    def export(self) -> tuple:
        n = self.symb.n
        nz = self.symb.nnz_L
        Lp = np.zeros(n + 1, dtype=np.int64)
        Li = np.zeros(max(nz, 1), dtype=np.int32)
        Lx = np.zeros(max(nz, 1), dtype=np.float64)
        st = _check(lib().sc_export_L(self.h, _ptr(Lp), _ptr(Li), _ptr(Lx)), "export_L")
        return st, csc_matrix(n, n, Lp, Li[:nz], Lx[:nz], sym.none)

    def export_cols(self, j0: int, j1: int) -> tuple:
        """Columns [j0, j1) of L from the panels: (cp, ri, rx), column j's rows
        ri[cp[j-j0]:cp[j-j0+1]] (its front's rows from j down, relaxed zeros included)."""
        cp = np.zeros(j1 - j0 + 1, dtype=np.int64)
        tot = _check(lib().sc_export_L_cols(self.h, j0, j1, _ptr(cp), None, None), "export_cols")
        ri = np.zeros(max(tot, 1), dtype=np.int32)
        rx = np.zeros(max(tot, 1), dtype=np.float64)
        _check(lib().sc_export_L_cols(self.h, j0, j1, _ptr(cp), _ptr(ri), _ptr(rx)), "export_cols")
        return cp, ri[:tot], rx[:tot]

    def solve(self, b: np.ndarray) -> np.ndarray:
        """x = A^{-1} b on the GPU (host vectors in / out).  b of shape (n,): one solve
        (sc_solve_host).  b of shape (n, k), any memory order: k right-hand sides through the
        16-column panel solve (sc_solve_host_multi), returned as (n, k); its columns agree
        with the 1-D solve to rounding, not bitwise."""
        if np.ndim(b) == 2:
            B = np.asfortranarray(b, dtype=np.float64)
            n, k = B.shape
            if n != self.symb.n:
                raise ValueError(f"solve: b has {n} rows, the matrix {self.symb.n}")
            X = np.zeros((n, k), dtype=np.float64, order="F")
            ld = max(n, 1)
            st = _check(lib().sc_solve_host_multi(self.h, k, _ptr(B), ld, _ptr(X), ld), "solve")
            if st > 0:
                raise LibraryError(f"solve: A is not positive definite (column {st})")
            return X
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros_like(b)
        st = _check(lib().sc_solve_host(self.h, _ptr(b), _ptr(x)), "solve")
        if st > 0:
            raise LibraryError(f"solve: A is not positive definite (column {st})")
        return x

    def solve_device(self, d_b_ptr: int, d_x_ptr: int) -> int:
        """x = A^{-1} b with device vectors (may alias)."""
        st = _check(lib().sc_solve_device(self.h, C.c_void_p(d_b_ptr), C.c_void_p(d_x_ptr)), "solve_device")
        if st > 0:
            raise LibraryError(f"solve_device: A is not positive definite (column {st})")
        return st

    def solve_device_multi(self, d_B_ptr: int, nrhs: int, ldb: int, d_X_ptr: int, ldx: int) -> int:
        """X = A^{-1} B with device arrays, column-major: column j of B at d_B_ptr + 8 j ldb,
        of X at d_X_ptr + 8 j ldx (ldb, ldx >= n; X may be B when ldx == ldb)."""
        st = _check(lib().sc_solve_device_multi(self.h, nrhs, C.c_void_p(d_B_ptr), ldb, C.c_void_p(d_X_ptr), ldx),
                    "solve_device_multi")
        if st > 0:
            raise LibraryError(f"solve_device_multi: A is not positive definite (column {st})")
        return st

    def apply(self, b: np.ndarray, op: int) -> np.ndarray:
        """op(b) with the factor P A P^T = L L^T on the GPU (host arrays in / out); op is one
        of the SC_OP_* constants, L the matrix :meth:`export` returns, in its numbering.  b of
        shape (n,): the single-vector entry point (sc_apply_host); b of shape (n, k): the
        16-column panel family (sc_apply_host_multi), returned as (n, k)."""
        if np.ndim(b) == 2:
            B = np.asfortranarray(b, dtype=np.float64)
            n, k = B.shape
            if n != self.symb.n:
                raise ValueError(f"apply: b has {n} rows, the matrix {self.symb.n}")
            X = np.zeros((n, k), dtype=np.float64, order="F")
            ld = max(n, 1)
            st = _check(lib().sc_apply_host_multi(self.h, int(op), k, _ptr(B), ld, _ptr(X), ld), "apply")
            if st > 0:
                raise LibraryError(f"apply: A is not positive definite (column {st})")
            return X
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.shape[0] != self.symb.n:
            raise ValueError(f"apply: b has {b.shape[0]} rows, the matrix {self.symb.n}")
        x = np.zeros_like(b)
        st = _check(lib().sc_apply_host(self.h, int(op), _ptr(b), _ptr(x)), "apply")
        if st > 0:
            raise LibraryError(f"apply: A is not positive definite (column {st})")
        return x

    def solve_L(self, b: np.ndarray) -> np.ndarray:
        """L^-1 b."""
        return self.apply(b, SC_OP_SOLVE_L)

    def solve_Lt(self, b: np.ndarray) -> np.ndarray:
        """L^-T b."""
        return self.apply(b, SC_OP_SOLVE_LT)

    def mul_L(self, z: np.ndarray) -> np.ndarray:
        """L z."""
        return self.apply(z, SC_OP_MUL_L)

    def mul_Lt(self, z: np.ndarray) -> np.ndarray:
        """L^T z."""
        return self.apply(z, SC_OP_MUL_LT)

    def apply_P(self, b: np.ndarray) -> np.ndarray:
        """P b: x[k] = b[perm[k]] with perm = :meth:`Symbolic.perm`."""
        return self.apply(b, SC_OP_PERM)

    def apply_Pt(self, b: np.ndarray) -> np.ndarray:
        """P^T b: x[perm[k]] = b[k]."""
        return self.apply(b, SC_OP_PERM_T)

    def apply_device(self, op: int, d_b_ptr: int, d_x_ptr: int) -> int:
        """x = op(b) with device vectors (may alias)."""
        st = _check(lib().sc_apply_device(self.h, int(op), C.c_void_p(d_b_ptr), C.c_void_p(d_x_ptr)), "apply_device")
        if st > 0:
            raise LibraryError(f"apply_device: A is not positive definite (column {st})")
        return st

    def apply_device_multi(self, op: int, d_B_ptr: int, nrhs: int, ldb: int, d_X_ptr: int, ldx: int) -> int:
        """X = op(B) with device arrays, column-major as for :meth:`solve_device_multi`."""
        st = _check(lib().sc_apply_device_multi(self.h, int(op), nrhs, C.c_void_p(d_B_ptr), ldb, C.c_void_p(d_X_ptr),
                                                ldx), "apply_device_multi")
        if st > 0:
            raise LibraryError(f"apply_device_multi: A is not positive definite (column {st})")
        return st

    def logdet(self) -> float:
        """log det A = 2 sum_j log L(j, j), reduced on the GPU in a fixed order."""
        v = C.c_double()
        st = _check(lib().sc_logdet(self.h, C.byref(v)), "logdet")
        if st > 0:
            raise LibraryError(f"logdet: A is not positive definite (column {st})")
        return v.value

    def updown(self, W, sign: int) -> int:
        """L <- factor of P (A + sign W W^T) P^T in place on the GPU (sc_updown_host), sign +1
        or -1.  W: a dense (n, k) array whose nonzeros are the pattern, or a CSC triple
        ``(Wp, Wi, Wx)`` (explicit zeros count), rows in A's own numbering; every column must
        be admissible (:meth:`Symbolic.updown_check`).  Returns the status: 0, or the failing
        column + 1 of a downdate that leaves the matrix not positive definite (the handle's
        status until the next :meth:`factor`)."""
        Wp, Wi, Wx, k = _updown_W(W, self.symb.n)
        return _check(lib().sc_updown_host(self.h, int(sign), k, _ptr(Wp), _ptr(Wi), _ptr(Wx)), "updown")

    def update(self, W) -> int:
        """A <- A + W W^T (:meth:`updown` with sign +1)."""
        return self.updown(W, 1)

    def downdate(self, W) -> int:
        """A <- A - W W^T (:meth:`updown` with sign -1)."""
        return self.updown(W, -1)

    def _schur_dense(self, fn, what: str) -> np.ndarray:
        ns = len(self.symb.schur_indices())
        out = np.zeros((ns, ns), dtype=np.float64, order="F")
        st = _check(fn(self.h, _ptr(out), max(ns, 1)), what)
        if st > 0:
            raise LibraryError(f"{what}: A is not positive definite (column {st})")
        return out

    def schur_factor(self) -> np.ndarray:
        """D = L_SS, the (ns, ns) lower-triangular trailing block of L of a Schur analysis, row
        and column q standing for ``schur_indices()[q]``; S_c = D D^T (sc_schur_factor_host)."""
        return self._schur_dense(lib().sc_schur_factor_host, "schur_factor")

    def schur_complement(self) -> np.ndarray:
        """S_c = A_SS - A_SI inv(A_II) A_IS, (ns, ns), exactly symmetric, numbered as
        ``schur_indices()`` (sc_schur_matrix_host)."""
        return self._schur_dense(lib().sc_schur_matrix_host, "schur_complement")

    def schur_factor_device(self, d_D_ptr: int, ldd: int) -> int:
        """:meth:`schur_factor` into device memory, column-major with leading dimension ldd >= ns."""
        return _check(lib().sc_schur_factor_device(self.h, C.c_void_p(d_D_ptr), ldd), "schur_factor_device")

    def schur_complement_device(self, d_S_ptr: int, lds: int) -> int:
        """:meth:`schur_complement` into device memory, column-major with leading dimension lds >= ns."""
        return _check(lib().sc_schur_matrix_device(self.h, C.c_void_p(d_S_ptr), lds), "schur_complement_device")

    def schur_condense(self, B: np.ndarray) -> np.ndarray:
        """G = B_S - A_SI inv(A_II) B_I, the right-hand side of the interface problem S_c X_S = G.
        B of shape (n,) or (n, k) in A's own order; G of shape (ns,) or (ns, k) in the order
        of ``schur_indices()`` (sc_schur_condense_host_multi)."""
        one = np.ndim(B) == 1
        Bf = np.asfortranarray(np.asarray(B, dtype=np.float64).reshape(len(B), -1))
        n, k = Bf.shape
        if n != self.symb.n:
            raise ValueError(f"schur_condense: B has {n} rows, the matrix {self.symb.n}")
        ns = len(self.symb.schur_indices())
        G = np.zeros((ns, k), dtype=np.float64, order="F")
        st = _check(lib().sc_schur_condense_host_multi(self.h, k, _ptr(Bf), max(n, 1), _ptr(G), max(ns, 1)),
                    "schur_condense")
        if st > 0:
            raise LibraryError(f"schur_condense: A is not positive definite (column {st})")
        return G[:, 0].copy() if one else G

    def schur_expand(self, B: np.ndarray, XS: np.ndarray) -> np.ndarray:
        """X with X_S = XS (bit for bit) and X_I = inv(A_II) (B_I - A_IS XS): the solution of
        A X = B when XS solves S_c XS = :meth:`schur_condense` (B).  B (n,) or (n, k), XS (ns,)
        or (ns, k) (sc_schur_expand_host_multi)."""
        one = np.ndim(B) == 1
        Bf = np.asfortranarray(np.asarray(B, dtype=np.float64).reshape(len(B), -1))
        n, k = Bf.shape
        ns = len(self.symb.schur_indices())
        Xs = np.asfortranarray(np.asarray(XS, dtype=np.float64).reshape(ns, -1))
        if n != self.symb.n or Xs.shape[1] != k:
            raise ValueError(f"schur_expand: B is {Bf.shape}, XS {Xs.shape}, the matrix has {self.symb.n} rows")
        X = np.zeros((n, k), dtype=np.float64, order="F")
        st = _check(lib().sc_schur_expand_host_multi(self.h, k, _ptr(Bf), max(n, 1), _ptr(Xs), max(ns, 1), _ptr(X),
                                                     max(n, 1)), "schur_expand")
        if st > 0:
            raise LibraryError(f"schur_expand: A is not positive definite (column {st})")
        return X[:, 0].copy() if one else X

    def schur_condense_device_multi(self, d_B_ptr: int, nrhs: int, ldb: int, d_G_ptr: int, ldg: int) -> int:
        """:meth:`schur_condense` with device arrays, column-major as for :meth:`solve_device_multi`."""
        return _check(lib().sc_schur_condense_device_multi(self.h, nrhs, C.c_void_p(d_B_ptr), ldb, C.c_void_p(d_G_ptr),
                                                           ldg), "schur_condense_device_multi")

    def schur_expand_device_multi(self, d_B_ptr: int, nrhs: int, ldb: int, d_XS_ptr: int, ldxs: int, d_X_ptr: int,
                                  ldx: int) -> int:
        """:meth:`schur_expand` with device arrays (X may be B when ldx == ldb)."""
        return _check(lib().sc_schur_expand_device_multi(self.h, nrhs, C.c_void_p(d_B_ptr), ldb, C.c_void_p(d_XS_ptr),
                                                         ldxs, C.c_void_p(d_X_ptr), ldx), "schur_expand_device_multi")

    def _panel_in(self, A: np.ndarray, what: str):
        """(n,) or (n, k) host input as a Fortran (n, k) array, with whether it was 1-D."""
        one = np.ndim(A) == 1
        F = np.asfortranarray(np.reshape(A, (-1, 1)) if one else A, dtype=np.float64)
        if F.ndim != 2 or F.shape[0] != self.symb.n:
            raise ValueError(f"{what}: the array is {np.shape(A)}, the matrix has {self.symb.n} rows")
        return F, one

    @staticmethod
    def _values(Ax):
        return None if Ax is None else np.ascontiguousarray(Ax, dtype=np.float64)

    def spmv(self, X: np.ndarray, Ax=None) -> np.ndarray:
        """Y = A X on the GPU (host arrays; X (n,) or (n, k), returned in the same shape), A
        being the matrix the analysis saw with the values ``Ax`` (the order :meth:`factor`
        takes), or, with ``Ax=None``, the values of the last :meth:`factor`
        (sc_spmv_host_multi)."""
        Xf, one = self._panel_in(X, "spmv")
        n, k = Xf.shape
        Y = np.zeros((n, k), dtype=np.float64, order="F")
        ld = max(n, 1)
        _check(lib().sc_spmv_host_multi(self.h, k, _ptr(self._values(Ax)), _ptr(Xf), ld, _ptr(Y), ld), "spmv")
        return Y[:, 0] if one else Y

    def residual(self, B: np.ndarray, X: np.ndarray, Ax=None, mode: str = "dd") -> tuple:
        """(R, berr_norm, berr_comp): R = B - A X with, per column, the normwise and the
        componentwise (Oettli-Prager) backward error; ``mode`` "dd" accumulates the residual
        as a compensated dot product, "fp64" in working precision (sc_residual_host_multi).
        B and X (n,) or (n, k); the errors are arrays of k entries (floats for 1-D input)."""
        Bf, one = self._panel_in(B, "residual")
        Xf, _ = self._panel_in(X, "residual")
        if Xf.shape != Bf.shape:
            raise ValueError(f"residual: B is {Bf.shape}, X {Xf.shape}")
        n, k = Bf.shape
        R = np.zeros((n, k), dtype=np.float64, order="F")
        bn, bc = np.zeros(max(k, 1)), np.zeros(max(k, 1))
        ld = max(n, 1)
        _check(lib().sc_residual_host_multi(self.h, _RESIDUAL_MODES[mode], k, _ptr(self._values(Ax)), _ptr(Bf), ld,
                                            _ptr(Xf), ld, _ptr(R), ld, _ptr(bn), _ptr(bc)), "residual")
        return (R[:, 0], float(bn[0]), float(bc[0])) if one else (R, bn[:k], bc[:k])

    @staticmethod
    def _refine_options(max_iter: int, residual: str, rho_max: float) -> RefineOptions:
        o = RefineOptions()
        lib().sc_default_refine_options(C.byref(o))
        o.max_iter, o.residual, o.rho_max = max_iter, _RESIDUAL_MODES[residual], rho_max
        return o

    @staticmethod
    def _refine_info(info, k: int, one: bool) -> dict:
        d = {f: np.array([getattr(info[j], f) for j in range(k)]) for f, _ in RefineInfo._fields_}
        return {f: v[0].item() for f, v in d.items()} if one else d

    def solve_refined(self, B: np.ndarray, Ax=None, max_iter: int = 10, residual: str = "dd",
                      rho_max: float = 0.5) -> tuple:
        """(X, info): X = A^-1 B by the panel solve plus iterative refinement against the
        values ``Ax`` (``None``: those of the last :meth:`factor`), the residual accumulated
        as ``residual`` says ("dd": as if in twice the working precision).  ``info``: a dict
        of arrays over the columns -- iters, state (SC_REFINE_*), berr_norm, berr_comp,
        dx_ratio -- describing the returned X (scalars for 1-D input).  B (n,) or (n, k)
        (sc_solve_refine_host_multi)."""
        Bf, one = self._panel_in(B, "solve_refined")
        n, k = Bf.shape
        X = np.zeros((n, k), dtype=np.float64, order="F")
        info = (RefineInfo * max(k, 1))()
        o = self._refine_options(max_iter, residual, rho_max)
        ld = max(n, 1)
        st = _check(lib().sc_solve_refine_host_multi(self.h, C.byref(o), k, _ptr(self._values(Ax)), _ptr(Bf), ld,
                                                     _ptr(X), ld, info), "solve_refined")
        if st > 0:
            raise LibraryError(f"solve_refined: A is not positive definite (column {st})")
        return (X[:, 0] if one else X), self._refine_info(info, k, one)

    def spmv_device_multi(self, d_Ax_ptr: int, d_X_ptr: int, nrhs: int, ldx: int, d_Y_ptr: int, ldy: int) -> int:
        """:meth:`spmv` with device arrays, column-major as for :meth:`solve_device_multi`;
        d_Ax_ptr 0: the values of the last :meth:`factor`."""
        return _check(lib().sc_spmv_device_multi(self.h, nrhs, C.c_void_p(d_Ax_ptr or None), C.c_void_p(d_X_ptr), ldx,
                                                 C.c_void_p(d_Y_ptr), ldy), "spmv_device_multi")

    def residual_device_multi(self, d_Ax_ptr: int, d_B_ptr: int, nrhs: int, ldb: int, d_X_ptr: int, ldx: int,
                              d_R_ptr: int, ldr: int, mode: str = "dd") -> tuple:
        """:meth:`residual` with device arrays; returns (berr_norm, berr_comp), host arrays."""
        bn, bc = np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1))
        _check(lib().sc_residual_device_multi(self.h, _RESIDUAL_MODES[mode], nrhs, C.c_void_p(d_Ax_ptr or None),
                                              C.c_void_p(d_B_ptr), ldb, C.c_void_p(d_X_ptr), ldx, C.c_void_p(d_R_ptr),
                                              ldr, _ptr(bn), _ptr(bc)), "residual_device_multi")
        return bn[:nrhs], bc[:nrhs]

    def solve_refined_device_multi(self, d_Ax_ptr: int, d_B_ptr: int, nrhs: int, ldb: int, d_X_ptr: int, ldx: int,
                                   max_iter: int = 10, residual: str = "dd", rho_max: float = 0.5) -> dict:
        """:meth:`solve_refined` with device arrays (X must not be B); returns the info dict."""
        info = (RefineInfo * max(nrhs, 1))()
        o = self._refine_options(max_iter, residual, rho_max)
        st = _check(lib().sc_solve_refine_device_multi(self.h, C.byref(o), nrhs, C.c_void_p(d_Ax_ptr or None),
                                                       C.c_void_p(d_B_ptr), ldb, C.c_void_p(d_X_ptr), ldx, info),
                    "solve_refined_device_multi")
        if st > 0:
            raise LibraryError(f"solve_refined_device_multi: A is not positive definite (column {st})")
        return self._refine_info(info, nrhs, False)

    @staticmethod
    def _pcg_options(tol: float, max_iter: int, use_x0: bool) -> PcgOptions:
        o = PcgOptions()
        lib().sc_default_pcg_options(C.byref(o))
        o.tol, o.max_iter, o.use_x0 = tol, max_iter, int(use_x0)
        return o

    @staticmethod
    def _pcg_info(info, k: int, one: bool) -> dict:
        d = {f: np.array([getattr(info[j], f) for j in range(k)]) for f, _ in PcgInfo._fields_}
        return {f: v[0].item() for f, v in d.items()} if one else d

    def solve_pcg(self, B: np.ndarray, Ax=None, tol: float = 1e-10, max_iter: int = 100, x0=None) -> tuple:
        """(X, info): X = A'^-1 B by conjugate gradients on the values ``Ax`` (``None``: those
        of the last :meth:`factor`), preconditioned with the factor this handle holds, until
        the 2-norm of the residual is at most ``tol`` times that of B's column.  ``x0``: a
        starting array of B's shape (``None``: the panel solve of B).  ``info``: a dict of
        arrays over the columns -- iters, state (SC_PCG_*), relres, relres_true, berr_norm,
        berr_comp -- describing the returned X (scalars for 1-D input).  B (n,) or (n, k)
        (sc_solve_pcg_host_multi)."""
        Bf, one = self._panel_in(B, "solve_pcg")
        n, k = Bf.shape
        if x0 is None:
            X = np.zeros((n, k), dtype=np.float64, order="F")
        else:
            X0, _ = self._panel_in(x0, "solve_pcg")
            if X0.shape != Bf.shape:
                raise ValueError(f"solve_pcg: B is {Bf.shape}, x0 {X0.shape}")
            X = np.array(X0, dtype=np.float64, order="F", copy=True)
        info = (PcgInfo * max(k, 1))()
        o = self._pcg_options(tol, max_iter, x0 is not None)
        ld = max(n, 1)
        st = _check(lib().sc_solve_pcg_host_multi(self.h, C.byref(o), k, _ptr(self._values(Ax)), _ptr(Bf), ld,
                                                  _ptr(X), ld, info), "solve_pcg")
        if st > 0:
            raise LibraryError(f"solve_pcg: A is not positive definite (column {st})")
        return (X[:, 0] if one else X), self._pcg_info(info, k, one)

    def solve_pcg_device_multi(self, d_Ax_ptr: int, d_B_ptr: int, nrhs: int, ldb: int, d_X_ptr: int, ldx: int,
                               tol: float = 1e-10, max_iter: int = 100, use_x0: bool = False) -> dict:
        """:meth:`solve_pcg` with device arrays (X must not be B; with ``use_x0`` X holds the
        starting vectors); returns the info dict."""
        info = (PcgInfo * max(nrhs, 1))()
        o = self._pcg_options(tol, max_iter, use_x0)
        st = _check(lib().sc_solve_pcg_device_multi(self.h, C.byref(o), nrhs, C.c_void_p(d_Ax_ptr or None),
                                                    C.c_void_p(d_B_ptr), ldb, C.c_void_p(d_X_ptr), ldx, info),
                    "solve_pcg_device_multi")
        if st > 0:
            raise LibraryError(f"solve_pcg_device_multi: A is not positive definite (column {st})")
        return self._pcg_info(info, nrhs, False)

    @staticmethod
    def _eigs_options(sigma: float, tol: float, max_blocks: int, use_x0: bool, seed: int) -> EigsOptions:
        o = EigsOptions()
        lib().sc_default_eigs_options(C.byref(o))
        o.sigma, o.tol, o.max_blocks, o.use_x0, o.seed = sigma, tol, max_blocks, int(use_x0), seed
        return o

    @staticmethod
    def _eigs_info(info, k: int) -> dict:
        return {f: np.array([getattr(info[j], f) for j in range(k)]) for f, _ in EigsInfo._fields_}

    def eigsh(self, nev: int, *, sigma: float = 0.0, tol: float = 1e-10, max_blocks: int = 32, X0=None, seed: int = 1,
              values=None, return_info: bool = False):
        """(lam, X): the ``nev`` eigenvalues nearest ``sigma`` of the matrix whose shifted form A -
        sigma I this handle holds the factor of (the smallest of A for ``sigma = 0``), ascending,
        and their unit eigenvectors as the columns of X (n, nev), by block shift-invert Lanczos
        on the GPU with at most ``max_blocks`` basis blocks of 16 columns.  ``X0``: a start block
        (n, k), k >= min(16, n), whose first min(16, n) columns are used (``None``: the library's
        own, a function of ``seed``).  ``values``: the factored values, for the reported
        residuals (``None``: those of the last :meth:`factor`).  With ``return_info`` a third
        result: a dict of arrays over the pairs -- state (SC_EIGS_*), blocks, est, resid
        (sc_eigs_host)."""
        n = self.symb.n
        X = np.zeros((n, nev), dtype=np.float64, order="F")
        lam = np.zeros(max(nev, 0), dtype=np.float64)
        info = (EigsInfo * max(nev, 1))()
        X0f, ld0 = None, max(n, 1)
        if X0 is not None:
            X0f, _ = self._panel_in(X0, "eigsh")
            if X0f.shape[1] < min(16, n):
                raise ValueError(f"eigsh: X0 has {X0f.shape[1]} columns, the start block needs {min(16, n)}")
        o = self._eigs_options(sigma, tol, max_blocks, X0 is not None, seed)
        st = _check(lib().sc_eigs_host(self.h, C.byref(o), nev, _ptr(self._values(values)), _ptr(X0f), ld0, _ptr(lam),
                                       _ptr(X), max(n, 1), info), "eigsh")
        if st > 0:
            raise LibraryError(f"eigsh: A is not positive definite (column {st})")
        return (lam, X, self._eigs_info(info, nev)) if return_info else (lam, X)

    def eigsh_device(self, nev: int, *, sigma: float = 0.0, tol: float = 1e-10, max_blocks: int = 32, X0=None,
                     seed: int = 1, values=None, return_info: bool = False):
        """:meth:`eigsh` with torch tensors on the handle's device: ``values`` a float64 vector,
        ``X0`` an (n, k) float64 tensor (copied unless it is column-major already).  Returns
        lam (a numpy array: the eigenvalues are decided on the host) and X, an (n, nev)
        column-major float64 tensor on the device of the tensors passed (the current one when
        there is none) (sc_eigs_device)."""
        import torch

        n = self.symb.n
        dev = next((t.device for t in (X0, values) if isinstance(t, torch.Tensor)), torch.device("cuda"))

        def check(t, what):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64):
                raise ValueError(f"eigsh_device: {what} must be a float64 tensor on the GPU")

        Xt = torch.zeros((max(nev, 0), n), dtype=torch.float64, device=dev)  # column c of X is row c
        lam = np.zeros(max(nev, 0), dtype=np.float64)
        info = (EigsInfo * max(nev, 1))()
        p0, pv = None, None
        if X0 is not None:
            check(X0, "X0")
            if X0.ndim != 2 or X0.shape[0] != n or X0.shape[1] < min(16, n):
                raise ValueError(f"eigsh_device: X0 is {tuple(X0.shape)}, the start block is ({n}, {min(16, n)})")
            X0t = X0.t().contiguous()
            p0 = X0t.data_ptr()
        if values is not None:
            check(values, "values")
            values = values.contiguous()
            pv = values.data_ptr()
        o = self._eigs_options(sigma, tol, max_blocks, X0 is not None, seed)
        st = _check(lib().sc_eigs_device(self.h, C.byref(o), nev, C.c_void_p(pv), C.c_void_p(p0), max(n, 1), _ptr(lam),
                                         C.c_void_p(Xt.data_ptr() if nev > 0 and n > 0 else None), max(n, 1), info),
                    "eigsh_device")
        if st > 0:
            raise LibraryError(f"eigsh_device: A is not positive definite (column {st})")
        X = Xt.t()
        return (lam, X, self._eigs_info(info, nev)) if return_info else (lam, X)

    def _nvalues(self) -> int:
        return int(self.symb.A.p[self.symb.n]) if self.symb.n > 0 else 0

    def _value_array(self, G, what: str) -> np.ndarray:
        G = np.ascontiguousarray(G, dtype=np.float64)
        if G.shape != (self._nvalues(),):
            raise ValueError(f"{what}: the array is {G.shape}, the value array has {self._nvalues()} entries")
        return G

    def logdet_grad(self) -> np.ndarray:
        """d logdet A / d values: per slot of the value array c inv(A)[i, j], c = 1 on the
        diagonal and 2 off it (a stored entry stands for both mirrored positions), +0.0 on the
        slots the analysis ignores (:meth:`Symbolic.value_entries`).  Gathered on the GPU from
        the Z panel of :meth:`selinv`, which runs first when needed (sc_logdet_grad_host)."""
        G = np.zeros(max(self._nvalues(), 1), dtype=np.float64)
        st = _check(lib().sc_logdet_grad_host(self.h, _ptr(G)), "logdet_grad")
        if st > 0:
            raise LibraryError(f"logdet_grad: A is not positive definite (column {st})")
        return G[:self._nvalues()]

    def logdet_grad_device(self, d_G_ptr: int) -> int:
        """:meth:`logdet_grad` into device memory of the value array's length at ``d_G_ptr``."""
        st = _check(lib().sc_logdet_grad_device(self.h, C.c_void_p(d_G_ptr or None)), "logdet_grad_device")
        if st > 0:
            raise LibraryError(f"logdet_grad_device: A is not positive definite (column {st})")
        return st

    def pattern_outer(self, U: np.ndarray, V: np.ndarray, alpha: float = 1.0, beta: float = 0.0, G=None) -> np.ndarray:
        """Per effective entry (i, j) of the value array: beta G + alpha sum_c (U[i, c] V[j, c]
        + [i != j] U[j, c] V[i, c]), +0.0 on the ignored slots; U and V (n,) or (n, k).  With
        ``beta == 0`` G is not read (and may be None).  Needs no factorization
        (sc_pattern_outer_host)."""
        Uf, _ = self._panel_in(U, "pattern_outer")
        Vf, _ = self._panel_in(V, "pattern_outer")
        if Uf.shape != Vf.shape:
            raise ValueError(f"pattern_outer: U is {Uf.shape}, V {Vf.shape}")
        if G is None:
            if beta != 0.0:
                raise ValueError("pattern_outer: beta != 0 needs G")
            out = np.zeros(max(self._nvalues(), 1), dtype=np.float64)
        else:
            out = np.array(self._value_array(G, "pattern_outer"), copy=True)
            if out.size == 0:
                out = np.zeros(1, dtype=np.float64)
        n, k = Uf.shape
        ld = max(n, 1)
        _check(lib().sc_pattern_outer_host(self.h, alpha, k, _ptr(Uf), ld, _ptr(Vf), ld, beta, _ptr(out)),
               "pattern_outer")
        return out[:self._nvalues()]

    def pattern_outer_device(self, d_U_ptr: int, d_V_ptr: int, nrhs: int, ldu: int, ldv: int, d_G_ptr: int,
                             alpha: float = 1.0, beta: float = 0.0) -> int:
        """:meth:`pattern_outer` with device arrays, column-major as for :meth:`solve_device_multi`."""
        return _check(lib().sc_pattern_outer_device(self.h, alpha, nrhs, C.c_void_p(d_U_ptr or None), ldu,
                                                    C.c_void_p(d_V_ptr or None), ldv, beta,
                                                    C.c_void_p(d_G_ptr or None)), "pattern_outer_device")

    def pattern_dot(self, G: np.ndarray, H: np.ndarray) -> float:
        """sum of G[k] H[k] over the effective entries, on the GPU in a fixed tree; with
        G = :meth:`logdet_grad` and H = dA the directional derivative tr(inv(A) dA)
        (sc_pattern_dot_host)."""
        Gf, Hf = self._value_array(G, "pattern_dot"), self._value_array(H, "pattern_dot")
        out = _D(0.0)
        _check(lib().sc_pattern_dot_host(self.h, _ptr(Gf) if Gf.size else None, _ptr(Hf) if Hf.size else None,
                                         C.byref(out)), "pattern_dot")
        return out.value

    def pattern_dot_device(self, d_G_ptr: int, d_H_ptr: int) -> float:
        """:meth:`pattern_dot` with device arrays; the result comes back to the host."""
        out = _D(0.0)
        _check(lib().sc_pattern_dot_device(self.h, C.c_void_p(d_G_ptr or None), C.c_void_p(d_H_ptr or None),
                                           C.byref(out)), "pattern_dot_device")
        return out.value

    def solve_grad(self, Xbar: np.ndarray, X: np.ndarray) -> tuple:
        """(Bbar, G) for X = inv(A) B and an upstream gradient ``Xbar``: Bbar = inv(A) Xbar, the
        gradient with respect to B (the panel solve, as :meth:`solve` of a 2-D array returns it),
        and G = -:meth:`pattern_outer` (Bbar, X), the gradient with respect to the value array.
        Xbar and X (n,) or (n, k); Bbar has their shape (sc_solve_grad_host)."""
        Xb, one = self._panel_in(Xbar, "solve_grad")
        Xf, _ = self._panel_in(X, "solve_grad")
        if Xb.shape != Xf.shape:
            raise ValueError(f"solve_grad: Xbar is {Xb.shape}, X {Xf.shape}")
        n, k = Xb.shape
        Bbar = np.zeros((n, k), dtype=np.float64, order="F")
        G = np.zeros(max(self._nvalues(), 1), dtype=np.float64)
        ld = max(n, 1)
        st = _check(lib().sc_solve_grad_host(self.h, k, _ptr(Xb), ld, _ptr(Xf), ld, _ptr(Bbar), ld, _ptr(G)),
                    "solve_grad")
        if st > 0:
            raise LibraryError(f"solve_grad: A is not positive definite (column {st})")
        return (Bbar[:, 0] if one else Bbar), G[:self._nvalues()]

    def solve_grad_device(self, d_Xbar_ptr: int, d_X_ptr: int, nrhs: int, ldxb: int, ldx: int, d_Bbar_ptr: int,
                          ldbb: int, d_G_ptr: int) -> int:
        """:meth:`solve_grad` with device arrays, column-major as for :meth:`solve_device_multi`."""
        st = _check(lib().sc_solve_grad_device(self.h, nrhs, C.c_void_p(d_Xbar_ptr or None), ldxb,
                                               C.c_void_p(d_X_ptr or None), ldx, C.c_void_p(d_Bbar_ptr or None), ldbb,
                                               C.c_void_p(d_G_ptr or None)), "solve_grad_device")
        if st > 0:
            raise LibraryError(f"solve_grad_device: A is not positive definite (column {st})")
        return st

    def selinv(self) -> int:
        """Selected inversion: every entry of A^-1 on the pattern of L into the handle's Z
        panel on the GPU (synchronous; single-device handles).  The accessors below call it
        themselves when no result of the current factorization exists."""
        st = _check(lib().sc_selinv(self.h), "selinv")
        if st > 0:
            raise LibraryError(f"selinv: A is not positive definite (column {st})")
        return st

    def inverse_diagonal(self) -> np.ndarray:
        """diag(A^-1), in A's own order (length n)."""
        d = np.zeros(self.symb.n, dtype=np.float64)
        st = _check(lib().sc_selinv_diag_host(self.h, _ptr(d)), "inverse_diagonal")
        if st > 0:
            raise LibraryError(f"inverse_diagonal: A is not positive definite (column {st})")
        return d

    def inverse_diagonal_device(self, d_ptr: int) -> int:
        """diag(A^-1), in A's own order, into n doubles of device memory at ``d_ptr``."""
        st = _check(lib().sc_selinv_diag_device(self.h, C.c_void_p(d_ptr)), "inverse_diagonal_device")
        if st > 0:
            raise LibraryError(f"inverse_diagonal_device: A is not positive definite (column {st})")
        return st

    def selected_inverse(self) -> tuple:
        """(Lp, Li, Zx): Z = (P A P^T)^-1 on the pattern of L, in :meth:`export`'s layout and
        numbering: Zx[p] = Z[Li[p], j] for p in [Lp[j], Lp[j+1]), Z[k, l] = A^-1[perm[k], perm[l]]."""
        n = self.symb.n
        nz = self.symb.nnz_L
        Lp = np.zeros(n + 1, dtype=np.int64)
        Li = np.zeros(max(nz, 1), dtype=np.int32)
        Zx = np.zeros(max(nz, 1), dtype=np.float64)
        st = _check(lib().sc_selinv_export(self.h, _ptr(Lp), _ptr(Li), _ptr(Zx)), "selected_inverse")
        if st > 0:
            raise LibraryError(f"selected_inverse: A is not positive definite (column {st})")
        return Lp, Li[:nz], Zx[:nz]

    def selected_inverse_cols(self, j0: int, j1: int) -> tuple:
        """Columns [j0, j1) of Z from the Z panel, in :meth:`export_cols`'s form (debug hook
        sc_debug_selinv_cols; for factors too large for :meth:`selected_inverse`)."""
        cp = np.zeros(j1 - j0 + 1, dtype=np.int64)
        tot = _check(lib().sc_debug_selinv_cols(self.h, j0, j1, _ptr(cp), None, None), "selected_inverse_cols")
        ri = np.zeros(max(tot, 1), dtype=np.int32)
        rx = np.zeros(max(tot, 1), dtype=np.float64)
        _check(lib().sc_debug_selinv_cols(self.h, j0, j1, _ptr(cp), _ptr(ri), _ptr(rx)), "selected_inverse_cols")
        return cp, ri[:tot], rx[:tot]

    def selinv_times(self, profile: bool = False) -> dict:
        """Time split (ms) of the last profiled :meth:`selinv` over its kernel classes;
        ``profile`` switches the per-launch HIP events of the next calls on or off."""
        t = np.zeros(4)
        _check(lib().sc_debug_selinv_times(self.h, 1 if profile else 0, _ptr(t)), "selinv_times")
        return dict(W=float(t[0]), Z_RK=float(t[1]), Z_KK=float(t[2]), push=float(t[3]))

    def __del__(self):
        h = getattr(self, "h", None)
        if h and _lib is not None:
            _lib.sc_free_numeric(h)
            self.h = None


class NormalEquations:
    """The weighted normal equations S = C + J^T diag(w) J + diag(d) + damping I of a
    rectangular sparse ``J`` (a :class:`csc_matrix`, m x n, ``S = sym.none``), formed and
    factored on the GPU.  ``base``: the upper-triangular pattern of C as a :class:`csc_matrix`
    (n x n), or ``None``.  The handle holds structure only: J's values (default: ``J.x``), the
    weights, C's values and d come with every call.  Pass :meth:`matrix` to :class:`Symbolic`,
    a :class:`Numeric` of that analysis to :meth:`factor`, and use every solve, refinement,
    ``logdet`` or gradient of that :class:`Numeric` as usual."""

    def __init__(self, J: csc_matrix, base: Optional[csc_matrix] = None, device: int = -1):
        self.J = J
        self.m, self.n = int(J.n_rows), int(J.n_cols)
        self.base = base
        if base is not None and (base.n_rows != self.n or base.n_cols != self.n):
            raise ValueError(f"NormalEquations: the base is {base.n_rows} x {base.n_cols}, J has {self.n} columns")
        Jp = np.ascontiguousarray(J.p, dtype=np.int64)
        Ji = np.ascontiguousarray(J.i, dtype=np.int32)
        Cp = None if base is None else np.ascontiguousarray(base.p, dtype=np.int64)
        Ci = None if base is None else np.ascontiguousarray(base.i, dtype=np.int32)
        h = C.c_void_p()
        _check(lib().sc_normal_create(self.m, self.n, _ptr(Jp), _ptr(Ji), _ptr(Cp), _ptr(Ci), device, C.byref(h)),
               "normal_create")
        self.h = h
        self.nnz = int(Jp[self.n]) if self.n > 0 else 0
        self.nnz_base = 0 if base is None else int(Cp[self.n]) if self.n > 0 else 0
        self.nvalues = _check(lib().sc_normal_pattern(self.h, None, None), "normal_pattern")

    @staticmethod
    def constants() -> dict:
        """The boundaries between the form kernel's mappings and the products' chunk."""
        v = np.zeros(4, dtype=np.int32)
        _check(lib().sc_normal_constants(_ptr(v), 4), "normal_constants")
        return dict(short=int(v[0]), lanes=int(v[1]), chunk=int(v[2]), product_chunk=int(v[3]))

    def matrix(self) -> csc_matrix:
        """The pattern of S as an upper :class:`csc_matrix` (values zero), for :class:`Symbolic`."""
        Sp = np.zeros(self.n + 1, dtype=np.int64)
        Si = np.zeros(max(self.nvalues, 1), dtype=np.int32)
        _check(lib().sc_normal_pattern(self.h, _ptr(Sp), _ptr(Si)), "normal_pattern")
        return csc_matrix(self.n, self.n, Sp, Si[:self.nvalues], np.zeros(self.nvalues), sym.upper)

    @property
    def terms(self) -> int:
        return _check(lib().sc_normal_terms(self.h), "normal_terms")

    def term_lists(self) -> tuple:
        """(tp, pa, pb, r, cpos): entry e of :meth:`matrix` sums the terms [tp[e], tp[e + 1]),
        term t being J.x[pa[t]] w[r[t]] J.x[pb[t]]; cpos[e]: the entry's position in the base's
        values, or -1.  Host only."""
        T = self.terms
        tp = np.zeros(self.nvalues + 1, dtype=np.int64)
        pa, pb, r = (np.zeros(max(T, 1), dtype=np.int32) for _ in range(3))
        cpos = np.zeros(max(self.nvalues, 1), dtype=np.int64)
        _check(lib().sc_normal_term_lists(self.h, _ptr(tp), _ptr(pa), _ptr(pb), _ptr(r), _ptr(cpos)), "normal_term_lists")
        return tp, pa[:T], pb[:T], r[:T], cpos[:self.nvalues]

    def rows(self) -> tuple:
        """J by rows: (rp, ci, sp) with ascending columns ci per row and sp the position of each
        value in J's value array (sc_normal_rows).  Host only."""
        rp = np.zeros(self.m + 1, dtype=np.int64)
        ci = np.zeros(max(self.nnz, 1), dtype=np.int32)
        sp = np.zeros(max(self.nnz, 1), dtype=np.int64)
        _check(lib().sc_normal_rows(self.h, _ptr(rp), _ptr(ci), _ptr(sp)), "normal_rows")
        return rp, ci[:self.nnz], sp[:self.nnz]

    def memory(self) -> dict:
        v = np.zeros(4, dtype=np.int64)
        _check(lib().sc_normal_memory(self.h, _ptr(v), 4), "normal_memory")
        return dict(host_bytes=int(v[0]), device_bytes=int(v[1]), terms=int(v[2]), entries=int(v[3]))

    def _vec(self, a, count: int, what: str):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (count,):
            raise ValueError(f"NormalEquations: {what} is {a.shape}, expected ({count},)")
        return a

    def _form_args(self, Jx, w, base_values, d):
        Jx = self._vec(self.J.x if Jx is None else Jx, self.nnz, "Jx")
        return Jx, self._vec(w, self.m, "w"), self._vec(base_values, self.nnz_base, "base_values"), self._vec(d, self.n, "d")

    def values(self, Jx=None, w=None, base_values=None, d=None, damping: float = 0.0) -> np.ndarray:
        """S's values in the order of :meth:`matrix`, formed on the GPU (sc_normal_values_host)."""
        Jx, w, cx, d = self._form_args(Jx, w, base_values, d)
        Sx = np.zeros(self.nvalues, dtype=np.float64)
        _check(lib().sc_normal_values_host(self.h, _ptr(Jx), _ptr(w), _ptr(cx), _ptr(d), float(damping), _ptr(Sx)),
               "normal_values")
        return Sx

    def factor(self, num: "Numeric", Jx=None, w=None, base_values=None, d=None, damping: float = 0.0) -> int:
        """Forms S into the handle's device buffer and factors it with ``num``; returns the
        factorization's status (> 0: not positive definite, the failing column + 1)
        (sc_normal_factor_host)."""
        Jx, w, cx, d = self._form_args(Jx, w, base_values, d)
        return _check(lib().sc_normal_factor_host(self.h, num.h, _ptr(Jx), _ptr(w), _ptr(cx), _ptr(d), float(damping)),
                      "normal_factor")

    @property
    def values_ptr(self) -> int:
        """Device address of the values the last :meth:`factor` formed (0 before the first one)."""
        return int(lib().sc_normal_values_ptr(self.h) or 0)

    def _panel(self, A, rows: int, what: str):
        one = np.ndim(A) == 1
        F = np.asfortranarray(np.reshape(A, (-1, 1)) if one else A, dtype=np.float64)
        if F.ndim != 2 or F.shape[0] != rows:
            raise ValueError(f"{what}: the array is {np.shape(A)}, expected {rows} rows")
        return F, one

    def mul(self, X, Jx=None) -> np.ndarray:
        """Y = J X on the GPU; X (n,) or (n, k) (sc_normal_mul_host_multi)."""
        Xf, one = self._panel(X, self.n, "mul")
        Jx = self._vec(self.J.x if Jx is None else Jx, self.nnz, "Jx")
        k = Xf.shape[1]
        Y = np.zeros((self.m, k), dtype=np.float64, order="F")
        _check(lib().sc_normal_mul_host_multi(self.h, k, _ptr(Jx), _ptr(Xf), max(self.n, 1), _ptr(Y), max(self.m, 1)),
               "normal_mul")
        return Y[:, 0] if one else Y

    def mul_t(self, Y, w=None, Jx=None) -> np.ndarray:
        """G = J^T diag(w) Y on the GPU; Y (m,) or (m, k) (sc_normal_mult_host_multi)."""
        Yf, one = self._panel(Y, self.m, "mul_t")
        Jx = self._vec(self.J.x if Jx is None else Jx, self.nnz, "Jx")
        w = self._vec(w, self.m, "w")
        k = Yf.shape[1]
        G = np.zeros((self.n, k), dtype=np.float64, order="F")
        _check(lib().sc_normal_mult_host_multi(self.h, k, _ptr(Jx), _ptr(w), _ptr(Yf), max(self.m, 1), _ptr(G),
                                               max(self.n, 1)), "normal_mul_t")
        return G[:, 0] if one else G

    @staticmethod
    def _lstsq_info(info, k: int, one: bool) -> dict:
        d = {f: np.array([getattr(info[j], f) for j in range(k)]) for f, _ in LstsqInfo._fields_}
        return {f: v[0].item() for f, v in d.items()} if one else d

    def lstsq(self, num: "Numeric", B, Jx=None, w=None, max_iter: int = 10, residual: str = "dd",
              rho_max: float = 0.5) -> tuple:
        """(X, info): the minimiser of ||W^1/2 (J x - b)||^2 + x^T (C + diag d + damping I) x per
        column of B ((m,) or (m, k)) with the factor ``num`` holds from :meth:`factor`, whose
        ``Jx`` and ``w`` should be passed again: the normal-equations solve plus corrected
        semi-normal steps.  ``info``: iters, state (SC_REFINE_*), grad_norm, resid_norm,
        dx_ratio per column (scalars for 1-D input) (sc_normal_lstsq_host_multi)."""
        Bf, one = self._panel(B, self.m, "lstsq")
        Jx = self._vec(self.J.x if Jx is None else Jx, self.nnz, "Jx")
        w = self._vec(w, self.m, "w")
        k = Bf.shape[1]
        X = np.zeros((self.n, k), dtype=np.float64, order="F")
        info = (LstsqInfo * max(k, 1))()
        o = Numeric._refine_options(max_iter, residual, rho_max)
        st = _check(lib().sc_normal_lstsq_host_multi(self.h, num.h, C.byref(o), k, _ptr(Jx), _ptr(w), _ptr(Bf),
                                                     max(self.m, 1), _ptr(X), max(self.n, 1), info), "normal_lstsq")
        if st > 0:
            raise LibraryError(f"lstsq: S is not positive definite (column {st})")
        return (X[:, 0] if one else X), self._lstsq_info(info, k, one)

    # ---- device forms: float64 torch tensors on the handle's device ----
    @staticmethod
    def _tensor_ptr(t, count, what: str):
        import torch

        if t is None:
            return None, None
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64):
            raise ValueError(f"NormalEquations: {what} must be a float64 tensor on the GPU")
        t = t.contiguous()
        if count is not None and tuple(t.shape) != (count,):
            raise ValueError(f"NormalEquations: {what} is {tuple(t.shape)}, expected ({count},)")
        return t, C.c_void_p(t.data_ptr())

    @staticmethod
    def _torch_done(t):
        # the library works on its own stream and its calls are synchronous: what torch has
        # queued for the arrays (copies by contiguous(), the zero fill of an output) must be
        # done before the pointers are handed over
        import torch

        torch.cuda.current_stream(t.device).synchronize()

    def values_device(self, Jx, w=None, base_values=None, d=None, damping: float = 0.0, out=None):
        """:meth:`values` with torch tensors; returns (or fills ``out``) a float64 vector on the
        device, in the order :meth:`Numeric.factor_device` reads (sc_normal_values_device)."""
        import torch

        Jx, pj = self._tensor_ptr(Jx, self.nnz, "Jx")
        w, pw = self._tensor_ptr(w, self.m, "w")
        cx, pc = self._tensor_ptr(base_values, self.nnz_base, "base_values")
        d, pd = self._tensor_ptr(d, self.n, "d")
        if out is None:
            out = torch.zeros(self.nvalues, dtype=torch.float64, device=Jx.device)
        if not out.is_contiguous():
            raise ValueError("NormalEquations: out must be contiguous")
        _, po = self._tensor_ptr(out, self.nvalues, "out")
        self._torch_done(out)
        _check(lib().sc_normal_values_device(self.h, pj, pw, pc, pd, float(damping), po), "normal_values_device")
        return out

    def factor_device(self, num: "Numeric", Jx, w=None, base_values=None, d=None, damping: float = 0.0) -> int:
        """:meth:`factor` with torch tensors (sc_normal_factor_device)."""
        Jx, pj = self._tensor_ptr(Jx, self.nnz, "Jx")
        w, pw = self._tensor_ptr(w, self.m, "w")
        cx, pc = self._tensor_ptr(base_values, self.nnz_base, "base_values")
        d, pd = self._tensor_ptr(d, self.n, "d")
        self._torch_done(Jx)
        return _check(lib().sc_normal_factor_device(self.h, num.h, pj, pw, pc, pd, float(damping)),
                      "normal_factor_device")

    def _panel_device(self, A, rows: int, what: str):
        import torch

        if not (isinstance(A, torch.Tensor) and A.is_cuda and A.dtype == torch.float64):
            raise ValueError(f"{what}: the panel must be a float64 tensor on the GPU")
        one = A.ndim == 1
        A2 = A.reshape(-1, 1) if one else A
        if A2.ndim != 2 or A2.shape[0] != rows:
            raise ValueError(f"{what}: the tensor is {tuple(A.shape)}, expected {rows} rows")
        return A2.t().contiguous(), one  # row c of the copy is column c: column-major memory

    def _product_device(self, transposed: bool, A, Jx, w, what: str):
        import torch

        nin, nout = (self.m, self.n) if transposed else (self.n, self.m)
        At, one = self._panel_device(A, nin, what)
        Jx, pj = self._tensor_ptr(Jx, self.nnz, "Jx")
        k = At.shape[0]
        Ot = torch.zeros((k, nout), dtype=torch.float64, device=At.device)
        pa = C.c_void_p(At.data_ptr() if nin > 0 and k > 0 else None)
        po = C.c_void_p(Ot.data_ptr() if nout > 0 and k > 0 else None)
        w, pw = self._tensor_ptr(w if transposed else None, self.m, "w")
        self._torch_done(Ot)
        if transposed:
            _check(lib().sc_normal_mult_device_multi(self.h, k, pj, pw, pa, max(nin, 1), po, max(nout, 1)), what)
        else:
            _check(lib().sc_normal_mul_device_multi(self.h, k, pj, pa, max(nin, 1), po, max(nout, 1)), what)
        return Ot[0] if one else Ot.t()

    def mul_device(self, X, Jx):
        """:meth:`mul` with torch tensors; returns a column-major (m, k) tensor."""
        return self._product_device(False, X, Jx, None, "normal_mul_device")

    def mul_t_device(self, Y, Jx, w=None):
        """:meth:`mul_t` with torch tensors; returns a column-major (n, k) tensor."""
        return self._product_device(True, Y, Jx, w, "normal_mul_t_device")

    def lstsq_device(self, num: "Numeric", B, Jx, w=None, max_iter: int = 10, residual: str = "dd",
                     rho_max: float = 0.5) -> tuple:
        """:meth:`lstsq` with torch tensors; returns (X, info), X a column-major (n, k) tensor."""
        import torch

        Bt, one = self._panel_device(B, self.m, "normal_lstsq_device")
        Jx, pj = self._tensor_ptr(Jx, self.nnz, "Jx")
        w, pw = self._tensor_ptr(w, self.m, "w")
        k = Bt.shape[0]
        Xt = torch.zeros((k, self.n), dtype=torch.float64, device=Bt.device)
        info = (LstsqInfo * max(k, 1))()
        o = Numeric._refine_options(max_iter, residual, rho_max)
        self._torch_done(Xt)
        st = _check(lib().sc_normal_lstsq_device_multi(
            self.h, num.h, C.byref(o), k, pj, pw, C.c_void_p(Bt.data_ptr() if self.m > 0 and k > 0 else None),
            max(self.m, 1), C.c_void_p(Xt.data_ptr() if self.n > 0 and k > 0 else None), max(self.n, 1), info),
            "normal_lstsq_device")
        if st > 0:
            raise LibraryError(f"lstsq_device: S is not positive definite (column {st})")
        return (Xt[0] if one else Xt.t()), self._lstsq_info(info, k, one)

    def __del__(self):
        h = getattr(self, "h", None)
        if h and _lib is not None:
            _lib.sc_normal_free(h)
            self.h = None


_XPORT_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64)


class GlooHostTransport:
    """Host-staged transport for :class:`Numeric` over ``torch.distributed`` (gloo):
    every comm step's buffers go device -> host -> gloo isend/irecv -> host -> device.
    For tests and debugging of the multi-process protocol without RCCL (several
    processes may then share one GPU); not a performance path."""

    def __init__(self, group=None):
        import torch.distributed as tdist

        self._dist = tdist
        self._group = group
        self._pending = []
        self.error = None
        self.fn = _XPORT_FN(self._callback)  # kept alive with the transport

    def _callback(self, ctx, op, peer, buf, nbytes):
        try:
            if op == 2:
                for w in self._pending:
                    w.wait()
                self._pending = []
                return 0
            import torch

            t = torch.frombuffer((C.c_char * nbytes).from_address(buf), dtype=torch.uint8)
            if op == 0:
                self._pending.append(self._dist.isend(t, int(peer), group=self._group))
            else:
                self._pending.append(self._dist.irecv(t, int(peer), group=self._group))
            return 0
        except Exception as e:  # reported through the library's status
            self.error = repr(e)
            return 1


def dist_unique_id() -> bytes:
    """RCCL unique id (128 bytes) for sc_numeric_create_dist; create on rank 0, broadcast."""
    buf = C.create_string_buffer(128)
    _check(lib().sc_dist_unique_id(buf), "dist_unique_id")
    return buf.raw


# --------------------------------------------------------------------------
# drop-in entry points
# --------------------------------------------------------------------------
def schol(A: csc_matrix, **kw) -> SChol:
    """Symbolic factorization (chol.hpp:873-946)."""
    s = Symbolic(A, **kw)
    Lp, Li = s.pattern()
    parent, _ = s.etree()
    return SChol(Lp, Li, parent)


def chol(A: csc_matrix, S=None, device: int = -1, **kw) -> Expected:
    """Numeric Cholesky on the GPU (chol.hpp:749-863; README's chol(A, S) form too).

    ``S`` may be a :class:`Symbolic` from a previous analysis of the same pattern.
    Returns an :class:`Expected` holding L (CSC, lower, reference layout) or the
    reference's error string.
    """
    symb = S if isinstance(S, Symbolic) else Symbolic(A, **kw)
    num = Numeric(symb, device)
    st = num.factor(A.x)
    if st > 0:
        return Expected(None, "A is not positive definite.", st)
    _, L = num.export()
    return Expected(L, None, 0)


def chol_sn(A: csc_matrix, **kw) -> Expected:
    """The reference's supernodal entry point (chol.hpp:1407); same GPU path as chol()."""
    return chol(A, **kw)
