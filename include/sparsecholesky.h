/*
 * sparsecholesky.h -- C-ABI of the MI355X-native supernodal sparse Cholesky.
 *
 * This is the drop-in boundary for the numeric path of evanwporter/SparseCholesky.
 * The reference has no FFI: its API is header-only C++ templates
 * (include/chol.hpp).  Each entry point below names the reference interface it
 * replaces (file:line in the reference).  The C++ drop-in header
 * include/sparsecholesky/chol.hpp rebuilds the reference's templates
 * (csc_matrix, SChol, schol, chol, chol_sn, ...) on top of these calls.
 *
 * Conventions
 *   - Plain pointers and sizes only.  Column pointers are int64 (the reference's
 *     int overflows past 2^31-1 nonzeros, chol.hpp:52,765); row indices int32.
 *   - Matrices are CSC.  "A upper" means the reference's csc_matrix<T,sym::upper>
 *     (chol.hpp:134): entries with row > col are ignored, exactly as the
 *     reference's etree/ereach/col_count ignore them (chol.hpp:392,696,539).
 *   - Status: 0 = OK; >0 = 1-based global (natural) column whose pivot was not
 *     positive ("A is not positive definite.", chol.hpp:849-850; LAPACK info
 *     style); <0 = an sc_status error code below.
 *   - The caller owns every host array it passes; the library owns device memory.
 *     One handle per host thread; all device work runs on the stream given at
 *     numeric creation (or the library's own stream).
 */
#ifndef SPARSECHOLESKY_H
#define SPARSECHOLESKY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define SC_VERSION 121 /* still 1.2.1, additive: gradients of logdet and solve on A's pattern sc_value_entries / sc_pattern_outer_host / sc_pattern_outer_device / sc_pattern_dot_host / sc_pattern_dot_device / sc_logdet_grad_host / sc_logdet_grad_device / sc_solve_grad_host / sc_solve_grad_device; still 1.2.1, additive: eigenpairs nearest zero by block shift-invert Lanczos sc_eigs_host / sc_eigs_device / sc_default_eigs_options; still 1.2.1, additive: conjugate gradients preconditioned with the factor sc_solve_pcg_*_multi / sc_default_pcg_options; still 1.2.1, additive: products with A, residuals and iterative refinement sc_spmv_structure / sc_spmv_*_multi / sc_residual_*_multi / sc_solve_refine_*_multi / sc_default_refine_options; still 1.2.1, additive: Schur complement sc_analyze_schur / sc_symbolic_schur / sc_schur_factor_* / sc_schur_matrix_* / sc_schur_condense_*_multi / sc_schur_expand_*_multi; still 1.2.1, additive: rank-k update / downdate sc_updown_check / sc_updown_host; still 1.2.1, additive: selected inversion sc_selinv / sc_selinv_diag_host / sc_selinv_diag_device / sc_selinv_export / sc_selinv_flops; still 1.2.1, additive: the factor operators sc_apply_host / sc_apply_device / sc_apply_host_multi / sc_apply_device_multi (enum sc_factor_op) and sc_logdet; still 1.2.1, additive: sc_solve_host_multi / sc_solve_device_multi (nrhs right-hand sides); 1.2.1:small merged fronts amalgamated past relax_wmax (different supernode partition of some inputs, same L); 1.2.0: persistent slab chain options removed; panel_prefactor, dist_local_pieces and SC_ORDER_AMD added; out-of-range lookahead / inner_order / ordering rejected */

enum sc_status {
    SC_OK = 0,
    SC_ERR_ARG = -1,      /* bad argument / malformed CSC */
    SC_ERR_NOMEM = -2,    /* host allocation failed */
    SC_ERR_HIP = -3,      /* HIP runtime error (device missing, launch failure) */
    SC_ERR_DEVMEM = -4,   /* device allocation failed */
    SC_ERR_STATE = -5,    /* call out of order (e.g. export before factor) */
    SC_ERR_COMM = -6,     /* RCCL / transport error */
    SC_ERR_NOTIMPL = -7,
    SC_ERR_NOTSYM = -8,   /* MatrixMarket input that is not symmetric (general / skew-symmetric) */
    SC_ERR_IO = -9        /* file could not be opened */
};

typedef struct sc_symbolic sc_symbolic;
typedef struct sc_numeric sc_numeric;

/* Analysis options.  Defaults: sc_default_options(), which also sets struct_size;
 * sc_analyze rejects (SC_ERR_ARG) options whose struct_size is not this header's
 * sizeof(sc_options), so a caller built against another layout fails loudly instead
 * of misreading fields. */
typedef struct sc_options {
    int32_t struct_size;     /* sizeof(sc_options) of the caller's header (set by sc_default_options) */
    int32_t relax;           /* 1 = relaxed supernode amalgamation (CHOLMOD-style) */
    int32_t nrelax[3];       /* width thresholds for amalgamation */
    double zrelax[3];        /* zero-fraction thresholds for amalgamation */
    int32_t small_front_max; /* fronts with m <= this run in the fused one-workgroup kernel (clamped to [0, 128]) */
    int32_t panel_nb;        /* inner panel block (potrf/trsm width), 64 */
    int32_t panel_nb_outer;  /* slab width NBO: rank-NBO outer panel updates at slab ends (default 1024) */
    int32_t use_graph;       /* capture the level schedule into a hipGraph and replay it */
    int32_t relax_wmax;      /* a child and its parent that are both wider than this are not amalgamated when
                                the parent has other children (chains still merge; 0 = no limit; default 1) */
    int32_t syrk_tile;       /* 0 = auto (128x128/8 waves for wide, deep updates, else 64x64/4 waves); 64; 128 */
    int32_t lookahead;       /* 0 or 1 (other values: SC_ERR_ARG); 1 (default): at a slab end the next slab's columns are updated on the main stream
                                and every later column on a second stream, overlapping the next slab's
                                POTRF/TRSM chain; 0: the whole trailing update on the main stream */
    int32_t inner_order;     /* updates inside a slab: 0 right-looking (K = 64), 1 recursive (K = 64..NBO/2);
                                other values: SC_ERR_ARG */
    int32_t asm_tile_min_m;  /* fronts with m >= this use the write-once tiled assembly (0 = default 8192) */
    int32_t dist_split;      /* multi-GPU: a shared front with a contribution block keeps its panel on one rank and
                                has its contribution block computed by the other ranks of its group, slab-streamed
                                (1, default); 0: every front on one rank */
    int32_t dist_cbb;        /* multi-GPU: column-block width of contribution-block ownership and transfers (1024) */
    int32_t ordering;        /* SC_ORDER_NATURAL (default: the given order, as the reference), SC_ORDER_ND or
                                SC_ORDER_AMD: factor P A P^T with a nested-dissection / approximate-minimum-degree
                                P (sc_symbolic_perm); L, the pattern and the statistics are then those of P A P^T,
                                solves take and return A's order; other values: SC_ERR_ARG */
    int32_t dist_early;      /* multi-GPU: a large child whose parent runs on another rank computes its CB in
                                4-block column groups and sends each group as soon as it is done (1, default) */
    int32_t dist_panel;      /* multi-GPU: a shared front wider than one slab (panel_nb_outer) has its panel
                                factored 1D slab-cyclic over its rank group, each final slab sent to the ranks
                                that update later slabs or its contribution block (1, default); 0: the panel
                                on the front's owner */
    int32_t cb_gather;       /* 1 (default): a large front's contribution block is not assembled; its CB SYRK
                                gathers the children's entries into each output tile (C = sum - L21 L21^T,
                                written once); 0: assembly writes the whole front, the SYRK updates it */
    int32_t dist_slab_block; /* multi-GPU distributed panels: consecutive slabs per rank in the cyclic deal
                                (default 2: every other slab hand-over is rank-local, off the critical path;
                                capped at slabs / ranks so that every rank of the group gets a block) */
    int32_t trsm_split_wg;   /* a 64-column chain step whose TRSM launch spans more than this many 256-row
                                workgroups (more than the GPU holds at once) factors its diagonal blocks in a
                                launch of their own (one workgroup per block) and the TRSM workgroups load the
                                factored blocks instead of each refactoring them (default 1024; 0: always fused) */
    int32_t syrk_lean_kmax;  /* SYRK launches on 64 x 64 tiles whose deepest K is at most this use the lean
                                kernel instance (K staged 8 deep, 32-row extend-add chunks: half the LDS, six
                                workgroups per CU instead of four); default 128, 0: never */
    int32_t cb_tail_split;   /* 1 (default): the last, partial round of a deep-K CB launch on 128 x 128 tiles
                                runs as 64 x 64 tiles in a launch of its own (a shorter tail); 0: one launch */
    int32_t tiny_dense;      /* 1 (default): on one device, a matrix with n <= 64 factors as one dense n x n
                                lower triangle in a single wave (the symbolic pattern is exact: entries outside
                                it come out as exact zeros and are not exported); 0: the tiny-tree launch */
    int32_t dist_asm;        /* multi-GPU: 1 (default): a shared front with a distributed panel or split CB is
                                assembled where its columns live (each rank its own slabs / CB blocks; child CB
                                columns go straight to the rank owning the parent columns they map into, no
                                assembled-front hand-out); 0: its owner assembles it and sends the pieces */
    int32_t dist_pieces;     /* multi-GPU distributed panels: each final slab is handed over in this many column
                                pieces (default 4: 256 of a 1024-column slab), each sent as soon as the chain has
                                finished it, so the next slab's owner starts updating before the slab is done */
    int32_t dist_local_pieces; /* multi-GPU distributed panels: when a rank owns two consecutive slabs, its update of
                                the second by each finished piece of the first runs on the lookahead stream while
                                the first slab's chain goes on (1, default), instead of after the chain on the
                                main stream (0) */
    int32_t panel_prefactor; /* 1 (default): in the 64-column panel chain, the recursive inner update after a step
                                (K = 64 or 128) also forms and factors the NEXT step's 64 x 64 diagonal block in one
                                extra workgroup, so that step's TRSM loads L11 instead of every TRSM workgroup
                                factoring it (the POTRF runs beside the update's tiles, off the chain's critical
                                path; bitwise-identical factor); 0: every full step fuses its POTRF */
} sc_options;

enum { SC_ORDER_NATURAL = 0, SC_ORDER_ND = 1, SC_ORDER_AMD = 2 };

/* Symbolic statistics (host analysis). */
typedef struct sc_symbolic_stats {
    int64_t n;
    int64_t nnz_A;            /* stored upper entries used */
    int64_t nnz_L;            /* sum of column counts (reference L pattern) */
    double flops;             /* F = sum_j colcount[j]^2 */
    int64_t etree_depth;
    int64_t n_fundamental;    /* supernodes by the reference rule, in postorder */
    int64_t n_supernodes;     /* after relaxed amalgamation */
    int64_t n_levels;         /* assembly-tree height + 1 */
    int64_t max_front_m;
    int64_t max_front_w;
    int64_t panel_entries;    /* sum m*w (L storage incl. relaxed zeros) */
    int64_t cb_entries;       /* sum (m-w)^2 (contribution-block storage) */
    double flops_executed;    /* dense flops the fronts actually execute */
    double flops_syrk_w256;   /* SYRK flops mb*(mb+1)*w of fronts with w >= 256 */
    int64_t n_small_fronts;
    int64_t n_large_fronts;
} sc_symbolic_stats;

/* Version / status text. */
int32_t sc_version(void);
const char* sc_status_string(int64_t status);
void sc_default_options(sc_options* opt);

/* ---------------- host symbolic analysis ----------------
 * Replaces: schol(A)            chol.hpp:873-946  (pattern of L)
 *           etree/post_order/col_count inside chol() and schol()
 *           compute_supernodes / atree / compute_levels  src/chol.cpp:7-136
 * The supernode partition used numerically is the reference rule
 * (src/chol.cpp:75-85) applied in etree postorder, plus relaxed amalgamation.
 */
int64_t sc_analyze(int64_t n, const int64_t* Ap, const int32_t* Ai, const sc_options* opt,
                   sc_symbolic** out);
int64_t sc_symbolic_get_stats(const sc_symbolic* sym, sc_symbolic_stats* stats);
int64_t sc_nnz_L(const sc_symbolic* sym);
double sc_flops(const sc_symbolic* sym);
/* Pattern of L in the reference layout (schol(A).p()/i(), chol.hpp:873-946):
 * Lp[n+1], Li[nnz_L]; lower, diagonal first, rows ascending. */
int64_t sc_symbolic_pattern(const sc_symbolic* sym, int64_t* Lp, int32_t* Li);
/* etree parent (chol.hpp:377) and postorder (chol.hpp:466), natural numbering. */
int64_t sc_symbolic_etree(const sc_symbolic* sym, int32_t* parent, int32_t* post);
/* The relaxed supernode partition used on the device (internal = postorder
 * numbering): sn_start[ns+1] first internal column, sn_m[ns] front rows,
 * sn_parent[ns] assembly-tree parent (-1 = root), level[ns] height.  Any may be NULL. */
int64_t sc_symbolic_supernodes(const sc_symbolic* sym, int32_t* sn_start, int32_t* sn_m, int32_t* sn_parent,
                               int32_t* level);
/* The ordering used: perm[new] = old (identity for SC_ORDER_NATURAL); returns 1
 * when a fill-reducing permutation is in effect, else 0. */
int64_t sc_symbolic_perm(const sc_symbolic* sym, int32_t* perm);
void sc_free_symbolic(sc_symbolic* sym);

/* ---------------- device numeric factorization ----------------
 * Replaces: chol(A)     chol.hpp:749-863  (simplicial, the parity oracle)
 *           chol_sn(A)  chol.hpp:1406-1446 (supernodal: dpotrf_ 1263,
 *                       cblas_dtrsm 1292, cblas_dsyrk 1322, apply_update 1196)
 * sc_numeric_create allocates the device pools for L panels and contribution
 * blocks on HIP device `device` (-1 = current) and builds the level schedule.
 */
int64_t sc_numeric_create(const sc_symbolic* sym, int32_t device, sc_numeric** out);
/* Factor with host values Ax[nnz(A)] (same order as Ai).  Includes H2D copy. */
int64_t sc_factor(sc_numeric* num, const double* Ax);
/* Factor with device-resident values d_Ax (HBM).  Asynchronous on the library
 * stream unless sync != 0; sc_numeric_status() syncs and returns the status. */
int64_t sc_factor_device(sc_numeric* num, const double* d_Ax, int32_t sync);
/* Status of the last factorization: 0, or the 1-based natural column of the first failing
 * pivot (not positive definite): when several pivots fail, the smallest such column, which
 * is what the reference's column-by-column chol() returns, on every kind of handle.  Under
 * a fill-reducing ordering the column is counted in the order of P A P^T (column k there is
 * column perm[k] of A, sc_symbolic_perm), the matrix that is factored: the reference's
 * answer for P A P^T.  COLLECTIVE on a one-rank-per-process handle
 * (sc_numeric_create_dist / _dist_host): the first call after each factorization
 * reduces the minimum failing column over all ranks, so every rank must make it, in
 * the same order relative to the handle's other collective calls -- and so must
 * sc_factor, sc_factor_device(sync != 0), sc_export_L, sc_export_L_cols(rx != NULL)
 * and the solves, which read the status.  A rank that skips it leaves the others
 * waiting.  Later calls before the next factorization are local. */
int64_t sc_numeric_status(sc_numeric* num);
/* Export L in the reference CSC layout (chol() output, chol.hpp:749-863):
 * Lp[n+1], Li[nnz_L], Lx[nnz_L]; any of the three may be NULL.  On a multi-rank
 * handle the call is collective (every rank calls it): the ranks exchange their
 * panels and every rank receives the whole L, as the reference's chol() returns it
 * (chol.hpp:858-862). */
int64_t sc_export_L(sc_numeric* num, int64_t* Lp, int32_t* Li, double* Lx);
/* Columns [j0, j1) of L straight from the supernodal panels (no pattern pass; for
 * factors too large for sc_export_L): column j holds its front's rows from j down
 * (row indices in the same numbering as Lp/Li, relaxed zeros included), values
 * in rx.  cp[j1-j0+1] offsets; ri / rx may be NULL to query the count.  Returns
 * the entry count (>= 0) or an error.  Collective on multi-rank handles when rx != NULL. */
int64_t sc_export_L_cols(sc_numeric* num, int64_t j0, int64_t j1, int64_t* cp, int32_t* ri, double* rx);
/* Device pointer of the library stream (hipStream_t) for event timing. */
void* sc_numeric_stream(sc_numeric* num);
/* Per-phase timing of the last factorization, milliseconds (HIP events):
 * t[0]=total, t[1]=CB transfers (multi-GPU), t[2]=small fronts, t[3]=assembly, t[4]=potrf,
 * t[5]=trsm, t[6]=panel update, t[7]=CB syrk.  sc_numeric_set_profile(num, 1): HIP
 * events around every launch (eager runs; sets use_graph aside); 2: timestamp
 * kernels around the CB SYRK launches only, which also works under hipGraph
 * replay (feeds sc_numeric_syrk_stats). */
int64_t sc_numeric_set_profile(sc_numeric* num, int32_t on);
int64_t sc_numeric_timing(sc_numeric* num, double* t, int32_t nt);
/* Wall time (ms) of each assembly-tree level of the last profiled factorization;
 * returns the number of levels. */
int64_t sc_numeric_level_times(sc_numeric* num, double* ms, int32_t nl);
/* Per-launch trace of the last profiled factorization (kind: 0 small fronts,
 * 1 assembly, 2 potrf, 3 trsm, 4 panel SYRK, 5 CB SYRK, 6 CB transfer); returns
 * the launch count; arrays may be NULL to query it. */
int64_t sc_numeric_launch_trace(sc_numeric* num, int32_t* kind, int32_t* level, int32_t* stream, double* ms,
                                double* flops, int64_t cap);
/* SYRK flops and kernel time (ms) of the last factorization restricted to
 * fronts with w >= wmin (north-star gate: wmin = 256); wmin = 0: every CB launch;
 * wmin = -1: the panel-update launches; wmin = -2: the CB launches on 128 x 128
 * tiles (one kernel instance, comparable with a kernel trace). */
int64_t sc_numeric_syrk_stats(sc_numeric* num, int32_t wmin, double* flops, double* ms,
                              int64_t* launches);
/* Algorithmic HBM bytes of the same launch selection as sc_numeric_syrk_stats: the
 * operand rows read once (8 M K per task), C written once (gathered CB) or read and
 * written (assembled C), and every gathered child's CB entries read once.  A launch
 * whose tail tiles are re-cut into a launch of their own splits its bytes in
 * proportion to the flops. */
int64_t sc_numeric_syrk_bytes(sc_numeric* num, int32_t wmin, double* bytes);
/* Timeline of the last profiled (sc_numeric_set_profile(num, 1)) factorization: per
 * launch its start and end (ms from the first main-stream launch), its kind (the
 * launch-trace kinds; 6 = a comm step), for comm steps the step index of the plan
 * (sc_dist_steps, else -1) and its stream (0 main, 1 lookahead, 2 comm).  Returns the
 * number of launches (t0 == NULL: count only). */
int64_t sc_numeric_launch_times(sc_numeric* num, double* t0, double* t1, int32_t* kind, int32_t* step,
                                int32_t* stream, int64_t cap);
/* Device memory of the handle, bytes: info[0] everything allocated (pools, plan,
 * staging, a gathered factor), info[1] panel arenas (L), info[2] work arenas (the
 * interval-planned contribution blocks), info[3] the work arenas' lower bound (the
 * largest sum of regions live at one level).  n = entries wanted (<= 4). */
int64_t sc_numeric_memory(sc_numeric* num, int64_t* info, int32_t n);
/* The memory plan without a device: per rank (nranks entries each) the panel arena,
 * the work arena and its lower bound, bytes.  nranks = 1: the single-device plan. */
int64_t sc_memory_plan(const sc_symbolic* sym, int32_t nranks, int64_t* panel_bytes, int64_t* work_bytes,
                       int64_t* work_lower_bound_bytes);
/* Test hook: checks the memory plan of every rank (no two regions overlap while both
 * are live, all inside the arena); returns the number of violations (0 = sound). */
int64_t sc_memory_plan_check(const sc_symbolic* sym, int32_t nranks);
void sc_free_numeric(sc_numeric* num);

/* Solve A x = b with the factor on the GPU (not in the reference):
 * level-scheduled supernodal forward (L y = P b) and backward (L^T z = y) sweeps,
 * x = P^T z.  sc_solve_host: host vectors b, x (length n; copies over PCIe);
 * sc_solve_device: device vectors (may alias), synchronous; d_b must be complete
 * on the device when the call is made (the library's stream does not order against
 * the caller's).  Returns the factor's status (> 0: not positive definite, nothing
 * solved).  Multi-rank handles: collective; the first solve after a factorization
 * gathers the whole factor onto every rank, then every rank solves. */
int64_t sc_solve_host(sc_numeric* num, const double* b, double* x);
int64_t sc_solve_device(sc_numeric* num, const double* d_b, double* d_x);
/* X = A^-1 B for nrhs right-hand sides, column-major: column j of B at B + j*ldb (n
 * entries used), of X at X + j*ldx; ldb, ldx >= n.  Any nrhs >= 0: the library works
 * through it in panels of 16 columns (one read of L per sweep and panel instead of
 * one per right-hand side); a last, partial panel is padded with zero columns inside
 * the library, never read from or written to the caller's memory.  The result for a
 * right-hand side is bitwise repeatable and does not depend on how many other
 * columns travel with it or on its position.  These entry points always run the
 * panel kernels, also for nrhs == 1; sc_solve_host / sc_solve_device keep their own
 * kernels and their bits, so the two families agree to rounding, not bitwise.
 * d_X may be d_B when ldx == ldb (in place).  Returns, ordering and collective rules
 * are those of sc_solve_host / sc_solve_device: the factor's status (> 0: not positive
 * definite, nothing solved, X untouched), SC_ERR_STATE before a factorization,
 * collective on multi-rank handles, synchronous.  nrhs == 0 or n == 0: SC_OK, nothing
 * touched.  SC_ERR_ARG (message in sc_last_error): num == NULL, nrhs < 0, ldb < n or
 * ldx < n, a null B or X with nrhs > 0, X == B with ldx != ldb.  The first call
 * allocates the panel work buffers (about 3 * 16 * 8 bytes per row plus the sweeps'
 * scratch, counted in sc_numeric_memory info[0]); single-vector users never pay it. */
int64_t sc_solve_device_multi(sc_numeric* num, int32_t nrhs, const double* d_B, int64_t ldb,
                              double* d_X, int64_t ldx);
int64_t sc_solve_host_multi(sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb,
                            double* X, int64_t ldx);

/* Factor operators on the GPU (CHOLMOD's cholmod_solve systems L, Lt, P, Pt; the
 * products and the log-determinant besides).  P A P^T = L L^T with L exactly the
 * matrix sc_export_L returns, in the same numbering: the order of P A P^T, (P A P^T)[k,
 * l] = A[perm[k], perm[l]] with perm = sc_symbolic_perm (the identity under
 * SC_ORDER_NATURAL, where PERM and PERM_T are copies).  Hence A^-1 = P^T L^-T L^-1 P
 * and A = P^T L L^T P; the etree postorder the kernels work in stays internal. */
enum sc_factor_op {
    SC_OP_SOLVE_A = 0,  /* X = A^-1 B   (what sc_solve_* compute) */
    SC_OP_SOLVE_L = 1,  /* X = L^-1 B */
    SC_OP_SOLVE_LT = 2, /* X = L^-T B */
    SC_OP_MUL_L = 3,    /* X = L B */
    SC_OP_MUL_LT = 4,   /* X = L^T B */
    SC_OP_PERM = 5,     /* X = P B  : X[k] = B[perm[k]] */
    SC_OP_PERM_T = 6    /* X = P^T B: X[perm[k]] = B[k] */
};
/* X = op(B).  The single-vector entry points take vectors of length n and run the
 * single-vector kernels of sc_solve_host / sc_solve_device for the half solves; the
 * _multi entry points take column-major B and X as sc_solve_*_multi do and run the
 * 16-column panel kernels.  The products (SC_OP_MUL_L, SC_OP_MUL_LT) exist as panel
 * kernels only: the single-vector entry points run them on a panel of one column, so a
 * single-vector product equals column 0 of the _multi call bitwise.  SC_OP_SOLVE_A is
 * the sc_solve_* path of the same family.  SC_OP_PERM, SC_OP_SOLVE_L, SC_OP_SOLVE_LT,
 * SC_OP_PERM_T applied in this order give sc_solve_*'s result of the same family
 * bitwise.  Every op: x may be b (X may be B when ldx == ldb); results are bitwise
 * repeatable and a column does not depend on what travels with it.  The products never
 * read the diagonal-block inverses the solves store after a factorization, and give the
 * same bits before and after them.  Returns, argument checks, synchrony and the
 * collective rule on multi-rank handles are those of sc_solve_device /
 * sc_solve_device_multi (status > 0: nothing computed, X untouched; SC_ERR_STATE before
 * a factorization; nrhs == 0 or n == 0: SC_OK); an op outside the enum: SC_ERR_ARG.
 * Device memory: the solves' buffers (a product or a _multi call allocates the panel
 * work buffers where sc_solve_*_multi has not yet) and one int32 per row when a
 * fill-reducing ordering is in effect; nothing else. */
int64_t sc_apply_device(sc_numeric* num, int32_t op, const double* d_b, double* d_x);
int64_t sc_apply_host(sc_numeric* num, int32_t op, const double* b, double* x);
int64_t sc_apply_device_multi(sc_numeric* num, int32_t op, int32_t nrhs, const double* d_B, int64_t ldb,
                              double* d_X, int64_t ldx);
int64_t sc_apply_host_multi(sc_numeric* num, int32_t op, int32_t nrhs, const double* B, int64_t ldb,
                            double* X, int64_t ldx);
/* log det A = 2 sum_j log L(j, j), from the panels' diagonals on the device, reduced in
 * a fixed order: bitwise repeatable across calls and handles.  Status and collective
 * rules of the solves (> 0: *logdet untouched). */
int64_t sc_logdet(sc_numeric* num, double* logdet);

/* Selected inversion on the GPU: the entries of A^-1 that lie on the pattern of L (the
 * marginal variances diag(A^-1) and the covariances between neighbours of a precision
 * matrix A; CHOLMOD-family users know it as the sparse inverse subset).  Takahashi
 * recurrence over the supernodal factor, top-down, as fp64 MFMA products on the fronts
 * already on the device: with Z = (P A P^T)^-1, per 128-column block K of a front's
 * pivots, R the front rows after it and X = inv(L_KK),
 *     W = L_RK X,   Z_RK = -Z_RR W,   Z_KK = X^T X - W^T Z_RK.
 * sc_selinv computes every selected entry into a second panel arena of the handle (the
 * "Z panel", the layout of the L panels), synchronously, on the handle's stream.  L is
 * not overwritten: solves, operators and sc_logdet keep working, with the same bits.
 * Results are bitwise repeatable across calls and handles (no atomics, fixed order).
 * Numbering: sc_selinv_export returns Z in sc_export_L's layout and numbering (the order
 * of P A P^T): Zx[p] = Z[Li[p], j] for p in [Lp[j], Lp[j+1]), Z[k, l] = A^-1[perm[k],
 * perm[l]] with perm = sc_symbolic_perm; any of the three arrays may be NULL.  The
 * diagonal accessors return diag(A^-1) in A's OWN order, length n (host / device memory).
 * An accessor computes first when the Z panel does not belong to the current
 * factorization (never called, or a newer sc_factor since), so it never serves a stale
 * result.  Entries of Z at relaxed-zero positions of the supernodes (L = 0 there, Z in
 * general not) are computed and kept in the Z panel, but are outside the exported pattern.
 * Status rules of the solves: SC_ERR_STATE before a factorization; a failed factorization
 * returns its status > 0 and computes nothing (outputs untouched); n == 0: SC_OK;
 * SC_ERR_ARG for a null handle or output.  Multi-rank and emulated handles: SC_ERR_NOTIMPL
 * with a message in sc_last_error -- the recurrence keeps a front's Z_II block in the work
 * arena, and those arenas are per rank.
 * Device memory, all counted in sc_numeric_memory info[0], allocated at the first call and
 * kept until sc_free_numeric: the Z panel (info[1] bytes again: the factor's size, 26.4 GB
 * for the 128^3 Laplacian), the W scratch (8 bytes times the largest sum of nr nb over the
 * blocks of one step, at most the largest front's m times 128 for the upper levels), the
 * partials of the deep Z_KK products (a product with K = nb + nr > 512 is cut into
 * ceil(K / 256) chunks; 32 KiB per chunk and 64 x 64 tile of the block's lower triangle,
 * the largest sum over one step) and the task lists (16 bytes per block, 8 bytes per 64-row
 * tile of a block's rows below, 16 bytes per Z_KK tile and chunk plus 16 per tile that is
 * cut, 16 bytes per 64 x 64 tile of a contribution block), besides the solves' plan when no solve has run yet.  A later call
 * allocates nothing.  The work arena is only borrowed: the next factorization reuses it.
 * The first call after a factorization also forms the diagonal-block inverses the solves
 * store in L's unused upper triangles, if no solve has yet. */
int64_t sc_selinv(sc_numeric* num);
int64_t sc_selinv_diag_host(sc_numeric* num, double* d);
int64_t sc_selinv_diag_device(sc_numeric* num, double* d_d);
int64_t sc_selinv_export(sc_numeric* num, int64_t* Lp, int32_t* Li, double* Zx);
/* Dense flops the sweep executes, from the symbolic structure alone (no device): the sum
 * over every supernode (m front rows, w pivots) and every block k0 = 0, 128, .. < w, with
 * nb = min(128, w - k0) and nr = m - k0 - nb, of
 *     2 nr nb^2  (W)  +  2 nr^2 nb  (Z_RK)  +  nb (nb + 1) (nb + nr)  (Z_KK, lower triangle). */
int64_t sc_selinv_flops(const sc_symbolic* sym, double* flops);

/* Rank-k update and downdate of the factor on the GPU (CHOLMOD users know it as updown):
 * given P A P^T = L L^T on the handle and a sparse n x k matrix W (CSC, rows in A's own
 * numbering), sc_updown_host replaces L in place by the factor of P (A + sign W W^T) P^T,
 * sign = +1 an update, -1 a downdate, without a new factorization: conditioning a
 * precision matrix on point observations, leave-one-out downdates, active-set steps.
 * The pattern of L does not change, so W must be ADMISSIBLE: every column w, its rows
 * permuted to the order of P A P^T and j0 the smallest of them, has struct(w) within the
 * true pattern of L(:, j0) (what sc_symbolic_pattern returns).  A unit vector always is.
 * sc_updown_check tests that on the host alone (no device; the pattern of L is not formed)
 * and returns first_col[k] (may be NULL: j0 per column in the order of P A P^T, -1 for an
 * empty column) and path[3] (may be NULL: the supernodes on the assembly-tree paths from
 * the columns j0 to the root, their 64-column block steps, their panel entries m w -- the
 * part of the factor a sweep reads and writes once).  Explicit zeros of Wx count as
 * pattern entries; an empty column is a no-op; k == 0 or n == 0: SC_OK, nothing touched.
 * SC_ERR_ARG, the entry point's name and the reason in sc_last_error: a null handle or
 * array with k > 0, k < 0, a sign other than +1 / -1, a row out of range or twice in a
 * column, an inadmissible column (the message names the column of W and the row).
 * The sweep works on the finished panels, whichever kernels produced them, in chunks of
 * 16 columns of W (a last partial chunk is padded with zero columns), each one pass over
 * the touched supernodes in ascending order: per 64-column block one workgroup rotates
 * the block's rows of W into L11 (Givens rotations for an update, hyperbolic ones for a
 * downdate) and leaves the accumulated transform T, then the front rows below take
 * [L21 W2] T as an fp64 MFMA product.  No atomics, fixed order: bitwise repeatable, and
 * one call with k columns equals the calls with its 16-column chunks in order.
 * The call is synchronous on the handle's stream.  SC_ERR_STATE before a factorization; a
 * failed factorization returns its status > 0 and computes nothing; multi-rank and
 * emulated handles: SC_ERR_NOTIMPL with a message.  Afterwards solves, operators,
 * sc_logdet, sc_selinv and the exports describe A + sign W W^T (the stored block inverses
 * and the Z panel are recomputed at their next use); a later sc_factor starts from the
 * values it is given, the update is forgotten.  A downdate that leaves the matrix not
 * positive definite returns the failing column + 1 (> 0, in the order of P A P^T, as
 * sc_numeric_status counts; the smallest recorded before the sweep stopped) with L partly
 * modified; that value is the handle's status until the next sc_factor.
 * Device memory, counted in sc_numeric_memory info[0], allocated at the first call and
 * kept: the n x 16 workspace (128 n bytes), the 80 x 80 transform, the staging of one
 * chunk (16 times the longest column of L, 16 bytes per entry), besides the solves' plan
 * when no solve has run yet.  A later call allocates nothing.
 * Measured on one MI355X, 128^3 Laplacian in ND order, next to 493 ms for sc_factor on the
 * same handle: one unit vector at a random grid point 83 ms (16 supernodes, 599 block
 * steps, 10.5 GB read and written: 126 GB/s), 16 of them 340 ms (180 supernodes, 2444 block
 * steps, 32.3 GB: 95 GB/s), 16 unit vectors in the root separator 39 ms (257 block steps).
 * The sweep is bound by the one-workgroup block kernel and its launches (about 140 us per
 * block step), not by HBM; it beats the factorization 1.45 to 12.5 times in these cases, and a
 * W whose columns start in many more supernodes than these 180 is a refactorization's job. */
int64_t sc_updown_check(const sc_symbolic* sym, int32_t k, const int64_t* Wp, const int32_t* Wi,
                        int32_t* first_col, int64_t* path);
int64_t sc_updown_host(sc_numeric* num, int32_t sign, int32_t k, const int64_t* Wp, const int32_t* Wi,
                       const double* Wx);

/* Schur complement of a chosen index set on the GPU (MUMPS, PARDISO and cuDSS users know it
 * as the Schur-complement feature): the caller names ns variables S, the interior I (every
 * other index) is eliminated, and the dense interface problem comes back:
 *     S_c = A_SS - A_SI inv(A_II) A_IS,
 * for substructuring, coupling a sparse block to a dense one, or marginalising a precision
 * matrix onto a few nodes.  sc_analyze_schur is sc_analyze with S ordered last: the interior
 * first, ordered by opt->ordering applied to the induced graph A_II (natural: ascending
 * index), then schur_idx in the GIVEN order, perm[n - ns + q] = schur_idx[q]
 * (sc_symbolic_perm; always a permutation in effect).  Then P A P^T = L L^T with
 *     L = [ L_II 0 ; L_SI L_SS ]   and   S_c = L_SS L_SS^T,
 *     g = b_S - A_SI inv(A_II) b_I = L_SS y_S  with  y = L^-1 P b           (condense),
 *     x_I  from  L^T (P x) = [ y_I ; L_SS^T x_S ]  for any x_S               (expand),
 * so that x = A^-1 b when x_S = S_c^-1 g.  The factorization, its schedule and every other
 * entry point (solves, operators, sc_logdet, sc_selinv, sc_updown_host, the exports) work on
 * such a handle unchanged: to them it is one more permutation.  schur_idx: ns distinct rows
 * of A; SC_ERR_ARG with a message naming the entry for a value out of range or given twice,
 * for ns < 0, ns > n, or a null list with ns > 0.  ns == 0 is sc_analyze; ns == n is legal
 * (S_c = A in the order of the list).  sc_symbolic_schur returns ns (0 for a plain handle)
 * and, when schur_idx is not NULL, the list.
 * Numbering: D = L_SS and S_c are ns x ns, column-major (ldd, lds >= ns), row and column q
 * standing for schur_idx[q]; G and XS are ns x nrhs in the same order; B and X are n x nrhs
 * in A's own order, as in sc_solve_*_multi.  D is lower triangular with an exactly zero
 * upper triangle and equals the trailing block of sc_export_L bit for bit; S_c is written
 * to both triangles from one computed value, exactly symmetric.  Entries outside the ns x ns
 * window (the padding of a larger leading dimension) are never written.
 * sc_schur_expand_*_multi returns in the rows of X at schur_idx the caller's XS bit for bit.
 * X may be B when ldx == ldb; argument rules of sc_apply_device_multi plus ldg, ldxs >= ns;
 * nrhs == 0: SC_OK.  Calls are synchronous on the handle's stream.
 * Status rules of sc_selinv: SC_ERR_STATE before a factorization; a failed factorization
 * returns its status > 0 and writes nothing; multi-rank and emulated handles SC_ERR_NOTIMPL
 * with a message; SC_ERR_ARG for a null handle or output or a leading dimension below ns.
 * On a handle without a Schur set (ns == 0) the factor, matrix and condense calls return
 * SC_OK and touch nothing; expand is then the solve.
 * Kernels: a gather copies L_SS out of the finished panels (any path of the factorization
 * leaves them in one layout) into a buffer of the handle, once per generation of the factor
 * -- a new sc_factor or an sc_updown_host makes it stale and the next call gathers again, so
 * no call serves a stale S_c.  S_c = D D^T runs as fp64 MFMA products, one workgroup per
 * 64 x 64 tile of the lower triangle with K only up to the tile's last column (ns^3 / 3
 * flops), what lies above the diagonal of D never used.  The partial solves are the panel
 * family's P, L^-1, L^-T and P^T in panels of 16 columns with a dense triangular product by
 * D in between.  No atomics, fixed order: every result is bitwise repeatable across calls
 * and handles, and a column of G or X does not depend on the columns it travels with.
 * Device memory, counted in sc_numeric_memory info[0], allocated at first use and kept:
 * D (8 ns^2 bytes), 12 bytes per Schur index, the solves' plan and 4 n bytes of postorder
 * when no solve or operator has run yet; the partial solves add one n x 16 panel (128 n
 * bytes) and the panel solves' buffers.  A later call allocates nothing.  The _host forms
 * stage their arrays in device memory for the length of the call (sc_schur_matrix_host:
 * 8 ns^2 bytes; the partial solves: their B and G / XS), not counted in info[0]. */
int64_t sc_analyze_schur(int64_t n, const int64_t* Ap, const int32_t* Ai, const sc_options* opt, int32_t ns,
                         const int32_t* schur_idx, sc_symbolic** out);
int64_t sc_symbolic_schur(const sc_symbolic* sym, int32_t* schur_idx);
int64_t sc_schur_factor_device(sc_numeric* num, double* d_D, int64_t ldd);
int64_t sc_schur_factor_host(sc_numeric* num, double* D, int64_t ldd);
int64_t sc_schur_matrix_device(sc_numeric* num, double* d_S, int64_t lds);
int64_t sc_schur_matrix_host(sc_numeric* num, double* S, int64_t lds);
int64_t sc_schur_condense_device_multi(sc_numeric* num, int32_t nrhs, const double* d_B, int64_t ldb, double* d_G,
                                       int64_t ldg);
int64_t sc_schur_condense_host_multi(sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb, double* G,
                                     int64_t ldg);
int64_t sc_schur_expand_device_multi(sc_numeric* num, int32_t nrhs, const double* d_B, int64_t ldb,
                                     const double* d_XS, int64_t ldxs, double* d_X, int64_t ldx);
int64_t sc_schur_expand_host_multi(sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb, const double* XS,
                                   int64_t ldxs, double* X, int64_t ldx);

/* Products with A, residuals with backward errors, and iterative refinement on the GPU (what
 * CHOLMOD, MUMPS, PARDISO and cuDSS users know as refinement steps and LAPACK's as xPORFS /
 * xPOSVXX): how good a solution is, and a better one.
 *   sc_spmv_*_multi          Y = A X
 *   sc_residual_*_multi      R = B - A X with, per column, the normwise backward error
 *                            berr_norm = |r|_inf / (|A|_inf |x|_inf + |b|_inf) and the componentwise
 *                            one (Oettli-Prager) berr_comp = max_i |r_i| / (|b| + |A| |x|)_i, where
 *                            0 / 0 counts as 0 and nonzero / 0 as +inf; both are host arrays of
 *                            nrhs entries in the _device form too, and either may be NULL
 *   sc_solve_refine_*_multi  X = A^-1 B by the panel solve and refinement steps
 * A is the matrix the analysis saw: entries with row > column ignored, of duplicates of one
 * (row, column) the last one, mirrored to the full symmetric matrix (sc_spmv_structure returns
 * it by rows: rp[n + 1], ascending columns ci, and sp, the index of each value in the value
 * array; two-phase like sc_triplet_to_csc: with ci == NULL it returns the entry count and
 * fills rp if given; host only).  Numbering: every array is n x nrhs column-major in A's own
 * order, whatever the ordering or the Schur set of the handle; leading dimensions >= n.
 * Values: Ax (host forms) / d_Ax (device forms) has the length and order of Ai, exactly what
 * sc_factor / sc_factor_device take, and is read where it lies.  NULL stands for the copy
 * sc_factor made and is legal only when the handle's last factorization was an sc_factor
 * (after sc_factor_device the library holds only a pointer of the caller's that it must not
 * trust): SC_ERR_ARG with a message otherwise.  The values need not be the factored ones:
 * the factor of A then serves a nearby A' as a preconditioner, each step costs one panel
 * solve and contracts the error by rho(I - inv(A) A').  After sc_updown_host the factor
 * describes A +- W W^T while Ax still describes A: refinement with those values converges to
 * the solution of the Ax system if it converges at all.
 * Residual precision: SC_RESIDUAL_FP64 accumulates b - sum a x with one fma per entry;
 * SC_RESIDUAL_DD as a compensated dot product (Ogita, Rump, Oishi: Dot2), as if in twice the
 * working precision, rounded to fp64 once -- which is what lets a refinement step return the
 * correctly rounded solution of an ill-conditioned system.  |b| + |A| |x| is plain fp64.
 * Refinement, per column, with d_k the k-th increment, |d_0| := |x_0|_inf, u = 2^-53:
 *   x_0 = sc_solve_*_multi's result bit for bit (max_iter = 0 returns exactly that);
 *   repeat: r = b - A x; d = solve(r);
 *     DIVERGED   |d_k| >= |d_k-1| (or not a number): d_k is NOT applied, the column stops
 *     otherwise x += d_k, iters += 1, and with the new x
 *     CONVERGED  |d_k| <= u |x|; in FP64 mode also when berr_comp <= 2 u (xPORFS's rule)
 *     STALLED    |d_k| > rho_max |d_k-1|
 *     MAXITER    iters == max_iter
 *   Before the first step a column whose residual is exactly zero (and in FP64 mode one
 *   with berr_comp <= 2 u) is CONVERGED with iters = 0.
 * A column that has stopped is frozen: later steps of its panel do not change a bit of it,
 * and its result does not depend on the columns it travels with or on its position.
 * sc_refine_info (nrhs entries, host memory, may be NULL) describes the returned X: iters,
 * state, berr_norm, berr_comp (from one more residual pass after the last applied increment)
 * and dx_ratio = |d_last| / |x| with d_last the last increment computed, applied or not.
 * No atomics, fixed order: every result is bitwise repeatable across calls and handles.
 * Status: refinement follows the solves -- SC_ERR_STATE before a factorization; a failed
 * factorization returns its status > 0 and writes nothing; nrhs == 0 or n == 0: SC_OK.  The
 * product and the residual never look at the factor and work, with explicit values, right
 * after sc_numeric_create.  SC_ERR_ARG with the entry point's name in sc_last_error for a
 * null handle or array, a leading dimension below n, nrhs < 0, an options struct of the
 * wrong struct_size, max_iter < 0, rho_max outside (0, 1), an unknown residual mode, and for
 * an output that is an input: refinement needs B after X exists, so in-place calls (X == B)
 * are rejected, as are R == B, R == X and Y == X (partial overlaps are not detected and not
 * allowed).  Multi-rank and emulated handles:
 * SC_ERR_NOTIMPL with a message.  Calls are synchronous on the handle's stream.
 * Device memory, counted in sc_numeric_memory info[0], allocated at the first of these calls
 * and kept until sc_free_numeric (nz = entries of sc_spmv_structure, a task = a row or, of a
 * row longer than 256 entries, one chunk of 256; every term at least one element):
 *   8 (n + 1) + 12 nz            the structure
 *   16 per task, 8 per row longer than 256, 512 per chunk of such a row
 *   640 per 256 tasks and per 16 rows longer than 256 (both rounded up)    norm partials
 *   2 x 128 n                    the transposed X panel and the R / D panel
 *   8960                         norms
 * plus, for refinement, what the first sc_solve_*_multi allocates.  The _host forms stage
 * their arrays (and Ax when given) in device memory for the length of the call. */
enum { SC_RESIDUAL_FP64 = 0, SC_RESIDUAL_DD = 1 };
enum { SC_REFINE_CONVERGED = 0, SC_REFINE_STALLED = 1, SC_REFINE_MAXITER = 2, SC_REFINE_DIVERGED = 3 };
typedef struct sc_refine_options {
    int32_t struct_size; /* sizeof(sc_refine_options), set by sc_default_refine_options */
    int32_t max_iter;    /* increments applied at most (10) */
    int32_t residual;    /* SC_RESIDUAL_DD */
    double rho_max;      /* 0.5, as in xGERFSX */
} sc_refine_options;
typedef struct sc_refine_info {
    int32_t iters, state;
    double berr_norm, berr_comp, dx_ratio;
} sc_refine_info;
void sc_default_refine_options(sc_refine_options* opt);
int64_t sc_spmv_structure(const sc_symbolic* sym, int64_t* rp, int32_t* ci, int64_t* sp);
int64_t sc_spmv_host_multi(sc_numeric* num, int32_t nrhs, const double* Ax, const double* X, int64_t ldx, double* Y,
                           int64_t ldy);
int64_t sc_spmv_device_multi(sc_numeric* num, int32_t nrhs, const double* d_Ax, const double* d_X, int64_t ldx,
                             double* d_Y, int64_t ldy);
int64_t sc_residual_host_multi(sc_numeric* num, int32_t residual, int32_t nrhs, const double* Ax, const double* B,
                               int64_t ldb, const double* X, int64_t ldx, double* R, int64_t ldr, double* berr_norm,
                               double* berr_comp);
int64_t sc_residual_device_multi(sc_numeric* num, int32_t residual, int32_t nrhs, const double* d_Ax,
                                 const double* d_B, int64_t ldb, const double* d_X, int64_t ldx, double* d_R,
                                 int64_t ldr, double* berr_norm, double* berr_comp);
int64_t sc_solve_refine_host_multi(sc_numeric* num, const sc_refine_options* opt, int32_t nrhs, const double* Ax,
                                   const double* B, int64_t ldb, double* X, int64_t ldx, sc_refine_info* info);
int64_t sc_solve_refine_device_multi(sc_numeric* num, const sc_refine_options* opt, int32_t nrhs, const double* d_Ax,
                                     const double* d_B, int64_t ldb, double* d_X, int64_t ldx, sc_refine_info* info);

/* Conjugate gradients on the GPU with the factor as the preconditioner: X = A'^-1 B for the
 * values A' the caller passes, which need not be the factored ones -- a Newton or interior-
 * point step, a time step with drifted coefficients, Q(theta) under an optimiser, a
 * modification sc_updown_host rejects.  Where sc_solve_refine_*_multi contracts the error by
 * rho(I - inv(A) A') per step and cannot work once an eigenvalue of inv(A) A' reaches 2, CG
 * needs A' symmetric positive definite and nothing else: k eigenvalues of inv(A) A' away from
 * 1 cost k + 1 steps in exact arithmetic (A' = 3 A: one step), the rest sqrt(cond(inv(A) A'))
 * per digit.  Arrays, numbering, leading dimensions and the values Ax / d_Ax (NULL: the copy
 * sc_factor made) follow the rules of the refinement entry points above.
 * Per column, with M the factor's solve (sc_solve_*_multi) and 2-norms:
 *   x_0 = M b, sc_solve_*_multi's result bit for bit (use_x0 = 0), or X as the caller left it
 *         (use_x0 = 1: a warm start; the host form then reads X);
 *   r = b - A' x_0 (one fma per entry, as SC_RESIDUAL_FP64);
 *   CONVERGED with iters = 0 when |r| <= tol |b| (an all-zero b: x = 0, CONVERGED);
 *   MAXITER   with iters = 0 when max_iter = 0;
 *   z = M r; rho = r.z; p = z;
 *   repeat: q = A' p; pq = p.q;
 *     BREAKDOWN  pq <= 0 or not finite: x stays at the last iterate
 *     alpha = rho / pq; x += alpha p; r -= alpha q; iters += 1;
 *     CONVERGED  |r| <= tol |b|
 *     MAXITER    iters == max_iter
 *     z = M r; rho' = r.z;
 *     BREAKDOWN  rho' <= 0 or not finite (the same test guards the first rho)
 *     p = z + (rho' / rho) p.
 * BREAKDOWN is how values that are not positive definite show: p.A'p <= 0 for some direction
 * (A' = -A breaks down at once with x = x_0).  An indefinite A' may also run to MAXITER; it is
 * never reported CONVERGED unless the residual it returns is that small.  tol = 0 is legal and
 * runs to max_iter or breakdown.  With the factored values and the default tol the first
 * test holds and the call returns the panel solve bit for bit with iters = 0.
 * Every sum is an fma chain in an order fixed by n alone, alpha, beta and the decisions are
 * taken on the host per column, and a column that has stopped is not written again: a
 * column's result does not depend on the columns it travels with or on its position, and is
 * bitwise repeatable across calls and handles.  No atomics.
 * sc_pcg_info (nrhs entries, host memory, may be NULL) describes the returned X: iters, state,
 * relres = |r| / |b| of the recurrence's r (0 / 0 = 0), and from one more residual pass over
 * the returned X relres_true = |b - A' x| / |b| and the two backward errors of
 * sc_residual_*_multi (SC_RESIDUAL_FP64).
 * Status: as sc_solve_refine_*_multi -- SC_ERR_STATE before a factorization; a failed
 * factorization returns its status > 0 and writes nothing; nrhs == 0 or n == 0: SC_OK; multi-
 * rank and emulated handles SC_ERR_NOTIMPL with a message.  SC_ERR_ARG with the entry point's
 * name in sc_last_error for a null handle or array, a leading dimension below n, nrhs < 0, an
 * options struct of the wrong struct_size, max_iter < 0, tol outside [0, 1), use_x0 other than
 * 0 or 1, and X == B.  Calls are synchronous on the handle's stream.
 * Device memory, counted in sc_numeric_memory info[0], allocated at the first call and kept
 * until sc_free_numeric, besides what the refinement section lists (allocated by whichever
 * call comes first) and what the first sc_solve_*_multi allocates:
 *   3 x 128 n                    the z, p and q panels (n at least 1)
 *   256 per 1024 rows (rounded up, at least one)    partial sums
 *   512                          the sums of a step */
enum { SC_PCG_CONVERGED = 0, SC_PCG_MAXITER = 1, SC_PCG_BREAKDOWN = 2 };
typedef struct sc_pcg_options {
    int32_t struct_size; /* sizeof(sc_pcg_options), set by sc_default_pcg_options */
    int32_t max_iter;    /* steps at most (100) */
    int32_t use_x0;      /* 0: start from the panel solve; 1: from X as passed */
    double tol;          /* 1e-10; stop at |r|_2 <= tol |b|_2 */
} sc_pcg_options;
typedef struct sc_pcg_info {
    int32_t iters, state;
    double relres, relres_true, berr_norm, berr_comp;
} sc_pcg_info;
void sc_default_pcg_options(sc_pcg_options* opt);
int64_t sc_solve_pcg_host_multi(sc_numeric* num, const sc_pcg_options* opt, int32_t nrhs, const double* Ax,
                                const double* B, int64_t ldb, double* X, int64_t ldx, sc_pcg_info* info);
int64_t sc_solve_pcg_device_multi(sc_numeric* num, const sc_pcg_options* opt, int32_t nrhs, const double* d_Ax,
                                  const double* d_B, int64_t ldb, double* d_X, int64_t ldx, sc_pcg_info* info);

/* The eigenpairs of the factored matrix nearest zero, by block shift-invert Lanczos on the GPU:
 * vibration and buckling modes with the stiffness factor, the Fiedler vector of a graph
 * Laplacian, the slow modes of a precision matrix, lambda_min for cond_2 or the largest safe
 * downdate.  The handle holds the factor of F = A - sigma I (the caller factored those values;
 * sigma only shifts what is reported).  The call returns the nev eigenvalues of F nearest zero
 * plus sigma -- the smallest of A when sigma = 0 -- ascending in lambda (host, nev doubles),
 * and their eigenvectors as the columns of X (n x nev, leading dimension ldx >= n, A's own
 * numbering, each of unit 2-norm).  Ax / d_Ax: the factored values, under the rules of the
 * refinement entry points (NULL: the copy sc_factor made, legal only after sc_factor); they are
 * used for the reported residuals alone, resid_i = |F x_i - x_i / theta_i|_2, so values other
 * than the factored ones show there and not silently.
 * The algorithm, with b = min(16, n) the block width (columns >= b of a panel do not exist for
 * the kernels), u = 2^-53, and all panels n x b:
 *   start block: use_x0 = 0: entry (i, c) = 2 v - 1 with v = (splitmix64(seed + (16 i + c + 1)
 *     g) >> 11) 2^-53, g = 0x9E3779B97F4A7C15, z -> splitmix64(z): z = (z ^ z >> 30)
 *     0xBF58476D1CE4E5B9; z = (z ^ z >> 27) 0x94D049BB133111EB; z ^ z >> 31 (64-bit wrapping): it
 *     depends on seed, i and c alone.  use_x0 = 1: the first b columns of X0 (ldx0 >= n).
 *   orth(W), twice: scale every column by 1 / sqrt of its Gram diagonal (0 for a zero column);
 *     G = W^T W (Gram kernel); G = R^T R by Cholesky on the host (16 x 16), a column whose pivot
 *     is <= 2 (n + 16) u or not finite is dropped (left out of R, its column of inv(R) zero: it
 *     becomes a zero column of W); W <- W inv(R) (block-update kernel, in place).
 *   V_0 = orth(start).  Step j = 0, 1, ..:
 *     1. W = inv(F) V_j (sc_solve_device_multi's panel solve)
 *     2. twice: H_i = V_i^T W for all i <= j (one Gram launch), W -= sum_i V_i H_i (one block-
 *        update launch); the H of the two passes add up
 *     3. column block j of T = that H, row block j its transpose, the diagonal block (H_j + H_j^T)
 *        / 2: T is m x m, m = b (j + 1), symmetric, on the host
 *     4. G = W^T W of the projected W
 *     5. T = S diag(theta) S^T on the host (Householder tridiagonalisation, implicit QL); the
 *        wanted pairs are the nev largest theta (fewer while m < nev: not converged)
 *     6. est_i = sqrt(s_i^T G s_i), s_i the last b entries of S's column: the residual of
 *        (theta_i, V s_i) for inv(F), needing no factor of G
 *     stop when   est_i <= tol theta_i for every wanted pair,
 *       or        j + 1 == max_blocks,
 *       or        the space cannot grow: m + b > n, or W is rank-deficient -- a diagonal entry of
 *                 G not positive, or a pivot <= 2 (n + 16) u in the Cholesky of G scaled to a unit
 *                 diagonal (indistinguishable from the rounding of the Gram entries, gamma_n, and
 *                 of the elimination, gamma_17);
 *     else V_{j+1} = orth(W).
 *   At the stop: X = sum_i V_i S_i over the wanted columns (one block-update launch per 16
 *   pairs), lambda_i = sigma + 1 / theta_i, resid from one product with F and one sum pass.
 * sc_eigs_info (nev entries, host, may be NULL), per pair: blocks = j + 1; est; resid; state
 *   SC_EIGS_CONVERGED  est_i <= tol theta_i at the stop
 *   SC_EIGS_MAXBLOCKS  not converged, and the block cap was reached
 *   SC_EIGS_EXHAUSTED  not converged, and the space could not grow.
 * With |x| = 1: resid = |F r| / theta <= |F| est / theta <= tol |F| for a converged pair (r =
 * inv(F) x - theta x, |r| = est), and |lambda_i - an eigenvalue of A| <= resid_i.  A space that
 * stops below nev columns (m + b > n with n no multiple of 16) has no Ritz pair for the last
 * nev - m: they come back as lambda = +inf, x = 0, est = resid = +inf, not converged.
 * Every sum has an order fixed by n and the block count alone and there are no atomics: results
 * repeat bit for bit across calls and handles.  The basis is kept whole (no restarts), so
 * max_blocks bounds the memory as well as the work; the host eigensolver costs O(m^3) per step.
 * Status: as sc_solve_pcg_*_multi -- SC_ERR_STATE before a factorization; a failed
 * factorization returns its status > 0 and writes nothing; multi-rank and emulated handles
 * SC_ERR_NOTIMPL with a message; nev == 0 or n == 0: SC_OK, nothing touched.  SC_ERR_ARG with the
 * entry point's name in sc_last_error for a null handle, a null lambda or X (or X0 with use_x0),
 * nev < 0, nev > min(n, 16 max_blocks), ldx < n, ldx0 < n with use_x0, an options struct of the
 * wrong struct_size, max_blocks outside 1..32, tol outside [0, 1), use_x0 other than 0 or 1,
 * and a sigma that is not finite; also, with a message, when the QL iteration on T does not
 * converge in 60 sweeps (a start block or a factor that is not finite).  NULL options: the
 * defaults.  Calls are synchronous.
 * Device memory, counted in sc_numeric_memory info[0], allocated at the first call and kept
 * until sc_free_numeric, besides what the refinement section lists (n at least 1 below):
 *   (max_blocks + 1) x 128 n      the basis; replaced by a larger one, with the next two, when
 *                                 a later call asks for more blocks
 *   2048 max_blocks per 1024 rows (rounded up, at least one)    Gram partials
 *   4096 max_blocks               Gram results and update coefficients
 *   128 n                         the residual panel */
enum { SC_EIGS_CONVERGED = 0, SC_EIGS_MAXBLOCKS = 1, SC_EIGS_EXHAUSTED = 2 };
typedef struct sc_eigs_options {
    int32_t struct_size; /* sizeof(sc_eigs_options), set by sc_default_eigs_options */
    int32_t max_blocks;  /* 32; basis blocks of 16 columns at most, 1..32 */
    int32_t use_x0;      /* 0: the library's start block; 1: the first min(16, n) columns of X0 */
    uint64_t seed;       /* 1; the start block when use_x0 = 0 */
    double tol;          /* 1e-10, in [0, 1) */
    double sigma;        /* 0; the handle holds the factor of A - sigma I; lambda = sigma + 1 / theta */
} sc_eigs_options;
typedef struct sc_eigs_info {
    int32_t state, blocks;
    double est, resid;
} sc_eigs_info;
void sc_default_eigs_options(sc_eigs_options* opt);
int64_t sc_eigs_host(sc_numeric* num, const sc_eigs_options* opt, int32_t nev, const double* Ax, const double* X0,
                     int64_t ldx0, double* lambda, double* X, int64_t ldx, sc_eigs_info* info);
int64_t sc_eigs_device(sc_numeric* num, const sc_eigs_options* opt, int32_t nev, const double* d_Ax,
                       const double* d_X0, int64_t ldx0, double* lambda, double* d_X, int64_t ldx, sc_eigs_info* info);

/* ---------------- gradients on A's pattern (single device) ----------------
 * The derivatives of log det A and of X = inv(A) B with respect to the stored values of A, as
 * sparse arrays of the length and order of the value array sc_factor takes.  Definitions, which
 * every entry point below follows:
 *   - An effective entry is a value slot k that the analysis uses: its row i_k is <= its column
 *     j_k, and of several duplicates of one (row, column) it is the last.  These are exactly the
 *     slots sc_spmv_structure's sp names.
 *   - Every other slot is ignored; its derivative is zero.
 *   - Every gradient array G has the length and order of Ai.
 *   - Ignored slots of an output are written +0.0.
 *   - Numbering is A's own, whatever the ordering or the Schur set of the handle.
 * A stored entry stands for both mirrored positions, so with c_k = 1 on the diagonal and 2 off it
 *     d logdet A / d a_k = c_k inv(A)[i_k, j_k],
 * and for X = inv(A) B with an upstream Xbar: Bbar = inv(A) Xbar and
 *     Abar_k = -sum_c (Bbar[i,c] X[j,c] + [i != j] Bbar[j,c] X[i,c]).
 *   sc_value_entries       host only, no device: per value slot its row, its column and 0 / 1
 *                          (effective); any array may be NULL; returns the slot count
 *   sc_pattern_outer_*     per effective entry G_k = beta G_k + alpha sum_c (U[i,c] V[j,c] +
 *                          [i != j] U[j,c] V[i,c]); beta == 0 does not read G.  U, V: n x nrhs
 *                          column-major, any nrhs >= 0, taken in panels of 16: within a panel the
 *                          16 columns are added by halving (absent columns count as zero), the
 *                          first panel applies beta, later panels add in order.  Needs no
 *                          factorization: works right after sc_numeric_create, like sc_spmv_*_multi
 *   sc_pattern_dot_*       *out (host) = sum over the effective entries of G_k H_k, in a fixed
 *                          tree; with H = dA this is the directional derivative tr(inv(A) dA)
 *   sc_logdet_grad_*       G_k = c_k inv(A)[i_k, j_k], gathered from the Z panel of the selected
 *                          inversion, which is computed first when it does not belong to the
 *                          current factorization (the rules of sc_selinv_diag_*); after
 *                          sc_updown_host it belongs to the updated matrix
 *   sc_solve_grad_*        Bbar = the panel solve of Xbar, bit for bit what sc_solve_*_multi
 *                          returns (Bbar may be Xbar when ldbb == ldxb), then G = the outer product
 *                          with alpha = -1, beta = 0, U = Bbar, V = X
 * No kernel uses atomics and every sum has an order fixed by n, the entry count and nrhs: results
 * repeat bit for bit across calls and handles.
 * Status: sc_logdet_grad_* and sc_solve_grad_* return SC_ERR_STATE before a factorization, and a
 * failed factorization's status > 0, writing nothing; nrhs == 0 and n == 0 are legal; multi-rank
 * and emulated handles SC_ERR_NOTIMPL with a message.  SC_ERR_ARG with the entry point's name in
 * sc_last_error for a null handle, a null array (U, V, Xbar, X, Bbar with nrhs > 0 and n > 0; G,
 * H with a non-empty value array; out), nrhs < 0, a leading dimension below n, G equal to U or V
 * (sc_solve_grad_*: to Xbar, X or Bbar, or Bbar equal to X).  Calls are synchronous on the
 * handle's stream.
 * Device memory, counted in sc_numeric_memory info[0], allocated at the first of these calls and
 * kept until sc_free_numeric, in bytes (ne = effective entries, ni = ignored slots, each list at
 * least one element; n at least 1; nothing when n == 0 or the value array is empty):
 *   16 ne                         the entry list (row, column, slot), in slot order
 *   8 ni                          the ignored slots
 *   2 x 128 n                     the 16-wide row-major copies of the U and the V panel
 *   8 (ceil(ne / 1024) + 1)       the dot's partials and its result
 * sc_logdet_grad_* also brings what sc_selinv lists, sc_solve_grad_* what the panel solve does;
 * the host forms stage their arrays on the device for the length of the call. */
int64_t sc_value_entries(const sc_symbolic* sym, int32_t* row, int32_t* col, int32_t* effective);
int64_t sc_pattern_outer_host(sc_numeric* num, double alpha, int32_t nrhs, const double* U, int64_t ldu,
                              const double* V, int64_t ldv, double beta, double* G);
int64_t sc_pattern_outer_device(sc_numeric* num, double alpha, int32_t nrhs, const double* d_U, int64_t ldu,
                                const double* d_V, int64_t ldv, double beta, double* d_G);
int64_t sc_pattern_dot_host(sc_numeric* num, const double* G, const double* H, double* out);
int64_t sc_pattern_dot_device(sc_numeric* num, const double* d_G, const double* d_H, double* out);
int64_t sc_logdet_grad_host(sc_numeric* num, double* G);
int64_t sc_logdet_grad_device(sc_numeric* num, double* d_G);
int64_t sc_solve_grad_host(sc_numeric* num, int32_t nrhs, const double* Xbar, int64_t ldxb, const double* X,
                           int64_t ldx, double* Bbar, int64_t ldbb, double* G);
int64_t sc_solve_grad_device(sc_numeric* num, int32_t nrhs, const double* d_Xbar, int64_t ldxb, const double* d_X,
                             int64_t ldx, double* d_Bbar, int64_t ldbb, double* d_G);

/* Weighted normal equations, formed and factored on the GPU.  For a
 * rectangular sparse J (m x n, CSC), row weights w (m), an optional symmetric base matrix C
 * (n x n, its upper triangle in CSC), an optional diagonal d (n) and a damping lambda,
 *     S = C + J^T diag(w) J + diag(d) + lambda I:
 * the normal equations of Newton and interior-point steps, Gauss-Newton and Levenberg-Marquardt,
 * reweighted least squares, the posterior precision Q + A^T W A.  An sc_normal handle holds the
 * structure only (it is independent of sc_symbolic and sc_numeric); the values J, w, C, d come
 * with every call, so a new w or lambda per step costs one pass over the term lists.
 *   sc_normal_create    validates and builds.  SC_ERR_ARG with a message in sc_last_error when
 *                       J's row indices do not ascend strictly within a column or leave [0, m),
 *                       J has more than 2^31 - 1 entries (a term holds 32-bit positions) or more
 *                       than 2^40 terms, S would have more than 2^31 - 1 entries, or a base entry
 *                       has row > column.  Cp == NULL: no base.
 *                       No HIP call: the device side is built at the first call that needs it
 *                       (device < 0: the device of the sc_numeric of the first factor call, else
 *                       the current one).
 *   sc_normal_pattern   the pattern of S -- upper triangle, CSC, rows ascending: every diagonal
 *                       entry, every (i, j), i < j, whose J columns share a row, every entry of
 *                       C -- in the form sc_analyze / sc_analyze_schur take.  Two-phase: returns
 *                       the entry count; Sp (n + 1) and Si are filled when not NULL.
 *   sc_normal_terms     T = sum over J's rows of nnz_r (nnz_r + 1) / 2, the terms of all entries.
 *   sc_normal_term_lists  host copies for tests, two-phase (returns T): tp (entries + 1), per
 *                       term the positions pa, pb of J[r, i] and J[r, j] in J's value array and
 *                       the row r (rows ascend within an entry's list), per entry cpos, the
 *                       position of its value in C's array or -1.
 *   sc_normal_rows      J by rows, as sc_spmv_structure gives A: rp (m + 1), columns ci ascending,
 *                       sp the position in J's value array.  Two-phase, returns nnz(J).
 *   sc_normal_memory    out[0 .. 4): host bytes of the structure, device bytes held, T, entries
 *                       of S; returns 4.
 *   sc_normal_constants out[0 .. 4): the boundaries between the form kernel's mappings (lists of
 *                       at most out[0] terms: one lane per entry; up to out[2]: out[1] lanes per
 *                       entry; above: chunks of out[2] terms) and out[3], the entries per chunk of
 *                       a long column or row of the products; returns 4.
 * Values.  S_e = (c_e + [i = j] (d_i + lambda)) + sum_t (J[pa_t] w[r_t]) J[pb_t], every product
 * rounded twice (J w, then the fma with the other J), in this order: a list of at most 8 terms
 * is added to the base term by term in list order; a longer one is summed by 16 lanes -- lane l
 * takes the terms l, l + 16, .. in order, starting from zero, and the 16 lane sums are added by
 * halving (8, 4, 2, 1) -- and the base is added last; a list above 256 terms runs in chunks of
 * 256, each summed as such a list, the partials added in chunk order, then the base.  No
 * atomics: the values are bitwise repeatable across calls and handles.  Any order satisfies
 *     |S_e - exact| <= gamma_(t + 3) (|c_e| + |d_i + lambda| + sum |J w J|),  t the list length.
 *   sc_normal_values_*  the values into the caller's array (entries of S doubles, the order of
 *                       Si: what sc_factor_device reads).  w (ones), Cx (zeros) and d (zeros) may
 *                       be NULL.
 *   sc_normal_factor_*  forms into a buffer the handle owns and calls sc_factor_device(num,
 *                       buffer, 1); returns the factorization's status (> 0: the failing column
 *                       + 1 in the factored order, as for any matrix that is not positive
 *                       definite -- a rank-deficient J without damping ends there).  SC_ERR_ARG
 *                       when num's analysis has another n or value count or lives on another
 *                       device; multi-rank and emulated handles SC_ERR_NOTIMPL with a message.
 *   sc_normal_values_ptr  that device buffer (NULL until an sc_normal_factor_* has filled it),
 *                       valid until sc_normal_free, its contents until the next
 *                       sc_normal_factor_* on the handle: pass it as
 *                       d_Ax to sc_residual_*, sc_solve_refine_*, sc_solve_pcg_*, sc_solve_grad_*.
 * Products, in panels of 16 columns, column-major with leading dimensions (checked against the
 * row counts as in sc_spmv_*_multi; an output that is the input: SC_ERR_ARG):
 *   sc_normal_mul_*_multi   Y (m x nrhs) = J X, one fma per entry along a row, columns ascending
 *   sc_normal_mult_*_multi  G (n x nrhs) = J^T diag(w) Y, down J's columns: (J w) rounded, then
 *                           one fma per entry; w may be NULL (ones)
 * A row or column above 256 entries is summed in chunks of 256 whose partials are added in chunk
 * order.  A column's bits do not depend on the columns it travels with.
 * Device memory per handle, allocated at the first device call and kept until sc_normal_free:
 *   12 T                       the term lists (three int32 per term)
 *   20 ne + 24 tasks           per entry of S: list start, base position, diagonal column; a
 *                              task = a list above 8 terms or one chunk of it
 *   12 nnz(J) + 8 (n + 1)      J by columns;  20 nnz(J) + 8 (m + 1)  J by rows;  16 per task
 *   8 ne                       the value buffer;  128 max(m, n)  the 16-wide right-hand panel
 * plus the partial slots of chunked lists, rows and columns.  The _host forms stage their arrays
 * for the length of the call.  All calls are synchronous on the handle's stream.
 * Least squares.  sc_normal_lstsq_*_multi minimises
 *     ||W^1/2 (J x - b)||_2^2 + x^T (C + diag d + lambda I) x
 * per column of B (m x nrhs) with the factor num holds, which must come from sc_normal_factor_*
 * on this handle, and from the last such call (SC_ERR_STATE with a message otherwise: the handle
 * remembers one call's values, C, d and lambda, so a second sc_numeric factored through the
 * same handle retires the first for this entry point).  Jx and w are passed again and should be the factored ones.  The first iterate is
 * the plain normal-equations solve x_0 = inv(S) J^T W b, whose error grows with cond(J)^2; then
 * come corrected semi-normal steps
 *     r = b - J x,   g = J^T W r - (C + diag d + lambda I) x,   x += inv(S) g
 * with r and the base product accumulated as opt->residual says (SC_RESIDUAL_DD: compensated),
 * which bring the error down to what cond(J) allows.  Options, stopping states and rules are
 * those of sc_solve_refine_*_multi (sc_refine_options; per column: CONVERGED when the increment
 * falls below u ||x||_inf or the gradient is exactly zero, STALLED when it contracts by less than
 * rho_max, MAXITER, DIVERGED when it does not contract at all -- that increment is not applied;
 * a stopped column is never touched again).  max_iter = 0 returns x_0.  sc_lstsq_info (nrhs
 * entries, host, may be NULL) describes the returned X: grad_norm = ||g||_inf, resid_norm =
 * ||W^1/2 r||_2 (NaN for negative weights), dx_ratio = the last increment over ||x||_inf.
 * Status: SC_ERR_STATE before a factorization; a failed factorization returns its status > 0
 * and writes nothing; X == B and the argument errors of sc_solve_refine_*_multi: SC_ERR_ARG
 * with a message; multi-rank and emulated handles SC_ERR_NOTIMPL.  In the compensated mode the
 * residual and the gradient are kept as unevaluated pairs of doubles (as if in twice the working
 * precision) until the base product is off the gradient, which is then rounded once: with a
 * gradient in plain fp64 the increments of a problem with a large residual stop contracting at
 * cond(J)^2 u ||r|| and never reach u ||x||.  Allocated at the first call and kept: 384 (n + m)
 * bytes of panels (gradient, residual and their 16-wide row-major forms, each as a pair), the
 * base by rows (20 bytes per mirrored entry of C and per row) and what the first
 * sc_solve_*_multi allocates. */
typedef struct sc_normal sc_normal;
typedef struct sc_lstsq_info {
    int32_t iters, state;      /* increments applied; SC_REFINE_* */
    double grad_norm, resid_norm, dx_ratio;
} sc_lstsq_info;
int64_t sc_normal_create(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const int64_t* Cp,
                         const int32_t* Ci, int32_t device, sc_normal** out);
void sc_normal_free(sc_normal* normal);
int64_t sc_normal_pattern(const sc_normal* normal, int64_t* Sp, int32_t* Si);
int64_t sc_normal_terms(const sc_normal* normal);
int64_t sc_normal_term_lists(const sc_normal* normal, int64_t* tp, int32_t* pa, int32_t* pb, int32_t* r,
                             int64_t* cpos);
int64_t sc_normal_rows(const sc_normal* normal, int64_t* rp, int32_t* ci, int64_t* sp);
int64_t sc_normal_memory(const sc_normal* normal, int64_t* out, int32_t cap);
int64_t sc_normal_constants(int32_t* out, int32_t cap);
int64_t sc_normal_values_host(sc_normal* normal, const double* Jx, const double* w, const double* Cx,
                              const double* d, double lambda, double* Sx);
int64_t sc_normal_values_device(sc_normal* normal, const double* d_Jx, const double* d_w, const double* d_Cx,
                                const double* d_d, double lambda, double* d_Sx);
int64_t sc_normal_factor_host(sc_normal* normal, sc_numeric* num, const double* Jx, const double* w,
                              const double* Cx, const double* d, double lambda);
int64_t sc_normal_factor_device(sc_normal* normal, sc_numeric* num, const double* d_Jx, const double* d_w,
                                const double* d_Cx, const double* d_d, double lambda);
const double* sc_normal_values_ptr(const sc_normal* normal);
int64_t sc_normal_mul_host_multi(sc_normal* normal, int32_t nrhs, const double* Jx, const double* X, int64_t ldx,
                                 double* Y, int64_t ldy);
int64_t sc_normal_mul_device_multi(sc_normal* normal, int32_t nrhs, const double* d_Jx, const double* d_X,
                                   int64_t ldx, double* d_Y, int64_t ldy);
int64_t sc_normal_mult_host_multi(sc_normal* normal, int32_t nrhs, const double* Jx, const double* w,
                                  const double* Y, int64_t ldy, double* G, int64_t ldg);
int64_t sc_normal_mult_device_multi(sc_normal* normal, int32_t nrhs, const double* d_Jx, const double* d_w,
                                    const double* d_Y, int64_t ldy, double* d_G, int64_t ldg);
int64_t sc_normal_lstsq_host_multi(sc_normal* normal, sc_numeric* num, const sc_refine_options* opt, int32_t nrhs,
                                   const double* Jx, const double* w, const double* B, int64_t ldb, double* X,
                                   int64_t ldx, sc_lstsq_info* info);
int64_t sc_normal_lstsq_device_multi(sc_normal* normal, sc_numeric* num, const sc_refine_options* opt, int32_t nrhs,
                                     const double* d_Jx, const double* d_w, const double* d_B, int64_t ldb,
                                     double* d_X, int64_t ldx, sc_lstsq_info* info);

/* ---------------- reference-API helpers (host) ----------------
 * Each mirrors one reference function, with int64 column pointers. */
/* etree(A)  chol.hpp:377-410 */
int64_t sc_etree(int64_t n, const int64_t* Ap, const int32_t* Ai, int32_t* parent);
/* post_order(parent)  chol.hpp:466-499 */
int64_t sc_post_order(int64_t n, const int32_t* parent, int32_t* post);
/* col_count(A, parent, post)  chol.hpp:567-622 */
int64_t sc_col_count(int64_t n, const int64_t* Ap, const int32_t* Ai, const int32_t* parent,
                     const int32_t* post, int64_t* colcount);
/* ereach(A, k, parent, s, w[, x])  chol.hpp:680-739; returns top. Ax/x may be NULL. */
int64_t sc_ereach(int64_t n, const int64_t* Ap, const int32_t* Ai, const double* Ax, int64_t k,
                  const int32_t* parent, int32_t* s, int32_t* w, double* x);
/* compute_levels(parent)  src/chol.cpp:7-40: level_of[n] (0 = deepest level
 * processed first) ; returns number of levels. */
int64_t sc_compute_levels(int64_t n, const int32_t* parent, int32_t* level_of);
/* compute_supernodes(S, supernodes)  src/chol.cpp:42-100 on the reference
 * pattern (natural order): sn_id[n], supernodes[ns+1]; returns ns. */
int64_t sc_compute_supernodes(int64_t n, const int32_t* parent, const int64_t* Lp,
                              int32_t* sn_id, int64_t* supernodes);
/* atree(S, sn_id, supernodes)  src/chol.cpp:102-136 */
int64_t sc_atree(int64_t n, const int64_t* Lp, const int32_t* Li, const int32_t* sn_id,
                 const int64_t* supernodes, int64_t ns, int32_t* super_parent);
/* triplet_to_csc_matrix(ti, tj, tx, n)  chol.hpp:308-369: swaps to row<=col,
 * sorts by (col,row), sums duplicates.  Two-phase: call with Ap only to size,
 * then with Ai/Ax.  Returns nnz. */
int64_t sc_triplet_to_csc(int64_t n, int64_t nt, const int32_t* ti, const int32_t* tj,
                          const double* tx, int64_t* Ap, int32_t* Ai, double* Ax);
/* load_matrix_market_to_csc(filename)  include/mtx_reader.hpp:16-62, with the
 * banner honoured: coordinate real / integer / pattern (value 1); symmetric,
 * hermitian or no banner as the reference; general must hold a symmetric matrix
 * (both triangles, equal after summing duplicates; else SC_ERR_NOTSYM) and keeps
 * its upper entries; skew-symmetric SC_ERR_NOTSYM; array / complex
 * SC_ERR_NOTIMPL; out-of-range indices SC_ERR_ARG.  Two-phase like above:
 * first call with Ai==NULL returns n in *n and nnz; second fills. */
int64_t sc_read_mtx(const char* path, int64_t* n, int64_t* Ap, int32_t* Ai, double* Ax);
/* Synthetic 3D 7-point Laplacian on a k^3 grid in deterministic geometric
 * nested-dissection order.  n=k^3, nnz=n+3k^2(k-1).
 * Ap[n+1], Ai[nnz], Ax[nnz] (upper CSC); perm (new->old) may be NULL. */
int64_t sc_laplacian3d(int64_t k, int32_t nd_order, int64_t* Ap, int32_t* Ai, double* Ax,
                       int32_t* perm);

/* ---------------- multi-GPU (subtree partition over RCCL) ----------------
 * Proportional subtree-to-GPU mapping of the assembly tree; contribution
 * blocks cross GPUs only at subtree-merge fronts. */
/* RCCL unique id (128 bytes), created on rank 0 and broadcast by the caller. */
int64_t sc_dist_unique_id(void* id128);
int64_t sc_dist_owner_map(const sc_symbolic* sym, int32_t nranks, int32_t* owner_of_supernode,
                          double* work_per_rank);
/* This process is `rank` of `nranks` (one GPU each); it factors only the
 * supernodes it owns and exchanges contribution blocks with ncclSend/ncclRecv
 * after each assembly-tree level.  id128 == NULL: emulate all nranks ranks inside
 * this process on one device (sc_numeric_create_dist_emulated, device copies). */
int64_t sc_numeric_create_dist(const sc_symbolic* sym, int32_t device, int32_t rank,
                               int32_t nranks, const void* id128, sc_numeric** out);
/* Every rank of an nranks-rank plan in this process on one device, each with its
 * own memory plan and arenas; every message of the plan moves between them, as
 * device copies (use_rccl = 0) or as ncclSend / ncclRecv to self inside one
 * ncclGroupStart / ncclGroupEnd per comm step on a 1-rank RCCL communicator
 * (use_rccl = 1).  Validation of the partition and of the message plan. */
int64_t sc_numeric_create_dist_emulated(const sc_symbolic* sym, int32_t device, int32_t nranks, int32_t use_rccl,
                                        sc_numeric** out);
/* Per-rank message schedule for tests: returns number of messages; if the
 * arrays are non-NULL fills (comm step, peer, bytes, is_send) per message, in
 * posting order (comm steps ascending; all ranks follow one global step order). */
int64_t sc_dist_schedule(const sc_symbolic* sym, int32_t nranks, int32_t rank, int32_t* step,
                         int32_t* peer, int64_t* bytes, int32_t* is_send, int64_t cap);
/* The plan's comm steps in their global order: kind (0 INIT: assembled columns to
 * the ranks that factor / update them, 1 SLAB: a final panel slab to its users,
 * 2 DELIVER: contribution blocks to the parent's owner), assembly-tree level, front
 * (-1: a level's collective delivery), k (SLAB: the slab; DELIVER of an early child:
 * its column group) and p (SLAB: the column piece of the slab).  Any array may be
 * NULL.  Returns the step count. */
int64_t sc_dist_steps(const sc_symbolic* sym, int32_t nranks, int32_t* kind, int32_t* level, int32_t* front,
                      int32_t* k, int32_t* p, int64_t cap);
/* Plan summary: per supernode the rank-group size (1 = inside one rank's subtree),
 * for split fronts the number of ranks computing its contribution block (0 = not
 * split), for distributed panels the number of ranks factoring its slabs (0 = the
 * panel on one rank); *n_steps = comm steps.  Returns the total message count. */
int64_t sc_dist_plan_info(const sc_symbolic* sym, int32_t nranks, int32_t* gsize, int32_t* split_cb_ranks,
                          int32_t* slab_ranks, int64_t* n_steps);
/* Host-staged transport (tests / debugging without RCCL: several processes may
 * share one GPU).  The library calls fn(ctx, op, peer, buf, bytes) with op 0 =
 * post a send of host buffer buf, 1 = post a receive into buf, 2 = complete every
 * posted operation (buffers stay valid until then); nonzero return = failure. */
typedef int32_t (*sc_transport_fn)(void* ctx, int32_t op, int32_t peer, void* buf, int64_t bytes);
int64_t sc_numeric_create_dist_host(const sc_symbolic* sym, int32_t device, int32_t rank,
                                    int32_t nranks, sc_transport_fn fn, void* ctx, sc_numeric** out);
/* Timing projection: rank `rank`'s part of an nranks-GPU factorization alone on
 * this device; comm steps pack and unpack but move nothing (received blocks hold
 * stale values, so the numbers are not a factor). */
int64_t sc_numeric_create_dist_dry(const sc_symbolic* sym, int32_t device, int32_t rank, int32_t nranks,
                                   sc_numeric** out);

int64_t sc_device_count(void);
/* Message of the last failing call on this thread: after a call that returned a status < 0 it
 * reads "<entry point>: <reason>", with sc_status_string's text as the reason where the call has
 * none of its own, and never shows an earlier call's message.  Calls that return >= 0 (SC_OK, a
 * count, the not-positive-definite status) leave it as it was.  The pointer is valid until the
 * next library call on this thread. */
const char* sc_last_error(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif

#endif /* SPARSECHOLESKY_H */
