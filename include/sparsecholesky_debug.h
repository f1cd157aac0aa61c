/*
 * sparsecholesky_debug.h -- debug, probe and microbenchmark hooks of the library.
 *
 * Not part of the drop-in boundary (include/sparsecholesky.h): these entry points
 * have no counterpart in the reference.  They exist for the tests (the MFMA SYRK
 * kernel against numpy), for C-level timing of small configurations, and for the
 * measurement scripts under scripts/ (microbenchmarks, placement and contention
 * probes).  Same conventions as sparsecholesky.h.
 */
#ifndef SPARSECHOLESKY_DEBUG_H
#define SPARSECHOLESKY_DEBUG_H

#include "sparsecholesky.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* C[i,j] -= sum_k A[i,k] A[j,k] for i>=j over an M x N trapezoid (device
 * pointers, column-major) through the fp64 MFMA SYRK kernel. */
int64_t sc_debug_syrk(double* dC, int32_t ldc, const double* dA, int32_t lda, int32_t M, int32_t N,
                      int32_t K);
/* sc_debug_syrk on the kernel instance the caller names: bt = 64 or 128 (tile edge), lean
 * = 1 only with bt = 64, tag and epi 0 or 1.  Never gathers, never pre-factors.  Needs 1 <=
 * N <= M, K >= 1, lda and ldc >= M; an inconsistent combination returns SC_ERR_ARG before
 * any device call.  sc_debug_syrk is bt = 64, lean = (K <= 128), tag = epi = 0. */
int64_t sc_debug_syrk_ex(double* dC, int32_t ldc, const double* dA, int32_t lda, int32_t M, int32_t N, int32_t K,
                         int32_t bt, int32_t lean, int32_t tag, int32_t epi);
/* The panel kernels on block k0 (a multiple of 64, nb = min(64, w - k0) columns) of a
 * caller's m x w front panel (device, column-major, ld = m, 1 <= w <= m), through a
 * one-front plan with an identity post table.  mode 0: the diagonal-block POTRF alone; 1:
 * the TRSM with the POTRF fused; 2: the POTRF, then the TRSM on the factored block; 3: the
 * POTRF, then the partial-block TRSM.  Modes 1 and 2 need nb = 64, mode 3 nb < 64;
 * anything else returns SC_ERR_ARG before any device call.  *info receives the status
 * word: 0, or the first failing column of the panel + 1. */
int64_t sc_debug_panel(double* dF, int32_t m, int32_t w, int32_t k0, int32_t mode, int32_t* info);
/* The two kernels of one block step of sc_updown_host on block k0 (a multiple of 64, nb =
 * min(64, w - k0) columns) of a caller's m x w front panel (device, column-major, ld = m, 1
 * <= w <= m) and a caller's m x 16 workspace dW (device, ROW-major: entry (front row i,
 * column c) at 16 i + c), through a one-front plan whose row list is the identity: the
 * block kernel on rows [k0, k0 + nb) ([L11 W1] T = [L11' 0], those rows of dW zeroed),
 * then the row kernel on rows [k0 + nb, m) ([L21 W2] T in place).  sign +1 / -1.  Rows of
 * dF and dW above k0, other columns and the strict upper triangle of the diagonal block
 * are neither read nor written.  *info: 0, or the failing column of the panel + 1 of a
 * downdate (nothing of the block is then written). */
int64_t sc_debug_updown_block(double* dF, int32_t m, int32_t w, int32_t k0, double* dW, int32_t sign,
                              int32_t* info);
/* One step of the solve family on block k0 (a multiple of 128, nb = min(128, w - k0) columns)
 * of a caller's m x w front panel (device, column-major, ld = m, 1 <= w <= m < 2^20) through
 * a one-front plan whose row list is the identity, with the step's tasks cut as a solve cuts
 * them.  width 1: the single-vector kernels, vectors of doubles; width 16: the panel kernels,
 * vectors of 16-wide rows (entry (row, j) at 16 row + j).  dC: m rows (c over the front's
 * rows), dY: w rows (op 4: m rows), dU: m - w rows (may be NULL when m == w).
 *   op 0: the inverses of the block's one or two 64 x 64 diagonal blocks and, for nb > 64, the
 *         off-diagonal quadrant, into the block's strict upper triangle (vectors unused);
 *   op 1: the forward step: y_blk = X c_blk to dY, L(r, blk) y_blk subtracted from dC (rows r
 *         < w) or dU (row r at r - w) for the rows r below the block;
 *   op 2: the backward step: c_blk = X^T (c_blk - L(R, blk)^T c_R), R the rows below;
 *   op 3: the L Z step: L11 z_blk added to c_blk, L(r, blk) z_blk to dC / dU below; Z in dY;
 *   op 4: the L^T Z step: c_blk = L11^T z_blk + L(R, blk)^T z_R; Z in dY over all m rows.
 * Ops 1 and 2 need the inverses of an op 0 call in dF; ops 3 and 4 are width 16 only.  A null
 * pointer, k0 >= w, k0 % 128 != 0, another width or op, or a product with width 1 returns
 * SC_ERR_ARG before any device call.  Synchronous. */
int64_t sc_debug_solve_step(double* dF, int32_t m, int32_t w, int32_t k0, int32_t op, int32_t width, double* dC,
                            double* dY, double* dU);
/* The forward gather of the solves on one parent front of w >= 1 pivots and mb >= 0
 * contribution rows (row list the identity) with nchild children taken in the order given:
 * child q holds rel_ptr[q + 1] - rel_ptr[q] entries (width 16: 16-wide rows) of u,
 * consecutive in dUc, and entry i goes to front row t = relind[i]: added to dC[t] for t < w,
 * to dU[t - w] otherwise.  rel_ptr and relind are host arrays, validated before any device
 * call (rel_ptr ascending from 0, relind in [0, w + mb) and injective within a child); dUc,
 * dC (w rows) and dU (mb rows; NULL when mb == 0) device.  The gather runs on a copy of dUc
 * and dU in one buffer of the hook's own; dC is the caller's.  Synchronous. */
int64_t sc_debug_solve_gather(int32_t width, int32_t w, int32_t mb, int32_t nchild, const int64_t* rel_ptr,
                              const int32_t* relind, const double* dUc, double* dC, double* dU);
/* Best wall time (ms) of reps synchronous factorizations from device values
 * (sc_factor_device(num, d_Ax, 1): launch, run, status read-back), timed in C. */
int64_t sc_debug_time_factor(sc_numeric* num, const double* d_Ax, int32_t reps, double* best_ms);
/* Debug: eager = 1 launches the solve sweeps directly instead of replaying their graph. */
int64_t sc_debug_solve_eager(sc_numeric* num, int32_t eager);
/* Selected inversion: profile = 1 makes the next sc_selinv calls record a HIP event after
 * every launch; ms[4] (may be NULL) receives the split of the last profiled call over the
 * kernel classes W, Z_RK, Z_KK and push, milliseconds. */
int64_t sc_debug_selinv_times(sc_numeric* num, int32_t profile, double* ms);
/* sc_export_L_cols of the selected inverse: columns [j0, j1) of Z straight from the Z
 * panel (the column's front rows from j down, relaxed-zero positions included), for
 * factors too large for sc_selinv_export.  Computes first like the sc_selinv accessors;
 * returns the entry count; a failed factorization's status > 0 cannot be told from a
 * count, so check sc_selinv first. */
int64_t sc_debug_selinv_cols(sc_numeric* num, int64_t j0, int64_t j1, int64_t* cp, int32_t* ri, double* rx);
/* One step of the selected inversion's recurrence alone (no handle) on block k0 (a multiple of
 * 128) of a one-front plan whose row list is the identity: nb = min(128, w - k0), k1 = k0 + nb,
 * K = [k0, k1), R = [k1, m), nr = m - k1, mb = m - w, 1 <= w <= m < 2^20.  dL (the factor) and
 * dZ are m x w panels (device, column-major, ld = m); dL holds the rows below the block and, in
 * the block's strict upper triangle, the inverses an sc_debug_solve_step op 0 call stored on the
 * same buffer (X(i, k), k < i, at row k, column i of the block; the diagonal is L's).  dZii: mb
 * x mb (ld = mb, both triangles; may be NULL when mb == 0); dW: nr x nb (column-major, ld = nr;
 * may be NULL when nr == 0).  The tasks are cut as sc_selinv cuts them.
 *   op 0: W = L_RK X to dW.  Reads the block's diagonal and strict upper triangle and rows R of
 *         columns K of dL; nothing of dZ and dZii.
 *   op 1: Z_RK = -Z_RR W to rows R of columns K of dZ and, for the rows p < w of R, mirrored to
 *         rows K of column p.  Reads dW, rows R of columns [k1, w) of dZ (Z_RR's pivot part,
 *         straight and transposed) and dZii; nothing of dL, columns K or rows < k1.
 *   op 2: Z_KK = X^T X - W^T Z_RK to both triangles of rows K x columns K of dZ: one product per
 *         64 x 64 tile of the lower triangle for nb + nr <= 512, else chunks of 256 terms into a
 *         partials buffer of the hook's own and a reduction in chunk order.  Reads dW, rows R of
 *         columns K of dZ and the block's diagonal and strict upper triangle of dL.
 * Returns the number of workgroups launched (ops 0 and 1: the 64-row tiles; op 2: products plus
 * reductions); ops 0 and 1 with nr == 0 return SC_OK with no launch.  Everything is validated
 * before any device call: a null array, k0 >= w, k0 % 128 != 0, another op or sizes outside
 * the above return SC_ERR_ARG with a message.  Synchronous. */
int64_t sc_debug_selinv_step(const double* dL, double* dZ, int32_t m, int32_t w, int32_t k0, int32_t op,
                             const double* dZii, double* dW);
/* The push of the selected inversion alone (no handle): a child with mbc contribution rows
 * under a parent front (m, w) whose Z is in dZ (m x w, ld = m) and dZii (mb x mb, mb = m - w;
 * may be NULL when mb == 0): dOut[a + mbc b] = Zfront[relind[a], relind[b]], read from the lower
 * triangles alone (element (max, min)).  relind: host, in [0, m), strictly ascending (validated
 * before any device call, as are the sizes and pointers: SC_ERR_ARG with a message).  dOut (mbc
 * x mbc, device) must not overlap dZii.  mbc == 0: SC_OK, nothing launched.  Synchronous. */
int64_t sc_debug_selinv_push(int32_t m, int32_t w, const double* dZ, const double* dZii, int32_t mbc,
                             const int32_t* relind, double* dOut);
/* One of the four extend-add implementations alone (no handle) on one parent front of m rows
 * and w pivots (1 <= w <= m <= 65536, mb = m - w) with nchild prescribed children, taken in
 * the order given.  Host arrays, all validated before any device call (SC_ERR_ARG with a
 * message): rel_ptr (nchild + 1) ascending from 0; child q has mbc_q = rel_ptr[q + 1] -
 * rel_ptr[q] <= m contribution rows at the parent positions relind[rel_ptr[q] ..], each in
 * [0, m) and strictly ascending within the child; the A entries of pivot column j are a_ptr[j]
 * .. a_ptr[j + 1] (a_ptr ascending from 0, w + 1 long), entry e at front row a_pos[e] in [j, m)
 * (no row twice in a column) with the value d_Ax[a_src[e]], a_src in [0, nval).  Device
 * buffers of the caller: d_Ax (nval doubles); d_child_cb, the children's contribution blocks
 * back to back, child q mbc_q x mbc_q column-major of which only the lower triangle is read;
 * d_panel (m x w, ld = m); d_cb (mb x mb, ld = mb; may be NULL when mb == 0).  The one-parent
 * plan's bounds tables, gather table and tasks are built by the library's own code (symbolic.cpp
 * block_bounds, schedule.cpp gather_segments_front and asm_block_tasks).
 *   op 0: assemble_cols_kernel on the 16-column blocks of front columns [0, p0), p0 = w or m;
 *         p1 = p2 = 0.
 *   op 1: assemble_tile_kernel likewise on [0, p0); [p1, p2) with 0 <= p1 <= p2 <= m are handed
 *         to every task as its column limits (both < 0: no limits).  Tasks of blocks outside
 *         the limits are launched and write nothing.
 *         Ops 0 and 1 write entry (i, j >= i) of the columns they cover: 0.0, overwritten by the
 *         A entry if there is one, then += each child's entry in child order.
 *   op 2: front_small_kernel (one front per workgroup) on the bucket p0 >= m, p0 in {32, 64, 88,
 *         96, 128}: assembles as above in LDS, factors the w pivots, writes the panel's lower
 *         trapezoid and the lower triangle of the contribution block.
 *   op 3: the gathering contribution-block SYRK on the instance (bt = p0, lean = p1, epi = p2) of
 *         sc_debug_syrk_ex, tag 1: d_cb = sum of the children's entries - A A^T with A = rows [w, m)
 *         of d_panel, K = w.  d_cb is written, never read; needs mb >= 1; the A entries are unused.
 * *info (may be NULL but for op 2): the status word, the first failing panel column + 1, or 0.
 * Synchronous. */
int64_t sc_debug_extend_add(int32_t op, int32_t m, int32_t w, int32_t nchild, const int64_t* rel_ptr,
                            const int32_t* relind, const int64_t* a_ptr, const int32_t* a_pos, const int64_t* a_src,
                            int64_t nval, const double* d_Ax, const double* d_child_cb, double* d_panel, double* d_cb,
                            int32_t p0, int32_t p1, int32_t p2, int32_t* info);
/* The Schur complement's product kernel alone on caller data (device memory, no handle):
 * dS = dD dD^T for the lower triangle of dD (ns x ns, column-major, ldd, lds >= ns), both
 * triangles of dS written; what dD holds above its diagonal is never used, nothing outside
 * the ns x ns window of dS is written.  Synchronous. */
int64_t sc_debug_schur_llt(const double* dD, int32_t ns, int64_t ldd, double* dS, int64_t lds);
/* The product / residual kernels alone (no handle) on a caller's row structure -- host
 * arrays in the layout of sc_spmv_structure, validated before anything is launched: rp
 * ascending from 0, ci in [0, n), sp in [0, nval) -- with values d_Ax (nval doubles) and
 * panels in device memory: d_X, d_B, d_R, d_W are n x nrhs column-major (leading dimensions
 * >= n, nrhs <= 16).  mode 0: R = A X (B, W, norms unused); 1 / 2: R = B - A X accumulated
 * in fp64 / as a compensated dot product, W = |B| + |A| |X| (d_W may be NULL) and d_norms
 * (may be NULL; 5 x 16 doubles, value q of column c at 16 q + c): max |r|, max |x|, max |b|,
 * max |r| / w (0 / 0 = 0, nonzero / 0 = +inf), largest row sum of |A|; columns >= nrhs
 * zero.  Nothing outside the n x nrhs windows is read or written.  Synchronous. */
int64_t sc_debug_spmv(int32_t mode, int32_t n, const int64_t* rp, const int32_t* ci, const int64_t* sp, int64_t nval,
                      const double* d_Ax, int32_t nrhs, const double* d_X, int64_t ldx, const double* d_B, int64_t ldb,
                      double* d_R, int64_t ldr, double* d_W, int64_t ldw, double* d_norms);
/* The three kernels of the weighted normal equations alone (no handle) on a caller's
 * structures: host arrays, validated before anything is launched (pointer arrays ascending
 * from 0, every position, row and index inside the counts given), values and panels in
 * device memory.  Synchronous; SC_ERR_ARG with a message in sc_last_error.
 *   sc_debug_normal_form  d_Sx[e] for the ne entries whose term lists are tp / ta / tb / tr
 *                         (sc_normal_term_lists), cpos (position in d_Cx or -1) and dcol (the
 *                         entry's column when it is diagonal, else -1); nJ, nw, nC, nd: the
 *                         lengths of d_Jx, d_w, d_Cx, d_d (d_w, d_Cx, d_d may be NULL);
 *   sc_debug_normal_mul   mode 0: R = J X; 1 / 2: R = B - J X in fp64 / compensated, over the
 *                         row structure rp / ci / sp of m rows, ci in [0, n), sp in [0, nval);
 *                         X n x nrhs, B and R m x nrhs, nrhs <= 16;
 *   sc_debug_normal_mult  G = J^T diag(w) Y down the CSC columns Jp / Ji (row indices in [0, m));
 *                         Y m x nrhs, G n x nrhs, d_w may be NULL.
 *   sc_debug_normal_pair  the pair path of the least-squares gradient: (R, Rl) = B - J X as the
 *                         unevaluated pair the compensated residual leaves, over rp / ci / sp,
 *                         then (G, Gl) = J^T diag(w) (R + Rl) by the pair product down Jp / Ji,
 *                         as if in twice the working precision; |Rl| <= ulp(R) / 2, likewise Gl.
 *                         X n x nrhs, B, R, Rl m x nrhs (ldr for both), G, Gl n x nrhs (ldg).
 * Nothing outside the windows of the outputs is written. */
int64_t sc_debug_normal_pair(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const int64_t* rp,
                             const int32_t* ci, const int64_t* sp, const double* d_Jx, const double* d_w, int32_t nrhs,
                             const double* d_X, int64_t ldx, const double* d_B, int64_t ldb, double* d_R, double* d_Rl,
                             int64_t ldr, double* d_G, double* d_Gl, int64_t ldg);
int64_t sc_debug_normal_form(int64_t ne, const int64_t* tp, const int32_t* ta, const int32_t* tb, const int32_t* tr,
                             const int64_t* cpos, const int32_t* dcol, int64_t nJ, int64_t nw, int64_t nC, int64_t nd,
                             const double* d_Jx, const double* d_w, const double* d_Cx, const double* d_d,
                             double lambda, double* d_Sx);
int64_t sc_debug_normal_mul(int32_t mode, int64_t m, int64_t n, const int64_t* rp, const int32_t* ci,
                            const int64_t* sp, int64_t nval, const double* d_Jx, int32_t nrhs, const double* d_X,
                            int64_t ldx, const double* d_B, int64_t ldb, double* d_R, int64_t ldr);
int64_t sc_debug_normal_mult(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const double* d_Jx,
                             const double* d_w, int32_t nrhs, const double* d_Y, int64_t ldy, double* d_G,
                             int64_t ldg);
/* One vector kernel of the conjugate gradients alone (no handle) on caller panels in device
 * memory, n x nrhs column-major, nrhs <= 16, leading dimensions >= n; mask: bit c set = column
 * c takes part (bits >= nrhs are ignored); coef: 16 host doubles, one per column; out: 2 x 16
 * host doubles, value q of column c at 16 q + c, zero for a column outside the mask.
 *   which 0  dot:     out[c] = sum_i A(i, c) B(i, c) and, with d_C, out[16 + c] = sum_i A(i, c)
 *                     C(i, c) (d_C may be NULL, coef unused);
 *   which 1  update:  A += coef_c C, B -= coef_c D, each entry one fma; out[c] = sum_i B(i, c)^2
 *                     of the new B (the iteration's x, r, p, q);
 *   which 2  direction: A = C + coef_c A (one fma; the iteration's p and z); d_T (may be NULL):
 *                     n x 16 doubles, the new A in 16-wide row-major form, d_T[16 i + c], zero
 *                     in the columns outside the mask and those >= nrhs (out unused);
 *   which 3  the same with A = C: A is not read, coef unused.
 * Rows >= n, columns >= nrhs and columns outside the mask are neither read nor written.  The
 * sums are bitwise repeatable.  Everything is validated before a launch: an unknown kernel, n
 * < 0, nrhs outside [0, 16], a null array the kernel needs or a leading dimension below n
 * return SC_ERR_ARG with a message; n == 0 or nrhs == 0: SC_OK, out zero.  Synchronous. */
int64_t sc_debug_pcg_vec(int32_t which, int32_t n, int32_t nrhs, uint32_t mask, const double* coef, double* d_A,
                         int64_t lda, double* d_B, int64_t ldb, const double* d_C, int64_t ldc, const double* d_D,
                         int64_t ldd, double* d_T, double* out);
/* The two panel kernels of the eigensolver alone (no handle) on caller panels in device memory.
 * A panel is n x b column-major (b <= 16, leading dimension >= n), a basis nb <= 64 panels
 * vstride doubles apart (vstride >= b ldv when nb > 1); a tile is a 16 x 16 matrix in 256 host
 * doubles, M(a, c) at a + 16 c.  Rows >= n and columns >= b of a panel are neither read nor
 * written.
 *   gram:   out (nb tiles, host) = V_i^T W, i < nb; entries with a or c >= b are zero.  d_V may
 *           be d_W.  A block's tile has the same bits whatever nb and its place in the basis.
 *   update: Out = beta W + sum_{i < nb} V_i C_i with Out and W n x bc (bc <= 16), C nb tiles on
 *           the host (entries with a >= b or c >= bc are not read); beta == 0: d_W is not read
 *           and may be NULL; nb == 0 or b == 0: Out = beta W.  d_Out may be d_W and may be a block
 *           of d_V (a wave reads its rows of every operand before it writes them).
 * Both repeat bit for bit.  Everything is validated before a launch: n < 0, b or bc outside
 * [0, 16], nb outside [0, 64], a null array the kernel needs, a leading dimension below n or
 * overlapping blocks return SC_ERR_ARG with a message; gram with n == 0 or b == 0: SC_OK, out
 * zero; update with n == 0 or bc == 0: SC_OK.  Synchronous. */
int64_t sc_debug_eigs_gram(int32_t n, int32_t b, int32_t nb, const double* d_V, int64_t ldv, int64_t vstride,
                           const double* d_W, int64_t ldw, double* out);
int64_t sc_debug_eigs_update(int32_t n, int32_t b, int32_t bc, int32_t nb, double beta, double* d_Out, int64_t ldo,
                             const double* d_W, int64_t ldw, const double* d_V, int64_t ldv, int64_t vstride,
                             const double* C);
/* The eigensolver's host dense algebra alone (no GPU).  which 0: A (m x m row-major, symmetric,
 * m <= 512) is replaced by its unit eigenvectors (columns), d (m) gets the eigenvalues
 * ascending; returns 0, or 1 when the QL iteration did not converge.  which 1: A is a tile G
 * whose leading m x m part (m <= 16; upper triangle read) is factored G = R^T R with the pivot
 * threshold d[0]; d (256 doubles) gets the tile inv(R), the columns of dropped pivots zero;
 * returns the number of dropped columns. */
int64_t sc_debug_eigs_dense(int32_t which, int32_t m, double* A, double* d);
/* Chain launches (runs of single small-front levels): enable = 1 makes the next
 * eager factorizations record 8 shader-clock stamps per chained front (phase
 * boundaries); enable = 0 copies up to cap of them to out.  Returns the count. */
int64_t sc_debug_chain_stamps(sc_numeric* num, int32_t enable, uint64_t* out, int64_t cap);
/* Microbenchmarks: which=0 register-only fp64 MFMA probe (TFLOP/s; M blocks of
 * 4 waves, K iterations, arg accumulators); which=1/5 the SYRK kernel on an M x M
 * triangle with depth K, tile arg (64/128), with / without the XCD tile order
 * (TFLOP/s); which=2/3 the panel POTRF / TRSM kernel on an M x 64 front
 * (microseconds per launch). */
int64_t sc_debug_bench(int32_t which, int32_t M, int32_t K, int32_t reps, int32_t arg, double* tflops);
/* Placement probe: nwg workgroups of `threads` threads, each spinning spin_ticks of the
 * 100 MHz clock; out[2 i] = HW_ID, out[2 i + 1] = XCC_ID of workgroup i. */
int64_t sc_debug_hwid(int32_t nwg, int32_t threads, int32_t spin_ticks, uint32_t* out);
/* Dispatch-contention probe: a panel-update SYRK "hog" (M x M triangle, K deep) on a
 * low-priority stream against a chain of nchain fused POTRF + TRSM launches (chain_rows
 * x 64 front) on the high-priority stream.  mode bit 0: hog stream CU-masked (every
 * mask_stride-th CU off), bit 1: hog replayed from a hipGraph, bit 2: chain from a
 * hipGraph.  out[8]: chain alone, hog alone, chain under hog, hog under chain, both
 * (ms), CUs available to the hog. */
int64_t sc_debug_contention(int32_t M, int32_t K, int32_t chain_rows, int32_t nchain, int32_t mode,
                            int32_t mask_stride, double* out);

/* Digest of the launch schedule a handle would build, planned on the host (no device
 * needed): nranks == 1 and emulate == 0 as sc_numeric_create; otherwise as a multi-rank
 * handle of `rank` (emulate 0), or of every rank in one process with transfers as device
 * copies (1) or RCCL to self (2).  out[0] = a 64-bit hash of every decoded schedule
 * entry and every uploaded task array (pointers as arena + offset); then the entries
 * per call kind (front small, chain, tiny tree, tiny dense, assembly by columns / tiled
 * / tiled with limits, POTRF, TRSM fused / prefactored / partial, SYRK panel / CB, comm,
 * record, wait); then tail-split launches, pre-factor launches, comm steps, events,
 * messages and gather segments.  Writes at most cap values, returns their number. */
int64_t sc_debug_schedule_digest(const sc_symbolic* sym, int32_t nranks, int32_t rank, int32_t emulate,
                                 int64_t* out, int64_t cap);
/* The SYRK launches of the schedule sc_debug_schedule_digest plans (same arguments), in
 * schedule order, eight values each: kind (0 panel update, 1 contribution block), tile
 * edge bt, lean, epi, pf, tail, tile count, and whether any task of the launch gathers
 * its children (gs >= 0).  Writes at most cap values, returns their number. */
int64_t sc_debug_schedule_syrk(const sc_symbolic* sym, int32_t nranks, int32_t rank, int32_t emulate,
                               int64_t* out, int64_t cap);
/* The same digest of a live handle, hashed at creation from what it uploaded. */
int64_t sc_debug_numeric_digest(const sc_numeric* num, int64_t* out, int64_t cap);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif

#endif /* SPARSECHOLESKY_DEBUG_H */
