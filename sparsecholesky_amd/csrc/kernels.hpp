// Device-side plan layout and kernel launch wrappers (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace sc {

// Inner panel width (POTRF/TRSM block); the diagonal block lives in LDS.
constexpr int PNB = 64;
// Rows per TRSM workgroup (one lane per row).
constexpr int TRSM_ROWS = 256;
// Columns owned by one assembly workgroup (one wave per column at a time).
constexpr int ASM_COLS = 16;
constexpr int ASM_ROWS = 256;  // rows per LDS tile of the write-once assembly
constexpr int ASM_TILE_MIN_M = 512;   // fronts at least this tall use the write-once tile kernel
// Output tile edges of the MFMA SYRK kernel (per launch).
constexpr int SYRK_BT_SMALL = 64;
constexpr int SYRK_BT_LARGE = 128;

// C/D register map of v_mfma_f64_16x16x4_f64 on gfx950 (cdna_hip_programming.md
// section 3): col = lane & 15, row = (lane >> 4) + 4 * reg.
#define MFMA_F64_ROW(lane, r) (((lane) >> 4) + 4 * (r))

// child columns per batch of loads in the CB SYRK's extend-add gather
#ifndef SC_GATHER_Q
#define SC_GATHER_Q 4
#endif

// All device arrays of the numeric plan (internal numbering).
struct DevPlan {
    const int32_t* sn_start;    // ns+1
    const int32_t* sn_m;        // ns
    const int64_t* panel_off;   // ns+1
    const int64_t* cb_off;      // ns+1
    const int32_t* child_ptr;   // ns+1
    const int32_t* child_list;
    const int64_t* rel_ptr;     // ns+1
    const int32_t* relind;
    const int64_t* rb_ptr;      // ns+1
    const int32_t* rel_bnd;     // per child: CB row bounds of the parent's ASM_ROWS row tiles
    const int64_t* cbk_ptr;     // ns+1
    const int32_t* col_bnd;     // per child: CB row bounds of the parent's ASM_COLS column blocks
    const int64_t* tb_ptr;      // ns+1
    const int32_t* tile_bnd;    // per child: CB row bounds of the parent's 64-row CB blocks (symbolic.hpp)
    const int64_t* a_ptr;       // n+1 (internal columns)
    const int32_t* a_pos;       // row position in the column's front
    const int64_t* a_src;       // index into the input value array
    double* panel_pool;
    double* cb_pool;
    int32_t* info;              // min failing natural column + 1
    const int32_t* post;        // n: internal -> natural column (what a failing pivot reports)
    // per supernode (or null: every front whole): the front columns [0, asm_end) the large-front
    // assembly fills -- w where the CB SYRK gathers the contribution block itself, else m
    const int32_t* asm_end;
};

// One child's share of one 64 x 64 block (rb, cb) of a parent's contribution block
// (the CB SYRK's extend-add gather): its CB rows [ilo, ihi) map into the parent's CB
// rows [64 rb, 64 rb + 64) and its CB columns [jlo, jhi) into the parent's CB columns
// [64 cb, 64 cb + 64); cb / rel: the child's CB (ld mbc) and relative indices (parent
// front positions).  Host-built per gathering task (schedule.cpp gather_segments).
struct GSeg {
    const double* cb;
    const int32_t* rel;
    int32_t mbc, ilo, ihi, jlo, jhi, pad;
};

// The schedule's gather tables (device), kernel arguments of the CB SYRK launches.
struct GatherTab {
    const int64_t* blk = nullptr;
    const GSeg* seg = nullptr;
    int32_t* info = nullptr;  // status word (pivot failures of the panel pre-factor workgroups)
    const int32_t* post = nullptr;  // DevPlan.post
};

// One lower-trapezoid SYRK update: C[i,j] -= sum_k A[i,k] A[j,k], j < N, j <= i < M.
// gs >= 0 (CB updates only): C is front gs's whole contribution block and is not read;
// the children's CB entries that fall into it are gathered instead (the extend-add of
// the reference's apply_update, chol.hpp:1196) and C = sum(children) - A A^T is written.
// gv: the hosted rank that holds the children.  gb: the task's offset in the gather
// table's block list (GatherTab.blk: per 64 x 64 block (rb, cb <= rb) of the CB, at
// gb + rb (rb + 1) / 2 + cb, the block's first segment in GatherTab.seg; the next entry
// ends it).
struct GemmTask {
    double* C;
    const double* A;
    int64_t ldc;
    int64_t lda;
    int32_t M, N, K;
    int32_t gs = -1, gv = 0;
    int64_t gb = -1;
    int32_t gw = 0;  // gathering tasks: the front's width (the CB starts at front row gw; K may be one slab)
    // panel updates (launches with pf = 1): >= 0 = the internal column of the 64 x 64 diagonal
    // block at C's origin, which this task's pre-factor workgroup (tile marker y = -1) updates
    // and factors in registers, so the next chain step's TRSM loads L11 instead of factoring it
    int32_t pf = -1;
};
// Strided <-> packed copy of a rows x cols block (pack: a -> b; unpack: b -> a).
struct Copy2D {
    double* a;  // strided, leading dimension lda
    double* b;  // packed, leading dimension rows
    int64_t lda;
    int32_t rows, cols;
};

constexpr int COPY_COLS = 16;    // columns per copy workgroup
constexpr int COPY_ROWS = 2048;  // rows per copy workgroup
// copy tiles encode (column offset | row chunk << 16): the host cuts wider blocks into
// descriptors of at most this many columns (schedule.cpp emit_step)
constexpr int COPY_MAX_COLS = 32768;
static_assert(COPY_MAX_COLS + COPY_COLS <= 65536, "column offsets fit the tile's 16 low bits");
// tiles: (descriptor, first column | row chunk << 16) per workgroup
hipError_t launch_copy2d(const Copy2D* descs, const int2* tiles, int count, bool unpack, hipStream_t st);

// ---- triangular solves with the supernodal factor ----
struct SolvePlan {
    const int32_t* sn_start;
    const int32_t* sn_m;
    const int64_t* panel_off;
    const int64_t* rows_ptr;  // ns+1
    const int32_t* rows;      // front rows (internal numbering), first w = the pivots
    const double* panel_pool;
    double* c;                // right-hand side / solution, internal numbering
    double* y;                // forward result (fused steps write here; copied to c after the sweep)
    // deterministic accumulation (no atomics): the forward sweep leaves each front's
    // updates of its contribution-block rows in u (u + u_off[s], mb entries, multifrontal
    // style), and the parent's gather (solve_fwd_gather_kernel) adds its children's u in
    // child order; the backward GEMV leaves one partial column sum per workgroup in part
    // (SOLVE_NB per task of the launch), summed in task order by the diagonal kernel
    double* u;
    const int64_t* u_off;     // per supernode
    const int32_t* child_ptr; // ns+1
    const int32_t* child_list;
    const int64_t* rel_ptr;   // ns+1: child c's CB rows -> parent front rows
    const int32_t* relind;
    double* part;
};
constexpr int SOLVE_ROWS = 256;  // front rows per GEMV workgroup
constexpr int SOLVE_NB = 128;    // columns per solve step (two 64-blocks)
// X = inv(L11) of the 64 x 64 diagonal blocks (s, k0) (tasks) into their strict upper
// triangles, then (tasks2: 128-column blocks wider than 64) the off-diagonal quadrant
// E = -Xb B Xa of the 128-block inverse into the block's upper-right square; the
// factor's lower part is untouched.  Once per factorization, before the first solve.
hipError_t launch_solve_inv(const SolvePlan& P, const int2* tasks, int count, const int2* tasks2, int count2,
                            hipStream_t st);
// Forward step: tasks (s, k0, r0, writer) of 128-column blocks; every workgroup forms
// y = X128 c_blk and applies -L[r, blk] y for its SOLVE_ROWS rows: to c for the front's
// own later pivot rows, to u for its contribution-block rows (no atomics: each row has
// one writer per step); r0 < 0 = the diagonal block only.
hipError_t launch_solve_fwd(const SolvePlan& P, const int4* tasks, int count, hipStream_t st);
// Forward gather, before a level's first step: per front s of the list, its children's
// u in child order -- entries at s's pivot rows into c, the rest into u of s.
hipError_t launch_solve_fwd_gather(const SolvePlan& P, const int32_t* fronts, int count, hipStream_t st);
// Backward step: tasks (s, k0, r0): partial -L[rows, blk]^T x[rows] per workgroup into
// part, then tasks (s, k0, g0, ng): c_blk plus the block's ng partials (launch-relative
// GEMV tasks g0..) in order, x_blk = X128^T c_blk.
hipError_t launch_solve_gemv(const SolvePlan& P, const int4* tasks, int count, hipStream_t st);
hipError_t launch_solve_diag(const SolvePlan& P, const int4* tasks, int count, hipStream_t st);
// c[i] = b[perm[i]] (gather) or x[perm[i]] = c[i] (scatter)
hipError_t launch_permute(double* dst, const double* src, const int32_t* perm, int64_t n, bool scatter,
                          hipStream_t st);

// Panel solves (SOLVE_RHS right-hand sides at once): the same tasks with c, y, u and part
// of the plan holding SOLVE_RHS-wide rows (entry (row, j) at SOLVE_RHS row + j; part:
// SOLVE_NB x SOLVE_RHS per GEMV task); the products over the rows below a block run on
// v_mfma_f64_16x16x4_f64.  launch_solve_inv is shared with the single-vector solve.
constexpr int SOLVE_RHS = 16;
hipError_t launch_solve_fwd_multi(const SolvePlan& P, const int4* tasks, int count, hipStream_t st);
hipError_t launch_solve_fwd_gather_multi(const SolvePlan& P, const int32_t* fronts, int count, hipStream_t st);
hipError_t launch_solve_gemv_multi(const SolvePlan& P, const int4* tasks, int count, hipStream_t st);
hipError_t launch_solve_diag_multi(const SolvePlan& P, const int4* tasks, int count, hipStream_t st);
// c[SOLVE_RHS i + j] = io[perm[i] + j n] (gather) or back (scatter); io: n x SOLVE_RHS column-major
hipError_t launch_permute_multi(double* c, double* io, const int32_t* perm, int64_t n, bool scatter,
                                hipStream_t st);

// Products with the factor in the panel family (fp64 MFMA), on the solves' task lists:
// the input Z in P.y (read-only), the result in P.c.  Diagonal blocks are read through
// their lower triangle only, so the stored inverses (launch_solve_inv) are never seen.
// X = L Z: a bottom-up sweep, c and u zeroed first; per level launch_solve_fwd_gather_multi
// (children's u into c / u), then per step tasks (s, k0, r0, writer) add L(rows, blk) Z_blk
// into c (own later pivots) or u (contribution-block rows), the writer also L_blk Z_blk.
hipError_t launch_mul_l_multi(const SolvePlan& P, const int4* tasks, int count, hipStream_t st);
// X = L^T Z: tasks (s, k0, r0) leave L(rows, blk)^T Z(rows) in part, then tasks (s, k0, g0,
// ng) write X_blk = L_blk^T Z_blk + the ng partials in order.  Steps are independent of
// each other but for the part buffer they share.
hipError_t launch_mul_lt_gemv_multi(const SolvePlan& P, const int4* tasks, int count, hipStream_t st);
hipError_t launch_mul_lt_diag_multi(const SolvePlan& P, const int4* tasks, int count, hipStream_t st);
// out[0] = 2 sum_j log L(j, j) over the n panel diagonals (ns supernodes), in a fixed
// order: part[ceil(n / LOGDET_NT)] per-workgroup sums, then one workgroup over part.
constexpr int LOGDET_NT = 256;
hipError_t launch_logdet(const SolvePlan& P, int ns, int64_t n, double* part, double* out, hipStream_t st);

// ---- selected inversion: Z = (P A P^T)^-1 on the pattern of L (Takahashi recurrence) ----
// One 128-column block K = [k0, k1) of front s: R = front positions [k1, m), nr = m - k1;
// W = L_RK X (nr x nb, column-major, ld = nr) sits at wbuf + woff for the length of its step.
struct SelBlk {
    int32_t s, k0;
    int64_t woff;
};
struct SelPlan {
    const int32_t* sn_start;
    const int32_t* sn_m;
    const int64_t* panel_off;  // per supernode, of both the L panel and the Z panel (m x w, ld = m)
    const int64_t* cb_off;     // per supernode: Z_II (mb x mb, ld = mb, both triangles) in the work arena
    const int64_t* rel_ptr;    // child c's contribution-block rows -> parent front positions
    const int32_t* relind;
    const double* lpanel;      // the factor, with the stored diagonal-block inverses (launch_solve_inv)
    double* zpanel;            // Z panel: Z_JJ mirrored over the w x w pivot square, rows >= w below it
    double* zii;               // the work arena
    double* wbuf;
    double* part;              // 64 x 64 partials of the split Z_KK products
    const SelBlk* blk;
};
constexpr int SEL_NW = 4;             // waves of a W / Z_RK workgroup (8 = 128-row tiles measured 7 % slower at 128^3)
constexpr int SEL_BM = 16 * SEL_NW;   // its output rows (16 per wave)
constexpr int SEL_KT = 64;            // tile edge of the Z_KK products (four waves)
constexpr int SEL_BK = 16;   // K staged per round through LDS
// Z_KK products deeper than SEL_KSPLIT (K = nb + nr) are cut into chunks of SEL_KC, one
// workgroup each: a tall front's block would otherwise run on three workgroups
constexpr int SEL_KC = 256, SEL_KSPLIT = 512;
inline int selinv_kchunks(int64_t K) { return K <= SEL_KSPLIT ? 1 : (int)((K + SEL_KC - 1) / SEL_KC); }
// tiles (block, SEL_BM-row tile) of the nr x nb outputs, all nb columns per workgroup:
// W = L_RK X with X = inv(L_KK) read in its stored form (X(i, k), k < i, at block row k,
// column i; the diagonal as 1 / L(i, i)), then Z_RK = -Z_RR W on v_mfma_f64_16x16x4_f64 with
// Z_RR read from the Z panel (pivot square, rows >= w straight and transposed) and Z_II;
// Z_RK is also mirrored into the pivot square for rows < w.
hipError_t launch_selinv_w(const SelPlan& P, const int2* tiles, int count, hipStream_t st);
hipError_t launch_selinv_zrk(const SelPlan& P, const int2* tiles, int count, hipStream_t st);
// Z_KK = X^T X - W^T Z_RK on the 64 x 64 tiles (ti, tj <= ti) of its lower triangle, each
// written to both triangles of the block's square.  tasks (block, 2 ti + tj, chunk, slot):
// slot < 0 the whole product; else one K chunk into partial slot `slot`, and red (block,
// 2 ti + tj, first slot, chunks) sums a tile's partials in chunk order in a second launch.
hipError_t launch_selinv_zkk(const SelPlan& P, const int4* tasks, int count, const int4* red, int nred,
                             hipStream_t st);
// tasks (child c, parent s, ti, tj): 64 x 64 tile of Z_II(c)[a, b] = Zfront_s[rel_c[a], rel_c[b]].
hipError_t launch_selinv_push(const SelPlan& P, const int4* tasks, int count, hipStream_t st);
// diag[post[j]] = Z panel diagonal of internal column j (addressing of launch_logdet)
hipError_t launch_selinv_diag(const SelPlan& P, int ns, int64_t n, const int32_t* post, double* diag, hipStream_t st);

// ---- rank-k update / downdate of the factor: L <- factor of P (A + sign W W^T) P^T ----
// (updown.cpp).  The UPD_W columns of a chunk of W ride through the
// touched supernodes in wd (internal row r, column c at UPD_W r + c).  Per 64-column block
// (s, k0) of a touched front: [L11 W1] T = [L11' 0] by one workgroup, then [L21 W2] T for
// the front rows below on v_mfma_f64_16x16x4_f64.  T lives in the index space of UPD_K =
// 64 + UPD_W: k < nb the block's columns, [nb, 64) zero, 64 + c column c of W.
constexpr int UPD_W = 16;
constexpr int UPD_K = PNB + UPD_W;
constexpr int UPD_ROWS = 64;  // front rows per workgroup of the row kernel (16 per wave)
constexpr int32_t UPD_ARMED = 0x7f7f7f7f;  // status word before any report (as the factorization arms it)
struct UpdPlan {
    const int32_t* sn_start;
    const int32_t* sn_m;
    const int64_t* panel_off;
    const int64_t* rows_ptr;
    const int32_t* rows;    // front rows (internal numbering), first w = the pivots
    double* panel_pool;
    double* wd;             // n x UPD_W workspace
    double* tbuf;           // UPD_K x UPD_K: T(k, j) at UPD_K k + j
    int32_t* info;          // min failing natural column + 1 (downdates); a sweep's launches return once it is set
    const int32_t* post;    // internal -> natural column, or null (identity)
};
// wd[idx[e]] = val[e]
hipError_t launch_updown_scatter(double* wd, const int64_t* idx, const double* val, int64_t count, hipStream_t st);
// Block (s, k0), nb = min(64, w - k0): rotates W1 (wd rows of the block's pivots) into L11
// column by column (Givens for sign > 0, hyperbolic in mixed form for sign < 0; a zero
// entry of W1 is skipped, so an inactive column's part of T is exactly the identity), writes
// L11' (lower triangle only), zeroes those rows of wd and leaves T in tbuf.
hipError_t launch_updown_block(const UpdPlan& P, int s, int k0, int sign, hipStream_t st);
// [L21' W2'] = [L21 W2] T for the nr front rows below the block, W2 gathered from / scattered
// to wd through the front's row list; a wave loads its 16 rows whole before it stores.
hipError_t launch_updown_rows(const UpdPlan& P, int s, int k0, int nr, hipStream_t st);

// ---- Schur complement of an index set ordered last (schur.cpp) ----
// The last ns columns of P A P^T are the caller's set: L_SS, their trailing block of L, is
// gathered into a dense lower triangle D, and S_c = D D^T.
struct SchurPlan {
    const int32_t* sn_m;
    const int64_t* panel_off;
    const int64_t* rows_ptr;
    const int32_t* rows;      // front rows (internal numbering)
    const int32_t* post;      // internal -> row of P A P^T
    const double* panel_pool;
    const int2* cols;         // per Schur column q: (supernode, local column) of column n - ns + q
    int32_t n, ns;
};
constexpr int SCHUR_BT = 64;   // tile edge of the product (four waves, 16 rows each)
constexpr int SCHUR_RHS = 16;  // columns per panel of the partial solves (SOLVE_RHS)
// D(i - (n - ns), q) = L(i, n - ns + q) for the front rows r >= c of column q whose row i of
// P A P^T is >= the column; D (ld = ldd) was zero-filled by the caller.  One workgroup per
// column: Schur columns need not be contiguous in the internal numbering, nor a supernode's
// suffix.
hipError_t launch_schur_gather(const SchurPlan& P, double* D, int64_t ldd, hipStream_t st);
// S = D D^T for the lower triangle of D (ns x ns, column-major; what lies above its diagonal
// is never used), both triangles of S from one computed value.  One workgroup per 64 x 64
// tile (I >= J) of the lower triangle, K ascending over [0, min(ns, 64 (J + 1))) on
// v_mfma_f64_16x16x4_f64; no atomics.  Nothing outside the ns x ns window of S is written.
hipError_t launch_schur_llt(const double* D, int ns, int64_t ldd, double* S, int64_t lds, hipStream_t st);
// G = D Y (ns x nr, nr <= SCHUR_RHS; column c of Y at Y + c ldy), one thread per row, k ascending.
hipError_t launch_schur_mul(const double* D, int ns, int nr, const double* Y, int64_t ldy, double* G, int64_t ldg,
                            hipStream_t st);
// T = D^T X (ns x nr): one wave per row k of T, lanes over i >= k, lane sums added in lane order.
hipError_t launch_schur_mul_t(const double* D, int ns, int nr, const double* X, int64_t ldx, double* T, int64_t ldt,
                              hipStream_t st);
// X(idx[q], c) = XS(q, c) for q < ns, c < nr
hipError_t launch_schur_scatter(const int32_t* idx, int ns, int nr, const double* XS, int64_t ldxs, double* X,
                                int64_t ldx, hipStream_t st);

// ---- products with A itself and residuals (refine.cpp) ----
// The full symmetric A by rows, in A's own numbering (spmv.cpp): row i holds entries
// [rp[i], rp[i + 1]) with ascending columns ci and sp, the index of the value in the
// caller's Ax.  Rows are cut into tasks of at most SPMV_CH entries; a row of several tasks
// leaves one partial per task (slot >= 0, consecutive in chunk order) and is finished by
// the combine pass over the long-row list.
constexpr int SPMV_CH = 256;    // entries per task: a dense row must not run as one serial loop
constexpr int SPMV_TPB = 256;   // tasks per workgroup of the row pass (16 at a time, one per 16 lanes)
constexpr int SPMV_NQ = 5;      // norms per column: max |r|, max |x|, max |b|, max |r| / w, max row sum of |A|
constexpr int SPMV_PQ = 4;      // doubles per partial and column: sum, error term, w, row sum of |A|
enum SpmvMode : int32_t { SPMV_MUL = 0, SPMV_RES_FP64 = 1, SPMV_RES_DD = 2 };
struct SpmvTask {
    int64_t e0;      // first entry
    int32_t row;
    int32_t slot;    // partial slot, or -1: the task is the whole row
};
struct SpmvLong {
    int32_t row;
    int32_t slot0;   // first partial slot; the row has ceil(len / SPMV_CH) of them
};
struct SpmvPlan {
    const int64_t* rp;
    const int32_t* ci;
    const int64_t* sp;
    const SpmvTask* task;
    const SpmvLong* lrow;
    int64_t ntask;
    int32_t n, nlong;
    double* part;    // SPMV_PQ x SOLVE_RHS doubles per partial slot
    double* nrm;     // SPMV_NQ x SOLVE_RHS doubles per workgroup of the two passes
};
inline int64_t spmv_row_groups(int64_t ntask) { return (ntask + SPMV_TPB - 1) / SPMV_TPB; }
inline int64_t spmv_long_groups(int64_t nlong) { return (nlong + 15) / 16; }
// xt[SOLVE_RHS i + c] = X(i, c) for c < nrhs, else 0 (X: n x nrhs column-major, ld = ldx)
hipError_t launch_spmv_transpose(double* xt, const double* X, int64_t ldx, int64_t n, int nrhs, hipStream_t st);
// One pass over A for a panel of nrhs <= SOLVE_RHS columns, X in the 16-wide row-major form
// xt.  SPMV_MUL: R = A X (B, W, out unused).  SPMV_RES_*: R = B - A X, accumulated in fp64 or
// as a compensated dot product (Dot2) rounded once, with w = |B| + |A| |X| in plain fp64; W
// (may be null) receives w; out (may be null; SPMV_NQ x SOLVE_RHS, value q of column c at
// SOLVE_RHS q + c) the column norms, reduced as maxima in a fixed order: no atomics.  B, R
// and W are column-major; nothing outside their n x nrhs windows is read or written.
hipError_t launch_spmv_sym_panel(const SpmvPlan& P, int mode, const double* Ax, const double* xt, int nrhs,
                                 const double* B, int64_t ldb, double* R, int64_t ldr, double* W, int64_t ldw,
                                 double* out, hipStream_t st);
// out[c] = max_i |D(i, c)| for c < nrhs (part: SOLVE_RHS x REFINE_NG doubles), 0 for the rest
constexpr int REFINE_NG = 64;
hipError_t launch_refine_dnorm(const double* D, int64_t ldd, int64_t n, int nrhs, double* part, double* out,
                               hipStream_t st);
// X(i, c) += D(i, c) for the columns c whose bit is set in mask
hipError_t launch_refine_add(double* X, int64_t ldx, const double* D, int64_t ldd, int64_t n, int nrhs, uint32_t mask,
                             hipStream_t st);

// ---- vector passes of the preconditioned conjugate gradients (pcg.cpp) ----
// Panels are n x nrhs (<= SOLVE_RHS) column-major with a leading dimension; mask: bit c set =
// column c takes part, a column whose bit is clear (and every column >= nrhs) is neither read
// nor written.  The sums of a column run in one fixed tree that depends on n alone: a lane's
// PCG_ROWS / 256 rows (stride 256) by fma, the 64 lanes of a wave by halving, the four waves
// in order, one partial per workgroup of PCG_ROWS rows (part: PCG_NQ x SOLVE_RHS doubles per
// workgroup, pcg_groups(n) of them), then one workgroup adds the partials: slot s to lane group
// s % 16 in ascending order, the 16 group sums in order.  No atomics.
constexpr int PCG_ROWS = 1024;  // rows per workgroup of the dot and update passes
constexpr int PCG_NQ = 2;       // sums per column and pass
struct PcgCoef {
    double v[SOLVE_RHS];        // one coefficient per column, by value
};
inline int64_t pcg_groups(int64_t n) { return n > 0 ? (n + PCG_ROWS - 1) / PCG_ROWS : 1; }
// out[c] = sum_i U(i, c) V(i, c) and, with W, out[SOLVE_RHS + c] = sum_i U(i, c) W(i, c); the
// entries of out of a column outside the mask are set to zero (so is out's second row without W)
hipError_t launch_pcg_dot(const double* U, int64_t ldu, const double* V, int64_t ldv, const double* W, int64_t ldw,
                          int64_t n, int nrhs, uint32_t mask, double* part, double* out, hipStream_t st);
// X(i, c) = fma(alpha_c, P(i, c), X(i, c)), R(i, c) = fma(-alpha_c, Q(i, c), R(i, c)) and
// out[c] = sum_i R(i, c)^2 of the new R, on the columns of the mask (out as for the dot)
hipError_t launch_pcg_update(double* X, int64_t ldx, double* R, int64_t ldr, const double* P, int64_t ldp,
                             const double* Q, int64_t ldq, int64_t n, int nrhs, uint32_t mask, const PcgCoef& alpha,
                             double* part, double* out, hipStream_t st);
// P(i, c) = fma(beta_c, P(i, c), Z(i, c)), or Z(i, c) when first (P is then not read), on the
// columns of the mask; pt (may be null): the new P in the product's 16-wide row-major form,
// pt[SOLVE_RHS i + c], zero in the columns outside the mask
hipError_t launch_pcg_dir(double* P, int64_t ldp, const double* Z, int64_t ldz, int64_t n, int nrhs, uint32_t mask,
                          const PcgCoef& beta, bool first, double* pt, hipStream_t st);

// ---- dense algebra on tall panels for the block Lanczos eigensolver (eigs.cpp) ----
// A panel is n x b (b <= SOLVE_RHS) column-major with a leading dimension; a basis is nb panels
// vstride doubles apart.  Rows >= n and columns >= b are neither read nor written; they count as
// zeros.  A 16 x 16 matrix M sits column-major in EIGS_TILE doubles, M(a, c) at a + 16 c.  Both
// kernels run on v_mfma_f64_16x16x4_f64 and sum in an order fixed by n and nb alone.  No atomics.
constexpr int EIGS_ROWS = 1024;  // rows per workgroup of the Gram kernel
constexpr int EIGS_TILE = SOLVE_RHS * SOLVE_RHS;
inline int64_t eigs_groups(int64_t n) { return n > 0 ? (n + EIGS_ROWS - 1) / EIGS_ROWS : 1; }
// out[i] = V_i^T W for i < nb (entries with a or c >= b: zero).  Workgroup g owns the rows
// [EIGS_ROWS g, + EIGS_ROWS): it loads them of W once (consecutive lanes read consecutive rows of
// a column; through LDS into the MFMA's B operand, kept in registers), streams the same rows of
// V_0, V_1, .. past them the same way and leaves one partial tile per block in part
// (eigs_groups(n) x nb tiles: wave v sums its rows 256 q + 64 v + [0, 64), q < 4, four per MFMA
// in ascending order, then the four waves add in order).  A second pass adds the partials of a
// tile in workgroup order.  A block's result does not depend on nb or on its place in the basis.
// V may be W.
hipError_t launch_eigs_gram(const double* V, int64_t ldv, int64_t vstride, int nb, const double* W, int64_t ldw,
                            int64_t n, int b, double* part, double* out, hipStream_t st);
// Out = beta W + sum_{i < nb} V_i C_i; Out and W are n x bc, the V_i n x b and the C_i b x bc (nb
// tiles, device; entries with a >= b or c >= bc are not read).  A wave takes 16 rows per step (four steps in flight) with four MFMAs per V_i, as the
// transposed product C_i^T V_i^T: the result's rows lie on consecutive lanes.  beta == 0: W is
// not read (it may be null).  A wave reads all it needs of its rows -- of W and of every V_i --
// into registers before it writes them, and no wave touches another's rows, so Out may be W,
// any V_i, or both (the CholQR scaling W <- W inv(R) runs in place with nb = 1, V = W = Out).
hipError_t launch_eigs_update(double* Out, int64_t ldo, double beta, const double* W, int64_t ldw, const double* V,
                              int64_t ldv, int64_t vstride, int nb, const double* C, int64_t n, int b, int bc,
                              hipStream_t st);
// The library's start block: V(i, c) = 2 u - 1, u = (splitmix64(seed + (16 i + c + 1) golden) >> 11)
// 2^-53, golden = 0x9E3779B97F4A7C15 (the generator's own increment): a function of seed, i and c
hipError_t launch_eigs_start(double* V, int64_t ldv, int64_t n, int b, uint64_t seed, hipStream_t st);

// ---- gradients on A's pattern (grad.cpp) ----
// An effective entry of A: a value slot the analysis uses, row <= col in A's own numbering.
// The list is in ascending slot order, so a pass writes G in runs.
struct GradEntry {
    int32_t row, col;
    int64_t slot;
};
constexpr int GRAD_EPW = 256;    // entries per workgroup of the outer pass (16 at a time, one per 16 lanes)
constexpr int GRAD_ROWS = 1024;  // entries per workgroup of the dot pass
inline int64_t grad_dot_groups(int64_t ne) { return ne > 0 ? (ne + GRAD_ROWS - 1) / GRAD_ROWS : 1; }
// G[slot[q]] = +0.0 for q < count (the ignored slots of an output)
hipError_t launch_grad_zero_slots(double* G, const int64_t* slot, int64_t count, hipStream_t st);
// Sampled outer product of one panel of nrhs <= SOLVE_RHS columns, U and V in the 16-wide
// row-major form of launch_spmv_transpose.  Per entry (i, j, k), s = sum_c (ut[i, c] vt[j, c]
// + [i != j] ut[j, c] vt[i, c]): the products of a column by one multiply and one fma, the 16
// columns by halving (8, 4, 2, 1; columns >= nrhs count as zero and are not loaded).  first:
// G[k] = fma(alpha, s, beta G[k]), with beta == 0 G is not read; else G[k] = fma(alpha, s,
// G[k]).  Sixteen lanes per entry; nothing but the ne listed slots of G is touched.
hipError_t launch_grad_outer(const GradEntry* ent, int64_t ne, const double* ut, const double* vt, int nrhs,
                             double alpha, double beta, bool first, double* G, hipStream_t st);
// The assembly's A-entry map backwards over the Z panel of the selected inversion: for the
// entries q of internal column j (local column jl of supernode s, m front rows), G[a_src[q]] =
// c zpanel[panel_off[s] + jl m + a_pos[q]], c = 1 at the pivot row (a_pos[q] == jl), else 2.
// One thread per column; a_src is injective, so no slot has two writers.
hipError_t launch_grad_zgather(const SelPlan& P, int ns, int64_t n, const int64_t* a_ptr, const int32_t* a_pos,
                               const int64_t* a_src, double* G, hipStream_t st);
// out[0] = sum over the ne entries of G[slot] H[slot], in a fixed tree: a lane's GRAD_ROWS / 256
// entries (stride 256) by fma, the 64 lanes of a wave by halving, the four waves in order, one
// partial per workgroup (part: grad_dot_groups(ne) doubles); then one workgroup adds partial s
// on lane s % 256 in ascending order and the 256 lane sums by halving.  No atomics.
hipError_t launch_grad_dot(const GradEntry* ent, int64_t ne, const double* G, const double* H, double* part,
                           double* out, hipStream_t st);

// Small fronts (m <= maxm <= 128): one workgroup per front, factored in registers
// (4 x 4 tiles per thread); seq: one workgroup runs the fronts in order (a whole
// small tree in postorder, CBs through HBM).
hipError_t launch_front_small(const DevPlan& P, const int32_t* nodes, int count, int maxm, bool seq,
                              const double* Ax, hipStream_t st);

// Chain launches (a run of >= 2 single-front levels; each front the parent of the one
// before).  chain_init_kernel assembles every chained front's A entries and its
// children other than the chain child (all computed by earlier launches) into a
// packed image in HBM, all fronts in parallel; front_chain_kernel (one workgroup)
// then runs the chain, front i + 1's image streaming into registers while front i
// is factored and front i's CB added into front i + 1 straight from registers.
struct ChainDesc {
    int32_t s, c0, w, m;
    int32_t sp;      // the chain child (previous chained front), -1 for the first
    int32_t pad;
    int64_t panel_off, cb_off;
    int64_t init_off;  // doubles into ChainPlan::init (packed image, m (m + 1) / 2)
    int64_t relp_off;  // words into ChainPlan::relp: per tile row, the parent rows of its 4 rows
};
struct ChainPlan {
    const ChainDesc* desc;
    double* init;
    const uint32_t* relp;  // four 8-bit parent rows per word (relind < parent m <= 128)
    uint64_t* stamps;  // debug: per front 5 shader-clock stamps (thread 0; stride 8), or null
};
constexpr int CHAIN_NT = 768;        // threads of the chain workgroup (>= 528 tiles of m = 128; 3 waves per SIMD)
constexpr int CHAIN_MAXF = 256;      // chained fronts whose descriptors are staged in LDS
// Tiny trees (every front small, few of them, everything fits LDS): one workgroup
// runs the whole factorization with every front image and contribution block in
// LDS.  Host-built lists: the A stores (Ax index -> LDS), and per front and child the
// extend-add pairs (LDS CB entry -> LDS image entry), child by child.
struct TinyFront {
    int32_t s, c0, w, m;
    int32_t img, cb;  // LDS offsets (doubles) of the image (packed m x m lower) and the CB (packed)
    int32_t e0, np;   // the front's extend-add phases: ph[e0 .. e0 + np)
    int64_t panel_off;
};
struct TinyPlan {
    const TinyFront* fr;
    const int2* a;    // (Ax index, LDS image index)
    const int2* ph;   // (first pair, end pair) per phase
    const int2* pr;   // (LDS CB index, LDS image index)
    int32_t nf, na, nph, npr;
    int32_t lds;      // doubles of images + CBs
    int32_t* host_info;  // device view of the handle's pinned status word: the kernel owns the status
                         // (no reset / copy launches around it), or null
    int32_t nax = 0;     // tiny dense: A values (the range of the lane map's Ax indices)
    int32_t npan = 0;    // tiny dense: panel-pool doubles (the range of its panel offsets)
};
constexpr int TINY_MAX_FRONTS = 16;
constexpr int TINY_MAX_LDS = 12288;  // doubles of images + CBs (96 KB)
constexpr int TINY_PR_LDS = 2048;    // extend-add pairs staged in LDS with the A loads (the rest from HBM)
hipError_t launch_tiny_tree(const DevPlan& P, const TinyPlan& T, int maxm, const double* Ax, hipStream_t st);
// Tiny dense (n <= TINY_DENSE_N, one device): the whole matrix as one dense lower
// triangle in one wave, lane i holding row i in registers, four pivots per step.  The
// TinyPlan list a is reused as the lane map: a[c * 64 + r] = (Ax index of entry (r, c)
// or -1, its panel-pool offset or -1) for the kernel's padded order NP; na = NP * 64.
constexpr int TINY_DENSE_N = 64;
inline int tiny_dense_np(int n) { return n <= 16 ? 16 : n <= 32 ? 32 : n <= 48 ? 48 : 64; }
hipError_t launch_tiny_dense(const DevPlan& P, const TinyPlan& T, int n, const double* Ax, hipStream_t st);

hipError_t launch_front_chain(const DevPlan& P, const ChainPlan& C, int first, int count, int maxm,
                              const double* Ax, hipStream_t st);
// tiled: tasks are (front, (row tile << 16) | 16-column block) for the write-once
// tile kernel (fronts with m >= ASM_TILE_MIN_M), else (front, column block); lim (tiled
// only, may be null): per task the front columns [x, y) to assemble (distributed assembly)
hipError_t launch_assemble_large(const DevPlan& P, const int2* tasks, int count, const double* Ax,
                                 hipStream_t st, bool tiled, const int2* lim = nullptr);
// Large-front panel kernels (generated straight-line code, panel_gen.inc): the
// 64 x 64 diagonal POTRF (one wave per block) and the TRSM of the rows below it
// (TRSM_ROWS rows per task).  partial: every task is a partial last block (nb < 64).
hipError_t launch_potrf_diag(const DevPlan& P, const int2* tasks, int count, hipStream_t st);
// One workgroup of the panel TRSM of block k0 (columns k0 .. k0 + 64) of front s: rows
// [r0, min(r0 + TRSM_ROWS, r1)); ctr - 1 indexes the block's arrival counter (fused POTRF).
struct TrsmTask {
    int32_t s, k0, r0, r1, ctr;
};
// partial: blocks with nb < 64; else full blocks with the POTRF fused (arrive: the
// per-block arrival counters, zeroed)
// pre: 0 fused POTRF, 2 the diagonal blocks already factored by their own launch
// (trsm_split_wg)
hipError_t launch_trsm_panel(const DevPlan& P, const TrsmTask* tasks, int count, hipStream_t st, bool partial,
                             int32_t* arrive, int pre = 0);
// gt: the gather tables (CB tasks with gs >= 0 gather their children's entries)
// lean: 64 x 64 tiles with half the LDS (BK = 8; short-K launches, syrk_lean_kmax)
hipError_t launch_syrk(const GemmTask* tasks, const int2* tiles, int total_tiles, int bt, int tag, hipStream_t st,
                       int epi = 0, GatherTab gt = {}, bool lean = false, bool pf = false);
hipError_t launch_stamp(uint64_t* slot, hipStream_t st);
// the factorization's status word (d_info) to the pinned host word, d_info re-armed
hipError_t launch_status_publish(int32_t* info, int32_t* host, hipStream_t st);

hipError_t launch_hwid(uint32_t* out, int nwg, int threads, int spin, hipStream_t st);
hipError_t launch_fill_random(double* p, int64_t n, hipStream_t st);
hipError_t launch_mfma_peak(double* out, int blocks, int iters, int nacc, hipStream_t st);

// tiles of an M x N lower trapezoid with square BT tiles
inline int64_t syrk_tiles(int64_t M, int64_t N, int bt) {
    const int64_t TM = (M + bt - 1) / bt, TN = (N + bt - 1) / bt;
    return TN * TM - TN * (TN - 1) / 2;
}

// Append the lower-trapezoid tiles of `task` as {task, ti<<16 | tj}, walking
// G x G super-tiles so that consecutive tiles share row and column panels.
void append_tiles(std::vector<int2>& out, int task, int M, int N, int bt, int G = 8);
// Permute a launch's tile run so block b (XCD b % 8 under round-robin dispatch)
// takes a contiguous chunk: neighbouring tiles share one XCD's L2.
void xcd_order(int2* tiles, int64_t n);

}  // namespace sc
