// Weighted normal equations S = C + J^T diag(w) J + diag(d) + lambda I (DESIGN.md section
// 9.9): the host structure (normal.cpp, no HIP), the device plans and the launchers of the
// three kernels (normal_kernels.hip), and the handle's operations (normal_ops.cpp).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace sc {

// ---- the mappings of the form kernel; the tests read these through sc_normal_constants ----
constexpr int NORMAL_SHORT = 8;    // lists of at most this many terms: one lane per entry
constexpr int NORMAL_LANES = 16;   // lanes that share a longer list (or one chunk of it)
constexpr int NORMAL_CH = 256;     // terms per chunk: a list above it leaves one partial per chunk
constexpr int NORMAL_PCH = 256;    // entries per task of the two products (a column / row above it is chunked)
constexpr int NORMAL_RHS = 16;     // columns per panel of the products (= SOLVE_RHS)
constexpr int NORMAL_NG = 64;      // workgroups per column of the weighted residual norm

// Host structure of one J (m x n, CSC) and an optional upper-triangular base pattern C.
//   Sp / Si      the pattern of S: upper triangle, CSC, rows ascending; every diagonal entry,
//                every (i, j), i < j, whose J columns share a row, every entry of C
//   tp, ta/tb/tr entry e's terms are [tp[e], tp[e + 1]): ta = position of J[r, i], tb = position
//                of J[r, j] in J's value array, tr = r; rows ascend within a list
//   cpos         per entry: the position of its value in C's array, or -1
//   dcol         per entry: its column when it is a diagonal entry, else -1
//   rp / ci / sp J by rows: row r holds [rp[r], rp[r + 1]) with ascending columns ci and sp,
//                the position of the value in J's array
// 12 bytes per term (three int32), 8 + 8 + 4 per entry of S, 12 per entry of J by rows.
struct NormalStruct {
    int64_t m = 0, n = 0, nnzJ = 0, nnzC = 0, T = 0;
    bool has_base = false;
    std::vector<int64_t> Jp;
    std::vector<int32_t> Ji;
    std::vector<int64_t> Cp;
    std::vector<int32_t> Ci;
    std::vector<int64_t> Sp;
    std::vector<int32_t> Si;
    std::vector<int64_t> tp;
    std::vector<int32_t> ta, tb, tr;
    std::vector<int64_t> cpos;
    std::vector<int32_t> dcol;
    std::vector<int64_t> rp;
    std::vector<int32_t> ci;
    std::vector<int64_t> sp;
};
// Validates (err = who + ": " + reason, SC_ERR_ARG) and builds; Cp == nullptr: no base.
int64_t normal_build(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const int64_t* Cp, const int32_t* Ci,
                     NormalStruct& out, std::string& err);

// The base C + diag(d) + lambda I of the least-squares gradient by rows: the full symmetric C
// (pos: the position in C's value array) and one diagonal entry per row at position nnzC + row
// (the slot of d_row + lambda behind C's values); columns ascend within a row.
void normal_base_rows(const NormalStruct& H, std::vector<int64_t>& rp, std::vector<int32_t>& ci,
                      std::vector<int64_t>& pos);

// ---- device plans ----
struct NormalFormTask {  // a list longer than NORMAL_SHORT, or one chunk of a list longer than NORMAL_CH
    int64_t t0;          // first term
    int32_t e;           // entry of S
    int32_t cnt;         // terms of this task
    int32_t slot;        // partial slot, or -1: the task is the whole list
    int32_t pad;
};
struct NormalFormLong {
    int32_t e;
    int32_t slot0;       // first partial slot
    int32_t nch;         // chunks
    int32_t pad;
};
struct NormalFormPlan {
    const int64_t* tp;
    const int32_t* ta;
    const int32_t* tb;
    const int32_t* tr;
    const int64_t* cpos;
    const int32_t* dcol;
    const NormalFormTask* task;
    const NormalFormLong* lng;
    int64_t ne, ntask, nlong;
    double* part;        // one double per partial slot
};
void normal_form_tasks(int64_t ne, const int64_t* tp, std::vector<NormalFormTask>& task,
                       std::vector<NormalFormLong>& lng, int64_t& nslots);

// A gather structure cut into tasks: vector v (a column of J for the transposed product, a
// row for the product) holds entries [ptr[v], ptr[v + 1]); idx is the row of the right-hand
// panel an entry multiplies, pos the position of its value (null: the entry's own index).
struct NormalProdTask {
    int64_t e0;
    int32_t v;
    int32_t slot;        // partial slot, or -1: the task is the whole vector
};
struct NormalProdLong {
    int32_t v;
    int32_t slot0;       // ceil(len / NORMAL_PCH) consecutive slots
};
struct NormalProdPlan {
    const int64_t* ptr;
    const int32_t* idx;
    const int64_t* pos;
    const NormalProdTask* task;
    const NormalProdLong* lng;
    int64_t ntask;
    int32_t nvec, nlong;
    double* part;        // 2 x NORMAL_RHS doubles per slot: sums, error terms
};
void normal_prod_tasks(int64_t nvec, const int64_t* ptr, std::vector<NormalProdTask>& task,
                       std::vector<NormalProdLong>& lng, int64_t& nslots);

enum NormalMode : int32_t { NORMAL_MUL = 0, NORMAL_RES_FP64 = 1, NORMAL_RES_DD = 2, NORMAL_MULT_DD = 3 };

}  // namespace sc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace sc {
// S_e = (c_e + [i = j] (d_i + lambda)) + sum_t (Jx[ta_t] w[tr_t]) Jx[tb_t] for every entry of
// S, written to Sx[e]; w, Cx, d may be null (ones, zeros, zeros).  Summation order: a list of
// at most NORMAL_SHORT terms is added to the base term by term in list order; a longer one
// is summed by NORMAL_LANES lanes (lane l takes the terms l, l + 16, .. of the task in
// order, from zero; the lane sums are added by halving: 8, 4, 2, 1) and the base is added
// last; a list above NORMAL_CH terms runs as chunks of NORMAL_CH, each as such a task, whose
// partials are added in chunk order, then the base.  Every product is rounded twice: a w,
// then the fma with b.  No atomics.
hipError_t launch_normal_form(const NormalFormPlan& P, const double* Jx, const double* w, const double* Cx,
                              const double* d, double lambda, double* Sx, hipStream_t st);
// G = J^T diag(w) Y for a panel of nrhs <= NORMAL_RHS columns: P is J by columns (pos null),
// yt the m x 16 row-major form of Y (launch_spmv_transpose), G n x nrhs column-major.  Per
// (column j, right-hand side c): s = fma(Jx[p] w[Ji[p]], yt[Ji[p], c], s) down the column;
// columns above NORMAL_PCH entries in chunks whose partials are added in chunk order.
hipError_t launch_normal_mult(const NormalProdPlan& P, const double* Jx, const double* w, const double* yt, int nrhs,
                              double* G, int64_t ldg, hipStream_t st);
// The same as if in twice the working precision, for the least-squares gradient: Y is the pair
// (yt, ytl) in row-major form, every product J w and (J w) y is split exactly, the sum kept
// with an error term, and the result left as the pair (G, Gl), G + Gl with |Gl| <= ulp(G) / 2.
hipError_t launch_normal_mult_dd(const NormalProdPlan& P, const double* Jx, const double* w, const double* yt,
                                 const double* ytl, int nrhs, double* G, double* Gl, int64_t ldg, hipStream_t st);
// NORMAL_MUL: R = J X; NORMAL_RES_*: R = B - J X in fp64 (one fma per entry) or as a
// compensated dot product (Dot2) rounded once.  P is a row structure, xt the 16-wide
// row-major form of X; B and R column-major, R may be B.  NORMAL_RES_DD only: Ein (may be
// null; ldb) is an error term B comes with, and with Eout (may be null; ldr; may be Ein) the
// result is not rounded but left as the pair (R, Eout).
hipError_t launch_normal_mul(const NormalProdPlan& P, int mode, const double* val, const double* xt, int nrhs,
                             const double* B, int64_t ldb, const double* Ein, double* R, int64_t ldr, double* Eout,
                             hipStream_t st);
// out[i] = d_i + lambda for i < n (d may be null): the diagonal part of the least-squares base
hipError_t launch_normal_shift(double* out, const double* d, double lambda, int64_t n, hipStream_t st);
// out[c] = sum_i w_i R(i, c)^2 for c < nrhs (w may be null), 0 for the rest, in a fixed tree
// that depends on m alone (part: NORMAL_NG x NORMAL_RHS doubles)
hipError_t launch_normal_wnorm(const double* R, int64_t ldr, const double* w, int64_t m, int nrhs, double* part,
                               double* out, hipStream_t st);
}  // namespace sc
#endif
