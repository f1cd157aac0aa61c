// The sc_normal handle (normal_ops.cpp).
#pragma once

#include "../../include/sparsecholesky.h"
#include "normal.hpp"
#include "numeric_impl.hpp"

namespace sc {

struct Normal {
    NormalStruct H;
    int device = -1;            // as given to sc_normal_create; resolved at the first device call
    bool dev_ready = false;     // stream created; allocs may hold memory
    bool plans_ready = false;   // every plan and buffer below is in place
    hipStream_t stream = nullptr;
    std::vector<void*> allocs;
    int64_t dev_bytes = 0;
    NormalFormPlan F {};
    NormalProdPlan PC {};       // J by columns: the transposed product
    NormalProdPlan PR {};       // J by rows: the product and the residual
    double* Sbuf = nullptr;     // S's values of the last sc_normal_factor_* (values_valid: one has filled it)
    bool values_valid = false;
    const Numeric* last_num = nullptr;  // the handle that call factored, and its factor_gen afterwards:
    int64_t last_gen = -1;              // what sc_normal_lstsq_* accepts
    double* xt = nullptr;       // max(m, n) x NORMAL_RHS: the right-hand panel in row-major form
    // least squares: the base of the last sc_normal_factor_* (C's values, then d + lambda per
    // row; base_active: any of them was given) and, allocated at the first sc_normal_lstsq_*,
    // its row structure, the gradient and residual panels (ld n, ld m), X in row-major form
    // and the norm scratch
    bool base_active = false;
    double* bval = nullptr;
    bool lsq_ready = false;
    NormalProdPlan PB {};
    double* G = nullptr;
    double* R = nullptr;
    double* xtn = nullptr;
    double* Gl = nullptr;       // the low halves of the compensated mode: gradient, residual,
    double* Rl = nullptr;       // and the residual's in row-major form
    double* xtl = nullptr;
    double* nrm = nullptr;      // 4 x NORMAL_RHS results, then the partials
    std::string err;
};

int64_t normal_create(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const int64_t* Cp, const int32_t* Ci,
                      int device, Normal*& out, std::string& err);
void normal_free(Normal* N);
// out[0 .. 4): host bytes of the structure, device bytes held, terms, entries of S; returns 4
int64_t normal_memory(const Normal& N, int64_t* out, int32_t cap);
// the device side, built at the first call that needs it (want_device: used when the handle
// was created with device < 0; < 0: the current device)
int64_t normal_ensure(Normal& N, int want_device);
// Sx (entries of S, device or host by `host`) = the values of S; w, Cx, d may be null
int64_t normal_values(Normal& N, const double* Jx, const double* w, const double* Cx, const double* d, double lambda,
                      double* Sx, bool host, const char* who);
// forms into the handle's buffer and factors it with num; returns the factorization's status
int64_t normal_factor(Normal& N, Numeric& num, const double* Jx, const double* w, const double* Cx, const double* d,
                      double lambda, bool host, const char* who);
// transposed: Y (n x nrhs) = J^T diag(w) X, X m x nrhs; else Y (m x nrhs) = J X, X n x nrhs (w unused)
int64_t normal_product(Normal& N, bool transposed, int32_t nrhs, const double* Jx, const double* w, const double* X,
                       int64_t ldx, double* Y, int64_t ldy, bool host, const char* who);

// min ||W^1/2 (J x - b)||^2 + x^T (C + diag d + lambda I) x with the factor num holds (made by
// normal_factor on this handle, whose base it remembers): x_0 = inv(S) J^T W b, then corrected
// semi-normal steps under the stopping rules of numeric_solve_refine.  opt: validated by the caller.
int64_t normal_lstsq(Normal& N, Numeric& num, const sc_refine_options& opt, int32_t nrhs, const double* Jx,
                     const double* w, const double* B, int64_t ldb, double* X, int64_t ldx, sc_lstsq_info* info,
                     bool host, const char* who);

// the kernels alone (include/sparsecholesky_debug.h has the contracts)
int64_t debug_normal_form(int64_t ne, const int64_t* tp, const int32_t* ta, const int32_t* tb, const int32_t* tr,
                          const int64_t* cpos, const int32_t* dcol, int64_t nJ, int64_t nw, int64_t nC, int64_t nd,
                          const double* d_Jx, const double* d_w, const double* d_Cx, const double* d_d, double lambda,
                          double* d_Sx, std::string& err);
int64_t debug_normal_prod(bool transposed, int32_t mode, int64_t nvec, int64_t nin, const int64_t* ptr,
                          const int32_t* idx, const int64_t* pos, int64_t nval, const double* d_val, const double* d_w,
                          int32_t nrhs, const double* d_X, int64_t ldx, const double* d_B, int64_t ldb, double* d_R,
                          int64_t ldr, std::string& err);
int64_t debug_normal_pair(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const int64_t* rp,
                          const int32_t* ci, const int64_t* sp, const double* d_Jx, const double* d_w, int32_t nrhs,
                          const double* d_X, int64_t ldx, const double* d_B, int64_t ldb, double* d_R, double* d_Rl,
                          int64_t ldr, double* d_G, double* d_Gl, int64_t ldg, std::string& err);

}  // namespace sc
