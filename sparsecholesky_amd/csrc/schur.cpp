// Schur complement of a chosen index set.  A Schur analysis
// (sc_analyze_schur) orders the caller's set S last: P A P^T = L L^T with
//     L = [ L_II  0 ; L_SI  L_SS ],
// so that, with D = L_SS (ns x ns, lower triangular, numbered as the caller's list),
//     S_c = A_SS - A_SI inv(A_II) A_IS = D D^T,
//     g   = b_S - A_SI inv(A_II) b_I  = D y_S,     y = L^-1 P b          (condense)
//     x_I from L^T (P x) = [ y_I ; D^T x_S ]  for any x_S                (expand)
// and x = A^-1 b when x_S = S_c^-1 g.  Nothing of the factorization changes: the gather
// reads the finished panels, whichever kernels produced them.
//
// D is gathered once per generation of the factor (factor_gen: a new factorization or an
// update / downdate makes it stale) into a buffer of the handle; the product kernel writes
// straight into the caller's array.  The partial solves are compositions of the panel-family
// operators (P, L^-1, L^-T, P^T through numeric_apply_device_multi, 16 columns at a time
// through the handle's n x 16 panel W) with two dense triangular products by D in between:
// W's last ns rows are y_S, in the caller's numbering, because S is ordered last in the
// given order.
#include "numeric_impl.hpp"

namespace sc {

namespace {

// status rules of the selected inversion; SC_OK: factored, positive definite, single device
int64_t schur_state(Numeric& N, const char* who) {
    if (!N.factored) return SC_ERR_STATE;
    if (!N.owner.empty() || N.emulated || N.R.size() != 1) {
        N.err = std::string(who) + ": the Schur complement runs on single-device handles only (the panels of a "
                                   "multi-rank or emulated handle are spread over the ranks' arenas)";
        return SC_ERR_NOTIMPL;
    }
    return numeric_status(N);
}

int64_t schur_build(Numeric& N) {
    const Symbolic& S = *N.S;
    const int32_t ns = S.n_schur;
    std::vector<int2> cols((size_t)ns);
    for (int32_t q = 0; q < ns; ++q) {
        const int32_t c = S.ipost[S.n - ns + q], s = S.sn_of[c];
        cols[q] = make_int2(s, c - S.sn_start[s]);
    }
    std::vector<int32_t> idx(S.perm.end() - ns, S.perm.end());
    int2* d_cols = nullptr;
    TRY(upload(N, cols, d_cols));
    TRY(upload(N, idx, N.d_schidx));
    void* p = nullptr;
    TRY(dalloc(N, (size_t)ns * ns * sizeof(double), p));
    N.d_schD = (double*)p;
    N.SCH.sn_m = N.SP.sn_m;
    N.SCH.panel_off = N.SP.panel_off;
    N.SCH.rows_ptr = N.SP.rows_ptr;
    N.SCH.rows = N.SP.rows;
    N.SCH.post = N.d_etpost;
    N.SCH.cols = d_cols;
    N.SCH.n = (int32_t)S.n;
    N.SCH.ns = ns;
    N.sch_ready = true;
    return SC_OK;
}

// D of the current generation of the factor in N.d_schD (enqueued, not synchronised)
int64_t schur_ensure(Numeric& N) {
    TRY(apply_prepare(N));  // the front row lists, the panel offsets and the postorder on the device
    if (!N.sch_ready) TRY(schur_build(N));
    if (N.sch_gen == N.factor_gen) return SC_OK;
    const int64_t ns = N.SCH.ns;
    N.SCH.panel_pool = N.gpanel;
    HIP_TRY(hipMemsetAsync(N.d_schD, 0, (size_t)ns * ns * sizeof(double), N.stream));
    HIP_TRY(launch_schur_gather(N.SCH, N.d_schD, ns, N.stream));
    N.sch_gen = N.factor_gen;
    return SC_OK;
}

int64_t schur_panel(Numeric& N) {
    if (N.d_schW) return SC_OK;
    void* p = nullptr;
    TRY(dalloc(N, (size_t)N.S->n * SCHUR_RHS * sizeof(double), p));
    N.d_schW = (double*)p;
    return SC_OK;
}

// a device buffer for the length of one host call
struct Temp {
    void* p = nullptr;
    ~Temp() {
        if (p) (void)hipFree(p);
    }
    int64_t get(Numeric& N, size_t bytes) {
        if (hipMalloc(&p, std::max<size_t>(bytes, 8)) != hipSuccess) {
            p = nullptr;
            N.err = "Schur complement: device allocation of a host call's staging failed";
            return SC_ERR_DEVMEM;
        }
        return SC_OK;
    }
};

}  // namespace

int64_t numeric_schur_factor(Numeric& N, double* D, int64_t ldd, bool host) {
    const int64_t st = schur_state(N, "sc_schur_factor");
    if (st != SC_OK) return st;
    const int64_t ns = N.S->n_schur;
    if (ns == 0) return SC_OK;
    TRY(schur_ensure(N));
    HIP_TRY(hipMemcpy2DAsync(D, (size_t)ldd * sizeof(double), N.d_schD, (size_t)ns * sizeof(double),
                             (size_t)ns * sizeof(double), (size_t)ns,
                             host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, N.stream));
    HIP_TRY(hipStreamSynchronize(N.stream));
    return SC_OK;
}

int64_t numeric_schur_matrix(Numeric& N, double* Sc, int64_t lds, bool host) {
    const int64_t st = schur_state(N, "sc_schur_matrix");
    if (st != SC_OK) return st;
    const int64_t ns = N.S->n_schur;
    if (ns == 0) return SC_OK;
    TRY(schur_ensure(N));
    if (!host) {
        HIP_TRY(launch_schur_llt(N.d_schD, (int)ns, ns, Sc, lds, N.stream));
        HIP_TRY(hipStreamSynchronize(N.stream));
        return SC_OK;
    }
    Temp t;
    TRY(t.get(N, (size_t)ns * ns * sizeof(double)));
    HIP_TRY(launch_schur_llt(N.d_schD, (int)ns, ns, (double*)t.p, ns, N.stream));
    HIP_TRY(hipMemcpy2DAsync(Sc, (size_t)lds * sizeof(double), t.p, (size_t)ns * sizeof(double),
                             (size_t)ns * sizeof(double), (size_t)ns, hipMemcpyDeviceToHost, N.stream));
    HIP_TRY(hipStreamSynchronize(N.stream));
    return SC_OK;
}

static int64_t condense_device(Numeric& N, int32_t nrhs, const double* B, int64_t ldb, double* G, int64_t ldg) {
    const int64_t n = N.S->n, ns = N.S->n_schur;
    TRY(schur_ensure(N));
    TRY(schur_panel(N));
    double* W = N.d_schW;
    for (int32_t j0 = 0; j0 < nrhs; j0 += SCHUR_RHS) {
        const int32_t nr = std::min<int32_t>(SCHUR_RHS, nrhs - j0);
        TRY(numeric_apply_device_multi(N, SC_OP_PERM, nr, B + (int64_t)j0 * ldb, ldb, W, n));
        TRY(numeric_apply_device_multi(N, SC_OP_SOLVE_L, nr, W, n, W, n));
        HIP_TRY(launch_schur_mul(N.d_schD, (int)ns, nr, W + (n - ns), n, G + (int64_t)j0 * ldg, ldg, N.stream));
    }
    HIP_TRY(hipStreamSynchronize(N.stream));
    return SC_OK;
}

int64_t numeric_schur_condense(Numeric& N, int32_t nrhs, const double* B, int64_t ldb, double* G, int64_t ldg,
                               bool host) {
    const int64_t st = schur_state(N, "sc_schur_condense");
    if (st != SC_OK) return st;
    const int64_t n = N.S->n, ns = N.S->n_schur;
    if (ns == 0 || nrhs == 0) return SC_OK;
    if (!host) return condense_device(N, nrhs, B, ldb, G, ldg);
    HIP_TRY(hipSetDevice(N.device));
    Temp tb, tg;
    TRY(tb.get(N, (size_t)n * nrhs * sizeof(double)));
    TRY(tg.get(N, (size_t)ns * nrhs * sizeof(double)));
    HIP_TRY(hipMemcpy2D(tb.p, (size_t)n * sizeof(double), B, (size_t)ldb * sizeof(double), (size_t)n * sizeof(double),
                        (size_t)nrhs, hipMemcpyHostToDevice));
    TRY(condense_device(N, nrhs, (const double*)tb.p, n, (double*)tg.p, ns));
    HIP_TRY(hipMemcpy2D(G, (size_t)ldg * sizeof(double), tg.p, (size_t)ns * sizeof(double), (size_t)ns * sizeof(double),
                        (size_t)nrhs, hipMemcpyDeviceToHost));
    return SC_OK;
}

static int64_t expand_device(Numeric& N, int32_t nrhs, const double* B, int64_t ldb, const double* XS, int64_t ldxs,
                             double* X, int64_t ldx) {
    const int64_t n = N.S->n, ns = N.S->n_schur;
    if (ns > 0) TRY(schur_ensure(N));
    TRY(schur_panel(N));
    double* W = N.d_schW;
    for (int32_t j0 = 0; j0 < nrhs; j0 += SCHUR_RHS) {
        const int32_t nr = std::min<int32_t>(SCHUR_RHS, nrhs - j0);
        const double* xs = XS + (int64_t)j0 * ldxs;
        double* x = X + (int64_t)j0 * ldx;
        TRY(numeric_apply_device_multi(N, SC_OP_PERM, nr, B + (int64_t)j0 * ldb, ldb, W, n));
        TRY(numeric_apply_device_multi(N, SC_OP_SOLVE_L, nr, W, n, W, n));
        // z = [ y_I ; D^T x_S ]
        if (ns > 0) HIP_TRY(launch_schur_mul_t(N.d_schD, (int)ns, nr, xs, ldxs, W + (n - ns), n, N.stream));
        TRY(numeric_apply_device_multi(N, SC_OP_SOLVE_LT, nr, W, n, W, n));
        TRY(numeric_apply_device_multi(N, SC_OP_PERM_T, nr, W, n, x, ldx));
        // the caller's x_S itself, not what the backward sweep reproduces of it
        if (ns > 0) HIP_TRY(launch_schur_scatter(N.d_schidx, (int)ns, nr, xs, ldxs, x, ldx, N.stream));
    }
    HIP_TRY(hipStreamSynchronize(N.stream));
    return SC_OK;
}

int64_t numeric_schur_expand(Numeric& N, int32_t nrhs, const double* B, int64_t ldb, const double* XS, int64_t ldxs,
                             double* X, int64_t ldx, bool host) {
    const int64_t st = schur_state(N, "sc_schur_expand");
    if (st != SC_OK) return st;
    const int64_t n = N.S->n, ns = N.S->n_schur;
    if (n == 0 || nrhs == 0) return SC_OK;
    if (!host) return expand_device(N, nrhs, B, ldb, XS, ldxs, X, ldx);
    HIP_TRY(hipSetDevice(N.device));
    Temp tb, ts;
    TRY(tb.get(N, (size_t)n * nrhs * sizeof(double)));
    TRY(ts.get(N, (size_t)ns * nrhs * sizeof(double)));
    HIP_TRY(hipMemcpy2D(tb.p, (size_t)n * sizeof(double), B, (size_t)ldb * sizeof(double), (size_t)n * sizeof(double),
                        (size_t)nrhs, hipMemcpyHostToDevice));
    if (ns > 0)
        HIP_TRY(hipMemcpy2D(ts.p, (size_t)ns * sizeof(double), XS, (size_t)ldxs * sizeof(double),
                            (size_t)ns * sizeof(double), (size_t)nrhs, hipMemcpyHostToDevice));
    TRY(expand_device(N, nrhs, (const double*)tb.p, n, (const double*)ts.p, ns, (double*)tb.p, n));
    HIP_TRY(hipMemcpy2D(X, (size_t)ldx * sizeof(double), tb.p, (size_t)n * sizeof(double), (size_t)n * sizeof(double),
                        (size_t)nrhs, hipMemcpyDeviceToHost));
    return SC_OK;
}

int64_t debug_schur_llt(const double* dD, int32_t ns, int64_t ldd, double* dS, int64_t lds) {
    if (launch_schur_llt(dD, ns, ldd, dS, lds, nullptr) != hipSuccess) return SC_ERR_HIP;
    return hipDeviceSynchronize() == hipSuccess ? SC_OK : SC_ERR_HIP;
}

}  // namespace sc
