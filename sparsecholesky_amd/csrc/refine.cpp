// Products with A itself, residuals with their backward errors, and iterative refinement of
// the panel solve.  The library never held A as a matrix: spmv.cpp
// turns the analysis' scatter map into a row-wise gather structure of the full symmetric
// matrix in A's own numbering, uploaded here at the first use together with its task lists
// (rows cut into chunks of SPMV_CH entries).  Values are read through the structure from
// the array the caller passes, in the order sc_factor takes them, so a refinement can run
// against other values than the ones that were factored: the factor is then a
// preconditioner and every step contracts the error by rho(I - inv(A_factored) A_values).
//
// Per panel of SOLVE_RHS columns, numeric_solve_refine runs
//     X = solve(B);  repeat { R = B - A X;  D = solve(R);  X += D on the columns still active }
// with the residual accumulated in fp64 or as a compensated dot product (Dot2: as if in
// twice the working precision, rounded once) and the stopping rules of LAPACK's xPORFS /
// xGERFSX on the increment norms, decided per column on the host from a handful of norms
// read back per step.  A column that has stopped is never touched again, and since every
// kernel and every solve treats the columns of a panel independently, a column's result does
// not depend on the columns it travels with.
#include <cmath>

#include "numeric_impl.hpp"

namespace sc {

namespace {

constexpr double UNIT = 1.1102230246251565e-16;  // 2^-53

// tasks of the row pass: every row at least one, a row longer than SPMV_CH one per chunk
// with consecutive partial slots, and the list of those rows for the combine pass
void spmv_tasks(int64_t n, const int64_t* rp, std::vector<SpmvTask>& task, std::vector<SpmvLong>& lrow,
                int64_t& nslots) {
    task.clear();
    lrow.clear();
    nslots = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = rp[i + 1] - rp[i];
        if (len <= SPMV_CH) {
            task.push_back({rp[i], (int32_t)i, -1});
            continue;
        }
        lrow.push_back({(int32_t)i, (int32_t)nslots});
        for (int64_t e = rp[i]; e < rp[i + 1]; e += SPMV_CH) task.push_back({e, (int32_t)i, (int32_t)nslots++});
    }
}

}  // namespace

int64_t single_device(Numeric& N, const char* who) {
    if (N.owner.empty() && !N.emulated && N.R.size() == 1) return SC_OK;
    N.err = std::string(who) + ": products with A and refinement run on single-device handles only";
    return SC_ERR_NOTIMPL;
}

namespace {

int64_t spmv_build(Numeric& N) {
    const Symbolic& S = *N.S;
    const int64_t n = S.n;
    std::vector<int64_t> rp((size_t)n + 1, 0);
    const int64_t nz = spmv_structure(S, rp.data(), nullptr, nullptr);
    std::vector<int32_t> ci((size_t)nz);
    std::vector<int64_t> sp((size_t)nz);
    spmv_structure(S, rp.data(), ci.data(), sp.data());
    std::vector<SpmvTask> task;
    std::vector<SpmvLong> lrow;
    int64_t nslots = 0;
    spmv_tasks(n, rp.data(), task, lrow, nslots);
    if (nslots > INT32_MAX / 2) {
        N.err = "refinement: too many row chunks";
        return SC_ERR_ARG;
    }
    int64_t* d_rp = nullptr;
    int32_t* d_ci = nullptr;
    int64_t* d_sp = nullptr;
    SpmvTask* d_task = nullptr;
    SpmvLong* d_lrow = nullptr;
    TRY(upload(N, rp, d_rp));
    TRY(upload(N, ci, d_ci));
    TRY(upload(N, sp, d_sp));
    TRY(upload(N, task, d_task));
    TRY(upload(N, lrow, d_lrow));
    SpmvPlan& P = N.SPMV;
    P.rp = d_rp;
    P.ci = d_ci;
    P.sp = d_sp;
    P.task = d_task;
    P.lrow = d_lrow;
    P.ntask = (int64_t)task.size();
    P.n = (int32_t)n;
    P.nlong = (int32_t)lrow.size();
    void* p = nullptr;
    TRY(dalloc(N, (size_t)std::max<int64_t>(nslots, 1) * SPMV_PQ * SOLVE_RHS * sizeof(double), p));
    P.part = (double*)p;
    const int64_t groups = spmv_row_groups(P.ntask) + spmv_long_groups(P.nlong);
    TRY(dalloc(N, (size_t)std::max<int64_t>(groups, 1) * SPMV_NQ * SOLVE_RHS * sizeof(double), p));
    P.nrm = (double*)p;
    const size_t panel = (size_t)std::max<int64_t>(n, 1) * SOLVE_RHS * sizeof(double);
    TRY(dalloc(N, panel, p));
    N.d_rfxt = (double*)p;
    TRY(dalloc(N, panel, p));
    N.d_rfR = (double*)p;
    TRY(dalloc(N, (size_t)(SPMV_NQ + 1 + REFINE_NG) * SOLVE_RHS * sizeof(double), p));
    N.d_rfnorm = (double*)p;
    N.spmv_ready = true;
    return SC_OK;
}

}  // namespace

int64_t spmv_ensure(Numeric& N, const char* who) {
    TRY(single_device(N, who));
    HIP_TRY(hipSetDevice(N.device));
    if (!N.spmv_ready) TRY(spmv_build(N));
    return SC_OK;
}

// the device values a call works with: the caller's, or the copy the last sc_factor made
int64_t device_values(Numeric& N, const double* Ax, bool host, DevTemp& stage, const double*& d_Ax,
                      const char* who) {
    const int64_t nnz = N.S->nnzA_in;
    if (!Ax) {
        if (nnz > 0 && (!N.d_Ax_owned || N.last_Ax != N.d_Ax_owned)) {
            N.err = std::string(who) + ": null values stand for the copy sc_factor made, but the last factorization "
                                       "of this handle was not an sc_factor";
            return SC_ERR_ARG;
        }
        d_Ax = N.d_Ax_owned;
        return SC_OK;
    }
    if (!host) {
        d_Ax = Ax;
        return SC_OK;
    }
    TRY(stage.get(N, (size_t)nnz * sizeof(double)));
    if (nnz > 0)
        HIP_TRY(hipMemcpyAsync(stage.p, Ax, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, N.stream));
    d_Ax = (const double*)stage.p;
    return SC_OK;
}

// One pass over A for a panel of nr columns: X transposed into the handle's panel, then
// Y = A X (mode SPMV_MUL) or R = B - A X; h (SPMV_NQ x SOLVE_RHS, may be null): the norms,
// on the host when the call returns.
int64_t spmv_panel(Numeric& N, int mode, const double* d_Ax, int nr, const double* X, int64_t ldx, const double* B,
                   int64_t ldb, double* R, int64_t ldr, double* h) {
    const int64_t n = N.S->n;
    hipStream_t s0 = N.stream;
    HIP_TRY(launch_spmv_transpose(N.d_rfxt, X, ldx, n, nr, s0));
    HIP_TRY(launch_spmv_sym_panel(N.SPMV, mode, d_Ax, N.d_rfxt, nr, B, ldb, R, ldr, nullptr, 0,
                                  h ? N.d_rfnorm : nullptr, s0));
    if (h) {
        HIP_TRY(hipMemcpyAsync(h, N.d_rfnorm, sizeof(double) * SPMV_NQ * SOLVE_RHS, hipMemcpyDeviceToHost, s0));
        HIP_TRY(hipStreamSynchronize(s0));
    }
    return SC_OK;
}

// the two backward errors of column c from a pass's norms (0 / 0 = 0)
void backward_errors(const double* h, int c, double& bnorm, double& bcomp) {
    const double r = h[c], x = h[SOLVE_RHS + c], b = h[2 * SOLVE_RHS + c], a = h[4 * SOLVE_RHS + c];
    const double den = a * x + b;
    bnorm = (r == 0.0 && den == 0.0) ? 0.0 : r / den;
    bcomp = h[3 * SOLVE_RHS + c];
}

namespace {

int64_t residual_device(Numeric& N, int32_t mode, int32_t nrhs, const double* d_Ax, const double* B, int64_t ldb,
                        const double* X, int64_t ldx, double* R, int64_t ldr, double* berr_norm, double* berr_comp) {
    double h[SPMV_NQ * SOLVE_RHS];
    const int kmode = mode == SC_RESIDUAL_DD ? SPMV_RES_DD : SPMV_RES_FP64;
    for (int32_t j0 = 0; j0 < nrhs; j0 += SOLVE_RHS) {
        const int nr = std::min<int32_t>(SOLVE_RHS, nrhs - j0);
        TRY(spmv_panel(N, kmode, d_Ax, nr, X + (int64_t)j0 * ldx, ldx, B + (int64_t)j0 * ldb, ldb,
                       R + (int64_t)j0 * ldr, ldr, h));
        for (int c = 0; c < nr; ++c) {
            double bn, bc;
            backward_errors(h, c, bn, bc);
            if (berr_norm) berr_norm[j0 + c] = bn;
            if (berr_comp) berr_comp[j0 + c] = bc;
        }
    }
    return SC_OK;
}

int64_t refine_device(Numeric& N, const sc_refine_options& opt, int32_t nrhs, const double* d_Ax, const double* B,
                      int64_t ldb, double* X, int64_t ldx, sc_refine_info* info) {
    const int64_t n = N.S->n;
    hipStream_t s0 = N.stream;
    const bool dd = opt.residual == SC_RESIDUAL_DD;
    const int kmode = dd ? SPMV_RES_DD : SPMV_RES_FP64;
    double* D = N.d_rfR;
    double* d_dn = N.d_rfnorm + SPMV_NQ * SOLVE_RHS;
    double* d_dpart = d_dn + SOLVE_RHS;
    double h[SPMV_NQ * SOLVE_RHS], dn[SOLVE_RHS];
    for (int32_t j0 = 0; j0 < nrhs; j0 += SOLVE_RHS) {
        const int nr = std::min<int32_t>(SOLVE_RHS, nrhs - j0);
        const double* Bp = B + (int64_t)j0 * ldb;
        double* Xp = X + (int64_t)j0 * ldx;
        // x_0: the panel solve itself, bit for bit
        TRY(numeric_solve_device_multi(N, nr, Bp, ldb, Xp, ldx));
        TRY(spmv_panel(N, kmode, d_Ax, nr, Xp, ldx, Bp, ldb, D, n, h));
        int32_t iters[SOLVE_RHS] = {0}, state[SOLVE_RHS];
        double dprev[SOLVE_RHS], dlast[SOLVE_RHS] = {0.0};
        bool active[SOLVE_RHS];
        int nactive = 0;
        for (int c = 0; c < nr; ++c) {
            dprev[c] = h[SOLVE_RHS + c];  // x_0 is the first increment, from zero
            active[c] = false;
            if (h[c] == 0.0)
                state[c] = SC_REFINE_CONVERGED;  // an exactly zero residual: nothing to improve
            else if (!dd && h[3 * SOLVE_RHS + c] <= 2.0 * UNIT)
                state[c] = SC_REFINE_CONVERGED;
            else if (opt.max_iter == 0)
                state[c] = SC_REFINE_MAXITER;
            else
                active[c] = true, ++nactive;
        }
        while (nactive > 0) {
            // D = solve(R) in place, through the panel solve and the handle's own buffers
            TRY(numeric_solve_device_multi(N, nr, D, n, D, n));
            HIP_TRY(launch_refine_dnorm(D, n, n, nr, d_dpart, d_dn, s0));
            HIP_TRY(hipMemcpyAsync(dn, d_dn, sizeof(dn), hipMemcpyDeviceToHost, s0));
            HIP_TRY(hipStreamSynchronize(s0));
            uint32_t mask = 0;
            for (int c = 0; c < nr; ++c) {
                if (!active[c]) continue;
                dlast[c] = dn[c];
                if (!(dn[c] < dprev[c])) {  // no contraction (or a NaN): the increment is not applied
                    state[c] = SC_REFINE_DIVERGED;
                    active[c] = false;
                    --nactive;
                } else {
                    mask |= 1u << c;
                    ++iters[c];
                }
            }
            if (mask == 0) break;
            HIP_TRY(launch_refine_add(Xp, ldx, D, n, n, nr, mask, s0));
            // the residual of the new X: the next step's right-hand side and, for a column
            // that stops here, the measures of what is returned (a frozen column's X has not
            // changed, so its norms come out as before, bit for bit)
            TRY(spmv_panel(N, kmode, d_Ax, nr, Xp, ldx, Bp, ldb, D, n, h));
            for (int c = 0; c < nr; ++c) {
                if (!((mask >> c) & 1u)) continue;
                const double dk = dn[c];
                int32_t st = -1;
                if (dk <= UNIT * h[SOLVE_RHS + c])
                    st = SC_REFINE_CONVERGED;
                else if (!dd && h[3 * SOLVE_RHS + c] <= 2.0 * UNIT)
                    st = SC_REFINE_CONVERGED;
                else if (dk > opt.rho_max * dprev[c])
                    st = SC_REFINE_STALLED;
                else if (iters[c] >= opt.max_iter)
                    st = SC_REFINE_MAXITER;
                if (st >= 0) {
                    state[c] = st;
                    active[c] = false;
                    --nactive;
                } else {
                    dprev[c] = dk;
                }
            }
        }
        if (info)
            for (int c = 0; c < nr; ++c) {
                sc_refine_info& I = info[j0 + c];
                I.iters = iters[c];
                I.state = state[c];
                backward_errors(h, c, I.berr_norm, I.berr_comp);
                const double xn = h[SOLVE_RHS + c];
                I.dx_ratio = (dlast[c] == 0.0 && xn == 0.0) ? 0.0 : dlast[c] / xn;
            }
    }
    return SC_OK;
}

}  // namespace

// n x nrhs host array (ld) into a packed device buffer.  Every staging copy runs on the
// handle's stream, like the kernels that read it: the stream is non-blocking, so a copy on
// the null stream would not be ordered with them.
int64_t stage_in(Numeric& N, DevTemp& t, const double* A, int64_t ld, int64_t n, int32_t nrhs, bool copy) {
    TRY(t.get(N, (size_t)n * nrhs * sizeof(double)));
    if (copy)
        HIP_TRY(hipMemcpy2DAsync(t.p, (size_t)n * sizeof(double), A, (size_t)ld * sizeof(double),
                                 (size_t)n * sizeof(double), (size_t)nrhs, hipMemcpyHostToDevice, N.stream));
    return SC_OK;
}

int64_t stage_out(Numeric& N, const DevTemp& t, double* A, int64_t ld, int64_t n, int32_t nrhs) {
    HIP_TRY(hipMemcpy2DAsync(A, (size_t)ld * sizeof(double), t.p, (size_t)n * sizeof(double),
                             (size_t)n * sizeof(double), (size_t)nrhs, hipMemcpyDeviceToHost, N.stream));
    HIP_TRY(hipStreamSynchronize(N.stream));
    return SC_OK;
}

int64_t numeric_spmv(Numeric& N, int32_t nrhs, const double* Ax, const double* X, int64_t ldx, double* Y, int64_t ldy,
                     bool host, const char* who) {
    TRY(single_device(N, who));
    const int64_t n = N.S->n;
    DevTemp ta, tx, ty;
    const double* d_Ax = nullptr;
    TRY(device_values(N, Ax, host, ta, d_Ax, who));
    if (n == 0 || nrhs == 0) return SC_OK;
    TRY(spmv_ensure(N, who));
    if (host) {
        TRY(stage_in(N, tx, X, ldx, n, nrhs, true));
        TRY(stage_in(N, ty, nullptr, 0, n, nrhs, false));
    }
    const double* dX = host ? (const double*)tx.p : X;
    double* dY = host ? (double*)ty.p : Y;
    const int64_t lx = host ? n : ldx, ly = host ? n : ldy;
    for (int32_t j0 = 0; j0 < nrhs; j0 += SOLVE_RHS) {
        const int nr = std::min<int32_t>(SOLVE_RHS, nrhs - j0);
        TRY(spmv_panel(N, SPMV_MUL, d_Ax, nr, dX + (int64_t)j0 * lx, lx, nullptr, 0, dY + (int64_t)j0 * ly, ly,
                       nullptr));
    }
    HIP_TRY(hipStreamSynchronize(N.stream));
    if (host) TRY(stage_out(N, ty, Y, ldy, n, nrhs));
    return SC_OK;
}

int64_t numeric_residual(Numeric& N, int32_t mode, int32_t nrhs, const double* Ax, const double* B, int64_t ldb,
                         const double* X, int64_t ldx, double* R, int64_t ldr, double* berr_norm, double* berr_comp,
                         bool host, const char* who) {
    TRY(single_device(N, who));
    const int64_t n = N.S->n;
    DevTemp ta, tb, tx, tr;
    const double* d_Ax = nullptr;
    TRY(device_values(N, Ax, host, ta, d_Ax, who));
    if (nrhs == 0) return SC_OK;
    if (n == 0) {
        for (int32_t c = 0; c < nrhs; ++c) {
            if (berr_norm) berr_norm[c] = 0.0;
            if (berr_comp) berr_comp[c] = 0.0;
        }
        return SC_OK;
    }
    TRY(spmv_ensure(N, who));
    if (!host) return residual_device(N, mode, nrhs, d_Ax, B, ldb, X, ldx, R, ldr, berr_norm, berr_comp);
    TRY(stage_in(N, tb, B, ldb, n, nrhs, true));
    TRY(stage_in(N, tx, X, ldx, n, nrhs, true));
    TRY(stage_in(N, tr, nullptr, 0, n, nrhs, false));
    TRY(residual_device(N, mode, nrhs, d_Ax, (const double*)tb.p, n, (const double*)tx.p, n, (double*)tr.p, n,
                        berr_norm, berr_comp));
    return stage_out(N, tr, R, ldr, n, nrhs);
}

int64_t numeric_solve_refine(Numeric& N, const sc_refine_options& opt, int32_t nrhs, const double* Ax, const double* B,
                             int64_t ldb, double* X, int64_t ldx, sc_refine_info* info, bool host, const char* who) {
    if (!N.factored) return SC_ERR_STATE;
    TRY(single_device(N, who));
    const int64_t st = numeric_status(N);
    if (st != SC_OK) return st;
    const int64_t n = N.S->n;
    DevTemp ta, tb, tx;
    const double* d_Ax = nullptr;
    TRY(device_values(N, Ax, host, ta, d_Ax, who));
    if (nrhs == 0) return SC_OK;
    if (n == 0) {
        if (info)
            for (int32_t c = 0; c < nrhs; ++c) info[c] = sc_refine_info{0, SC_REFINE_CONVERGED, 0.0, 0.0, 0.0};
        return SC_OK;
    }
    TRY(spmv_ensure(N, who));
    if (!host) return refine_device(N, opt, nrhs, d_Ax, B, ldb, X, ldx, info);
    TRY(stage_in(N, tb, B, ldb, n, nrhs, true));
    TRY(stage_in(N, tx, nullptr, 0, n, nrhs, false));
    TRY(refine_device(N, opt, nrhs, d_Ax, (const double*)tb.p, n, (double*)tx.p, n, info));
    return stage_out(N, tx, X, ldx, n, nrhs);
}

int64_t debug_spmv(int32_t mode, int32_t n, const int64_t* rp, const int32_t* ci, const int64_t* sp, int64_t nval,
                   const double* d_Ax, int32_t nrhs, const double* d_X, int64_t ldx, const double* d_B, int64_t ldb,
                   double* d_R, int64_t ldr, double* d_W, int64_t ldw, double* d_norms, std::string& err) {
    auto bad = [&](const char* what) {
        err = std::string("sc_debug_spmv: ") + what;
        return (int64_t)SC_ERR_ARG;
    };
    if (mode < SPMV_MUL || mode > SPMV_RES_DD) return bad("unknown mode");
    if (n < 0 || nrhs < 0 || nrhs > SOLVE_RHS) return bad("n < 0 or nrhs outside [0, 16]");
    if (n == 0 || nrhs == 0) return SC_OK;
    if (!rp || !d_X || !d_R || (mode != SPMV_MUL && !d_B)) return bad("null array");
    if (ldx < n || ldr < n || (mode != SPMV_MUL && ldb < n) || (d_W && ldw < n)) return bad("leading dimension below n");
    if (rp[0] != 0) return bad("rp[0] != 0");
    for (int32_t i = 0; i < n; ++i)
        if (rp[i + 1] < rp[i]) return bad("rp descends");
    const int64_t nz = rp[n];
    if (nz > 0 && (!ci || !sp || !d_Ax)) return bad("null array");
    for (int64_t e = 0; e < nz; ++e)
        if (ci[e] < 0 || ci[e] >= n || sp[e] < 0 || sp[e] >= nval) return bad("ci or sp out of range");
    std::vector<SpmvTask> task;
    std::vector<SpmvLong> lrow;
    int64_t nslots = 0;
    spmv_tasks(n, rp, task, lrow, nslots);
    const int64_t groups = spmv_row_groups((int64_t)task.size()) + spmv_long_groups((int64_t)lrow.size());
    // one device block: rp | sp | part | nrm | xt | task | lrow | ci (descending alignment)
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += (std::max<size_t>(bytes, 8) + 15) & ~(size_t)15;
        return o;
    };
    const size_t o_rp = take(sizeof(int64_t) * ((size_t)n + 1)), o_sp = take(sizeof(int64_t) * (size_t)nz);
    const size_t o_part = take(sizeof(double) * (size_t)nslots * SPMV_PQ * SOLVE_RHS);
    const size_t o_nrm = take(sizeof(double) * (size_t)groups * SPMV_NQ * SOLVE_RHS);
    const size_t o_xt = take(sizeof(double) * (size_t)n * SOLVE_RHS);
    const size_t o_task = take(sizeof(SpmvTask) * task.size()), o_lrow = take(sizeof(SpmvLong) * lrow.size());
    const size_t o_ci = take(sizeof(int32_t) * (size_t)nz);
    char* base = nullptr;
    if (hipMalloc((void**)&base, off) != hipSuccess) return SC_ERR_DEVMEM;
    int64_t rc = SC_OK;
    auto put = [&](size_t o, const void* src, size_t bytes) {
        if (rc == SC_OK && bytes > 0 && hipMemcpy(base + o, src, bytes, hipMemcpyHostToDevice) != hipSuccess)
            rc = SC_ERR_HIP;
    };
    put(o_rp, rp, sizeof(int64_t) * ((size_t)n + 1));
    put(o_sp, sp, sizeof(int64_t) * (size_t)nz);
    put(o_ci, ci, sizeof(int32_t) * (size_t)nz);
    put(o_task, task.data(), sizeof(SpmvTask) * task.size());
    put(o_lrow, lrow.data(), sizeof(SpmvLong) * lrow.size());
    if (rc == SC_OK) {
        SpmvPlan P {};
        P.rp = (const int64_t*)(base + o_rp);
        P.ci = (const int32_t*)(base + o_ci);
        P.sp = (const int64_t*)(base + o_sp);
        P.task = (const SpmvTask*)(base + o_task);
        P.lrow = (const SpmvLong*)(base + o_lrow);
        P.ntask = (int64_t)task.size();
        P.n = n;
        P.nlong = (int32_t)lrow.size();
        P.part = (double*)(base + o_part);
        P.nrm = (double*)(base + o_nrm);
        double* xt = (double*)(base + o_xt);
        if (launch_spmv_transpose(xt, d_X, ldx, n, nrhs, nullptr) != hipSuccess ||
            launch_spmv_sym_panel(P, mode, d_Ax, xt, nrhs, d_B, ldb, d_R, ldr, d_W, ldw, d_norms, nullptr) !=
                hipSuccess ||
            hipDeviceSynchronize() != hipSuccess)
            rc = SC_ERR_HIP;
    }
    (void)hipFree(base);
    return rc;
}

}  // namespace sc
