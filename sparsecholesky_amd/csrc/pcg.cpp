// Conjugate gradients on the values the caller passes, preconditioned with the factor the
// handle holds.  Where refinement (refine.cpp) contracts the error by
// rho(I - inv(A) A') per step and fails once an eigenvalue of inv(A) A' reaches 2, CG only
// needs A' positive definite: k eigenvalues of inv(A) A' away from 1 cost k + 1 steps.
//
// Per panel of SOLVE_RHS columns, every column on its own:
//     x = solve(b) (or the caller's x);  r = b - A' x;  stop if |r| <= tol |b|
//     z = solve(r);  rho = r.z;  p = z
//     repeat { q = A' p;  alpha = rho / p.q;  x += alpha p;  r -= alpha q;  stop on |r|;
//              z = solve(r);  rho' = r.z;  p = z + (rho' / rho) p }
// with 2-norms.  The solve is the panel solve, the product the gather pass of refine.cpp, the
// rest the three vector kernels of kernels.hip (dot, update, direction).  The sums come back
// to the host three times per step (p.q, r.r, r.z: alpha, the stopping rule and beta are
// decided there, per column) and go to the kernels by value with the mask of the columns
// still running.  A column that has stopped is not written again, every kernel treats the
// columns independently and sums in an order that depends on n alone, so a column's result
// depends neither on its company nor on its position, and repeats bit for bit.
#include <cmath>

#include "numeric_impl.hpp"

namespace sc {

namespace {

int64_t pcg_ensure(Numeric& N) {
    if (N.pcg_ready) return SC_OK;
    const int64_t n = N.S->n;
    const size_t panel = (size_t)std::max<int64_t>(n, 1) * SOLVE_RHS * sizeof(double);
    void* p = nullptr;
    TRY(dalloc(N, panel, p));
    N.d_pcgZ = (double*)p;
    TRY(dalloc(N, panel, p));
    N.d_pcgP = (double*)p;
    TRY(dalloc(N, panel, p));
    N.d_pcgQ = (double*)p;
    TRY(dalloc(N, (size_t)pcg_groups(n) * PCG_NQ * SOLVE_RHS * sizeof(double), p));
    N.d_pcgpart = (double*)p;
    TRY(dalloc(N, (size_t)2 * PCG_NQ * SOLVE_RHS * sizeof(double), p));
    N.d_pcgscal = (double*)p;
    N.pcg_ready = true;
    return SC_OK;
}

// |r| / |b| from the squares (0 / 0 = 0)
double relres(double rr, double bb) { return rr == 0.0 ? 0.0 : std::sqrt(rr) / std::sqrt(bb); }

// the stopping rule |r|_2 <= tol |b|_2 (false for a NaN)
bool small(double rr, double bb, double tol) { return std::sqrt(rr) <= tol * std::sqrt(bb); }

bool usable(double v) { return v > 0.0 && std::isfinite(v); }

int64_t pcg_device(Numeric& N, const sc_pcg_options& opt, int32_t nrhs, const double* d_Ax, const double* B,
                   int64_t ldb, double* X, int64_t ldx, sc_pcg_info* info) {
    const int64_t n = N.S->n;
    hipStream_t s0 = N.stream;
    double *R = N.d_rfR, *Z = N.d_pcgZ, *P = N.d_pcgP, *Q = N.d_pcgQ, *part = N.d_pcgpart, *scal = N.d_pcgscal;
    constexpr int BLK = PCG_NQ * SOLVE_RHS;  // one result of a sum pass
    double hs[2 * BLK], h[SPMV_NQ * SOLVE_RHS];
    // the sums of a pass (or of two) from the scalar block to hs
    auto fetch = [&](int blocks) -> int64_t {
        HIP_TRY(hipMemcpyAsync(hs, scal, sizeof(double) * BLK * blocks, hipMemcpyDeviceToHost, s0));
        HIP_TRY(hipStreamSynchronize(s0));
        return SC_OK;
    };
    for (int32_t j0 = 0; j0 < nrhs; j0 += SOLVE_RHS) {
        const int nr = std::min<int32_t>(SOLVE_RHS, nrhs - j0);
        const uint32_t all = nr >= 32 ? ~0u : (1u << nr) - 1u;
        const double* Bp = B + (int64_t)j0 * ldb;
        double* Xp = X + (int64_t)j0 * ldx;
        // x_0: the panel solve itself, bit for bit, or what the caller left in X
        if (!opt.use_x0) TRY(numeric_solve_device_multi(N, nr, Bp, ldb, Xp, ldx));
        TRY(spmv_panel(N, SPMV_RES_FP64, d_Ax, nr, Xp, ldx, Bp, ldb, R, n, nullptr));
        HIP_TRY(launch_pcg_dot(Bp, ldb, Bp, ldb, nullptr, 0, n, nr, all, part, scal, s0));
        HIP_TRY(launch_pcg_dot(R, n, R, n, nullptr, 0, n, nr, all, part, scal + BLK, s0));
        TRY(fetch(2));
        int32_t iters[SOLVE_RHS] = {0}, state[SOLVE_RHS];
        double bb[SOLVE_RHS], rr[SOLVE_RHS], rho[SOLVE_RHS] = {0.0};
        uint32_t mask = 0;
        for (int c = 0; c < nr; ++c) {
            bb[c] = hs[c];
            rr[c] = hs[BLK + c];
            if (small(rr[c], bb[c], opt.tol))
                state[c] = SC_PCG_CONVERGED;
            else if (opt.max_iter == 0)
                state[c] = SC_PCG_MAXITER;
            else
                mask |= 1u << c;
        }
        PcgCoef alpha {}, beta {};
        bool first = true;
        while (mask) {
            // z = solve(r) through the panel solve and the handle's own buffers; rho' = r.z
            TRY(numeric_solve_device_multi(N, nr, R, n, Z, n));
            HIP_TRY(launch_pcg_dot(R, n, Z, n, nullptr, 0, n, nr, mask, part, scal, s0));
            TRY(fetch(1));
            for (int c = 0; c < nr; ++c) {
                if (!((mask >> c) & 1u)) continue;
                const double rn = hs[c];
                if (!usable(rn)) {
                    state[c] = SC_PCG_BREAKDOWN;
                    mask &= ~(1u << c);
                    continue;
                }
                beta.v[c] = first ? 0.0 : rn / rho[c];
                rho[c] = rn;
            }
            if (!mask) break;
            // p = z + beta p, also in the product's row-major form, then q = A' p and p.q
            HIP_TRY(launch_pcg_dir(P, n, Z, n, n, nr, mask, beta, first, N.d_rfxt, s0));
            first = false;
            HIP_TRY(launch_spmv_sym_panel(N.SPMV, SPMV_MUL, d_Ax, N.d_rfxt, nr, nullptr, 0, Q, n, nullptr, 0, nullptr,
                                          s0));
            HIP_TRY(launch_pcg_dot(P, n, Q, n, nullptr, 0, n, nr, mask, part, scal, s0));
            TRY(fetch(1));
            for (int c = 0; c < nr; ++c) {
                if (!((mask >> c) & 1u)) continue;
                const double pq = hs[c];
                if (!usable(pq)) {  // A' is not positive definite along p (or a NaN): x stays
                    state[c] = SC_PCG_BREAKDOWN;
                    mask &= ~(1u << c);
                    continue;
                }
                alpha.v[c] = rho[c] / pq;
            }
            if (!mask) break;
            HIP_TRY(launch_pcg_update(Xp, ldx, R, n, P, n, Q, n, n, nr, mask, alpha, part, scal, s0));
            TRY(fetch(1));
            for (int c = 0; c < nr; ++c) {
                if (!((mask >> c) & 1u)) continue;
                rr[c] = hs[c];
                ++iters[c];
                if (small(rr[c], bb[c], opt.tol))
                    state[c] = SC_PCG_CONVERGED;
                else if (iters[c] >= opt.max_iter)
                    state[c] = SC_PCG_MAXITER;
                else
                    continue;
                mask &= ~(1u << c);
            }
        }
        // what is returned, measured: the true residual of X and its backward errors
        TRY(spmv_panel(N, SPMV_RES_FP64, d_Ax, nr, Xp, ldx, Bp, ldb, Q, n, h));
        HIP_TRY(launch_pcg_dot(Q, n, Q, n, nullptr, 0, n, nr, all, part, scal, s0));
        TRY(fetch(1));
        if (info)
            for (int c = 0; c < nr; ++c) {
                sc_pcg_info& I = info[j0 + c];
                I.iters = iters[c];
                I.state = state[c];
                I.relres = relres(rr[c], bb[c]);
                I.relres_true = relres(hs[c], bb[c]);
                backward_errors(h, c, I.berr_norm, I.berr_comp);
            }
    }
    return SC_OK;
}

}  // namespace

int64_t numeric_solve_pcg(Numeric& N, const sc_pcg_options& opt, int32_t nrhs, const double* Ax, const double* B,
                          int64_t ldb, double* X, int64_t ldx, sc_pcg_info* info, bool host, const char* who) {
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
            for (int32_t c = 0; c < nrhs; ++c) info[c] = sc_pcg_info{0, SC_PCG_CONVERGED, 0.0, 0.0, 0.0, 0.0};
        return SC_OK;
    }
    TRY(spmv_ensure(N, who));
    TRY(pcg_ensure(N));
    if (!host) return pcg_device(N, opt, nrhs, d_Ax, B, ldb, X, ldx, info);
    TRY(stage_in(N, tb, B, ldb, n, nrhs, true));
    TRY(stage_in(N, tx, X, ldx, n, nrhs, opt.use_x0 != 0));
    TRY(pcg_device(N, opt, nrhs, d_Ax, (const double*)tb.p, n, (double*)tx.p, n, info));
    return stage_out(N, tx, X, ldx, n, nrhs);
}

}  // namespace sc
