// The eigenpairs of the factored matrix F nearest zero by block shift-invert Lanczos (DESIGN.md
// section 9.7; include/sparsecholesky.h has the algorithm step by step).  The operator is
// inv(F), applied to a block of b = min(16, n) vectors by the panel solve; everything between
// two solves is dense algebra on tall n x b panels, done by the Gram and block-update kernels
// of kernels.hip, and small dense algebra on the host: the projected matrix T (m x m, m = b
// times the blocks so far), its eigendecomposition, the 16 x 16 Cholesky factors of CholQR.
// The loop is driven from the host like pcg.cpp's; a step reads a few 16 x 16 tiles back.
// Every sum has an order fixed by n and the block count, so results repeat bit for bit.
#include <cmath>
#include <limits>

#include "numeric_impl.hpp"

namespace sc {

// ---- host dense algebra ----

// Householder reduction to tridiagonal form, then implicit QL with the transformations
// accumulated (the classical EISPACK pair tred2 / tql2).  a: m x m row-major, symmetric (the
// lower triangle is read); on return column k of a is the unit eigenvector of d[k], d
// ascending.  false: QL did not converge within 60 sweeps for some eigenvalue.
bool eigs_sym_eig(int m, double* a, double* d) {
    if (m <= 0) return true;
    std::vector<double> ev((size_t)m, 0.0);
    double* e = ev.data();
    auto A = [&](int i, int j) -> double& { return a[(size_t)i * m + j]; };
    for (int i = m - 1; i > 0; --i) {
        const int l = i - 1;
        double h = 0.0, scale = 0.0;
        if (l > 0) {
            for (int k = 0; k <= l; ++k) scale += std::fabs(A(i, k));
            if (scale == 0.0)
                e[i] = A(i, l);
            else {
                for (int k = 0; k <= l; ++k) {
                    A(i, k) /= scale;
                    h += A(i, k) * A(i, k);
                }
                double f = A(i, l);
                double g = f >= 0.0 ? -std::sqrt(h) : std::sqrt(h);
                e[i] = scale * g;
                h -= f * g;
                A(i, l) = f - g;
                f = 0.0;
                for (int j = 0; j <= l; ++j) {
                    A(j, i) = A(i, j) / h;
                    g = 0.0;
                    for (int k = 0; k <= j; ++k) g += A(j, k) * A(i, k);
                    for (int k = j + 1; k <= l; ++k) g += A(k, j) * A(i, k);
                    e[j] = g / h;
                    f += e[j] * A(i, j);
                }
                const double hh = f / (h + h);
                for (int j = 0; j <= l; ++j) {
                    f = A(i, j);
                    e[j] = g = e[j] - hh * f;
                    for (int k = 0; k <= j; ++k) A(j, k) -= f * e[k] + g * A(i, k);
                }
            }
        } else
            e[i] = A(i, l);
        d[i] = h;
    }
    d[0] = 0.0;
    e[0] = 0.0;
    for (int i = 0; i < m; ++i) {
        if (d[i] != 0.0)
            for (int j = 0; j < i; ++j) {
                double g = 0.0;
                for (int k = 0; k < i; ++k) g += A(i, k) * A(k, j);
                for (int k = 0; k < i; ++k) A(k, j) -= g * A(k, i);
            }
        d[i] = A(i, i);
        A(i, i) = 1.0;
        for (int j = 0; j < i; ++j) A(j, i) = A(i, j) = 0.0;
    }
    // implicit QL on (d, e), the rotations applied to the columns of a
    for (int i = 1; i < m; ++i) e[i - 1] = e[i];
    e[m - 1] = 0.0;
    const double eps = std::numeric_limits<double>::epsilon();
    for (int l = 0; l < m; ++l) {
        int iter = 0, mm;
        do {
            for (mm = l; mm < m - 1; ++mm)
                if (std::fabs(e[mm]) <= eps * (std::fabs(d[mm]) + std::fabs(d[mm + 1]))) break;
            if (mm == l) break;
            if (iter++ == 60) return false;
            double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
            double r = std::hypot(g, 1.0);
            g = d[mm] - d[l] + e[l] / (g + std::copysign(r, g));
            double s = 1.0, c = 1.0, p = 0.0;
            int i;
            for (i = mm - 1; i >= l; --i) {
                double f = s * e[i];
                const double bb = c * e[i];
                e[i + 1] = r = std::hypot(f, g);
                if (r == 0.0) {
                    d[i + 1] -= p;
                    e[mm] = 0.0;
                    break;
                }
                s = f / r;
                c = g / r;
                g = d[i + 1] - p;
                r = (d[i] - g) * s + 2.0 * c * bb;
                p = s * r;
                d[i + 1] = g + p;
                g = c * r - bb;
                for (int k = 0; k < m; ++k) {
                    f = A(k, i + 1);
                    A(k, i + 1) = s * A(k, i) + c * f;
                    A(k, i) = c * A(k, i) - s * f;
                }
            }
            if (r == 0.0 && i >= l) continue;
            d[l] -= p;
            e[l] = g;
            e[mm] = 0.0;
        } while (mm != l);
    }
    // ascending, by selection (columns swapped with their values)
    for (int i = 0; i < m - 1; ++i) {
        int k = i;
        for (int j = i + 1; j < m; ++j)
            if (d[j] < d[k]) k = j;
        if (k == i) continue;
        std::swap(d[i], d[k]);
        for (int r = 0; r < m; ++r) std::swap(A(r, i), A(r, k));
    }
    return true;
}

// G = R^T R of the leading b x b part of a 16 x 16 tile (column-major, G(a, c) at a + 16 c; the
// upper triangle is read) and Rinv = inv(R), upper triangular, as a tile (rinv may be null).  A
// pivot <= thr (G is expected with a unit diagonal) or not finite marks its column dependent:
// it is dropped -- row and column of R left out, the column of Rinv zero.  Returns the number
// of dropped columns.
int eigs_chol_inv(const double* G, int b, double thr, double* rinv) {
    double R[SOLVE_RHS][SOLVE_RHS] = {};
    bool drop[SOLVE_RHS] = {};
    int ndrop = 0;
    for (int k = 0; k < b; ++k) {
        double piv = G[k + 16 * k];
        for (int p = 0; p < k; ++p) piv -= R[p][k] * R[p][k];
        if (!(piv > thr) || !std::isfinite(piv)) {
            drop[k] = true;
            ++ndrop;
            continue;
        }
        R[k][k] = std::sqrt(piv);
        for (int c = k + 1; c < b; ++c) {
            double v = G[k + 16 * c];
            for (int p = 0; p < k; ++p) v -= R[p][k] * R[p][c];
            R[k][c] = v / R[k][k];
        }
    }
    if (!rinv) return ndrop;
    std::fill(rinv, rinv + EIGS_TILE, 0.0);
    for (int c = 0; c < b; ++c) {
        if (drop[c]) continue;
        rinv[c + 16 * c] = 1.0 / R[c][c];
        for (int a = c - 1; a >= 0; --a) {
            if (drop[a]) continue;
            double v = 0.0;
            for (int p = a + 1; p <= c; ++p) v += R[a][p] * rinv[p + 16 * c];
            rinv[a + 16 * c] = -v / R[a][a];
        }
    }
    return ndrop;
}

namespace {

constexpr double UNIT = 1.1102230246251565e-16;  // 2^-53

void dfree(Numeric& N, double*& p, size_t bytes) {
    if (!p) return;
    auto it = std::find(N.allocs.begin(), N.allocs.end(), (void*)p);
    if (it != N.allocs.end()) N.allocs.erase(it);
    (void)hipFree(p);
    N.dev_bytes -= (int64_t)std::max<size_t>(bytes, 8);
    p = nullptr;
}

size_t panel_bytes(int64_t n) { return (size_t)std::max<int64_t>(n, 1) * SOLVE_RHS * sizeof(double); }
size_t part_bytes(int64_t n, int mb) { return (size_t)eigs_groups(n) * mb * EIGS_TILE * sizeof(double); }
size_t coef_bytes(int mb) { return (size_t)2 * mb * EIGS_TILE * sizeof(double); }

// the buffers of the handle for a basis of mb blocks: kept, and replaced by larger ones when a
// later call asks for more blocks
int64_t eigs_ensure(Numeric& N, int mb) {
    const int64_t n = N.S->n;
    void* p = nullptr;
    if (!N.d_egY) {
        TRY(dalloc(N, panel_bytes(n), p));
        N.d_egY = (double*)p;
    }
    if (N.eigs_blocks >= mb) return SC_OK;
    const int old = N.eigs_blocks;
    N.eigs_blocks = 0;
    dfree(N, N.d_egV, (size_t)(old + 1) * panel_bytes(n));
    dfree(N, N.d_egpart, part_bytes(n, old));
    dfree(N, N.d_egC, coef_bytes(old));
    TRY(dalloc(N, (size_t)(mb + 1) * panel_bytes(n), p));
    N.d_egV = (double*)p;
    TRY(dalloc(N, part_bytes(n, mb), p));
    N.d_egpart = (double*)p;
    TRY(dalloc(N, coef_bytes(mb), p));
    N.d_egC = (double*)p;
    N.eigs_blocks = mb;
    return SC_OK;
}

int64_t eigs_device(Numeric& N, const sc_eigs_options& opt, int32_t nev, const double* d_Ax, const double* X0,
                    int64_t ldx0, double* lambda, double* X, int64_t ldx, sc_eigs_info* info) {
    const int64_t n = N.S->n;
    const int b = (int)std::min<int64_t>(SOLVE_RHS, n), mb = opt.max_blocks;
    hipStream_t s0 = N.stream;
    const int64_t vstride = (int64_t)SOLVE_RHS * n;
    double* const Vb = N.d_egV;
    double* const dC = N.d_egC;                             // coefficient tiles of an update
    double* const dG = N.d_egC + (size_t)mb * EIGS_TILE;    // results of a Gram launch
    auto V = [&](int i) { return Vb + (int64_t)i * vstride; };
    std::vector<double> hG((size_t)mb * EIGS_TILE), hC((size_t)mb * EIGS_TILE), H((size_t)mb * EIGS_TILE);
    // out (nb tiles, host) = V_i^T W, i < nb
    auto gram = [&](const double* Vp, int nb, const double* Wp, double* out) -> int64_t {
        HIP_TRY(launch_eigs_gram(Vp, n, vstride, nb, Wp, n, n, b, N.d_egpart, dG, s0));
        HIP_TRY(hipMemcpyAsync(out, dG, sizeof(double) * EIGS_TILE * nb, hipMemcpyDeviceToHost, s0));
        HIP_TRY(hipStreamSynchronize(s0));
        return SC_OK;
    };
    // Out = beta W + sum V_i C_i with the nb tiles at C (host)
    auto update = [&](double* Out, int64_t ldo, int bc, double beta, const double* Wp, int64_t ldw, const double* Vp,
                      int64_t ldv, int nb, int bv, const double* C) -> int64_t {
        HIP_TRY(hipMemcpyAsync(dC, C, sizeof(double) * EIGS_TILE * nb, hipMemcpyHostToDevice, s0));
        HIP_TRY(launch_eigs_update(Out, ldo, beta, Wp, ldw, Vp, ldv, vstride, nb, dC, n, bv, bc, s0));
        HIP_TRY(hipStreamSynchronize(s0));  // C (host) is free again
        return SC_OK;
    };
    const double thr = 2.0 * (double)(n + 16) * UNIT;
    // CholQR twice, in place; a dependent column becomes a zero column
    auto orth = [&](double* Wp) -> int64_t {
        double* g = hG.data();
        double* c = hC.data();
        for (int pass = 0; pass < 2; ++pass) {
            TRY(gram(Wp, 1, Wp, g));
            std::fill(c, c + EIGS_TILE, 0.0);
            for (int k = 0; k < b; ++k) {
                const double v = g[k + 16 * k];
                c[k + 16 * k] = (v > 0.0 && std::isfinite(v)) ? 1.0 / std::sqrt(v) : 0.0;
            }
            TRY(update(Wp, n, b, 0.0, nullptr, 0, Wp, n, 1, b, c));
            TRY(gram(Wp, 1, Wp, g));
            eigs_chol_inv(g, b, thr, c);
            TRY(update(Wp, n, b, 0.0, nullptr, 0, Wp, n, 1, b, c));
        }
        return SC_OK;
    };

    if (opt.use_x0)
        HIP_TRY(hipMemcpy2DAsync(V(0), sizeof(double) * n, X0, sizeof(double) * ldx0, sizeof(double) * n, b,
                                 hipMemcpyDeviceToDevice, s0));
    else
        HIP_TRY(launch_eigs_start(V(0), n, n, b, opt.seed, s0));
    TRY(orth(V(0)));

    const int mcap = b * mb;
    std::vector<double> T((size_t)mcap * mcap, 0.0), S, theta((size_t)mcap), est((size_t)nev, INFINITY);
    int j = 0, m = 0, kw = 0;
    bool capped = false;
    for (;; ++j) {
        double* W = V(j + 1);
        TRY(numeric_solve_device_multi(N, b, V(j), n, W, n));
        const int nbj = j + 1;
        std::fill(H.begin(), H.begin() + (size_t)nbj * EIGS_TILE, 0.0);
        for (int pass = 0; pass < 2; ++pass) {
            TRY(gram(Vb, nbj, W, hG.data()));
            for (size_t e = 0; e < (size_t)nbj * EIGS_TILE; ++e) {
                H[e] += hG[e];
                hC[e] = -hG[e];
            }
            TRY(update(W, n, b, 1.0, W, n, Vb, n, nbj, b, hC.data()));
        }
        // column block j of T and its mirror; the diagonal block as the mean of H and H^T
        for (int i = 0; i <= j; ++i)
            for (int a = 0; a < b; ++a)
                for (int c = 0; c < b; ++c) {
                    double v = H[(size_t)i * EIGS_TILE + a + 16 * c];
                    if (i == j) v = 0.5 * (v + H[(size_t)i * EIGS_TILE + c + 16 * a]);
                    T[(size_t)(b * i + a) * mcap + (b * j + c)] = v;
                    T[(size_t)(b * j + c) * mcap + (b * i + a)] = v;
                }
        m = b * nbj;
        TRY(gram(W, 1, W, hG.data()));
        S.assign((size_t)m * m, 0.0);
        for (int r = 0; r < m; ++r) std::copy(&T[(size_t)r * mcap], &T[(size_t)r * mcap] + m, &S[(size_t)r * m]);
        if (!eigs_sym_eig(m, S.data(), theta.data())) {
            N.err = "eigs: the QL iteration on the projected matrix did not converge (values or a start block "
                    "that are not finite?)";
            return SC_ERR_ARG;
        }
        kw = std::min<int>(nev, m);
        bool conv = kw == nev;
        for (int i = 0; i < kw; ++i) {
            const int col = m - 1 - i;
            double q = 0.0;
            for (int a = 0; a < b; ++a) {
                double t = 0.0;
                for (int c = 0; c < b; ++c) t += hG[a + 16 * c] * S[(size_t)(m - b + c) * m + col];
                q += S[(size_t)(m - b + a) * m + col] * t;
            }
            est[i] = std::sqrt(std::max(q, 0.0));
            if (!(est[i] <= opt.tol * theta[col])) conv = false;
        }
        if (conv) break;
        if (nbj == mb) {
            capped = true;
            break;
        }
        if ((int64_t)m + b > n) break;
        // W rank-deficient: a dependent column in the Cholesky of its Gram matrix scaled to a unit diagonal
        double sg[EIGS_TILE];
        bool deficient = false;
        for (int c = 0; c < b && !deficient; ++c) deficient = !(hG[c + 16 * c] > 0.0) || !std::isfinite(hG[c + 16 * c]);
        if (!deficient) {
            for (int a = 0; a < b; ++a)
                for (int c = 0; c < b; ++c)
                    sg[a + 16 * c] = hG[a + 16 * c] / (std::sqrt(hG[a + 16 * a]) * std::sqrt(hG[c + 16 * c]));
            deficient = eigs_chol_inv(sg, b, thr, nullptr) > 0;
        }
        if (deficient) break;
        TRY(orth(W));
    }
    const int blocks = j + 1;

    // Ritz vectors, 16 at a time, straight into X; their residuals for F through one product each
    double* Y = N.d_egY;
    double hs[PCG_NQ * SOLVE_RHS];
    for (int g0 = 0; g0 < nev; g0 += SOLVE_RHS) {
        const int nc = std::min<int>(SOLVE_RHS, nev - g0), have = std::max(0, std::min(nc, kw - g0));
        double* Xg = X + (int64_t)g0 * ldx;
        std::fill(hC.begin(), hC.begin() + (size_t)blocks * EIGS_TILE, 0.0);
        for (int i = 0; i < blocks; ++i)
            for (int a = 0; a < b; ++a)
                for (int c = 0; c < have; ++c)
                    hC[(size_t)i * EIGS_TILE + a + 16 * c] = S[(size_t)(b * i + a) * m + (m - 1 - (g0 + c))];
        TRY(update(Xg, ldx, nc, 0.0, nullptr, 0, Vb, n, blocks, b, hC.data()));
        TRY(spmv_panel(N, SPMV_MUL, d_Ax, nc, Xg, ldx, nullptr, 0, Y, n, nullptr));
        std::fill(hC.begin(), hC.begin() + EIGS_TILE, 0.0);
        for (int c = 0; c < have; ++c) hC[c + 16 * c] = -1.0 / theta[m - 1 - (g0 + c)];
        TRY(update(Y, n, nc, 1.0, Y, n, Xg, ldx, 1, nc, hC.data()));
        const uint32_t all = (1u << nc) - 1u;
        HIP_TRY(launch_pcg_dot(Y, n, Y, n, nullptr, 0, n, nc, all, N.d_egpart, dG, s0));
        HIP_TRY(hipMemcpyAsync(hs, dG, sizeof(hs), hipMemcpyDeviceToHost, s0));
        HIP_TRY(hipStreamSynchronize(s0));
        for (int c = 0; c < nc; ++c) {
            const int i = g0 + c;
            const bool got = c < have;
            const double th = got ? theta[m - 1 - i] : 0.0;
            lambda[i] = opt.sigma + 1.0 / th;
            if (!info) continue;
            sc_eigs_info& I = info[i];
            I.blocks = blocks;
            I.est = got ? est[i] : INFINITY;
            I.resid = got ? std::sqrt(hs[c]) : INFINITY;
            I.state = (got && est[i] <= opt.tol * th) ? SC_EIGS_CONVERGED : capped ? SC_EIGS_MAXBLOCKS : SC_EIGS_EXHAUSTED;
        }
    }
    return SC_OK;
}

}  // namespace

int64_t numeric_eigs(Numeric& N, const sc_eigs_options& opt, int32_t nev, const double* Ax, const double* X0,
                     int64_t ldx0, double* lambda, double* X, int64_t ldx, sc_eigs_info* info, bool host,
                     const char* who) {
    if (!N.factored) return SC_ERR_STATE;
    TRY(single_device(N, who));
    const int64_t st = numeric_status(N);
    if (st != SC_OK) return st;
    const int64_t n = N.S->n;
    DevTemp ta, t0, tx;
    const double* d_Ax = nullptr;
    TRY(device_values(N, Ax, host, ta, d_Ax, who));
    if (nev == 0 || n == 0) return SC_OK;
    TRY(spmv_ensure(N, who));
    TRY(eigs_ensure(N, opt.max_blocks));
    if (!host) return eigs_device(N, opt, nev, d_Ax, X0, ldx0, lambda, X, ldx, info);
    const int32_t b = (int32_t)std::min<int64_t>(SOLVE_RHS, n);
    if (opt.use_x0) TRY(stage_in(N, t0, X0, ldx0, n, b, true));
    TRY(stage_in(N, tx, X, ldx, n, nev, false));
    std::vector<double> lam((size_t)nev);
    std::vector<sc_eigs_info> inf((size_t)nev);
    TRY(eigs_device(N, opt, nev, d_Ax, (const double*)t0.p, n, lam.data(), (double*)tx.p, n, inf.data()));
    TRY(stage_out(N, tx, X, ldx, n, nev));
    std::copy(lam.begin(), lam.end(), lambda);
    if (info) std::copy(inf.begin(), inf.end(), info);
    return SC_OK;
}

}  // namespace sc
