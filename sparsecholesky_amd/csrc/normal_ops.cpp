// The sc_normal handle on the device: the term lists and J's two
// gather structures are uploaded at the first device call, with their task lists; the form
// writes S's values in the order of the pattern's Si, into the caller's array or into the
// handle's own buffer, which sc_factor_device then reads.  Calls are synchronous on the
// handle's stream.
#include "normal_ops.hpp"

#include <cmath>
#include <memory>

namespace sc {

namespace {

template <class T>
int64_t nupload(Normal& N, const std::vector<T>& v, const T*& dptr) {
    dptr = nullptr;
    const size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        N.err = "sc_normal: device allocation of " + std::to_string(bytes) + " bytes failed";
        return SC_ERR_DEVMEM;
    }
    N.allocs.push_back(p);
    N.dev_bytes += (int64_t)bytes;
    if (!v.empty()) HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    dptr = (const T*)p;
    return SC_OK;
}

int64_t nalloc(Normal& N, size_t doubles, double*& p) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(doubles, 1) * sizeof(double);
    if (hipMalloc(&q, bytes) != hipSuccess) {
        N.err = "sc_normal: device allocation of " + std::to_string(bytes) + " bytes failed";
        return SC_ERR_DEVMEM;
    }
    N.allocs.push_back(q);
    N.dev_bytes += (int64_t)bytes;
    p = (double*)q;
    return SC_OK;
}

int64_t prod_plan(Normal& N, int64_t nvec, const std::vector<int64_t>& ptr, const std::vector<int32_t>& idx,
                  const std::vector<int64_t>* pos, NormalProdPlan& P) {
    std::vector<NormalProdTask> task;
    std::vector<NormalProdLong> lng;
    int64_t nslots = 0;
    normal_prod_tasks(nvec, ptr.data(), task, lng, nslots);
    if (nslots > INT32_MAX / 2) {
        N.err = "sc_normal: too many chunks";
        return SC_ERR_ARG;
    }
    P = NormalProdPlan{};
    TRY(nupload(N, ptr, P.ptr));
    TRY(nupload(N, idx, P.idx));
    if (pos) TRY(nupload(N, *pos, P.pos));
    TRY(nupload(N, task, P.task));
    TRY(nupload(N, lng, P.lng));
    P.ntask = (int64_t)task.size();
    P.nvec = (int32_t)nvec;
    P.nlong = (int32_t)lng.size();
    TRY(nalloc(N, (size_t)nslots * 2 * NORMAL_RHS, P.part));
    return SC_OK;
}

int64_t form_plan(Normal& N, int64_t ne, const std::vector<int64_t>& tp, const std::vector<int32_t>& ta,
                  const std::vector<int32_t>& tb, const std::vector<int32_t>& tr, const std::vector<int64_t>& cpos,
                  const std::vector<int32_t>& dcol, NormalFormPlan& F) {
    std::vector<NormalFormTask> task;
    std::vector<NormalFormLong> lng;
    int64_t nslots = 0;
    normal_form_tasks(ne, tp.data(), task, lng, nslots);
    if (nslots > INT32_MAX / 2) {
        N.err = "sc_normal: too many chunks";
        return SC_ERR_ARG;
    }
    F = NormalFormPlan{};
    TRY(nupload(N, tp, F.tp));
    TRY(nupload(N, ta, F.ta));
    TRY(nupload(N, tb, F.tb));
    TRY(nupload(N, tr, F.tr));
    TRY(nupload(N, cpos, F.cpos));
    TRY(nupload(N, dcol, F.dcol));
    TRY(nupload(N, task, F.task));
    TRY(nupload(N, lng, F.lng));
    F.ne = ne;
    F.ntask = (int64_t)task.size();
    F.nlong = (int64_t)lng.size();
    TRY(nalloc(N, (size_t)nslots, F.part));
    return SC_OK;
}

void release(Normal& N) {
    for (void* p : N.allocs) (void)hipFree(p);
    N.allocs.clear();
    N.dev_bytes = 0;
}

// a device array of the call: the caller's, or a staged copy of the host one
struct Stage {
    void* p = nullptr;
    ~Stage() {
        if (p) (void)hipFree(p);
    }
    int64_t in(Normal& N, const double* h, size_t count, bool host, const double*& dptr) {
        dptr = h;
        if (!host || !h) return SC_OK;
        if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(double)) != hipSuccess) {
            p = nullptr;
            N.err = "sc_normal: device allocation of a staging array failed";
            return SC_ERR_DEVMEM;
        }
        if (count > 0) HIP_TRY(hipMemcpyAsync(p, h, count * sizeof(double), hipMemcpyHostToDevice, N.stream));
        dptr = (const double*)p;
        return SC_OK;
    }
    int64_t out(Normal& N, size_t count, double*& dptr) {
        if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(double)) != hipSuccess) {
            p = nullptr;
            N.err = "sc_normal: device allocation of a staging array failed";
            return SC_ERR_DEVMEM;
        }
        dptr = (double*)p;
        return SC_OK;
    }
};

// rows x nrhs host panel (ld) into a packed staged one and back
int64_t panel_in(Normal& N, Stage& t, const double* A, int64_t ld, int64_t rows, int32_t nrhs, bool copy,
                 double*& dptr) {
    TRY(t.out(N, (size_t)rows * nrhs, dptr));
    if (copy && rows > 0 && nrhs > 0)
        HIP_TRY(hipMemcpy2DAsync(dptr, (size_t)rows * sizeof(double), A, (size_t)ld * sizeof(double),
                                 (size_t)rows * sizeof(double), (size_t)nrhs, hipMemcpyHostToDevice, N.stream));
    return SC_OK;
}

int64_t panel_out(Normal& N, const double* dptr, double* A, int64_t ld, int64_t rows, int32_t nrhs) {
    if (rows > 0 && nrhs > 0)
        HIP_TRY(hipMemcpy2DAsync(A, (size_t)ld * sizeof(double), dptr, (size_t)rows * sizeof(double),
                                 (size_t)rows * sizeof(double), (size_t)nrhs, hipMemcpyDeviceToHost, N.stream));
    HIP_TRY(hipStreamSynchronize(N.stream));
    return SC_OK;
}

}  // namespace

int64_t normal_create(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const int64_t* Cp, const int32_t* Ci,
                      int device, Normal*& out, std::string& err) {
    out = nullptr;
    std::unique_ptr<Normal> N(new Normal());  // released if the build throws
    const int64_t rc = normal_build(m, n, Jp, Ji, Cp, Ci, N->H, err);
    if (rc != SC_OK) return rc;
    N->device = device;
    out = N.release();
    return SC_OK;
}

void normal_free(Normal* N) {
    if (!N) return;
    if (N->dev_ready) {
        (void)hipSetDevice(N->device);
        release(*N);
        if (N->stream) (void)hipStreamDestroy(N->stream);
    }
    delete N;
}

int64_t normal_memory(const Normal& N, int64_t* out, int32_t cap) {
    const NormalStruct& H = N.H;
    auto bytes = [](const auto& v) { return (int64_t)(v.size() * sizeof(v[0])); };
    const int64_t host = bytes(H.Jp) + bytes(H.Ji) + bytes(H.Cp) + bytes(H.Ci) + bytes(H.Sp) + bytes(H.Si) +
                         bytes(H.tp) + bytes(H.ta) + bytes(H.tb) + bytes(H.tr) + bytes(H.cpos) + bytes(H.dcol) +
                         bytes(H.rp) + bytes(H.ci) + bytes(H.sp);
    const int64_t v[4] = {host, N.dev_bytes, H.T, (int64_t)H.Si.size()};
    for (int32_t k = 0; k < cap && k < 4; ++k) out[k] = v[k];
    return 4;
}

int64_t normal_ensure(Normal& N, int want_device) {
    if (N.dev_ready) {
        HIP_TRY(hipSetDevice(N.device));
        return SC_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        N.err = "sc_normal: no HIP device available";
        return SC_ERR_HIP;
    }
    int dev = N.device;
    if (dev < 0) dev = want_device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (dev >= ndev) {
        N.err = "sc_normal: device index out of range";
        return SC_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(dev));
    N.device = dev;
    HIP_TRY(hipStreamCreateWithFlags(&N.stream, hipStreamNonBlocking));
    N.dev_ready = true;  // from here on normal_free releases what was allocated
    const NormalStruct& H = N.H;
    TRY(form_plan(N, (int64_t)H.Si.size(), H.tp, H.ta, H.tb, H.tr, H.cpos, H.dcol, N.F));
    TRY(prod_plan(N, H.n, H.Jp, H.Ji, nullptr, N.PC));
    TRY(prod_plan(N, H.m, H.rp, H.ci, &H.sp, N.PR));
    TRY(nalloc(N, H.Si.size(), N.Sbuf));
    TRY(nalloc(N, (size_t)std::max(H.m, H.n) * NORMAL_RHS, N.xt));
    TRY(nalloc(N, (size_t)(H.nnzC + H.n), N.bval));
    N.plans_ready = true;
    return SC_OK;
}

static int64_t ensure_plans(Normal& N, int want_device, const char* who) {
    TRY(normal_ensure(N, want_device));
    if (!N.plans_ready) {
        N.err = std::string(who) + ": an earlier device allocation of this handle failed";
        return SC_ERR_STATE;
    }
    return SC_OK;
}

int64_t normal_values(Normal& N, const double* Jx, const double* w, const double* Cx, const double* d, double lambda,
                      double* Sx, bool host, const char* who) {
    const NormalStruct& H = N.H;
    const size_t ne = H.Si.size();
    if (ne == 0) return SC_OK;
    TRY(ensure_plans(N, -1, who));
    Stage sj, sw, sc_, sd, ss;
    const double *dJ, *dw, *dC, *dd;
    TRY(sj.in(N, Jx, (size_t)H.nnzJ, host, dJ));
    TRY(sw.in(N, w, (size_t)H.m, host, dw));
    TRY(sc_.in(N, Cx, (size_t)H.nnzC, host, dC));
    TRY(sd.in(N, d, (size_t)H.n, host, dd));
    double* dS = Sx;
    if (host) TRY(ss.out(N, ne, dS));
    HIP_TRY(launch_normal_form(N.F, dJ, dw, dC, dd, lambda, dS, N.stream));
    if (host) HIP_TRY(hipMemcpyAsync(Sx, dS, ne * sizeof(double), hipMemcpyDeviceToHost, N.stream));
    HIP_TRY(hipStreamSynchronize(N.stream));
    return SC_OK;
}

int64_t normal_check_numeric(Normal& N, Numeric& num, const char* who) {
    const int64_t rc = single_device(num, who);
    if (rc != SC_OK) {
        N.err = num.err;
        return rc;
    }
    if (num.S->n != N.H.n || num.S->nnzA_in != (int64_t)N.H.Si.size()) {
        N.err = std::string(who) + ": the numeric handle's analysis has n = " + std::to_string(num.S->n) + " and " +
                std::to_string(num.S->nnzA_in) + " values, the pattern of S n = " + std::to_string(N.H.n) + " and " +
                std::to_string(N.H.Si.size());
        return SC_ERR_ARG;
    }
    if (N.dev_ready && N.device != num.device) {
        N.err = std::string(who) + ": the two handles live on different devices";
        return SC_ERR_ARG;
    }
    return SC_OK;
}

int64_t normal_factor(Normal& N, Numeric& num, const double* Jx, const double* w, const double* Cx, const double* d,
                      double lambda, bool host, const char* who) {
    TRY(normal_check_numeric(N, num, who));
    TRY(ensure_plans(N, num.device, who));
    if (N.device != num.device) {
        N.err = std::string(who) + ": the two handles live on different devices";
        return SC_ERR_ARG;
    }
    const NormalStruct& H = N.H;
    if (!H.Si.empty()) {
        Stage sj, sw, sc_, sd;
        const double *dJ, *dw, *dC, *dd;
        TRY(sj.in(N, Jx, (size_t)H.nnzJ, host, dJ));
        TRY(sw.in(N, w, (size_t)H.m, host, dw));
        TRY(sc_.in(N, Cx, (size_t)H.nnzC, host, dC));
        TRY(sd.in(N, d, (size_t)H.n, host, dd));
        HIP_TRY(launch_normal_form(N.F, dJ, dw, dC, dd, lambda, N.Sbuf, N.stream));
        // what the least-squares gradient subtracts: C's values, then d + lambda per row
        N.base_active = Cx || d || lambda != 0.0;
        if (H.nnzC > 0) {
            if (dC)
                HIP_TRY(hipMemcpyAsync(N.bval, dC, (size_t)H.nnzC * sizeof(double), hipMemcpyDeviceToDevice, N.stream));
            else
                HIP_TRY(hipMemsetAsync(N.bval, 0, (size_t)H.nnzC * sizeof(double), N.stream));
        }
        HIP_TRY(launch_normal_shift(N.bval + H.nnzC, dd, lambda, H.n, N.stream));
        HIP_TRY(hipStreamSynchronize(N.stream));
    }
    N.values_valid = true;
    N.last_num = nullptr;  // whatever happens next, the buffer and the base are no longer an earlier factor's
    const int64_t rc = numeric_factor(num, N.Sbuf, true);
    if (rc < 0) {
        N.err = num.err;
        return rc;
    }
    N.last_num = &num;
    N.last_gen = num.factor_gen;
    return rc;
}

int64_t normal_product(Normal& N, bool transposed, int32_t nrhs, const double* Jx, const double* w, const double* X,
                       int64_t ldx, double* Y, int64_t ldy, bool host, const char* who) {
    const NormalStruct& H = N.H;
    const int64_t nin = transposed ? H.m : H.n, nout = transposed ? H.n : H.m;
    if (nrhs == 0 || nout == 0) return SC_OK;
    TRY(ensure_plans(N, -1, who));
    Stage sj, sw, sx, sy;
    const double *dJ, *dw;
    TRY(sj.in(N, Jx, (size_t)H.nnzJ, host, dJ));
    TRY(sw.in(N, transposed ? w : nullptr, (size_t)H.m, host, dw));
    const double* dX = X;
    double* dY = Y;
    int64_t lx = ldx, ly = ldy;
    if (host) {
        double* t = nullptr;
        TRY(panel_in(N, sx, X, ldx, nin, nrhs, true, t));
        dX = t;
        TRY(panel_in(N, sy, nullptr, 0, nout, nrhs, false, dY));
        lx = std::max<int64_t>(nin, 1);
        ly = std::max<int64_t>(nout, 1);
    }
    for (int32_t j0 = 0; j0 < nrhs; j0 += NORMAL_RHS) {
        const int nr = std::min<int32_t>(NORMAL_RHS, nrhs - j0);
        HIP_TRY(launch_spmv_transpose(N.xt, dX + (int64_t)j0 * lx, lx, nin, nr, N.stream));
        if (transposed)
            HIP_TRY(launch_normal_mult(N.PC, dJ, dw, N.xt, nr, dY + (int64_t)j0 * ly, ly, N.stream));
        else
            HIP_TRY(launch_normal_mul(N.PR, NORMAL_MUL, dJ, N.xt, nr, nullptr, 0, nullptr, dY + (int64_t)j0 * ly, ly, nullptr,
                                      N.stream));
    }
    if (host) return panel_out(N, dY, Y, ldy, nout, nrhs);
    HIP_TRY(hipStreamSynchronize(N.stream));
    return SC_OK;
}

// ---- least squares by corrected semi-normal equations ----
namespace {

constexpr double UNIT = 1.1102230246251565e-16;  // 2^-53

int64_t lsq_ensure(Normal& N) {
    if (N.lsq_ready) return SC_OK;
    const NormalStruct& H = N.H;
    std::vector<int64_t> rp, pos;
    std::vector<int32_t> ci;
    normal_base_rows(H, rp, ci, pos);
    TRY(prod_plan(N, H.n, rp, ci, &pos, N.PB));
    TRY(nalloc(N, (size_t)H.n * NORMAL_RHS, N.G));
    TRY(nalloc(N, (size_t)H.m * NORMAL_RHS, N.R));
    TRY(nalloc(N, (size_t)H.n * NORMAL_RHS, N.xtn));
    TRY(nalloc(N, (size_t)H.n * NORMAL_RHS, N.Gl));
    TRY(nalloc(N, (size_t)H.m * NORMAL_RHS, N.Rl));
    TRY(nalloc(N, (size_t)H.m * NORMAL_RHS, N.xtl));
    TRY(nalloc(N, (size_t)(4 + std::max(NORMAL_NG, REFINE_NG)) * NORMAL_RHS, N.nrm));
    N.lsq_ready = true;
    return SC_OK;
}

// R = B - J X, G = J^T W R - (C + D) X for the panel's nr columns, and h (host, 3 x NORMAL_RHS):
// max |g|, max |x|, sum w r^2
int64_t lsq_gradient(Normal& N, int kmode, int nr, const double* dJ, const double* dw, const double* Bp, int64_t ldb,
                     const double* Xp, int64_t ldx, double* h) {
    const NormalStruct& H = N.H;
    const int64_t m = H.m, n = H.n, lm = std::max<int64_t>(m, 1);
    hipStream_t s0 = N.stream;
    double* part = N.nrm + 4 * NORMAL_RHS;
    HIP_TRY(launch_spmv_transpose(N.xtn, Xp, ldx, n, nr, s0));
    if (kmode == NORMAL_RES_DD) {
        // as if in twice the working precision throughout: the residual stays a pair, so does
        // the gradient until the base product is off it; only then is it rounded
        HIP_TRY(launch_normal_mul(N.PR, kmode, dJ, N.xtn, nr, Bp, ldb, nullptr, N.R, lm, N.Rl, s0));
        HIP_TRY(launch_spmv_transpose(N.xt, N.R, lm, m, nr, s0));
        HIP_TRY(launch_spmv_transpose(N.xtl, N.Rl, lm, m, nr, s0));
        HIP_TRY(launch_normal_mult_dd(N.PC, dJ, dw, N.xt, N.xtl, nr, N.G, N.Gl, n, s0));
        if (N.base_active)
            HIP_TRY(launch_normal_mul(N.PB, kmode, N.bval, N.xtn, nr, N.G, n, N.Gl, N.G, n, nullptr, s0));
    } else {
        HIP_TRY(launch_normal_mul(N.PR, kmode, dJ, N.xtn, nr, Bp, ldb, nullptr, N.R, lm, nullptr, s0));
        HIP_TRY(launch_spmv_transpose(N.xt, N.R, lm, m, nr, s0));
        HIP_TRY(launch_normal_mult(N.PC, dJ, dw, N.xt, nr, N.G, n, s0));
        if (N.base_active)
            HIP_TRY(launch_normal_mul(N.PB, kmode, N.bval, N.xtn, nr, N.G, n, nullptr, N.G, n, nullptr, s0));
    }
    HIP_TRY(launch_refine_dnorm(N.G, n, n, nr, part, N.nrm, s0));
    HIP_TRY(launch_refine_dnorm(Xp, ldx, n, nr, part, N.nrm + NORMAL_RHS, s0));
    HIP_TRY(launch_normal_wnorm(N.R, lm, dw, m, nr, part, N.nrm + 2 * NORMAL_RHS, s0));
    HIP_TRY(hipMemcpyAsync(h, N.nrm, sizeof(double) * 3 * NORMAL_RHS, hipMemcpyDeviceToHost, s0));
    HIP_TRY(hipStreamSynchronize(s0));
    return SC_OK;
}

int64_t lsq_device(Normal& N, Numeric& num, const sc_refine_options& opt, int32_t nrhs, const double* dJ,
                   const double* dw, const double* B, int64_t ldb, double* X, int64_t ldx, sc_lstsq_info* info) {
    const NormalStruct& H = N.H;
    const int64_t m = H.m, n = H.n;
    hipStream_t s0 = N.stream;
    const int kmode = opt.residual == SC_RESIDUAL_DD ? NORMAL_RES_DD : NORMAL_RES_FP64;
    double* part = N.nrm + 4 * NORMAL_RHS;
    double* d_dn = N.nrm + 3 * NORMAL_RHS;
    double h[3 * NORMAL_RHS], dn[NORMAL_RHS];
    for (int32_t j0 = 0; j0 < nrhs; j0 += NORMAL_RHS) {
        const int nr = std::min<int32_t>(NORMAL_RHS, nrhs - j0);
        const double* Bp = B + (int64_t)j0 * ldb;
        double* Xp = X + (int64_t)j0 * ldx;
        // x_0 = inv(S) J^T W b: the plain normal-equations solve
        HIP_TRY(launch_spmv_transpose(N.xt, Bp, ldb, m, nr, s0));
        HIP_TRY(launch_normal_mult(N.PC, dJ, dw, N.xt, nr, N.G, n, s0));
        HIP_TRY(hipStreamSynchronize(s0));
        int64_t rc = numeric_solve_device_multi(num, nr, N.G, n, Xp, ldx);
        if (rc != SC_OK) {
            if (rc < 0) N.err = num.err;
            return rc;
        }
        TRY(lsq_gradient(N, kmode, nr, dJ, dw, Bp, ldb, Xp, ldx, h));
        int32_t iters[NORMAL_RHS] = {0}, state[NORMAL_RHS];
        double dprev[NORMAL_RHS], dlast[NORMAL_RHS] = {0.0};
        bool active[NORMAL_RHS];
        int nactive = 0;
        for (int c = 0; c < nr; ++c) {
            dprev[c] = h[NORMAL_RHS + c];  // x_0 is the first increment, from zero
            active[c] = false;
            if (h[c] == 0.0)
                state[c] = SC_REFINE_CONVERGED;  // an exactly zero gradient: nothing to improve
            else if (opt.max_iter == 0)
                state[c] = SC_REFINE_MAXITER;
            else
                active[c] = true, ++nactive;
        }
        while (nactive > 0) {
            // delta = inv(S) g, in place in the gradient panel
            rc = numeric_solve_device_multi(num, nr, N.G, n, N.G, n);
            if (rc != SC_OK) {
                if (rc < 0) N.err = num.err;
                return rc;
            }
            HIP_TRY(launch_refine_dnorm(N.G, n, n, nr, part, d_dn, s0));
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
            HIP_TRY(launch_refine_add(Xp, ldx, N.G, n, n, nr, mask, s0));
            // a frozen column's X has not changed: its gradient and norms come out as before
            TRY(lsq_gradient(N, kmode, nr, dJ, dw, Bp, ldb, Xp, ldx, h));
            for (int c = 0; c < nr; ++c) {
                if (!((mask >> c) & 1u)) continue;
                const double dk = dn[c];
                int32_t st = -1;
                if (dk <= UNIT * h[NORMAL_RHS + c] || h[c] == 0.0)
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
                sc_lstsq_info& I = info[j0 + c];
                I.iters = iters[c];
                I.state = state[c];
                I.grad_norm = h[c];
                I.resid_norm = std::sqrt(h[2 * NORMAL_RHS + c]);
                const double xn = h[NORMAL_RHS + c];
                I.dx_ratio = (dlast[c] == 0.0 && xn == 0.0) ? 0.0 : dlast[c] / xn;
            }
    }
    return SC_OK;
}

}  // namespace

int64_t normal_lstsq(Normal& N, Numeric& num, const sc_refine_options& opt, int32_t nrhs, const double* Jx,
                     const double* w, const double* B, int64_t ldb, double* X, int64_t ldx, sc_lstsq_info* info,
                     bool host, const char* who) {
    if (!num.factored) {
        N.err = std::string(who) + ": the numeric handle holds no factorization";
        return SC_ERR_STATE;
    }
    TRY(normal_check_numeric(N, num, who));
    const int64_t st = numeric_status(num);
    if (st != SC_OK) return st;
    // the buffer and the remembered base belong to the last sc_normal_factor_* of this handle:
    // only the factor that call made, still in place, may be used with them (a freed sc_numeric
    // whose address another one reuses would also need that count and a factorization from Sbuf)
    if (!N.plans_ready || N.last_num != &num || N.last_gen != num.factor_gen || num.last_Ax != N.Sbuf) {
        N.err = std::string(who) + ": the factor the numeric handle holds was not made by the last sc_normal_factor_* "
                                   "of this handle";
        return SC_ERR_STATE;
    }
    const NormalStruct& H = N.H;
    if (nrhs == 0) return SC_OK;
    if (H.n == 0) {
        if (info)
            for (int32_t c = 0; c < nrhs; ++c) info[c] = sc_lstsq_info{0, SC_REFINE_CONVERGED, 0.0, 0.0, 0.0};
        return SC_OK;
    }
    HIP_TRY(hipSetDevice(N.device));
    TRY(lsq_ensure(N));
    Stage sj, sw, sb, sx;
    const double *dJ, *dw;
    TRY(sj.in(N, Jx, (size_t)H.nnzJ, host, dJ));
    TRY(sw.in(N, w, (size_t)H.m, host, dw));
    if (!host) return lsq_device(N, num, opt, nrhs, dJ, dw, B, ldb, X, ldx, info);
    double *dB = nullptr, *dX = nullptr;
    TRY(panel_in(N, sb, B, ldb, H.m, nrhs, true, dB));
    TRY(panel_in(N, sx, nullptr, 0, H.n, nrhs, false, dX));
    TRY(lsq_device(N, num, opt, nrhs, dJ, dw, dB, std::max<int64_t>(H.m, 1), dX, H.n, info));
    return panel_out(N, dX, X, ldx, H.n, nrhs);
}

// ---- the kernels alone on caller structures ----
namespace {

struct Scratch : Normal {
    ~Scratch() { release(*this); }
};

}  // namespace

int64_t debug_normal_form(int64_t ne, const int64_t* tp, const int32_t* ta, const int32_t* tb, const int32_t* tr,
                          const int64_t* cpos, const int32_t* dcol, int64_t nJ, int64_t nw, int64_t nC, int64_t nd,
                          const double* d_Jx, const double* d_w, const double* d_Cx, const double* d_d, double lambda,
                          double* d_Sx, std::string& err) {
    auto bad = [&](const char* what) {
        err = std::string("sc_debug_normal_form: ") + what;
        return (int64_t)SC_ERR_ARG;
    };
    if (ne < 0 || nJ < 0 || nw < 0 || nC < 0 || nd < 0) return bad("negative count");
    if (ne == 0) return SC_OK;
    if (!tp || !cpos || !dcol || !d_Sx) return bad("null array");
    if (tp[0] != 0) return bad("tp[0] != 0");
    for (int64_t e = 0; e < ne; ++e) {
        if (tp[e + 1] < tp[e]) return bad("tp descends");
        if (cpos[e] < -1 || cpos[e] >= nC) return bad("cpos out of range");
        if (dcol[e] < -1 || dcol[e] >= nd) return bad("dcol out of range");
    }
    const int64_t T = tp[ne];
    if (T > 0 && (!ta || !tb || !tr || !d_Jx)) return bad("null array");
    for (int64_t t = 0; t < T; ++t)
        if (ta[t] < 0 || ta[t] >= nJ || tb[t] < 0 || tb[t] >= nJ || tr[t] < 0 || tr[t] >= nw)
            return bad("term position or row out of range");
    Scratch N;
    NormalFormPlan F;
    int64_t rc = form_plan(N, ne, std::vector<int64_t>(tp, tp + ne + 1), std::vector<int32_t>(ta, ta + T),
                           std::vector<int32_t>(tb, tb + T), std::vector<int32_t>(tr, tr + T),
                           std::vector<int64_t>(cpos, cpos + ne), std::vector<int32_t>(dcol, dcol + ne), F);
    if (rc == SC_OK && (launch_normal_form(F, d_Jx, d_w, d_Cx, d_d, lambda, d_Sx, nullptr) != hipSuccess ||
                        hipDeviceSynchronize() != hipSuccess))
        rc = SC_ERR_HIP;
    if (rc != SC_OK && err.empty()) err = N.err;
    return rc;
}

int64_t debug_normal_prod(bool transposed, int32_t mode, int64_t nvec, int64_t nin, const int64_t* ptr,
                          const int32_t* idx, const int64_t* pos, int64_t nval, const double* d_val, const double* d_w,
                          int32_t nrhs, const double* d_X, int64_t ldx, const double* d_B, int64_t ldb, double* d_R,
                          int64_t ldr, std::string& err) {
    const char* who = transposed ? "sc_debug_normal_mult: " : "sc_debug_normal_mul: ";
    auto bad = [&](const char* what) {
        err = std::string(who) + what;
        return (int64_t)SC_ERR_ARG;
    };
    if (mode < NORMAL_MUL || mode > NORMAL_RES_DD) return bad("unknown mode");
    if (nvec < 0 || nin < 0 || nvec > INT32_MAX || nin > INT32_MAX || nrhs < 0 || nrhs > NORMAL_RHS)
        return bad("negative size or nrhs outside [0, 16]");
    if (nvec == 0 || nrhs == 0) return SC_OK;
    if (!ptr || !d_R || (nin > 0 && !d_X) || (mode != NORMAL_MUL && !d_B)) return bad("null array");
    if (ldx < nin || ldr < nvec || (mode != NORMAL_MUL && ldb < nvec)) return bad("leading dimension below the row count");
    if (ptr[0] != 0) return bad("the pointer array does not start at 0");
    for (int64_t v = 0; v < nvec; ++v)
        if (ptr[v + 1] < ptr[v]) return bad("the pointer array descends");
    const int64_t nz = ptr[nvec];
    if (nz > 0 && (!idx || !d_val)) return bad("null array");
    for (int64_t e = 0; e < nz; ++e)
        if (idx[e] < 0 || idx[e] >= nin || (pos && (pos[e] < 0 || pos[e] >= nval))) return bad("index or position out of range");
    if (!pos && nz > nval) return bad("more entries than values");
    Scratch N;
    NormalProdPlan P;
    std::vector<int64_t> vpos;
    if (pos) vpos.assign(pos, pos + nz);
    int64_t rc = prod_plan(N, nvec, std::vector<int64_t>(ptr, ptr + nvec + 1), std::vector<int32_t>(idx, idx + nz),
                           pos ? &vpos : nullptr, P);
    double* xt = nullptr;
    if (rc == SC_OK) rc = nalloc(N, (size_t)nin * NORMAL_RHS, xt);
    if (rc == SC_OK) {
        hipError_t e = launch_spmv_transpose(xt, d_X, ldx, nin, nrhs, nullptr);
        if (e == hipSuccess)
            e = transposed ? launch_normal_mult(P, d_val, d_w, xt, nrhs, d_R, ldr, nullptr)
                           : launch_normal_mul(P, mode, d_val, xt, nrhs, d_B, ldb, nullptr, d_R, ldr, nullptr, nullptr);
        if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = SC_ERR_HIP;
    }
    if (rc != SC_OK && err.empty()) err = N.err;
    return rc;
}

// The pair path of the least-squares gradient alone: (R, Rl) = B - J X out of the compensated
// residual, then (G, Gl) = J^T diag(w) (R + Rl) by the pair product.
int64_t debug_normal_pair(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const int64_t* rp,
                          const int32_t* ci, const int64_t* sp, const double* d_Jx, const double* d_w, int32_t nrhs,
                          const double* d_X, int64_t ldx, const double* d_B, int64_t ldb, double* d_R, double* d_Rl,
                          int64_t ldr, double* d_G, double* d_Gl, int64_t ldg, std::string& err) {
    auto bad = [&](const char* what) {
        err = std::string("sc_debug_normal_pair: ") + what;
        return (int64_t)SC_ERR_ARG;
    };
    if (m < 0 || n < 0 || m > INT32_MAX || n > INT32_MAX || nrhs < 0 || nrhs > NORMAL_RHS)
        return bad("negative size or nrhs outside [0, 16]");
    if (nrhs == 0 || (m == 0 && n == 0)) return SC_OK;
    if (!Jp || !rp || (n > 0 && (!d_X || !d_G || !d_Gl)) || (m > 0 && (!d_B || !d_R || !d_Rl))) return bad("null array");
    if (ldx < n || ldg < n || ldb < m || ldr < m) return bad("leading dimension below the row count");
    if (Jp[0] != 0 || rp[0] != 0) return bad("a pointer array does not start at 0");
    for (int64_t j = 0; j < n; ++j)
        if (Jp[j + 1] < Jp[j]) return bad("Jp descends");
    for (int64_t r = 0; r < m; ++r)
        if (rp[r + 1] < rp[r]) return bad("rp descends");
    const int64_t nz = Jp[n];
    if (rp[m] != nz) return bad("the two structures differ in their entry counts");
    if (nz > 0 && (!Ji || !ci || !sp || !d_Jx)) return bad("null array");
    for (int64_t e = 0; e < nz; ++e)
        if (Ji[e] < 0 || Ji[e] >= m || ci[e] < 0 || ci[e] >= n || sp[e] < 0 || sp[e] >= nz)
            return bad("index or position out of range");
    Scratch N;
    NormalProdPlan PC, PR;
    const std::vector<int64_t> vsp(sp, sp + nz);
    int64_t rc = prod_plan(N, n, std::vector<int64_t>(Jp, Jp + n + 1), std::vector<int32_t>(Ji, Ji + nz), nullptr, PC);
    if (rc == SC_OK)
        rc = prod_plan(N, m, std::vector<int64_t>(rp, rp + m + 1), std::vector<int32_t>(ci, ci + nz), &vsp, PR);
    double *xtn = nullptr, *xt = nullptr, *xtl = nullptr;
    if (rc == SC_OK) rc = nalloc(N, (size_t)n * NORMAL_RHS, xtn);
    if (rc == SC_OK) rc = nalloc(N, (size_t)m * NORMAL_RHS, xt);
    if (rc == SC_OK) rc = nalloc(N, (size_t)m * NORMAL_RHS, xtl);
    if (rc == SC_OK) {
        hipError_t e = launch_spmv_transpose(xtn, d_X, ldx, n, nrhs, nullptr);
        if (e == hipSuccess)
            e = launch_normal_mul(PR, NORMAL_RES_DD, d_Jx, xtn, nrhs, d_B, ldb, nullptr, d_R, ldr, d_Rl, nullptr);
        if (e == hipSuccess) e = launch_spmv_transpose(xt, d_R, ldr, m, nrhs, nullptr);
        if (e == hipSuccess) e = launch_spmv_transpose(xtl, d_Rl, ldr, m, nrhs, nullptr);
        if (e == hipSuccess) e = launch_normal_mult_dd(PC, d_Jx, d_w, xt, xtl, nrhs, d_G, d_Gl, ldg, nullptr);
        if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = SC_ERR_HIP;
    }
    if (rc != SC_OK && err.empty()) err = N.err;
    return rc;
}

}  // namespace sc
