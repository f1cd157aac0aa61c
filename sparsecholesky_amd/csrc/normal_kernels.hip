// The three kernels of the weighted normal equations (normal.hpp has the contracts, DESIGN.md
// section 9.9 the reasons): forming S's values from term lists, G = J^T diag(w) Y down J's
// columns, and Y = J X / R = B - J X over J's rows.  Every sum runs in one fixed order, no
// atomics: the results are bitwise repeatable, and since a lane of the products owns one
// right-hand side, a column's bits do not depend on the columns it travels with.
#include <hip/hip_runtime.h>

#include "normal.hpp"

namespace sc {

namespace {

__device__ __forceinline__ double normal_base(const NormalFormPlan& P, int64_t e, const double* __restrict__ Cx,
                                              const double* __restrict__ d, double lambda) {
    const int64_t cp = P.cpos[e];
    const double c = (Cx && cp >= 0) ? Cx[cp] : 0.0;
    const int32_t j = P.dcol[e];
    return j >= 0 ? c + ((d ? d[j] : 0.0) + lambda) : c;
}

__device__ __forceinline__ double normal_term(const NormalFormPlan& P, int64_t t, const double* __restrict__ Jx,
                                              const double* __restrict__ w, double s) {
    const double a = Jx[P.ta[t]];
    const double aw = w ? a * w[P.tr[t]] : a;
    return fma(aw, Jx[P.tb[t]], s);
}

// short lists: one lane per entry, the base first, then the terms in list order
__global__ __launch_bounds__(256) void normal_form_short_kernel(NormalFormPlan P, const double* __restrict__ Jx,
                                                                const double* __restrict__ w,
                                                                const double* __restrict__ Cx,
                                                                const double* __restrict__ d, double lambda,
                                                                double* __restrict__ Sx) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < P.ne; e += (int64_t)gridDim.x * 256) {
        const int64_t t0 = P.tp[e], t1 = P.tp[e + 1];
        if (t1 - t0 > NORMAL_SHORT) continue;
        double s = normal_base(P, e, Cx, d, lambda);
        for (int64_t t = t0; t < t1; ++t) s = normal_term(P, t, Jx, w, s);
        Sx[e] = s;
    }
}

// grouped lists and chunks: NORMAL_LANES lanes per task, consecutive lanes on consecutive terms
__global__ __launch_bounds__(256) void normal_form_group_kernel(NormalFormPlan P, const double* __restrict__ Jx,
                                                                const double* __restrict__ w,
                                                                const double* __restrict__ Cx,
                                                                const double* __restrict__ d, double lambda,
                                                                double* __restrict__ Sx) {
    const int l = threadIdx.x & (NORMAL_LANES - 1);
    const int64_t k = (int64_t)blockIdx.x * (256 / NORMAL_LANES) + (threadIdx.x / NORMAL_LANES);
    const bool live = k < P.ntask;
    NormalFormTask T = {0, 0, 0, -1, 0};
    if (live) T = P.task[k];
    double s = 0.0;
    for (int q = l; q < T.cnt; q += NORMAL_LANES) s = normal_term(P, T.t0 + q, Jx, w, s);
#pragma unroll
    for (int h = NORMAL_LANES / 2; h > 0; h >>= 1) s += __shfl_down(s, h, NORMAL_LANES);
    if (live && l == 0) {
        if (T.slot < 0)
            Sx[T.e] = normal_base(P, T.e, Cx, d, lambda) + s;
        else
            P.part[T.slot] = s;
    }
}

// chunked lists: the partials in chunk order, then the base
__global__ __launch_bounds__(256) void normal_form_combine_kernel(NormalFormPlan P, const double* __restrict__ Cx,
                                                                  const double* __restrict__ d, double lambda,
                                                                  double* __restrict__ Sx) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= P.nlong) return;
    const NormalFormLong L = P.lng[k];
    double s = P.part[L.slot0];
    for (int c = 1; c < L.nch; ++c) s += P.part[L.slot0 + c];
    Sx[L.e] = normal_base(P, L.e, Cx, d, lambda) + s;
}

// ---- the products ----
// Dot2 (Ogita, Rump, Oishi 2005), as the residual of refine.cpp: contraction is switched off
// where it would fuse the product of TwoProd into the subtraction that recovers its error.
__device__ __forceinline__ void normal_two_sum(double a, double b, double& s, double& err) {
#pragma clang fp contract(off)
    s = a + b;
    const double bb = s - a;
    err = (a - (s - bb)) + (b - bb);
}

__device__ __forceinline__ void normal_dd_sub_prod(double a, double x, double& s, double& e) {
#pragma clang fp contract(off)
    const double h = a * x;
    const double pe = __builtin_fma(a, x, -h);
    double q;
    normal_two_sum(s, -h, s, q);
    e += q - pe;
}

// (s, e) += (p + pe) (x + xl), p + pe an exact product: the leading product split exactly,
// the three cross terms in plain fp64 (they are of the order of the error term)
__device__ __forceinline__ void normal_dd_add_prod2(double p, double pe, double x, double xl, double& s, double& e) {
#pragma clang fp contract(off)
    const double h = p * x;
    const double he = __builtin_fma(p, x, -h);
    double q;
    normal_two_sum(s, h, s, q);
    e += (q + he) + (pe * x + p * xl);
}

// Sixteen lanes share a task (a vector of the structure or one chunk of it) and each owns a
// right-hand side: the index, the position and the value of an entry are one broadcast load,
// the gathered row of the 16-wide panel one 128-byte line.  SCALED (the transposed product):
// the value is multiplied by scale[idx] first.  The compensated modes keep a sum and an error
// term: Ein (may be null) is the error term B comes with, Eout (may be null) receives the low
// half of the result, which is then left as the pair (R, Eout) instead of being rounded once.
// NORMAL_MULT_DD: the scaled product of a panel given as a pair (xt, xtl), as if in twice the
// working precision.
template <int MODE, bool SCALED>
__global__ __launch_bounds__(256) void normal_prod_kernel(NormalProdPlan P, const double* __restrict__ val,
                                                          const double* __restrict__ scale,
                                                          const double* __restrict__ xt,
                                                          const double* __restrict__ xtl, int nrhs,
                                                          const double* __restrict__ B, int64_t ldb,
                                                          const double* __restrict__ Ein, double* __restrict__ R,
                                                          int64_t ldr, double* __restrict__ Eout) {
    const int c = threadIdx.x & 15;
    const int64_t k = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (k >= P.ntask) return;
    const NormalProdTask T = P.task[k];
    const int64_t vb = P.ptr[T.v], ve = P.ptr[T.v + 1];
    const int64_t e1 = T.e0 + NORMAL_PCH < ve ? T.e0 + NORMAL_PCH : ve;
    double s = 0.0, err = 0.0;
    if ((MODE == NORMAL_RES_FP64 || MODE == NORMAL_RES_DD) && T.e0 == vb && c < nrhs) {
        s = B[T.v + (int64_t)c * ldb];
        if (MODE == NORMAL_RES_DD && Ein) err = Ein[T.v + (int64_t)c * ldb];
    }
#pragma unroll 4
    for (int64_t e = T.e0; e < e1; ++e) {
        const int32_t i = P.idx[e];
        double a = val[P.pos ? P.pos[e] : e];
        const double x = xt[(int64_t)NORMAL_RHS * i + c];
        if (MODE == NORMAL_MULT_DD) {
            double ae = 0.0;
            if (scale) {
#pragma clang fp contract(off)
                const double wv = scale[i], p = a * wv;
                ae = __builtin_fma(a, wv, -p);
                a = p;
            }
            normal_dd_add_prod2(a, ae, x, xtl[(int64_t)NORMAL_RHS * i + c], s, err);
            continue;
        }
        if (SCALED && scale) a *= scale[i];
        if (MODE == NORMAL_MUL)
            s = fma(a, x, s);
        else if (MODE == NORMAL_RES_FP64)
            s = fma(-a, x, s);
        else
            normal_dd_sub_prod(a, x, s, err);
    }
    if (T.slot >= 0) {
        double* p = P.part + (int64_t)T.slot * (2 * NORMAL_RHS) + c;
        p[0] = s;
        p[NORMAL_RHS] = err;
    } else if (c < nrhs) {
        if (MODE >= NORMAL_RES_DD && Eout) {
            double lo;
            normal_two_sum(s, err, s, lo);
            Eout[T.v + (int64_t)c * ldr] = lo;
            R[T.v + (int64_t)c * ldr] = s;
        } else {
            R[T.v + (int64_t)c * ldr] = MODE >= NORMAL_RES_DD ? s + err : s;
        }
    }
}

// chunked vectors: the partials in chunk order (pairs by TwoSum in the compensated modes)
template <int MODE>
__global__ __launch_bounds__(256) void normal_prod_combine_kernel(NormalProdPlan P, int nrhs, double* __restrict__ R,
                                                                  int64_t ldr, double* __restrict__ Eout) {
    const int c = threadIdx.x & 15;
    const int k = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (k >= P.nlong) return;
    const NormalProdLong L = P.lng[k];
    const int64_t len = P.ptr[L.v + 1] - P.ptr[L.v];
    const int nch = (int)((len + NORMAL_PCH - 1) / NORMAL_PCH);
    const double* p = P.part + (int64_t)L.slot0 * (2 * NORMAL_RHS) + c;
    double s = p[0], err = p[NORMAL_RHS];
    for (int j = 1; j < nch; ++j) {
        p += 2 * NORMAL_RHS;
        if (MODE >= NORMAL_RES_DD) {
            double q;
            normal_two_sum(s, p[0], s, q);
            err += q + p[NORMAL_RHS];
        } else {
            s += p[0];
        }
    }
    if (c >= nrhs) return;
    if (MODE >= NORMAL_RES_DD && Eout) {
        double lo;
        normal_two_sum(s, err, s, lo);
        Eout[L.v + (int64_t)c * ldr] = lo;
        R[L.v + (int64_t)c * ldr] = s;
    } else {
        R[L.v + (int64_t)c * ldr] = MODE >= NORMAL_RES_DD ? s + err : s;
    }
}

template <int MODE, bool SCALED>
hipError_t normal_prod_launch(const NormalProdPlan& P, const double* val, const double* scale, const double* xt,
                              const double* xtl, int nrhs, const double* B, int64_t ldb, const double* Ein, double* R,
                              int64_t ldr, double* Eout, hipStream_t st) {
    if (P.nvec <= 0 || P.ntask <= 0 || nrhs <= 0) return hipSuccess;
    hipLaunchKernelGGL((normal_prod_kernel<MODE, SCALED>), dim3((unsigned)((P.ntask + 15) / 16)), dim3(256), 0, st, P,
                       val, scale, xt, xtl, nrhs, B, ldb, Ein, R, ldr, Eout);
    if (P.nlong > 0)
        hipLaunchKernelGGL(normal_prod_combine_kernel<MODE>, dim3((unsigned)((P.nlong + 15) / 16)), dim3(256), 0, st, P,
                           nrhs, R, ldr, Eout);
    return hipGetLastError();
}

// bval[nC + i] = d_i + lambda: the diagonal part of the base, behind C's values
__global__ __launch_bounds__(256) void normal_shift_kernel(double* __restrict__ out, const double* __restrict__ d,
                                                           double lambda, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (d ? d[i] : 0.0) + lambda;
}

// part[NORMAL_RHS g + c] = sum of w_i R(i, c)^2 over workgroup g's rows (256 g + t, then every
// 256 NORMAL_NG-th): a lane's rows in ascending order by fma, the 256 lanes by halving
__global__ __launch_bounds__(256) void normal_wnorm_kernel(const double* __restrict__ R, int64_t ldr,
                                                           const double* __restrict__ w, int64_t m, int nrhs,
                                                           double* __restrict__ part) {
    __shared__ double red[256];
    const int c = blockIdx.y;
    double s = 0.0;
    if (c < nrhs)
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)NORMAL_NG * 256) {
            const double r = R[i + (int64_t)c * ldr];
            s = fma(w ? w[i] * r : r, r, s);
        }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x * NORMAL_RHS + c] = red[0];
}

// out[c] = the partials of column c in workgroup order
__global__ void normal_wnorm_final_kernel(const double* __restrict__ part, double* __restrict__ out) {
    const int c = threadIdx.x;
    if (c >= NORMAL_RHS) return;
    double s = part[c];
    for (int g = 1; g < NORMAL_NG; ++g) s += part[g * NORMAL_RHS + c];
    out[c] = s;
}

}  // namespace

hipError_t launch_normal_shift(double* out, const double* d, double lambda, int64_t n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(normal_shift_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out, d, lambda, n);
    return hipGetLastError();
}

hipError_t launch_normal_wnorm(const double* R, int64_t ldr, const double* w, int64_t m, int nrhs, double* part,
                               double* out, hipStream_t st) {
    hipLaunchKernelGGL(normal_wnorm_kernel, dim3(NORMAL_NG, NORMAL_RHS), dim3(256), 0, st, R, ldr, w, m, nrhs, part);
    hipLaunchKernelGGL(normal_wnorm_final_kernel, dim3(1), dim3(64), 0, st, part, out);
    return hipGetLastError();
}

hipError_t launch_normal_form(const NormalFormPlan& P, const double* Jx, const double* w, const double* Cx,
                              const double* d, double lambda, double* Sx, hipStream_t st) {
    if (P.ne <= 0) return hipSuccess;
    const int64_t gs = std::min<int64_t>((P.ne + 255) / 256, 8192);
    hipLaunchKernelGGL(normal_form_short_kernel, dim3((unsigned)gs), dim3(256), 0, st, P, Jx, w, Cx, d, lambda, Sx);
    if (P.ntask > 0) {
        const int per = 256 / NORMAL_LANES;
        hipLaunchKernelGGL(normal_form_group_kernel, dim3((unsigned)((P.ntask + per - 1) / per)), dim3(256), 0, st, P,
                           Jx, w, Cx, d, lambda, Sx);
    }
    if (P.nlong > 0)
        hipLaunchKernelGGL(normal_form_combine_kernel, dim3((unsigned)((P.nlong + 255) / 256)), dim3(256), 0, st, P, Cx,
                           d, lambda, Sx);
    return hipGetLastError();
}

hipError_t launch_normal_mult(const NormalProdPlan& P, const double* Jx, const double* w, const double* yt, int nrhs,
                              double* G, int64_t ldg, hipStream_t st) {
    if (nrhs < 0 || nrhs > NORMAL_RHS) return hipErrorInvalidValue;
    return normal_prod_launch<NORMAL_MUL, true>(P, Jx, w, yt, nullptr, nrhs, nullptr, 0, nullptr, G, ldg, nullptr, st);
}

hipError_t launch_normal_mult_dd(const NormalProdPlan& P, const double* Jx, const double* w, const double* yt,
                                 const double* ytl, int nrhs, double* G, double* Gl, int64_t ldg, hipStream_t st) {
    if (nrhs < 0 || nrhs > NORMAL_RHS || !ytl || !Gl) return hipErrorInvalidValue;
    return normal_prod_launch<NORMAL_MULT_DD, true>(P, Jx, w, yt, ytl, nrhs, nullptr, 0, nullptr, G, ldg, Gl, st);
}

hipError_t launch_normal_mul(const NormalProdPlan& P, int mode, const double* val, const double* xt, int nrhs,
                             const double* B, int64_t ldb, const double* Ein, double* R, int64_t ldr, double* Eout,
                             hipStream_t st) {
    if (nrhs < 0 || nrhs > NORMAL_RHS) return hipErrorInvalidValue;
    switch (mode) {
        case NORMAL_MUL:
            return normal_prod_launch<NORMAL_MUL, false>(P, val, nullptr, xt, nullptr, nrhs, B, ldb, nullptr, R, ldr,
                                                         nullptr, st);
        case NORMAL_RES_FP64:
            return normal_prod_launch<NORMAL_RES_FP64, false>(P, val, nullptr, xt, nullptr, nrhs, B, ldb, nullptr, R,
                                                              ldr, nullptr, st);
        case NORMAL_RES_DD:
            return normal_prod_launch<NORMAL_RES_DD, false>(P, val, nullptr, xt, nullptr, nrhs, B, ldb, Ein, R, ldr,
                                                            Eout, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace sc
