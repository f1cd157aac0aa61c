// Gradients on A's pattern: the derivatives of log det A and of
// X = inv(A) B with respect to the stored values of A, as arrays of the length and order of
// the caller's value array.  A stored entry a_k at (i, j), i <= j, stands for both mirrored
// positions, so
//     d logdet A / d a_k = c_k inv(A)[i, j],                c_k = 1 on the diagonal, 2 off it,
//     Abar_k = -sum_c (Bbar[i,c] X[j,c] + [i != j] Bbar[j,c] X[i,c]),   Bbar = inv(A) Xbar.
// Every inv(A)[i, j] on A's pattern lies in the Z panel of the selected inversion (A's pattern
// is inside L's), at the place the assembly writes a_k to in the L panel: the gather is the
// assembly's map a_ptr / a_pos / a_src run backwards.  The second formula is a sampled outer
// product over the list of effective entries (row, column, slot), built here from the same
// map in A's own numbering -- the entries sc_spmv_structure mirrors -- and kept in slot order.
// Slots the analysis ignores (row > column, superseded duplicates) are written +0.0.
#include "numeric_impl.hpp"

namespace sc {

namespace {

int64_t grad_build(Numeric& N) {
    const Symbolic& S = *N.S;
    const int64_t n = S.n, nnz = S.nnzA_in;
    auto nat = [&](int32_t v) -> int32_t {
        const int32_t p = S.post[v];
        return S.perm.empty() ? p : S.perm[p];
    };
    // slot -> (row, column) of the effective entries; row < 0: the slot is ignored
    std::vector<GradEntry> by_slot((size_t)nnz, GradEntry {-1, -1, 0});
    for (int32_t s = 0; s < S.ns; ++s) {
        const int32_t* rows = S.rows.data() + S.rows_ptr[s];
        for (int32_t c = S.sn_start[s]; c < S.sn_start[s + 1]; ++c) {
            const int32_t k = nat(c);
            for (int64_t q = S.a_ptr[c]; q < S.a_ptr[c + 1]; ++q) {
                const int32_t i = nat(rows[S.a_pos[q]]);
                by_slot[(size_t)S.a_src[q]] = GradEntry {std::min(i, k), std::max(i, k), S.a_src[q]};
            }
        }
    }
    std::vector<GradEntry> ent;
    std::vector<int64_t> ign;
    ent.reserve((size_t)S.nnzA_used);
    for (int64_t p = 0; p < nnz; ++p) {
        if (by_slot[(size_t)p].row >= 0)
            ent.push_back(by_slot[(size_t)p]);
        else
            ign.push_back(p);
    }
    TRY(upload(N, ent, N.d_gent));
    TRY(upload(N, ign, N.d_gign));
    N.grad_ne = (int64_t)ent.size();
    N.grad_nign = (int64_t)ign.size();
    const size_t panel = (size_t)std::max<int64_t>(n, 1) * SOLVE_RHS * sizeof(double);
    void* p = nullptr;
    TRY(dalloc(N, panel, p));
    N.d_gut = (double*)p;
    TRY(dalloc(N, panel, p));
    N.d_gvt = (double*)p;
    TRY(dalloc(N, (size_t)(grad_dot_groups(N.grad_ne) + 1) * sizeof(double), p));
    N.d_gpart = (double*)p;
    N.grad_ready = true;
    return SC_OK;
}

int64_t grad_ensure(Numeric& N) {
    HIP_TRY(hipSetDevice(N.device));
    if (!N.grad_ready) TRY(grad_build(N));
    return SC_OK;
}

// a host array of the value array's length on the device for the length of a call
int64_t stage_values(Numeric& N, DevTemp& t, const double* A, bool copy) {
    const int64_t nnz = N.S->nnzA_in;
    TRY(t.get(N, (size_t)nnz * sizeof(double)));
    if (copy && nnz > 0)
        HIP_TRY(hipMemcpyAsync(t.p, A, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, N.stream));
    return SC_OK;
}

int64_t values_out(Numeric& N, const DevTemp& t, double* A) {
    const int64_t nnz = N.S->nnzA_in;
    if (nnz > 0) HIP_TRY(hipMemcpyAsync(A, t.p, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost, N.stream));
    HIP_TRY(hipStreamSynchronize(N.stream));
    return SC_OK;
}

// the passes of the outer product on device arrays, left on the stream
int64_t outer_device(Numeric& N, double alpha, int32_t nrhs, const double* U, int64_t ldu, const double* V,
                     int64_t ldv, double beta, double* G) {
    const int64_t n = N.S->n;
    hipStream_t s0 = N.stream;
    HIP_TRY(launch_grad_zero_slots(G, N.d_gign, N.grad_nign, s0));
    // the first panel applies beta (an empty one when there are no columns), later panels add
    for (int32_t j0 = 0; j0 == 0 || j0 < nrhs; j0 += SOLVE_RHS) {
        const int nr = std::max<int32_t>(0, std::min<int32_t>(SOLVE_RHS, nrhs - j0));
        if (nr > 0) {
            HIP_TRY(launch_spmv_transpose(N.d_gut, U + (int64_t)j0 * ldu, ldu, n, nr, s0));
            HIP_TRY(launch_spmv_transpose(N.d_gvt, V + (int64_t)j0 * ldv, ldv, n, nr, s0));
        }
        HIP_TRY(launch_grad_outer(N.d_gent, N.grad_ne, N.d_gut, N.d_gvt, nr, alpha, beta, j0 == 0, G, s0));
    }
    return SC_OK;
}

}  // namespace

int64_t numeric_pattern_outer(Numeric& N, double alpha, int32_t nrhs, const double* U, int64_t ldu, const double* V,
                              int64_t ldv, double beta, double* G, bool host, const char* who) {
    TRY(single_device(N, who));
    const int64_t n = N.S->n;
    if (n == 0 || N.S->nnzA_in == 0) return SC_OK;
    TRY(grad_ensure(N));
    if (!host) {
        TRY(outer_device(N, alpha, nrhs, U, ldu, V, ldv, beta, G));
        HIP_TRY(hipStreamSynchronize(N.stream));
        return SC_OK;
    }
    DevTemp tu, tv, tg;
    TRY(stage_in(N, tu, U, ldu, n, nrhs, nrhs > 0));
    TRY(stage_in(N, tv, V, ldv, n, nrhs, nrhs > 0));
    TRY(stage_values(N, tg, G, beta != 0.0));
    TRY(outer_device(N, alpha, nrhs, (const double*)tu.p, n, (const double*)tv.p, n, beta, (double*)tg.p));
    return values_out(N, tg, G);
}

int64_t numeric_pattern_dot(Numeric& N, const double* G, const double* H, double* out, bool host, const char* who) {
    TRY(single_device(N, who));
    if (N.S->n == 0 || N.S->nnzA_in == 0) {
        *out = 0.0;
        return SC_OK;
    }
    TRY(grad_ensure(N));
    DevTemp tg, th;
    if (host) {
        TRY(stage_values(N, tg, G, true));
        TRY(stage_values(N, th, H, true));
        G = (const double*)tg.p;
        H = (const double*)th.p;
    }
    double* d_out = N.d_gpart + grad_dot_groups(N.grad_ne);
    HIP_TRY(launch_grad_dot(N.d_gent, N.grad_ne, G, H, N.d_gpart, d_out, N.stream));
    HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(double), hipMemcpyDeviceToHost, N.stream));
    HIP_TRY(hipStreamSynchronize(N.stream));
    return SC_OK;
}

int64_t numeric_logdet_grad(Numeric& N, double* G, bool host, const char* who) {
    TRY(single_device(N, who));
    const int64_t st = selinv_ensure(N);
    if (st != SC_OK) return st;
    const int64_t n = N.S->n;
    if (n == 0 || N.S->nnzA_in == 0) return SC_OK;
    TRY(grad_ensure(N));
    DevTemp tg;
    if (host) TRY(stage_values(N, tg, nullptr, false));
    double* dG = host ? (double*)tg.p : G;
    const DevPlan& P = N.R[0].P;
    HIP_TRY(launch_grad_zero_slots(dG, N.d_gign, N.grad_nign, N.stream));
    HIP_TRY(launch_grad_zgather(N.SEL, N.S->ns, n, P.a_ptr, P.a_pos, P.a_src, dG, N.stream));
    if (host) return values_out(N, tg, G);
    HIP_TRY(hipStreamSynchronize(N.stream));
    return SC_OK;
}

int64_t numeric_solve_grad(Numeric& N, int32_t nrhs, const double* Xbar, int64_t ldxb, const double* X, int64_t ldx,
                           double* Bbar, int64_t ldbb, double* G, bool host, const char* who) {
    if (!N.factored) return SC_ERR_STATE;
    TRY(single_device(N, who));
    const int64_t st = numeric_status(N);
    if (st != SC_OK) return st;
    if (N.S->n == 0) return SC_OK;
    // Bbar: the panel solve itself, bit for bit
    if (nrhs > 0)
        TRY(host ? numeric_solve_host_multi(N, nrhs, Xbar, ldxb, Bbar, ldbb)
                 : numeric_solve_device_multi(N, nrhs, Xbar, ldxb, Bbar, ldbb));
    return numeric_pattern_outer(N, -1.0, nrhs, Bbar, ldbb, X, ldx, 0.0, G, host, who);
}

}  // namespace sc
