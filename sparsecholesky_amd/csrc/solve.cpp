// Export of the supernodal factor in the reference CSC layout and the triangular
// solves on the GPU; multi-rank handles gather the panels first.
#include "numeric_impl.hpp"

namespace sc {

int64_t numeric_gather(Numeric& N) {
    if (!N.factored) return SC_ERR_STATE;
    const int64_t st = numeric_status(N);
    if (st < 0) return st;
    if (N.owner.empty()) return SC_OK;  // single device: the arena is the factor
    if (N.gather_gen == N.factor_gen) return SC_OK;
    // emulated handles: the hosted arenas, back to back, are the gathered layout
    if (!N.emulated) TRY(dist_gather_panels(N));
    // slabs of distributed panels into their owners' copies
    for (const Numeric::SlabFix& f : N.fix)
        HIP_TRY(hipMemcpy2DAsync(N.gpanel + f.dst, (size_t)f.ld * sizeof(double), N.gpanel + f.src,
                                 (size_t)f.ld * sizeof(double), (size_t)f.rows * sizeof(double), (size_t)f.cols,
                                 hipMemcpyDeviceToDevice, N.stream));
    HIP_TRY(hipStreamSynchronize(N.stream));
    N.gather_gen = N.factor_gen;
    return SC_OK;
}

int64_t numeric_export(Numeric& N, int64_t* Lp, int32_t* Li, double* Lx) {
    if (!N.factored) return SC_ERR_STATE;
    const int64_t st = numeric_status(N);
    if (st < 0) return st;
    const Symbolic& S = *N.S;
    std::vector<double> host;
    if (Lx) {
        TRY(numeric_gather(N));
        const int64_t tot = N.rank_base.back();
        host.resize((size_t)std::max<int64_t>(tot, 1));
        HIP_TRY(hipMemcpy(host.data(), N.gpanel, (size_t)tot * sizeof(double), hipMemcpyDeviceToHost));
    }
    export_L(S, Lx ? host.data() : nullptr, N.gpo.data(), Lp, Li, Lx);
    return st;
}

int64_t numeric_export_cols(Numeric& N, int64_t j0, int64_t j1, int64_t* cp, int32_t* ri, double* rx,
                            const double* pool) {
    if (!N.factored) return SC_ERR_STATE;
    const int64_t st = numeric_status(N);
    if (st < 0) return st;
    const Symbolic& S = *N.S;
    if (j0 < 0 || j1 < j0 || j1 > S.n || !cp) return SC_ERR_ARG;
    HIP_TRY(hipSetDevice(N.device));
    if (rx) TRY(numeric_gather(N));
    // per supernode touched, only the columns [lo, hi] the request needs, each copied
    // once (a column of supernode s holds rows [off, m) of its front: the copy starts
    // at the diagonal of column lo)
    std::vector<int64_t> lo, hi;
    std::vector<int32_t> touched;
    if (rx) {
        lo.assign((size_t)S.ns, INT64_MAX);
        hi.assign((size_t)S.ns, -1);
        for (int64_t j = j0; j < j1; ++j) {
            const int32_t c = S.ipost[j], s = S.sn_of[c];
            const int64_t off = c - S.sn_start[s];
            if (hi[s] < 0) touched.push_back(s);
            lo[s] = std::min(lo[s], off);
            hi[s] = std::max(hi[s], off);
        }
    }
    std::vector<int64_t> base((size_t)(rx ? S.ns : 0), -1);
    std::vector<double> buf;
    for (int32_t s : touched) {
        const int64_t m = S.sn_m[s];
        const int64_t first = lo[s] * m + lo[s], last = hi[s] * m + m;  // [first, last) in the panel
        base[s] = (int64_t)buf.size() - first;
        const size_t at = buf.size();
        buf.resize(at + (size_t)(last - first));
        HIP_TRY(hipMemcpy(buf.data() + at, (pool ? pool : N.gpanel) + N.gpo[s] + first,
                          (size_t)(last - first) * sizeof(double), hipMemcpyDeviceToHost));
    }
    int64_t tot = 0;
    cp[0] = 0;
    for (int64_t j = j0; j < j1; ++j) {
        const int32_t c = S.ipost[j], s = S.sn_of[c];
        const int64_t m = S.sn_m[s], off = c - S.sn_start[s];
        if (ri) {
            const int32_t* rows = S.rows.data() + S.rows_ptr[s];
            for (int64_t t = off; t < m; ++t) {
                ri[tot + t - off] = S.post[rows[t]];
                if (rx) rx[tot + t - off] = buf[(size_t)(base[s] + off * m + t)];
            }
        }
        tot += m - off;
        cp[j - j0 + 1] = tot;
    }
    return tot;
}

// One front's tasks of the 128-column step k0 (numeric_impl.hpp): the diagonal task with its
// ng GEMV partials, the 64-block and 128-quadrant inverse tasks, then SOLVE_ROWS rows per
// backward GEMV / forward task from the block's end down; the forward list keeps one task
// (r0 = -1) for a block with no rows below, and its first task is the writer of y.
void solve_cut_front(int32_t s, int w, int m, int k0, int64_t goff, SolveCut& C) {
    const int rb = std::min(w, k0 + SOLVE_NB);
    const int ng = rb < m ? (m - rb + SOLVE_ROWS - 1) / SOLVE_ROWS : 0;
    C.diag.push_back(make_int4(s, k0, (int)((int64_t)C.bwd.size() - goff), ng));
    C.inv64.push_back(make_int2(s, k0));
    if (w > k0 + PNB) {
        C.inv64.push_back(make_int2(s, k0 + PNB));
        C.inv128.push_back(make_int2(s, k0));
    }
    if (rb >= m) C.fwd.push_back(make_int4(s, k0, -1, 1));
    for (int r0 = rb; r0 < m; r0 += SOLVE_ROWS) {
        C.bwd.push_back(make_int4(s, k0, r0, 0));
        C.fwd.push_back(make_int4(s, k0, r0, r0 == rb ? 1 : 0));
    }
}

// ---------------- triangular solves ----------------
// A = P^T L L^T P (P = etree postorder): c = P b; L y = c (levels up); L^T x = y
// (levels down); x = P^T c.  Per level and 64-column step, over every supernode with
// w > k0: forward, one fused launch (each workgroup solves the diagonal block and
// applies its SOLVE_ROWS rows below); backward, in reverse order, the transposed
// GEMV over the rows below, then the one-wave diagonal solve.
static int64_t solve_build(Numeric& N) {
    const Symbolic& S = *N.S;
    std::vector<std::vector<int32_t>> by_level((size_t)S.nlevels);
    for (int32_t s = 0; s < S.ns; ++s) by_level[S.level[s]].push_back(s);
    SolveCut cut;
    std::vector<int2>&inv64 = cut.inv64, &inv128 = cut.inv128;
    std::vector<int4>&diag = cut.diag, &bwd = cut.bwd, &fwd = cut.fwd;
    std::vector<int32_t> gather;  // per level: the fronts with children (forward gather)
    int64_t max_g = 1;            // most GEMV workgroups in one backward step
    // internal index -> index in the caller's order (postorder, then the fill-reducing
    // permutation when one is in effect)
    std::vector<int32_t> solve_perm(S.post);
    if (!S.perm.empty())
        for (auto& v : solve_perm) v = S.perm[v];
    for (int32_t lev = 0; lev < S.nlevels; ++lev) {
        int maxw = 0;
        for (int32_t s : by_level[lev]) maxw = std::max(maxw, S.w(s));
        const int64_t g_off = (int64_t)gather.size();
        for (int32_t s : by_level[lev])
            if (S.child_ptr[s + 1] > S.child_ptr[s]) gather.push_back(s);
        for (int k0 = 0; k0 < maxw; k0 += SOLVE_NB) {
            Numeric::SolveStep st {};
            st.doff = (int64_t)diag.size();
            st.goff = (int64_t)bwd.size();
            st.foff = (int64_t)fwd.size();
            st.gaoff = g_off;
            st.gacount = k0 == 0 ? (int32_t)((int64_t)gather.size() - g_off) : 0;  // before the level's first step
            for (int32_t s : by_level[lev]) {
                const int w = S.w(s), m = S.sn_m[s];
                if (w <= k0) continue;
                solve_cut_front(s, w, m, k0, st.goff, cut);
            }
            st.dcount = (int32_t)((int64_t)diag.size() - st.doff);
            st.gcount = (int32_t)((int64_t)bwd.size() - st.goff);
            st.fcount = (int32_t)((int64_t)fwd.size() - st.foff);
            max_g = std::max<int64_t>(max_g, st.gcount);
            N.solve_steps.push_back(st);
        }
    }
    int64_t rc;
    int32_t* d_rows = nullptr;
    int64_t* d_rows_ptr = nullptr;
    N.n_sinv = (int32_t)inv64.size();
    N.n_sinv2 = (int32_t)inv128.size();
    if ((rc = upload(N, diag, N.d_sdiag)) || (rc = upload(N, inv64, N.d_sinv)) || (rc = upload(N, inv128, N.d_sinv2)) ||
        (rc = upload(N, bwd, N.d_sgemv)) || (rc = upload(N, fwd, N.d_sfwd)) || (rc = upload(N, gather, N.d_sgather)) ||
        (rc = upload(N, S.rows, d_rows)) ||
        (rc = upload(N, S.rows_ptr, d_rows_ptr)) || (rc = upload(N, solve_perm, N.d_post)))
        return rc;
    void* p = nullptr;
    if ((rc = dalloc(N, (size_t)std::max<int64_t>(S.n, 1) * 3 * sizeof(double), p))) return rc;
    N.d_sbuf = (double*)p;
    N.SP.y = N.d_sbuf + 2 * S.n;  // forward result of the fused steps
    N.SP.sn_start = N.R[0].P.sn_start;
    N.SP.sn_m = N.R[0].P.sn_m;
    N.SP.panel_off = N.d_gpo;
    N.SP.rows_ptr = d_rows_ptr;
    N.SP.rows = d_rows;
    N.SP.panel_pool = N.gpanel;
    N.SP.c = N.d_sbuf + S.n;  // internal-order work vector
    // u: each front's contribution-block rows (sum mb); part: the backward GEMV partials
    std::vector<int64_t> u_off((size_t)S.ns);
    int64_t u_tot = 0;
    for (int32_t s = 0; s < S.ns; ++s) {
        u_off[s] = u_tot;
        u_tot += S.mb(s);
    }
    int64_t* d_u_off = nullptr;
    if ((rc = upload(N, u_off, d_u_off))) return rc;
    if ((rc = dalloc(N, (size_t)std::max<int64_t>(u_tot, 1) * sizeof(double), p))) return rc;
    N.SP.u = (double*)p;
    N.u_total = u_tot;
    if ((rc = dalloc(N, (size_t)max_g * SOLVE_NB * sizeof(double), p))) return rc;
    N.SP.part = (double*)p;
    N.solve_max_g = max_g;
    N.SP.u_off = d_u_off;
    N.SP.child_ptr = N.R[0].P.child_ptr;
    N.SP.child_list = N.R[0].P.child_list;
    N.SP.rel_ptr = N.R[0].P.rel_ptr;
    N.SP.relind = N.R[0].P.relind;
    N.solve_ready = true;
    return SC_OK;
}

void numeric_drop_solve_graphs(Numeric& N) {
    for (int f = 0; f < 2; ++f)
        for (int op = 0; op < Numeric::APPLY_OPS; ++op) {
            if (N.apply_gexec[f][op]) (void)hipGraphExecDestroy(N.apply_gexec[f][op]);
            if (N.apply_graph[f][op]) (void)hipGraphDestroy(N.apply_graph[f][op]);
            N.apply_gexec[f][op] = nullptr;
            N.apply_graph[f][op] = nullptr;
        }
}

// What every sweep starts with: the whole factor in gpanel (multi-rank: collective), the
// plan built, and the captured sweeps dropped when they point at another panel pool.
int64_t solve_prepare(Numeric& N) {
    HIP_TRY(hipSetDevice(N.device));
    TRY(numeric_gather(N));  // multi-rank: every rank solves with the whole factor
    if (N.solve_ready && N.SP.panel_pool != N.gpanel) {
        N.SP.panel_pool = N.gpanel;  // gathered buffer allocated after the plan was built
        N.SPM.panel_pool = N.gpanel;
        numeric_drop_solve_graphs(N);
    }
    if (!N.solve_ready) TRY(solve_build(N));
    return SC_OK;
}

// ---------------- panel family (SOLVE_RHS right-hand sides per sweep) ----------------
// The 16-wide twins of the plan's work buffers, at the first panel sweep only.
static int64_t solve_multi_build(Numeric& N) {
    const int64_t n1 = std::max<int64_t>(N.S->n, 1);
    void* p = nullptr;
    N.SPM = N.SP;
    TRY(dalloc(N, (size_t)n1 * 3 * SOLVE_RHS * sizeof(double), p));
    N.d_mbuf = (double*)p;
    N.SPM.c = N.d_mbuf + n1 * SOLVE_RHS;
    N.SPM.y = N.d_mbuf + 2 * n1 * SOLVE_RHS;
    TRY(dalloc(N, (size_t)std::max<int64_t>(N.u_total, 1) * SOLVE_RHS * sizeof(double), p));
    N.SPM.u = (double*)p;
    TRY(dalloc(N, (size_t)N.solve_max_g * SOLVE_NB * SOLVE_RHS * sizeof(double), p));
    N.SPM.part = (double*)p;
    N.multi_ready = true;
    return SC_OK;
}

// ---------------- factor operators (sc_factor_op) ----------------
// L is the factor of P A P^T in the numbering of numeric_export; the kernels work in the
// etree postorder of that, so the L-level ops permute by post alone, where the solves'
// d_post is perm o post.  The half solves are the two halves of the solves' sweeps; the
// products are their transposes (kernels.hip).  P and P^T need perm alone, which is a
// gather by one of the two index arrays and a scatter by the other:
//   P:   c[i] = b[perm[post[i]]],  x[post[i]] = c[i]        =>  x[k] = b[perm[k]]
//   P^T: c[i] = b[post[i]],        x[perm[post[i]]] = c[i]  =>  x[perm[k]] = b[k]
int64_t apply_prepare(Numeric& N) {
    TRY(solve_prepare(N));
    if (!N.d_etpost) {
        if (N.S->perm.empty())
            N.d_etpost = N.d_post;
        else
            TRY(upload(N, N.S->post, N.d_etpost));
    }
    return SC_OK;
}

// What every entry point below starts with: a factor in good standing, then the plan
// (etpost: with the etree postorder, for the L-level ops).
static int64_t solve_begin(Numeric& N, bool etpost) {
    if (!N.factored) return SC_ERR_STATE;
    const int64_t st = numeric_status(N);
    if (st != SC_OK) return st;
    return etpost ? apply_prepare(N) : solve_prepare(N);
}

int64_t solve_inverses(Numeric& N) {
    if (N.inv_gen != N.factor_gen) {  // once per factorization
        HIP_TRY(launch_solve_inv(N.SP, N.d_sinv, N.n_sinv, N.d_sinv2, N.n_sinv2, N.stream));
        N.inv_gen = N.factor_gen;
    }
    return SC_OK;
}

// The launchers of a family's sweeps: 0 the single-vector kernels on N.SP, io the vector
// d_sbuf[0, n); 1 the panel kernels on N.SPM, io the panel d_mbuf[0, 16 n) (column-major,
// the caller's order).  permute: c <- io gathered by perm, or io <- c scattered.
using StepFn = hipError_t (*)(const SolvePlan&, const int4*, int, hipStream_t);
struct SweepFamily {
    hipError_t (*permute)(double* c, double* io, const int32_t* perm, int64_t n, bool scatter, hipStream_t st);
    hipError_t (*gather)(const SolvePlan&, const int32_t*, int, hipStream_t);
    StepFn fwd, gemv, diag;
};
static hipError_t permute_single(double* c, double* io, const int32_t* perm, int64_t n, bool scatter, hipStream_t st) {
    return scatter ? launch_permute(io, c, perm, n, true, st) : launch_permute(c, io, perm, n, false, st);
}
static const SweepFamily SWEEP[2] = {
    {permute_single, launch_solve_fwd_gather, launch_solve_fwd, launch_solve_gemv, launch_solve_diag},
    {launch_permute_multi, launch_solve_fwd_gather_multi, launch_solve_fwd_multi, launch_solve_gemv_multi,
     launch_solve_diag_multi}};

// Bottom-up pass: per level the children's u gathered, then one launch of step per
// 128-column step on the forward tasks.
static hipError_t sweep_up(const Numeric& N, const SolvePlan& P, const SweepFamily& K, StepFn step, hipStream_t s0) {
    hipError_t e = hipSuccess;
    for (size_t i = 0; e == hipSuccess && i < N.solve_steps.size(); ++i) {
        const Numeric::SolveStep& t = N.solve_steps[i];
        e = K.gather(P, N.d_sgather + t.gaoff, t.gacount, s0);
        if (e == hipSuccess) e = step(P, N.d_sfwd + t.foff, t.fcount, s0);
    }
    return e;
}

// Per step the partials over the rows below a block (gemv), then the diagonal blocks
// (diag): the steps last to first (top-down), or, up, in the forward order.
static hipError_t sweep_blocks(const Numeric& N, const SolvePlan& P, StepFn gemv, StepFn diag, bool up,
                               hipStream_t s0) {
    const size_t ns = N.solve_steps.size();
    hipError_t e = hipSuccess;
    for (size_t i = 0; e == hipSuccess && i < ns; ++i) {
        const Numeric::SolveStep& t = N.solve_steps[up ? i : ns - 1 - i];
        e = gemv(P, N.d_sgemv + t.goff, t.gcount, s0);
        if (e == hipSuccess) e = diag(P, N.d_sdiag + t.doff, t.dcount, s0);
    }
    return e;
}

// Enqueues op on the handle's stream, from the family's io and back into it.  The full
// solve permutes by d_post (perm o post), the L-level ops by the etree postorder alone.
static hipError_t sweep_enqueue(Numeric& N, int family, int32_t op) {
    const SweepFamily& K = SWEEP[family];
    const SolvePlan& P = family ? N.SPM : N.SP;
    double* io = family ? N.d_mbuf : N.d_sbuf;
    const size_t wide = (family ? SOLVE_RHS : 1) * sizeof(double);
    const int64_t n = N.S->n;
    hipStream_t s0 = N.stream;
    const int32_t* post = op == SC_OP_SOLVE_A ? N.d_post : N.d_etpost;
    auto zero_u = [&]() { return hipMemsetAsync(P.u, 0, (size_t)std::max<int64_t>(N.u_total, 1) * wide, s0); };
    hipError_t e = hipSuccess;
    switch (op) {
        case SC_OP_SOLVE_A:
        case SC_OP_SOLVE_L:
        case SC_OP_SOLVE_LT: {
            // L y = c bottom-up (c in place, y to P.y), L^T x = y top-down in place on c
            const bool up = op != SC_OP_SOLVE_LT, down = op != SC_OP_SOLVE_L;
            e = K.permute(P.c, io, post, n, false, s0);
            if (up && e == hipSuccess) e = zero_u();
            if (up && e == hipSuccess) e = sweep_up(N, P, K, K.fwd, s0);
            if (up && down && e == hipSuccess)
                e = hipMemcpyAsync(P.c, P.y, (size_t)n * wide, hipMemcpyDeviceToDevice, s0);
            if (down && e == hipSuccess) e = sweep_blocks(N, P, K.gemv, K.diag, false, s0);
            if (e == hipSuccess) e = K.permute(down ? P.c : P.y, io, post, n, true, s0);
            break;
        }
        case SC_OP_MUL_L:  // panels only; bottom-up: z in y (read-only), x accumulated in c and u
            e = family ? K.permute(P.y, io, post, n, false, s0) : hipErrorInvalidValue;
            if (e == hipSuccess) e = hipMemsetAsync(P.c, 0, (size_t)n * wide, s0);
            if (e == hipSuccess) e = zero_u();
            if (e == hipSuccess) e = sweep_up(N, P, K, launch_mul_l_multi, s0);
            if (e == hipSuccess) e = K.permute(P.c, io, post, n, true, s0);
            break;
        case SC_OP_MUL_LT:  // panels only; no front waits for another, the steps share the part buffer only
            e = family ? K.permute(P.y, io, post, n, false, s0) : hipErrorInvalidValue;
            if (e == hipSuccess) e = sweep_blocks(N, P, launch_mul_lt_gemv_multi, launch_mul_lt_diag_multi, true, s0);
            if (e == hipSuccess) e = K.permute(P.c, io, post, n, true, s0);
            break;
        default: {  // SC_OP_PERM, SC_OP_PERM_T
            const bool fwd = op == SC_OP_PERM;
            e = K.permute(P.c, io, fwd ? N.d_post : post, n, false, s0);
            if (e == hipSuccess) e = K.permute(P.c, io, fwd ? post : N.d_post, n, true, s0);
        }
    }
    return e;
}

// Runs op on the family's io: eagerly (sc_debug_solve_eager), or as the op's graph,
// captured at its first use (a single-stream chain: ~700 dependent steps per sweep at
// 128^3 replayed as one hipGraph) after the inverses a solve needs are in place.
static int64_t apply_run(Numeric& N, int family, int32_t op) {
    hipStream_t s0 = N.stream;
    if (op == SC_OP_SOLVE_A || op == SC_OP_SOLVE_L || op == SC_OP_SOLVE_LT) TRY(solve_inverses(N));
    if (N.solve_eager) {
        HIP_TRY(sweep_enqueue(N, family, op));
        return SC_OK;
    }
    hipGraphExec_t& gexec = N.apply_gexec[family][op];
    if (!gexec) {
        HIP_TRY(hipStreamBeginCapture(s0, hipStreamCaptureModeThreadLocal));
        hipError_t e = sweep_enqueue(N, family, op);
        hipGraph_t g = nullptr;
        hipError_t e2 = hipStreamEndCapture(s0, &g);
        HIP_TRY(e);
        HIP_TRY(e2);
        N.apply_graph[family][op] = g;
        HIP_TRY(hipGraphInstantiate(&gexec, g, nullptr, nullptr, 0));
    }
    HIP_TRY(hipGraphLaunch(gexec, s0));
    return SC_OK;
}

// The graphs work on the handle's own io, so each is captured once, whatever buffers the
// caller passes.  in / out: the copy kinds of the caller's B and X (device or host memory)
static int64_t apply_multi(Numeric& N, int32_t op, int32_t nrhs, const double* B, int64_t ldb, double* X, int64_t ldx,
                           hipMemcpyKind in, hipMemcpyKind out) {
    TRY(solve_begin(N, op != SC_OP_SOLVE_A));
    const int64_t n = N.S->n;
    if (n == 0 || nrhs == 0) return SC_OK;
    if (!N.multi_ready) TRY(solve_multi_build(N));
    hipStream_t s0 = N.stream;
    double* io = N.d_mbuf;
    const size_t colb = (size_t)n * sizeof(double);
    for (int32_t j0 = 0; j0 < nrhs; j0 += SOLVE_RHS) {
        const int nr = std::min<int32_t>(SOLVE_RHS, nrhs - j0);
        HIP_TRY(hipMemcpy2DAsync(io, colb, B + (int64_t)j0 * ldb, (size_t)ldb * sizeof(double), colb, (size_t)nr, in,
                                 s0));
        // a partial panel: true zero columns, never the caller's memory
        if (nr < SOLVE_RHS) HIP_TRY(hipMemsetAsync(io + (int64_t)nr * n, 0, (size_t)(SOLVE_RHS - nr) * colb, s0));
        TRY(apply_run(N, 1, op));
        HIP_TRY(hipMemcpy2DAsync(X + (int64_t)j0 * ldx, (size_t)ldx * sizeof(double), io, colb, colb, (size_t)nr, out,
                                 s0));
        // host memory: one panel staged at a time
        if (out != hipMemcpyDeviceToDevice) HIP_TRY(hipStreamSynchronize(s0));
    }
    HIP_TRY(hipStreamSynchronize(s0));
    return SC_OK;
}

int64_t numeric_apply_device_multi(Numeric& N, int32_t op, int32_t nrhs, const double* d_B, int64_t ldb, double* d_X,
                                   int64_t ldx) {
    return apply_multi(N, op, nrhs, d_B, ldb, d_X, ldx, hipMemcpyDeviceToDevice, hipMemcpyDeviceToDevice);
}

int64_t numeric_apply_host_multi(Numeric& N, int32_t op, int32_t nrhs, const double* B, int64_t ldb, double* X,
                                 int64_t ldx) {
    return apply_multi(N, op, nrhs, B, ldb, X, ldx, hipMemcpyHostToDevice, hipMemcpyDeviceToHost);
}

int64_t numeric_apply_device(Numeric& N, int32_t op, const double* d_b, double* d_x) {
    const int64_t n = N.S->n;
    // the products have panel kernels only: a panel of one column
    if (op == SC_OP_MUL_L || op == SC_OP_MUL_LT) return numeric_apply_device_multi(N, op, 1, d_b, n, d_x, n);
    TRY(solve_begin(N, op != SC_OP_SOLVE_A));
    if (n == 0) return SC_OK;
    hipStream_t s0 = N.stream;
    double* io = N.d_sbuf;
    const size_t nb = (size_t)n * sizeof(double);
    if (d_b != io) HIP_TRY(hipMemcpyAsync(io, d_b, nb, hipMemcpyDeviceToDevice, s0));
    TRY(apply_run(N, 0, op));
    if (d_x != io) HIP_TRY(hipMemcpyAsync(d_x, io, nb, hipMemcpyDeviceToDevice, s0));
    HIP_TRY(hipStreamSynchronize(s0));
    return SC_OK;
}

int64_t numeric_apply_host(Numeric& N, int32_t op, const double* b, double* x) {
    const int64_t n = N.S->n;
    if (op == SC_OP_MUL_L || op == SC_OP_MUL_LT) return numeric_apply_host_multi(N, op, 1, b, n, x, n);
    TRY(solve_begin(N, op != SC_OP_SOLVE_A));  // d_sbuf is the plan's
    const size_t nb = (size_t)n * sizeof(double);
    if (nb == 0) return SC_OK;
    HIP_TRY(hipMemcpy(N.d_sbuf, b, nb, hipMemcpyHostToDevice));
    TRY(numeric_apply_device(N, op, N.d_sbuf, N.d_sbuf));
    HIP_TRY(hipMemcpy(x, N.d_sbuf, nb, hipMemcpyDeviceToHost));
    return SC_OK;
}

// The solves are the operator SC_OP_SOLVE_A.
int64_t numeric_solve_device(Numeric& N, const double* d_b, double* d_x) {
    return numeric_apply_device(N, SC_OP_SOLVE_A, d_b, d_x);
}

int64_t numeric_solve_host(Numeric& N, const double* b, double* x) {
    return numeric_apply_host(N, SC_OP_SOLVE_A, b, x);
}

int64_t numeric_solve_device_multi(Numeric& N, int32_t nrhs, const double* d_B, int64_t ldb, double* d_X,
                                   int64_t ldx) {
    return numeric_apply_device_multi(N, SC_OP_SOLVE_A, nrhs, d_B, ldb, d_X, ldx);
}

int64_t numeric_solve_host_multi(Numeric& N, int32_t nrhs, const double* B, int64_t ldb, double* X, int64_t ldx) {
    return numeric_apply_host_multi(N, SC_OP_SOLVE_A, nrhs, B, ldb, X, ldx);
}

int64_t numeric_logdet(Numeric& N, double* logdet) {
    TRY(solve_begin(N, false));
    const int64_t n = N.S->n;
    if (n == 0) {
        *logdet = 0.0;  // the empty product
        return SC_OK;
    }
    // scratch in the single-vector plan's c and y (2 n doubles, no solve in flight): the
    // per-workgroup sums, then the result
    double* part = N.SP.c;
    double* out = part + (n + LOGDET_NT - 1) / LOGDET_NT;
    HIP_TRY(launch_logdet(N.SP, N.S->ns, n, part, out, N.stream));
    HIP_TRY(hipMemcpyAsync(logdet, out, sizeof(double), hipMemcpyDeviceToHost, N.stream));
    HIP_TRY(hipStreamSynchronize(N.stream));
    return SC_OK;
}

}  // namespace sc
