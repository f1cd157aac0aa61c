// Debug and microbenchmark hooks (sc_debug_syrk, sc_debug_syrk_ex, sc_debug_panel,
// sc_debug_updown_block, sc_debug_solve_step, sc_debug_solve_gather, sc_debug_selinv_step,
// sc_debug_selinv_push, sc_debug_extend_add, sc_debug_pcg_vec, sc_debug_eigs_gram,
// sc_debug_eigs_update, sc_debug_bench): the SYRK, panel, update / downdate, solve / factor-
// product, selected-inversion, extend-add (the two assembly kernels, the small-front kernel,
// the gathering CB SYRK), conjugate-gradient vector and eigensolver panel kernels on caller
// data, kernel ceilings on synthetic operands.
#include "numeric_impl.hpp"

namespace sc {

int64_t debug_pcg_vec(int32_t which, int32_t n, int32_t nrhs, uint32_t mask, const double* coef, double* dA,
                      int64_t lda, double* dB, int64_t ldb, const double* dC, int64_t ldc, const double* dD, int64_t ldd,
                      double* dT, double* out, std::string& err) {
    auto bad = [&](const char* what) {
        err = std::string("sc_debug_pcg_vec: ") + what;
        return (int64_t)SC_ERR_ARG;
    };
    if (which < 0 || which > 3) return bad("unknown kernel");
    if (n < 0 || nrhs < 0 || nrhs > SOLVE_RHS) return bad("n < 0 or nrhs outside [0, 16]");
    const bool sums = which <= 1, dir = which >= 2;
    if ((sums && !out) || (which != 0 && which != 3 && !coef)) return bad("null array");
    if (sums) std::fill(out, out + PCG_NQ * SOLVE_RHS, 0.0);
    if (n == 0 || nrhs == 0) return SC_OK;
    if (!dA || (!dir && !dB) || (which != 0 && !dC) || (which == 1 && !dD)) return bad("null array");
    if (lda < n || (!dir && ldb < n) || (dC && ldc < n) || (which == 1 && ldd < n))
        return bad("leading dimension below n");
    PcgCoef k {};
    if (coef) std::copy(coef, coef + SOLVE_RHS, k.v);
    double* scratch = nullptr;
    const size_t npart = (size_t)pcg_groups(n) * PCG_NQ * SOLVE_RHS, nout = PCG_NQ * SOLVE_RHS;
    if (hipMalloc((void**)&scratch, (npart + nout) * sizeof(double)) != hipSuccess) return SC_ERR_DEVMEM;
    hipError_t e;
    if (which == 0)
        e = launch_pcg_dot(dA, lda, dB, ldb, dC, ldc, n, nrhs, mask, scratch, scratch + npart, nullptr);
    else if (which == 1)
        e = launch_pcg_update(dA, lda, dB, ldb, dC, ldc, dD, ldd, n, nrhs, mask, k, scratch, scratch + npart, nullptr);
    else
        e = launch_pcg_dir(dA, lda, dC, ldc, n, nrhs, mask, k, which == 3, dT, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && sums) e = hipMemcpy(out, scratch + npart, nout * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(scratch);
    return e == hipSuccess ? SC_OK : SC_ERR_HIP;
}

namespace {

// what the two eigensolver hooks check alike; null: fine
const char* eigs_panels_bad(int32_t n, int32_t b, int32_t nb, const double* dV, int64_t ldv, int64_t vstride) {
    if (n < 0 || b < 0 || b > SOLVE_RHS) return "n < 0 or b outside [0, 16]";
    if (nb < 0 || nb > 64) return "nb outside [0, 64]";
    if (n == 0 || b == 0 || nb == 0) return nullptr;
    if (!dV) return "null array";
    if (ldv < n) return "leading dimension below n";
    if (nb > 1 && vstride < (int64_t)b * ldv) return "blocks of V closer than b columns";
    return nullptr;
}

}  // namespace

int64_t debug_eigs_gram(int32_t n, int32_t b, int32_t nb, const double* dV, int64_t ldv, int64_t vstride,
                        const double* dW, int64_t ldw, double* out, std::string& err) {
    auto bad = [&](const char* what) {
        err = std::string("sc_debug_eigs_gram: ") + what;
        return (int64_t)SC_ERR_ARG;
    };
    if (const char* w = eigs_panels_bad(n, b, nb, dV, ldv, vstride)) return bad(w);
    if (nb == 0) return SC_OK;
    if (!out) return bad("null array");
    std::fill(out, out + (size_t)nb * EIGS_TILE, 0.0);
    if (n == 0 || b == 0) return SC_OK;
    if (!dW) return bad("null array");
    if (ldw < n) return bad("leading dimension below n");
    double* scratch = nullptr;
    const size_t npart = (size_t)eigs_groups(n) * nb * EIGS_TILE, nout = (size_t)nb * EIGS_TILE;
    if (hipMalloc((void**)&scratch, (npart + nout) * sizeof(double)) != hipSuccess) return SC_ERR_DEVMEM;
    hipError_t e = launch_eigs_gram(dV, ldv, vstride, nb, dW, ldw, n, b, scratch, scratch + npart, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, scratch + npart, nout * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(scratch);
    return e == hipSuccess ? SC_OK : SC_ERR_HIP;
}

int64_t debug_eigs_update(int32_t n, int32_t b, int32_t bc, int32_t nb, double beta, double* dOut, int64_t ldo,
                          const double* dW, int64_t ldw, const double* dV, int64_t ldv, int64_t vstride,
                          const double* C, std::string& err) {
    auto bad = [&](const char* what) {
        err = std::string("sc_debug_eigs_update: ") + what;
        return (int64_t)SC_ERR_ARG;
    };
    if (const char* w = eigs_panels_bad(n, b, nb, dV, ldv, vstride)) return bad(w);
    if (bc < 0 || bc > SOLVE_RHS) return bad("bc outside [0, 16]");
    if (n == 0 || bc == 0) return SC_OK;
    if (!dOut || (beta != 0.0 && !dW) || (nb > 0 && b > 0 && !C)) return bad("null array");
    if (ldo < n || (beta != 0.0 && ldw < n)) return bad("leading dimension below n");
    double* dC = nullptr;
    const size_t nc = (size_t)std::max(nb, 1) * EIGS_TILE * sizeof(double);
    if (hipMalloc((void**)&dC, nc) != hipSuccess) return SC_ERR_DEVMEM;
    hipError_t e = nb > 0 && b > 0 ? hipMemcpy(dC, C, (size_t)nb * EIGS_TILE * sizeof(double), hipMemcpyHostToDevice)
                                   : hipSuccess;
    // no block, or blocks of no column: the sum is empty
    if (e == hipSuccess)
        e = launch_eigs_update(dOut, ldo, beta, dW, ldw, dV, ldv, vstride, b > 0 ? nb : 0, dC, n, b, bc, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipFree(dC);
    return e == hipSuccess ? SC_OK : SC_ERR_HIP;
}

int64_t debug_syrk_ex(double* dC, int ldc, const double* dA, int lda, int M, int Nn, int K, int bt, int lean, int tag,
                      int epi) {
    // every combination launch_syrk could not run as asked, and sizes whose byte offsets
    // would leave the kernels' 32-bit buffer ranges, are refused before any HIP call
    constexpr int LD_MAX = 1 << 21;
    if (!dC || !dA || M < 1 || Nn < 1 || Nn > M || K < 1 || lda < M || ldc < M || lda > LD_MAX || ldc > LD_MAX)
        return SC_ERR_ARG;
    if ((bt != SYRK_BT_SMALL && bt != SYRK_BT_LARGE) || (lean != 0 && lean != 1) || (lean && bt != SYRK_BT_SMALL) ||
        (tag != 0 && tag != 1) || (epi != 0 && epi != 1))
        return SC_ERR_ARG;
    GemmTask t {};
    t.C = dC;
    t.A = dA;
    t.ldc = ldc;
    t.lda = lda;
    t.M = M;
    t.N = Nn;
    t.K = K;
    std::vector<int2> tiles;
    append_tiles(tiles, 0, M, Nn, bt);
    xcd_order(tiles.data(), (int64_t)tiles.size());
    GemmTask* d = nullptr;
    int2* dt = nullptr;
    if (hipMalloc(&d, sizeof(GemmTask)) != hipSuccess) return SC_ERR_DEVMEM;
    if (hipMalloc(&dt, std::max<size_t>(tiles.size(), 1) * sizeof(int2)) != hipSuccess) {
        (void)hipFree(d);
        return SC_ERR_DEVMEM;
    }
    hipError_t e = hipMemcpy(d, &t, sizeof(t), hipMemcpyHostToDevice);
    if (e == hipSuccess && !tiles.empty())
        e = hipMemcpy(dt, tiles.data(), tiles.size() * sizeof(int2), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_syrk(d, dt, (int)tiles.size(), bt, tag, nullptr, epi, GatherTab {}, lean != 0);
    hipError_t e2 = hipDeviceSynchronize();
    (void)hipFree(d);
    (void)hipFree(dt);
    return (e == hipSuccess && e2 == hipSuccess) ? SC_OK : SC_ERR_HIP;
}

int64_t debug_syrk(double* dC, int ldc, const double* dA, int lda, int M, int Nn, int K) {
    if (M == 0 || Nn == 0 || K == 0) return SC_OK;  // an empty update
    // K <= 128: the lean instance (as the schedule's default syrk_lean_kmax picks it)
    return debug_syrk_ex(dC, ldc, dA, lda, M, Nn, K, SYRK_BT_SMALL, K <= 128, 0, 0);
}

namespace {

// One front (m rows, w columns, internal columns 0 .. w - 1) as a device plan over a
// caller's panel pool, with the task arrays of one 64-column step: what the panel
// microbenchmark and the panel debug hook share.
struct PanelRig {
    void *d_s = nullptr, *d_m = nullptr, *d_o = nullptr, *d_info = nullptr, *d_pt = nullptr, *d_tr = nullptr,
         *d_arr = nullptr, *d_post = nullptr;
    DevPlan P {};
    int nt = 0;
    // tr: the step's TRSM tasks; identity_post: failing pivots report through a post table
    // (internal = natural) as in a factorization, else through none (the harness numbering)
    int64_t init(double* pool, int m, int w, int k0, const std::vector<TrsmTask>& tr, bool identity_post) {
        const int32_t hs[2] = {0, w}, hm[1] = {m};
        const int64_t ho[2] = {0, (int64_t)m * w};
        const int2 pt = make_int2(0, k0);
        nt = (int)tr.size();
        if (hipMalloc(&d_s, 8) || hipMalloc(&d_m, 4) || hipMalloc(&d_o, 16) || hipMalloc(&d_info, 4) ||
            hipMalloc(&d_pt, 8) || hipMalloc(&d_tr, std::max<size_t>(1, tr.size()) * sizeof(TrsmTask)) ||
            hipMalloc(&d_arr, 4) || (identity_post && hipMalloc(&d_post, (size_t)w * 4)))
            return SC_ERR_DEVMEM;
        if (hipMemset(d_arr, 0, 4) || hipMemset(d_info, 0, 4) || hipMemcpy(d_s, hs, 8, hipMemcpyHostToDevice) ||
            hipMemcpy(d_m, hm, 4, hipMemcpyHostToDevice) || hipMemcpy(d_o, ho, 16, hipMemcpyHostToDevice) ||
            hipMemcpy(d_pt, &pt, 8, hipMemcpyHostToDevice))
            return SC_ERR_HIP;
        if (!tr.empty() && hipMemcpy(d_tr, tr.data(), tr.size() * sizeof(TrsmTask), hipMemcpyHostToDevice))
            return SC_ERR_HIP;
        if (identity_post) {
            std::vector<int32_t> id((size_t)w);
            for (int j = 0; j < w; ++j) id[(size_t)j] = j;
            if (hipMemcpy(d_post, id.data(), id.size() * 4, hipMemcpyHostToDevice)) return SC_ERR_HIP;
        }
        P.sn_start = (const int32_t*)d_s;
        P.sn_m = (const int32_t*)d_m;
        P.panel_off = (const int64_t*)d_o;
        P.info = (int32_t*)d_info;
        P.post = (const int32_t*)d_post;
        P.panel_pool = pool;
        return SC_OK;
    }
    hipError_t potrf() const { return launch_potrf_diag(P, (const int2*)d_pt, 1, nullptr); }
    hipError_t trsm(bool partial, int pre) const {
        return launch_trsm_panel(P, (const TrsmTask*)d_tr, nt, nullptr, partial, (int32_t*)d_arr, pre);
    }
    ~PanelRig() {
        for (void* p : {d_s, d_m, d_o, d_info, d_pt, d_tr, d_arr, d_post})
            if (p) (void)hipFree(p);
    }
};

}  // namespace

int64_t debug_panel(double* dF, int m, int w, int k0, int mode, int32_t* info) {
    // m * 64 * 8 bytes is the TRSM kernels' buffer range (32 bits)
    if (!dF || !info || m < 1 || m > (1 << 22) || w < 1 || w > m || k0 < 0 || k0 >= w || k0 % PNB != 0 || mode < 0 ||
        mode > 3)
        return SC_ERR_ARG;
    const int nb = std::min(PNB, w - k0), k1 = k0 + nb;
    if ((mode == 1 || mode == 2) && nb != PNB) return SC_ERR_ARG;  // the full-block TRSM kernels
    if (mode == 3 && nb == PNB) return SC_ERR_ARG;                 // the partial-block TRSM kernel
    // the step's tasks as the schedule cuts them (ScheduleBuilder::trsm_tasks): TRSM_ROWS
    // rows each from row k1 down; the fused instance keeps one task for a block with no rows
    std::vector<TrsmTask> tr;
    const int ctr = mode == 1 ? 1 : 0;
    if (mode != 0)
        for (int r0 = k1; r0 < (ctr ? std::max(m, k1 + 1) : m); r0 += TRSM_ROWS) tr.push_back(TrsmTask {0, k0, r0, m, ctr});
    PanelRig rig;
    int64_t rc = rig.init(dF, m, w, k0, tr, true);
    // the status word armed as a factorization arms it (failing pivots report by atomicMin)
    constexpr int32_t ARMED = 0x7f7f7f7f;
    if (rc == SC_OK && hipMemset(rig.d_info, 0x7f, sizeof(int32_t)) != hipSuccess) rc = SC_ERR_HIP;
    if (rc == SC_OK) {
        hipError_t e = hipSuccess;
        if (mode != 1) e = rig.potrf();
        if (e == hipSuccess && mode == 1) e = rig.trsm(false, 0);
        if (e == hipSuccess && mode == 2) e = rig.trsm(false, 2);
        if (e == hipSuccess && mode == 3) e = rig.trsm(true, 0);
        const hipError_t e2 = hipDeviceSynchronize();
        int32_t st = 0;
        const hipError_t e3 = e2 == hipSuccess ? hipMemcpy(&st, rig.d_info, 4, hipMemcpyDeviceToHost) : e2;
        if (e != hipSuccess || e2 != hipSuccess || e3 != hipSuccess)
            rc = SC_ERR_HIP;
        else
            *info = (st == ARMED || st <= 0) ? 0 : st;
    }
    return rc;
}

int64_t debug_updown_block(double* dF, int m, int w, int k0, double* dW, int sign, int32_t* info) {
    if (!dF || !dW || !info || m < 1 || m > (1 << 22) || w < 1 || w > m || k0 < 0 || k0 >= w || k0 % PNB != 0 ||
        (sign != 1 && sign != -1))
        return SC_ERR_ARG;
    // one front whose row list is the identity: dW is the workspace itself; post: none (the
    // status word numbers the panel's columns)
    const int32_t hs[2] = {0, w}, hm[1] = {m};
    const int64_t ho[1] = {0}, hrp[2] = {0, m};
    std::vector<int32_t> rows((size_t)m);
    for (int i = 0; i < m; ++i) rows[(size_t)i] = i;
    void *d_s = nullptr, *d_m = nullptr, *d_o = nullptr, *d_rp = nullptr, *d_r = nullptr, *d_t = nullptr, *d_i = nullptr;
    int64_t rc = SC_OK;
    if (hipMalloc(&d_s, 8) || hipMalloc(&d_m, 4) || hipMalloc(&d_o, 8) || hipMalloc(&d_rp, 16) ||
        hipMalloc(&d_r, (size_t)m * 4) || hipMalloc(&d_t, (size_t)UPD_K * UPD_K * sizeof(double)) || hipMalloc(&d_i, 4))
        rc = SC_ERR_DEVMEM;
    else if (hipMemcpy(d_s, hs, 8, hipMemcpyHostToDevice) || hipMemcpy(d_m, hm, 4, hipMemcpyHostToDevice) ||
             hipMemcpy(d_o, ho, 8, hipMemcpyHostToDevice) || hipMemcpy(d_rp, hrp, 16, hipMemcpyHostToDevice) ||
             hipMemcpy(d_r, rows.data(), (size_t)m * 4, hipMemcpyHostToDevice) || hipMemset(d_i, 0x7f, 4))
        rc = SC_ERR_HIP;
    if (rc == SC_OK) {
        UpdPlan P {};
        P.sn_start = (const int32_t*)d_s;
        P.sn_m = (const int32_t*)d_m;
        P.panel_off = (const int64_t*)d_o;
        P.rows_ptr = (const int64_t*)d_rp;
        P.rows = (const int32_t*)d_r;
        P.panel_pool = dF;
        P.wd = dW;
        P.tbuf = (double*)d_t;
        P.info = (int32_t*)d_i;
        P.post = nullptr;
        hipError_t e = launch_updown_block(P, 0, k0, sign, nullptr);
        if (e == hipSuccess) e = launch_updown_rows(P, 0, k0, m - std::min(w, k0 + PNB), nullptr);
        const hipError_t e2 = hipDeviceSynchronize();
        int32_t st = 0;
        const hipError_t e3 = e2 == hipSuccess ? hipMemcpy(&st, d_i, 4, hipMemcpyDeviceToHost) : e2;
        if (e != hipSuccess || e2 != hipSuccess || e3 != hipSuccess)
            rc = SC_ERR_HIP;
        else
            *info = (st == UPD_ARMED || st <= 0) ? 0 : st;
    }
    for (void* p : {d_s, d_m, d_o, d_rp, d_r, d_t, d_i})
        if (p) (void)hipFree(p);
    return rc;
}

namespace {

// Device copies of small host arrays, freed together.
struct DevArrays {
    std::vector<void*> ptrs;
    int64_t rc = SC_OK;
    void* raw(size_t bytes) {
        void* d = nullptr;
        if (rc != SC_OK) return nullptr;
        if (hipMalloc(&d, std::max<size_t>(bytes, 8)) != hipSuccess) {
            rc = SC_ERR_DEVMEM;
            return nullptr;
        }
        ptrs.push_back(d);
        return d;
    }
    template <class T>
    const T* put(const std::vector<T>& h) {
        void* d = raw(h.size() * sizeof(T));
        if (d && !h.empty() && hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
            rc = SC_ERR_HIP;
        return (const T*)d;
    }
    ~DevArrays() {
        for (void* p : ptrs) (void)hipFree(p);
    }
};

}  // namespace

int64_t debug_solve_step(double* dF, int m, int w, int k0, int op, int width, double* dC, double* dY, double* dU) {
    if (!dF || !dC || !dY || m < 1 || m >= (1 << 20) || w < 1 || w > m || (!dU && m > w) || k0 < 0 || k0 >= w ||
        k0 % SOLVE_NB != 0 || op < 0 || op > 4 || (width != 1 && width != SOLVE_RHS) || (op >= 3 && width != SOLVE_RHS))
        return SC_ERR_ARG;
    // the step's tasks of the one front, as solve_build cuts them
    SolveCut cut;
    solve_cut_front(0, w, m, k0, 0, cut);
    std::vector<int32_t> rows((size_t)m);
    for (int i = 0; i < m; ++i) rows[(size_t)i] = i;
    DevArrays A;
    SolvePlan P {};
    P.sn_start = A.put(std::vector<int32_t> {0, w});
    P.sn_m = A.put(std::vector<int32_t> {m});
    P.panel_off = A.put(std::vector<int64_t> {0});
    P.rows_ptr = A.put(std::vector<int64_t> {0, m});
    P.rows = A.put(rows);
    P.u_off = A.put(std::vector<int64_t> {0});
    P.panel_pool = dF;
    P.c = dC;
    P.y = dY;
    P.u = dU;
    P.part = (double*)A.raw(std::max<size_t>(cut.bwd.size(), 1) * SOLVE_NB * (size_t)width * sizeof(double));
    const int2 *d_i64 = A.put(cut.inv64), *d_i128 = A.put(cut.inv128);
    const int4 *d_diag = A.put(cut.diag), *d_bwd = A.put(cut.bwd), *d_fwd = A.put(cut.fwd);
    if (A.rc != SC_OK) return A.rc;
    const int nf = (int)cut.fwd.size(), ng = (int)cut.bwd.size(), nd = (int)cut.diag.size();
    const bool one = width == 1;
    hipError_t e = hipSuccess;
    switch (op) {
        case 0: e = launch_solve_inv(P, d_i64, (int)cut.inv64.size(), d_i128, (int)cut.inv128.size(), nullptr); break;
        case 1: e = one ? launch_solve_fwd(P, d_fwd, nf, nullptr) : launch_solve_fwd_multi(P, d_fwd, nf, nullptr); break;
        case 2:
            e = one ? launch_solve_gemv(P, d_bwd, ng, nullptr) : launch_solve_gemv_multi(P, d_bwd, ng, nullptr);
            if (e == hipSuccess)
                e = one ? launch_solve_diag(P, d_diag, nd, nullptr) : launch_solve_diag_multi(P, d_diag, nd, nullptr);
            break;
        case 3: e = launch_mul_l_multi(P, d_fwd, nf, nullptr); break;
        default:
            e = launch_mul_lt_gemv_multi(P, d_bwd, ng, nullptr);
            if (e == hipSuccess) e = launch_mul_lt_diag_multi(P, d_diag, nd, nullptr);
    }
    const hipError_t e2 = hipDeviceSynchronize();
    return (e == hipSuccess && e2 == hipSuccess) ? SC_OK : SC_ERR_HIP;
}

int64_t debug_solve_gather(int width, int w, int mb, int nchild, const int64_t* rel_ptr, const int32_t* relind,
                           const double* dUc, double* dC, double* dU) {
    if ((width != 1 && width != SOLVE_RHS) || w < 1 || mb < 0 || (int64_t)w + mb >= (1 << 20) || nchild < 0 ||
        nchild > (1 << 20) || !rel_ptr || !dC || (!dU && mb > 0) || rel_ptr[0] != 0)
        return SC_ERR_ARG;
    for (int q = 0; q < nchild; ++q)
        if (rel_ptr[q + 1] < rel_ptr[q] || rel_ptr[q + 1] - rel_ptr[q] > w + mb) return SC_ERR_ARG;  // injective: <= w + mb
    const int64_t tot = rel_ptr[nchild];
    if (tot > 0 && (!relind || !dUc)) return SC_ERR_ARG;
    {
        std::vector<int32_t> seen((size_t)(w + mb), -1);
        for (int q = 0; q < nchild; ++q)
            for (int64_t i = rel_ptr[q]; i < rel_ptr[q + 1]; ++i) {
                const int32_t t = relind[i];
                if (t < 0 || t >= w + mb || seen[(size_t)t] == q) return SC_ERR_ARG;
                seen[(size_t)t] = q;
            }
    }
    // supernodes 0 .. nchild - 1 the children (only their u and relind are looked at), nchild
    // the parent; u: the children's entries back to back, then the parent's mb rows
    const int ns = nchild + 1;
    std::vector<int32_t> sn_start((size_t)ns + 1, 0), child_ptr((size_t)ns + 1, 0), child_list((size_t)nchild);
    std::vector<int64_t> rows_ptr((size_t)ns + 1, 0), u_off((size_t)ns), relp((size_t)ns + 1);
    std::vector<int32_t> rows((size_t)(w + mb)), front {nchild};
    sn_start[(size_t)ns] = w;
    rows_ptr[(size_t)ns] = w + mb;
    child_ptr[(size_t)ns] = nchild;
    for (int q = 0; q < nchild; ++q) {
        child_list[(size_t)q] = q;
        u_off[(size_t)q] = rel_ptr[q];
        relp[(size_t)q] = rel_ptr[q];
    }
    u_off[(size_t)nchild] = tot;
    relp[(size_t)nchild] = relp[(size_t)ns] = tot;
    for (int i = 0; i < w + mb; ++i) rows[(size_t)i] = i;
    DevArrays A;
    SolvePlan P {};
    P.sn_start = A.put(sn_start);
    P.rows_ptr = A.put(rows_ptr);
    P.rows = A.put(rows);
    P.u_off = A.put(u_off);
    P.child_ptr = A.put(child_ptr);
    P.child_list = A.put(child_list);
    P.rel_ptr = A.put(relp);
    P.relind = A.put(std::vector<int32_t>(relind, relind + tot));
    const int32_t* d_front = A.put(front);
    const size_t wide = (size_t)width * sizeof(double);
    double* u = (double*)A.raw((size_t)(tot + mb) * wide);
    if (A.rc != SC_OK) return A.rc;
    P.c = dC;
    P.u = u;
    if (tot > 0 && hipMemcpy(u, dUc, (size_t)tot * wide, hipMemcpyDeviceToDevice) != hipSuccess) return SC_ERR_HIP;
    if (mb > 0 && hipMemcpy(u + tot * width, dU, (size_t)mb * wide, hipMemcpyDeviceToDevice) != hipSuccess)
        return SC_ERR_HIP;
    hipError_t e = width == 1 ? launch_solve_fwd_gather(P, d_front, 1, nullptr)
                              : launch_solve_fwd_gather_multi(P, d_front, 1, nullptr);
    const hipError_t e2 = hipDeviceSynchronize();
    if (e == hipSuccess && e2 == hipSuccess && mb > 0)
        e = hipMemcpy(dU, u + tot * width, (size_t)mb * wide, hipMemcpyDeviceToDevice);
    return (e == hipSuccess && e2 == hipSuccess) ? SC_OK : SC_ERR_HIP;
}

int64_t debug_selinv_step(const double* dL, double* dZ, int m, int w, int k0, int op, const double* dZii, double* dW,
                          std::string& err) {
    auto bad = [&](const char* what) {
        err = std::string("sc_debug_selinv_step: ") + what;
        return (int64_t)SC_ERR_ARG;
    };
    if (m < 1 || m >= (1 << 20) || w < 1 || w > m) return bad("need 1 <= w <= m < 2^20");
    if (k0 < 0 || k0 >= w || k0 % SOLVE_NB != 0) return bad("k0 is not a multiple of 128 in [0, w)");
    if (op < 0 || op > 2) return bad("unknown op");
    const int nb = std::min(SOLVE_NB, w - k0), nr = m - k0 - nb;
    if (!dL || !dZ || (!dZii && m > w) || (!dW && nr > 0)) return bad("null array");
    if (op != 2 && nr == 0) return SC_OK;  // no row below the block: W and Z_RK are empty
    // the block's tasks of the one front, as selinv_build cuts them
    SelCut cut;
    int64_t slot = 0;
    selinv_cut_block(0, w, m, k0, slot, cut);
    DevArrays A;
    SelPlan P {};
    P.sn_start = A.put(std::vector<int32_t> {0, w});
    P.sn_m = A.put(std::vector<int32_t> {m});
    P.panel_off = A.put(std::vector<int64_t> {0});
    P.cb_off = A.put(std::vector<int64_t> {0});
    P.blk = A.put(std::vector<SelBlk> {SelBlk {0, k0, 0}});
    P.lpanel = dL;
    P.zpanel = dZ;
    P.zii = const_cast<double*>(dZii);  // a step only reads Z_II
    P.wbuf = dW;
    P.part = (double*)A.raw((size_t)std::max<int64_t>(slot, 1) * SEL_KT * SEL_KT * sizeof(double));
    const int2* d_tiles = A.put(cut.tiles);
    const int4 *d_kk = A.put(cut.kk), *d_red = A.put(cut.red);
    if (A.rc != SC_OK) return A.rc;
    const int nt = (int)cut.tiles.size(), nk = (int)cut.kk.size(), nred = (int)cut.red.size();
    hipError_t e;
    switch (op) {
        case 0: e = launch_selinv_w(P, d_tiles, nt, nullptr); break;
        case 1: e = launch_selinv_zrk(P, d_tiles, nt, nullptr); break;
        default: e = launch_selinv_zkk(P, d_kk, nk, d_red, nred, nullptr);
    }
    const hipError_t e2 = hipDeviceSynchronize();
    if (e != hipSuccess || e2 != hipSuccess) return SC_ERR_HIP;
    return op == 2 ? nk + nred : nt;
}

int64_t debug_selinv_push(int m, int w, const double* dZ, const double* dZii, int mbc, const int32_t* relind,
                          double* dOut, std::string& err) {
    auto bad = [&](const char* what) {
        err = std::string("sc_debug_selinv_push: ") + what;
        return (int64_t)SC_ERR_ARG;
    };
    if (m < 1 || m >= (1 << 20) || w < 1 || w > m) return bad("need 1 <= w <= m < 2^20");
    if (mbc < 0 || mbc > m) return bad("mbc outside [0, m]");
    if (mbc == 0) return SC_OK;
    if (!dZ || (!dZii && m > w) || !relind || !dOut) return bad("null array");
    for (int a = 0; a < mbc; ++a) {
        if (relind[a] < 0 || relind[a] >= m) return bad("relind outside [0, m)");
        if (a > 0 && relind[a] <= relind[a - 1]) return bad("relind is not strictly ascending");
    }
    // the kernel addresses the parent's Z_II and the child's both relative to one arena
    const uintptr_t base = (uintptr_t)(dZii ? dZii : dOut), out = (uintptr_t)dOut;
    if (base % sizeof(double) != 0 || out % sizeof(double) != 0) return bad("array not aligned to a double");
    const int64_t off = out >= base ? (int64_t)((out - base) / sizeof(double)) : -(int64_t)((base - out) / sizeof(double));
    // supernode 0 the child (one pivot, mbc rows below; only its Z_II and relind are looked
    // at), 1 the parent front (m, w)
    SelCut cut;
    selinv_cut_push(0, 1, mbc, cut);
    DevArrays A;
    SelPlan P {};
    P.sn_start = A.put(std::vector<int32_t> {0, 1, 1 + w});
    P.sn_m = A.put(std::vector<int32_t> {1 + mbc, m});
    P.panel_off = A.put(std::vector<int64_t> {0, 0});
    P.cb_off = A.put(std::vector<int64_t> {off, 0});
    P.rel_ptr = A.put(std::vector<int64_t> {0, mbc});
    P.relind = A.put(std::vector<int32_t>(relind, relind + mbc));
    P.zpanel = const_cast<double*>(dZ);  // the push only reads the parent's panel
    P.zii = (double*)base;
    const int4* d_push = A.put(cut.push);
    if (A.rc != SC_OK) return A.rc;
    const hipError_t e = launch_selinv_push(P, d_push, (int)cut.push.size(), nullptr);
    const hipError_t e2 = hipDeviceSynchronize();
    return (e == hipSuccess && e2 == hipSuccess) ? SC_OK : SC_ERR_HIP;
}

int64_t debug_extend_add(int op, int m, int w, int nchild, const int64_t* rel_ptr, const int32_t* relind,
                         const int64_t* a_ptr, const int32_t* a_pos, const int64_t* a_src, int64_t nval,
                         const double* dAx, const double* dKids, double* dPanel, double* dCb, int p0, int p1, int p2,
                         int32_t* info, std::string& err) {
    auto bad = [&](const char* what) {
        err = std::string("sc_debug_extend_add: ") + what;
        return (int64_t)SC_ERR_ARG;
    };
    // ---- everything a kernel will index with, checked on the host before any device call ----
    if (op < 0 || op > 3) return bad("unknown op");
    if (m < 1 || m > (1 << 16) || w < 1 || w > m) return bad("need 1 <= w <= m <= 65536");
    if (nchild < 0 || nchild > (1 << 16)) return bad("nchild outside [0, 65536]");
    if (!rel_ptr || !a_ptr) return bad("null array");
    if (rel_ptr[0] != 0) return bad("rel_ptr does not start at 0");
    for (int q = 0; q < nchild; ++q) {
        if (rel_ptr[q + 1] < rel_ptr[q]) return bad("rel_ptr descends");
        if (rel_ptr[q + 1] - rel_ptr[q] > m) return bad("a child has more rows than the parent");
    }
    const int64_t tot = rel_ptr[nchild];
    if (tot > 0 && !relind) return bad("null array");
    int64_t kids_len = 0;
    for (int q = 0; q < nchild; ++q) {
        for (int64_t i = rel_ptr[q]; i < rel_ptr[q + 1]; ++i) {
            if (relind[i] < 0 || relind[i] >= m) return bad("relind outside [0, m)");
            if (i > rel_ptr[q] && relind[i] <= relind[i - 1]) return bad("relind is not strictly ascending within a child");
        }
        const int64_t mbc = rel_ptr[q + 1] - rel_ptr[q];
        kids_len += mbc * mbc;
    }
    if (a_ptr[0] != 0) return bad("a_ptr does not start at 0");
    for (int j = 0; j < w; ++j)
        if (a_ptr[j + 1] < a_ptr[j]) return bad("a_ptr descends");
    const int64_t na = a_ptr[w];
    if (nval < 0) return bad("nval < 0");
    if (na > 0 && (!a_pos || !a_src)) return bad("null array");
    {
        std::vector<int32_t> seen((size_t)m, -1);
        for (int j = 0; j < w; ++j)
            for (int64_t q = a_ptr[j]; q < a_ptr[j + 1]; ++q) {
                if (a_pos[q] < j || a_pos[q] >= m) return bad("a_pos outside [j, m) of its column j");
                if (seen[(size_t)a_pos[q]] == j) return bad("a_pos names a position twice in a column");
                seen[(size_t)a_pos[q]] = j;
                if (a_src[q] < 0 || a_src[q] >= nval) return bad("a_src outside [0, nval)");
            }
    }
    const int mb = m - w;
    int ncol = m;
    bool limited = false;
    if (op <= 1) {
        ncol = p0;
        if (ncol != w && ncol != m) return bad("ncol is neither w nor m");
        if (op == 0 && (p1 != 0 || p2 != 0)) return bad("cols takes no limits");
        limited = op == 1 && !(p1 < 0 && p2 < 0);
        if (limited && (p1 < 0 || p2 < p1 || p2 > m)) return bad("limits are not 0 <= lo <= hi <= m");
    } else if (op == 2) {
        if (p0 != 32 && p0 != 64 && p0 != 88 && p0 != 96 && p0 != 128) return bad("maxm is no bucket (32, 64, 88, 96, 128)");
        if (m > p0) return bad("m above the bucket");
        if (!info) return bad("null array");
    } else {
        if (mb < 1) return bad("gather needs a contribution block (m > w)");
        if ((p0 != SYRK_BT_SMALL && p0 != SYRK_BT_LARGE) || (p1 != 0 && p1 != 1) || (p1 && p0 != SYRK_BT_SMALL) ||
            (p2 != 0 && p2 != 1))
            return bad("no such SYRK instance (bt 64 or 128, lean with 64 only, epi 0 or 1)");
    }
    if (!dPanel || (mb > 0 && !dCb) || (kids_len > 0 && !dKids) || (na > 0 && op != 3 && !dAx)) return bad("null array");
    // the kernels address the children's CBs and the parent's relative to one arena
    const uintptr_t base = (uintptr_t)(dKids ? (const void*)dKids : (const void*)dCb), out = (uintptr_t)dCb;
    if (base % sizeof(double) != 0 || out % sizeof(double) != 0 || (uintptr_t)dPanel % sizeof(double) != 0)
        return bad("array not aligned to a double");
    const int64_t off = !dCb ? 0
                             : out >= base ? (int64_t)((out - base) / sizeof(double))
                                           : -(int64_t)((base - out) / sizeof(double));
    // supernode 0 the parent front (m, w; internal columns 0 .. w - 1, so that with no post
    // table a failing pivot reports its panel column + 1), 1 + q child q (one pivot, mbc
    // rows below; only its CB and relind are looked at), children in the caller's order
    const int ns = nchild + 1;
    std::vector<int32_t> sn_start((size_t)ns + 1), sn_m((size_t)ns), child_ptr((size_t)ns + 1, nchild), child_list((size_t)nchild);
    std::vector<int64_t> panel_off((size_t)ns + 1, 0), cb_off((size_t)ns + 1, 0), relp((size_t)ns + 1, 0);
    std::vector<int64_t> rb_ptr((size_t)ns + 1, 0), cbk_ptr((size_t)ns + 1, 0), aptr((size_t)(w + nchild) + 1, na);
    std::vector<int32_t> rel_bnd, col_bnd;
    sn_start[0] = 0;
    sn_m[0] = m;
    child_ptr[0] = 0;
    cb_off[0] = off;
    int64_t koff = 0;
    for (int q = 0; q < nchild; ++q) {
        const int32_t mbc = (int32_t)(rel_ptr[q + 1] - rel_ptr[q]);
        sn_start[(size_t)q + 1] = w + q;
        sn_m[(size_t)q + 1] = 1 + mbc;
        child_list[(size_t)q] = q + 1;
        cb_off[(size_t)q + 1] = koff;
        koff += (int64_t)mbc * mbc;
        relp[(size_t)q + 1] = rel_ptr[q];
        block_bounds(relind + rel_ptr[q], mbc, 0, kAsmRows, rel_bnd);
        block_bounds(relind + rel_ptr[q], mbc, 0, kAsmCols, col_bnd);
        rb_ptr[(size_t)q + 2] = (int64_t)rel_bnd.size();
        cbk_ptr[(size_t)q + 2] = (int64_t)col_bnd.size();
    }
    sn_start[(size_t)ns] = w + nchild;
    relp[(size_t)ns] = tot;
    for (int j = 0; j <= w; ++j) aptr[(size_t)j] = a_ptr[j];
    DevArrays A;
    DevPlan P {};
    P.sn_start = A.put(sn_start);
    P.sn_m = A.put(sn_m);
    P.panel_off = A.put(panel_off);
    P.cb_off = A.put(cb_off);
    P.child_ptr = A.put(child_ptr);
    P.child_list = A.put(child_list);
    P.rel_ptr = A.put(relp);
    P.relind = A.put(std::vector<int32_t>(relind, relind + tot));
    P.rb_ptr = A.put(rb_ptr);
    P.rel_bnd = A.put(rel_bnd);
    P.cbk_ptr = A.put(cbk_ptr);
    P.col_bnd = A.put(col_bnd);
    P.a_ptr = A.put(aptr);
    P.a_pos = A.put(std::vector<int32_t>(a_pos, a_pos + na));
    P.a_src = A.put(std::vector<int64_t>(a_src, a_src + na));
    P.panel_pool = dPanel;
    P.cb_pool = (double*)base;
    P.info = (int32_t*)A.raw(sizeof(int32_t));
    P.post = nullptr;
    {  // the assembly ends at ncol, as the schedule ends a gathered front's at w
        std::vector<int32_t> asm_end(sn_m);
        asm_end[0] = ncol;
        P.asm_end = A.put(asm_end);
    }
    if (A.rc != SC_OK) return A.rc;
    // the status word armed as a factorization arms it
    if (hipMemset(P.info, 0x7f, sizeof(int32_t)) != hipSuccess) return SC_ERR_HIP;
    hipError_t e = hipSuccess;
    if (op <= 1) {
        // the front's assembly tasks as the schedule cuts them (front_asm_tasks); limits: the
        // same [lo, hi) on every task, as a distributed assembly hands one run's
        std::vector<int2> tasks;
        for (int cb = 0; cb * ASM_COLS < ncol; ++cb) asm_block_tasks(tasks, 0, cb, m, op == 1);
        const int2* d_tasks = A.put(tasks);
        const int2* d_lim = limited ? A.put(std::vector<int2>(tasks.size(), make_int2(p1, p2))) : nullptr;
        if (A.rc != SC_OK) return A.rc;
        e = launch_assemble_large(P, d_tasks, (int)tasks.size(), dAx, nullptr, op == 1, d_lim);
    } else if (op == 2) {
        const int32_t* d_nodes = A.put(std::vector<int32_t> {0});
        if (A.rc != SC_OK) return A.rc;
        e = launch_front_small(P, d_nodes, 1, p0, false, dAx, nullptr);
    } else {
        // the CB SYRK of the front as emit_cb_launches makes it: K = w over rows [w, m) of the
        // panel, the gather table of schedule.cpp's own builder
        std::vector<int64_t> gblk;
        std::vector<GSeg> gseg;
        std::vector<const double*> cbs((size_t)nchild);
        for (int q = 0; q < nchild; ++q) cbs[(size_t)q] = (const double*)base + cb_off[(size_t)q + 1];
        gather_segments_front(w, mb, child_list.data(), nchild, relp.data(), relind, P.relind, cbs.data(), gblk, gseg);
        GemmTask t {};
        t.C = dCb;
        t.A = dPanel + w;
        t.ldc = mb;
        t.lda = m;
        t.M = t.N = mb;
        t.K = w;
        t.gs = 0;
        t.gb = 0;
        t.gw = w;
        std::vector<int2> tiles;
        append_tiles(tiles, 0, mb, mb, p0);
        xcd_order(tiles.data(), (int64_t)tiles.size());
        GatherTab gt;
        gt.blk = A.put(gblk);
        gt.seg = A.put(gseg);
        gt.info = P.info;
        const GemmTask* d_task = A.put(std::vector<GemmTask> {t});
        const int2* d_tiles = A.put(tiles);
        if (A.rc != SC_OK) return A.rc;
        e = launch_syrk(d_task, d_tiles, (int)tiles.size(), p0, 1, nullptr, p2, gt, p1 != 0);
    }
    const hipError_t e2 = hipDeviceSynchronize();
    int32_t st = 0;
    const hipError_t e3 = e2 == hipSuccess ? hipMemcpy(&st, P.info, sizeof(int32_t), hipMemcpyDeviceToHost) : e2;
    if (e != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return SC_ERR_HIP;
    if (info) *info = (st == 0x7f7f7f7f || st <= 0) ? 0 : st;
    return SC_OK;
}

// Panel-kernel microbenchmarks on one synthetic front (m = M rows, w = 64):
// which 2 = POTRF (us per launch), 3 = TRSM with the fused POTRF (us per launch).
static int64_t bench_panel(int which, int M, int reps, double* out) {
    const int w = PNB;
    if (M < w || reps < 1) return SC_ERR_ARG;
    const size_t nel = (size_t)M * w;
    std::vector<double> h(nel + PNB, 0.0);
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return (double)(x >> 11) / 9007199254740992.0 - 0.5;
    };
    for (int j = 0; j < w; ++j)
        for (int i = 0; i < M; ++i) h[(size_t)j * M + i] = (i == j) ? 64.0 : rnd();
    std::vector<TrsmTask> tr;
    for (int r0 = w; r0 < M; r0 += TRSM_ROWS) tr.push_back(TrsmTask {0, 0, r0, M, 1});
    void *d_pan = nullptr, *d_ref = nullptr;
    const size_t bytes = (nel + PNB) * sizeof(double);
    int64_t rc = SC_OK;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    PanelRig rig;
    if (hipMalloc(&d_pan, bytes) || hipMalloc(&d_ref, bytes) || hipEventCreate(&e0) || hipEventCreate(&e1)) {
        rc = SC_ERR_DEVMEM;
    } else if ((rc = rig.init((double*)d_pan, M, w, 0, tr, false)) == SC_OK) {
        (void)hipMemcpy(d_ref, h.data(), bytes, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_pan, d_ref, bytes, hipMemcpyDeviceToDevice);
        (void)rig.potrf();
        double tot = 0.0;
        for (int r = 0; r < reps + 1; ++r) {
            if (which == 2) (void)hipMemcpy(d_pan, d_ref, bytes, hipMemcpyDeviceToDevice);
            (void)hipEventRecord(e0, nullptr);
            if (which == 2)
                (void)rig.potrf();
            else
                (void)rig.trsm(false, 0);
            (void)hipEventRecord(e1, nullptr);
            (void)hipEventSynchronize(e1);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            if (r > 0) tot += ms;
        }
        *out = 1e3 * tot / reps;
        if (hipGetLastError() != hipSuccess) rc = SC_ERR_HIP;
    }
    for (void* p : {d_pan, d_ref})
        if (p) (void)hipFree(p);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

// Dispatch-contention probe (the chain-vs-lookahead question of DESIGN.md 5): a "hog" --
// the 128-tile panel-update SYRK (TAG 0, trickle epilogue) on an M x M triangle, K deep,
// on a low-priority stream -- and a "chain" of nchain dependent fused POTRF + TRSM
// launches on a chain_rows x 64 front, on the high-priority stream.  mode bit 0: the hog
// stream is CU-masked (every mask_stride-th CU off); bit 1: the hog is replayed from a
// captured hipGraph; bit 2: the chain too (its own graph).  out[0] chain alone, out[1] hog
// alone, out[2] chain under the hog (first chain start -> last chain end), out[3] hog
// under the chain, out[4] both (wall), all ms; out[5] CUs the hog may use.
int64_t debug_contention(int M, int K, int chain_rows, int nchain, int mode, int mask_stride, double* out) {
    for (int i = 0; i < 8; ++i) out[i] = 0.0;
    if (M < 128 || K < 16 || chain_rows < 128 || nchain < 1 || nchain > 4096) return SC_ERR_ARG;
    int64_t rc = SC_OK;
    hipStream_t s_chain = nullptr, s_hog = nullptr;
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    hipDeviceProp_t prop {};
    (void)hipGetDeviceProperties(&prop, 0);
    const int ncu = prop.multiProcessorCount;
    int used = ncu;
    if (hipStreamCreateWithPriority(&s_chain, hipStreamNonBlocking, prio_hi) != hipSuccess) return SC_ERR_HIP;
    if (mode & 1) {
        std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
        used = 0;
        for (int c = 0; c < ncu; ++c)
            if (mask_stride <= 0 || c % mask_stride != 0) {
                mask[c / 32] |= 1u << (c % 32);
                ++used;
            }
        if (hipExtStreamCreateWithCUMask(&s_hog, (uint32_t)mask.size(), mask.data()) != hipSuccess) rc = SC_ERR_HIP;
    } else if (hipStreamCreateWithPriority(&s_hog, hipStreamNonBlocking, prio_lo) != hipSuccess) {
        rc = SC_ERR_HIP;
    }
    out[5] = used;
    // hog operands
    const size_t na = (size_t)M * K, nc = (size_t)M * M;
    void *bufA = nullptr, *bufC = nullptr, *bt = nullptr, *bl = nullptr;
    int ntiles = 0;
    // chain front (as bench_panel)
    const int w = PNB, Mc = chain_rows;
    const size_t nel = (size_t)Mc * w;
    void *d_pan = nullptr, *d_s = nullptr, *d_m = nullptr, *d_o = nullptr, *d_info = nullptr, *d_tr = nullptr,
         *d_arr = nullptr;
    std::vector<TrsmTask> tr;
    for (int r0 = w; r0 < Mc; r0 += TRSM_ROWS) tr.push_back(TrsmTask {0, 0, r0, Mc, 1});
    hipEvent_t ev[8] = {};
    hipGraph_t g_hog = nullptr, g_chain = nullptr;
    hipGraphExec_t x_hog = nullptr, x_chain = nullptr;
    DevPlan P {};
    auto hog_direct = [&]() { return launch_syrk((GemmTask*)bt, (int2*)bl, ntiles, SYRK_BT_LARGE, 0, s_hog); };
    auto hog = [&]() {
        if (x_hog) return hipGraphLaunch(x_hog, s_hog);
        return hog_direct();
    };
    auto chain_direct = [&]() {
        hipError_t e = hipSuccess;
        for (int i = 0; i < nchain && e == hipSuccess; ++i)
            e = launch_trsm_panel(P, (const TrsmTask*)d_tr, (int)tr.size(), s_chain, false, (int32_t*)d_arr);
        return e;
    };
    auto chain = [&]() { return x_chain ? hipGraphLaunch(x_chain, s_chain) : chain_direct(); };
    auto elapsed = [&](int a, int b) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev[a], ev[b]);
        return (double)ms;
    };
    if (rc == SC_OK) {
        if (hipMalloc(&bufA, na * 8) || hipMalloc(&bufC, nc * 8) || hipMalloc(&d_pan, (nel + PNB) * 8) ||
            hipMalloc(&d_s, 8) || hipMalloc(&d_m, 4) || hipMalloc(&d_o, 16) || hipMalloc(&d_info, 4) ||
            hipMalloc(&d_tr, tr.size() * sizeof(TrsmTask)) || hipMalloc(&d_arr, 4))
            rc = SC_ERR_DEVMEM;
    }
    if (rc == SC_OK) {
        (void)launch_fill_random((double*)bufA, (int64_t)na, nullptr);
        (void)launch_fill_random((double*)bufC, (int64_t)nc, nullptr);
        GemmTask t {};
        t.C = (double*)bufC;
        t.A = (const double*)bufA;
        t.ldc = M;
        t.lda = M;
        t.M = M;
        t.N = M;
        t.K = K;
        std::vector<int2> tiles;
        append_tiles(tiles, 0, M, M, SYRK_BT_LARGE);
        xcd_order(tiles.data(), (int64_t)tiles.size());
        ntiles = (int)tiles.size();
        (void)hipMalloc(&bt, sizeof(GemmTask));
        (void)hipMalloc(&bl, tiles.size() * sizeof(int2));
        (void)hipMemcpy(bt, &t, sizeof(t), hipMemcpyHostToDevice);
        (void)hipMemcpy(bl, tiles.data(), tiles.size() * sizeof(int2), hipMemcpyHostToDevice);
        // chain front: a diagonally dominant 64-column panel
        std::vector<double> h(nel + PNB, 0.0);
        for (int j = 0; j < w; ++j)
            for (int i = 0; i < Mc; ++i) h[(size_t)j * Mc + i] = (i == j) ? 64.0 : 1e-3 * ((i * 7 + j * 3) % 11);
        int32_t hs[2] = {0, w}, hm[1] = {Mc};
        int64_t ho[2] = {0, (int64_t)nel};
        (void)hipMemcpy(d_pan, h.data(), h.size() * 8, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_s, hs, 8, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_m, hm, 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_o, ho, 16, hipMemcpyHostToDevice);
        (void)hipMemset(d_info, 0, 4);
        (void)hipMemset(d_arr, 0, 4);
        (void)hipMemcpy(d_tr, tr.data(), tr.size() * sizeof(TrsmTask), hipMemcpyHostToDevice);
        P.sn_start = (const int32_t*)d_s;
        P.sn_m = (const int32_t*)d_m;
        P.panel_off = (const int64_t*)d_o;
        P.info = (int32_t*)d_info;
        P.panel_pool = (double*)d_pan;
        for (auto& e : ev) (void)hipEventCreate(&e);
        (void)hipDeviceSynchronize();
        if (mode & 2) {  // the hog as a captured graph
            (void)hipStreamBeginCapture(s_hog, hipStreamCaptureModeThreadLocal);
            (void)hog_direct();
            (void)hipStreamEndCapture(s_hog, &g_hog);
            if (!g_hog || hipGraphInstantiate(&x_hog, g_hog, nullptr, nullptr, 0) != hipSuccess) rc = SC_ERR_HIP;
        }
        if (rc == SC_OK && (mode & 4)) {
            (void)hipStreamBeginCapture(s_chain, hipStreamCaptureModeThreadLocal);
            (void)chain_direct();
            (void)hipStreamEndCapture(s_chain, &g_chain);
            if (!g_chain || hipGraphInstantiate(&x_chain, g_chain, nullptr, nullptr, 0) != hipSuccess) rc = SC_ERR_HIP;
        }
    }
    if (rc == SC_OK) {
        // warm up both, then alone, alone, together (best of 3 for each)
        (void)hog();
        (void)chain();
        (void)hipDeviceSynchronize();
        double best[5] = {1e30, 1e30, 1e30, 1e30, 1e30};
        for (int rep = 0; rep < 3; ++rep) {
            (void)hipEventRecord(ev[0], s_chain);
            (void)chain();
            (void)hipEventRecord(ev[1], s_chain);
            (void)hipDeviceSynchronize();
            best[0] = std::min(best[0], elapsed(0, 1));
            (void)hipEventRecord(ev[2], s_hog);
            (void)hog();
            (void)hipEventRecord(ev[3], s_hog);
            (void)hipDeviceSynchronize();
            best[1] = std::min(best[1], elapsed(2, 3));
            // together: the hog first (its workgroups fill the GPU), the chain right after
            (void)hipEventRecord(ev[2], s_hog);
            (void)hog();
            (void)hipEventRecord(ev[3], s_hog);
            (void)hipStreamWaitEvent(s_chain, ev[2], 0);
            (void)hipEventRecord(ev[0], s_chain);
            (void)chain();
            (void)hipEventRecord(ev[1], s_chain);
            (void)hipDeviceSynchronize();
            best[2] = std::min(best[2], elapsed(0, 1));
            best[3] = std::min(best[3], elapsed(2, 3));
            best[4] = std::min(best[4], std::max(elapsed(2, 1), elapsed(2, 3)));
        }
        for (int i = 0; i < 5; ++i) out[i] = best[i];
        if (hipGetLastError() != hipSuccess) rc = SC_ERR_HIP;
    }
    (void)hipDeviceSynchronize();
    if (x_hog) (void)hipGraphExecDestroy(x_hog);
    if (g_hog) (void)hipGraphDestroy(g_hog);
    if (x_chain) (void)hipGraphExecDestroy(x_chain);
    if (g_chain) (void)hipGraphDestroy(g_chain);
    for (void* p : {bufA, bufC, bt, bl, d_pan, d_s, d_m, d_o, d_info, d_tr, d_arr})
        if (p) (void)hipFree(p);
    for (auto e : ev)
        if (e) (void)hipEventDestroy(e);
    if (s_chain) (void)hipStreamDestroy(s_chain);
    if (s_hog) (void)hipStreamDestroy(s_hog);
    return rc;
}

// which 0: register-only fp64 MFMA peak probe (M blocks of 4 waves, K iterations,
// arg accumulators); 1 / 5: the SYRK kernel on an M x M triangle, K deep, tile arg
// (64 / 128), with / without the XCD tile order; 2 / 3: bench_panel.  TFLOP/s or us.
int64_t debug_bench(int which, int M, int K, int reps, int arg, double* tflops) {
    *tflops = 0.0;
    if (which == 2 || which == 3) return bench_panel(which, M, reps, tflops);
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return SC_ERR_HIP;
    double flops = 0.0;
    void *bufA = nullptr, *bufC = nullptr, *bt = nullptr, *bl = nullptr;
    int64_t rc = SC_OK;
    if (which == 0) {
        if (hipMalloc(&bufC, 8 * (size_t)std::max(M, 1)) != hipSuccess) return SC_ERR_DEVMEM;
        (void)launch_mfma_peak((double*)bufC, M, K, arg, nullptr);
        (void)hipDeviceSynchronize();
        (void)hipEventRecord(e0, nullptr);
        for (int r = 0; r < reps; ++r) (void)launch_mfma_peak((double*)bufC, M, K, arg, nullptr);
        (void)hipEventRecord(e1, nullptr);
        flops = 2.0 * 16 * 16 * 4 * (double)arg * K * M * 4.0 * reps;  // 4 waves per block
    } else {
        const size_t na = (size_t)M * K, nc = (size_t)M * M;
        if (hipMalloc(&bufA, na * 8) != hipSuccess || hipMalloc(&bufC, nc * 8) != hipSuccess) {
            rc = SC_ERR_DEVMEM;
            goto done;
        }
        (void)launch_fill_random((double*)bufA, (int64_t)na, nullptr);
        (void)launch_fill_random((double*)bufC, (int64_t)nc, nullptr);
        {
            GemmTask t {};
            t.C = (double*)bufC;
            t.A = (const double*)bufA;
            t.ldc = M;
            t.lda = M;
            t.M = M;
            t.N = M;
            t.K = K;
            const int tb = arg == 128 ? 128 : 64;
            std::vector<int2> tiles;
            append_tiles(tiles, 0, M, M, tb);
            if (which != 5) xcd_order(tiles.data(), (int64_t)tiles.size());
            (void)hipMalloc(&bt, sizeof(GemmTask));
            (void)hipMalloc(&bl, tiles.size() * sizeof(int2));
            (void)hipMemcpy(bt, &t, sizeof(t), hipMemcpyHostToDevice);
            (void)hipMemcpy(bl, tiles.data(), tiles.size() * sizeof(int2), hipMemcpyHostToDevice);
            (void)launch_syrk((GemmTask*)bt, (int2*)bl, (int)tiles.size(), tb, 1, nullptr);
            (void)hipDeviceSynchronize();
            (void)hipEventRecord(e0, nullptr);
            for (int r = 0; r < reps; ++r) (void)launch_syrk((GemmTask*)bt, (int2*)bl, (int)tiles.size(), tb, 1, nullptr);
            (void)hipEventRecord(e1, nullptr);
            flops = (double)M * (M + 1.0) * K * reps;
        }
    }
    {
        (void)hipEventSynchronize(e1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *tflops = flops / (ms * 1e-3) / 1e12;
        if (hipGetLastError() != hipSuccess) rc = SC_ERR_HIP;
    }
done:
    if (bufA) (void)hipFree(bufA);
    if (bufC) (void)hipFree(bufC);
    if (bt) (void)hipFree(bt);
    if (bl) (void)hipFree(bl);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

}  // namespace sc
