// Selected inversion: the entries of Z = (P A P^T)^-1 on the pattern of L, by the
// Takahashi recurrence over the supernodal factor.
//
// Internal numbering (etree postorder).  Front s: rows[0..m), pivots at positions [0, w),
// mb = m - w rows below.  For a 128-column block K = [k0, k1) of the pivots, R = front
// positions [k1, m) and X = inv(L_KK):
//   W = L_RK X,   Z_RK = -Z_RR W,   Z_KK = X^T X - W^T Z_RK.
// Z_RR is the front's own Z columns of the later pivots plus Z_II, the mb x mb block over
// the contribution-block rows, every entry of which belongs to an ancestor's front.  So
// the blocks of a front run last to first and the fronts top-down: the order of the
// backward solve.
//
// Storage.  Z lives in a second panel arena with gpanel's layout (the w x w pivot square
// holds both triangles); L is only read.  Z_II(s) lives in s's contribution-block region
// of the work arena.  The memory plan gives that region the lifetime [level(s),
// level(parent)] (plan_check verifies that it is live through the parent's level), and the
// top-down sweep needs it from the parent's level, where it is written, to level(s), where
// it is read and s's own children are served from it: the same interval walked backwards,
// so the factorization's offsets are valid as they stand.  That forces a PUSH: after a
// level's blocks, one launch copies Z_II(c) out of the front of its parent s for every
// child c of that level's fronts.  A child pulling at its own, lower level would read a
// parent region the plan may have recycled in between.
//
// The stored-inverse hazard: X is read from the strict upper triangles of L's diagonal
// blocks, which launch_solve_inv fills once per factorization and a new factorization
// overwrites; numeric_selinv runs it itself when inv_gen is stale.
#include "numeric_impl.hpp"

namespace sc {

// Per block (nb columns, nr = m - k1 rows below it):
//   W      2 nr nb^2                 (dense nr x nb x nb)
//   Z_RK   2 nr^2 nb                 (dense nr x nr x nb)
//   Z_KK   nb (nb + 1) (nb + nr)     (the lower triangle with its diagonal, K = nb + nr deep)
double selinv_flops(const Symbolic& S) {
    double f = 0.0;
    for (int32_t s = 0; s < S.ns; ++s) {
        const int64_t w = S.w(s), m = S.sn_m[s];
        for (int64_t k0 = 0; k0 < w; k0 += SOLVE_NB) {
            const int64_t nb = std::min<int64_t>(SOLVE_NB, w - k0), nr = m - k0 - nb;
            f += (double)(2 * nr * nb * nb + 2 * nr * nr * nb + nb * (nb + 1) * (nb + nr));
        }
    }
    return f;
}

void selinv_cut_block(int bi, int w, int m, int k0, int64_t& slot, SelCut& C) {
    const int nb = std::min(SOLVE_NB, w - k0), nr = m - k0 - nb;
    for (int ti = 0; ti * SEL_BM < nr; ++ti) C.tiles.push_back(make_int2(bi, ti));
    const int nch = selinv_kchunks((int64_t)nb + nr);
    for (int code : {0, 2, 3}) {  // tiles (0, 0), (1, 0), (1, 1) of the lower triangle
        if (code && nb <= 64) break;
        if (nch == 1) {
            C.kk.push_back(make_int4(bi, code, 0, -1));
            continue;
        }
        C.red.push_back(make_int4(bi, code, (int)slot, nch));
        for (int c = 0; c < nch; ++c) C.kk.push_back(make_int4(bi, code, c, (int)(slot + c)));
        slot += nch;
    }
}

void selinv_cut_push(int32_t c, int32_t s, int mbc, SelCut& C) {
    const int nt = (mbc + 63) / 64;
    for (int tj = 0; tj < nt; ++tj)
        for (int ti = 0; ti < nt; ++ti) C.push.push_back(make_int4(c, s, ti, tj));
}

static int64_t selinv_build(Numeric& N) {
    const Symbolic& S = *N.S;
    const RankMem& R = N.R[0];
    std::vector<std::vector<int32_t>> by_level((size_t)S.nlevels);
    for (int32_t s = 0; s < S.ns; ++s) by_level[S.level[s]].push_back(s);
    std::vector<SelBlk> blk;
    SelCut C;
    int64_t wmax = 1;   // W scratch: the largest step's sum of nr nb
    int64_t smax = 1;   // partial slots of the split Z_KK products: the largest step's
    for (int32_t lev = S.nlevels - 1; lev >= 0; --lev) {
        int maxw = 0;
        for (int32_t s : by_level[lev]) maxw = std::max(maxw, S.w(s));
        for (int k0 = (maxw - 1) / SOLVE_NB * SOLVE_NB; k0 >= 0 && maxw > 0; k0 -= SOLVE_NB) {
            Numeric::SelStep st {};
            st.toff = (int64_t)C.tiles.size();
            st.koff = (int64_t)C.kk.size();
            st.poff = (int64_t)C.push.size();
            st.roff = (int64_t)C.red.size();
            int64_t woff = 0, slot = 0;
            for (int32_t s : by_level[lev]) {
                const int w = S.w(s), m = S.sn_m[s];
                if (w <= k0) continue;
                const int nb = std::min(SOLVE_NB, w - k0), nr = m - k0 - nb;
                const int bi = (int)blk.size();
                blk.push_back(SelBlk {s, k0, woff});
                woff += (int64_t)nr * nb;
                selinv_cut_block(bi, w, m, k0, slot, C);
            }
            wmax = std::max(wmax, woff);
            smax = std::max(smax, slot);
            if (k0 == 0)  // the level is done: its fronts' children get their Z_II
                for (int32_t s : by_level[lev])
                    for (int32_t q = S.child_ptr[s]; q < S.child_ptr[s + 1]; ++q)
                        selinv_cut_push(S.child_list[q], s, S.mb(S.child_list[q]), C);
            st.tcount = (int32_t)((int64_t)C.tiles.size() - st.toff);
            st.kcount = (int32_t)((int64_t)C.kk.size() - st.koff);
            st.pcount = (int32_t)((int64_t)C.push.size() - st.poff);
            st.rcount = (int32_t)((int64_t)C.red.size() - st.roff);
            N.sel_steps.push_back(st);
        }
    }
    if (blk.size() > (size_t)INT32_MAX) {
        N.err = "selected inversion: more than 2^31 - 1 blocks";
        return SC_ERR_NOTIMPL;
    }
    SelBlk* d_blk = nullptr;
    TRY(upload(N, blk, d_blk));
    TRY(upload(N, C.tiles, N.d_seltile));
    TRY(upload(N, C.kk, N.d_selkk));
    TRY(upload(N, C.red, N.d_selred));
    TRY(upload(N, C.push, N.d_selpush));
    void* p = nullptr;
    // the Z panel: the panel arena's size, zeroed once (every entry is rewritten by each call)
    TRY(dalloc(N, (size_t)R.panel_total * sizeof(double), p));
    N.SEL.zpanel = (double*)p;
    HIP_TRY(hipMemsetAsync(p, 0, (size_t)R.panel_total * sizeof(double), N.stream));
    TRY(dalloc(N, (size_t)wmax * sizeof(double), p));
    N.SEL.wbuf = (double*)p;
    TRY(dalloc(N, (size_t)smax * SEL_KT * SEL_KT * sizeof(double), p));
    N.SEL.part = (double*)p;
    N.SEL.sn_start = R.P.sn_start;
    N.SEL.sn_m = R.P.sn_m;
    N.SEL.panel_off = N.d_gpo;
    N.SEL.cb_off = R.P.cb_off;
    N.SEL.rel_ptr = R.P.rel_ptr;
    N.SEL.relind = R.P.relind;
    N.SEL.lpanel = N.gpanel;
    N.SEL.zii = R.P.cb_pool;
    N.SEL.blk = d_blk;
    N.sel_ready = true;
    return SC_OK;
}

int64_t numeric_selinv(Numeric& N) {
    if (!N.factored) return SC_ERR_STATE;
    if (!N.owner.empty() || N.emulated || N.R.size() != 1) {
        N.err = "selected inversion runs on single-device handles only (the work arenas of a multi-rank or "
                "emulated handle are per rank)";
        return SC_ERR_NOTIMPL;
    }
    const int64_t st = numeric_status(N);
    if (st != SC_OK) return st;
    TRY(solve_prepare(N));
    if (N.S->n == 0) {
        N.sel_gen = N.factor_gen;
        return SC_OK;
    }
    if (!N.sel_ready) TRY(selinv_build(N));
    TRY(solve_inverses(N));
    hipStream_t s0 = N.stream;
    const SelPlan& P = N.SEL;
    // profiling: an event after every launch; the time up to it goes to the launch's class
    std::vector<hipEvent_t> ev;
    std::vector<int> cls;
    auto mark = [&](int c) -> hipError_t {
        if (!N.sel_profile) return hipSuccess;
        hipEvent_t e = nullptr;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        ev.push_back(e);
        cls.push_back(c);
        return hipEventRecord(e, s0);
    };
    hipError_t e = mark(-1);
    // eager, on the handle's stream: each step's three products, then (after a level's
    // last block) the push of that level
    for (size_t i = 0; e == hipSuccess && i < N.sel_steps.size(); ++i) {
        const Numeric::SelStep& t = N.sel_steps[i];
        e = launch_selinv_w(P, N.d_seltile + t.toff, t.tcount, s0);
        if (e == hipSuccess) e = mark(0);
        if (e == hipSuccess) e = launch_selinv_zrk(P, N.d_seltile + t.toff, t.tcount, s0);
        if (e == hipSuccess) e = mark(1);
        if (e == hipSuccess) e = launch_selinv_zkk(P, N.d_selkk + t.koff, t.kcount, N.d_selred + t.roff, t.rcount, s0);
        if (e == hipSuccess) e = mark(2);
        if (e == hipSuccess) e = launch_selinv_push(P, N.d_selpush + t.poff, t.pcount, s0);
        if (e == hipSuccess) e = mark(3);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s0);
    if (e == hipSuccess && N.sel_profile) {
        for (double& v : N.sel_ms) v = 0.0;
        for (size_t q = 1; q < ev.size(); ++q) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[q - 1], ev[q]) == hipSuccess) N.sel_ms[cls[q]] += ms;
        }
    }
    for (hipEvent_t x : ev) (void)hipEventDestroy(x);
    HIP_TRY(e);
    N.sel_gen = N.factor_gen;
    return SC_OK;
}

// the Z panel of the current factorization, computed if it is not there
int64_t selinv_ensure(Numeric& N) {
    if (N.factored && N.sel_gen == N.factor_gen && N.sel_ready) return numeric_status(N);
    return numeric_selinv(N);
}

int64_t numeric_selinv_diag_device(Numeric& N, double* d_d) {
    const int64_t st = selinv_ensure(N);
    if (st != SC_OK) return st;
    const int64_t n = N.S->n;
    if (n == 0) return SC_OK;
    // d_post = perm o post: internal column -> index in A's own order
    HIP_TRY(launch_selinv_diag(N.SEL, N.S->ns, n, N.d_post, d_d, N.stream));
    HIP_TRY(hipStreamSynchronize(N.stream));
    return SC_OK;
}

int64_t numeric_selinv_diag_host(Numeric& N, double* d) {
    const int64_t st = selinv_ensure(N);
    if (st != SC_OK) return st;
    const int64_t n = N.S->n;
    if (n == 0) return SC_OK;
    TRY(numeric_selinv_diag_device(N, N.d_sbuf));  // the solves' staging vector
    HIP_TRY(hipMemcpy(d, N.d_sbuf, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return SC_OK;
}

int64_t numeric_selinv_export(Numeric& N, int64_t* Lp, int32_t* Li, double* Zx) {
    const int64_t st = selinv_ensure(N);
    if (st != SC_OK) return st;
    const Symbolic& S = *N.S;
    std::vector<double> host;
    if (Zx) {
        const int64_t tot = N.R[0].panel_total;
        host.resize((size_t)std::max<int64_t>(tot, 1));
        if (S.n > 0)
            HIP_TRY(hipMemcpy(host.data(), N.SEL.zpanel, (size_t)tot * sizeof(double), hipMemcpyDeviceToHost));
    }
    export_L(S, Zx ? host.data() : nullptr, N.gpo.data(), Lp, Li, Zx);
    return SC_OK;
}

int64_t numeric_selinv_export_cols(Numeric& N, int64_t j0, int64_t j1, int64_t* cp, int32_t* ri, double* rx) {
    const int64_t st = selinv_ensure(N);
    if (st != SC_OK) return st;
    if (N.S->n == 0) return numeric_export_cols(N, j0, j1, cp, nullptr, nullptr);
    return numeric_export_cols(N, j0, j1, cp, ri, rx, N.SEL.zpanel);
}

}  // namespace sc
