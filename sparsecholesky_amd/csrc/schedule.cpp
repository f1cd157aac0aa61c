// Static launch schedule of the numeric factorization (host).  Per assembly-tree
// level: small fronts (register kernels, chains, tiny trees), then the large fronts'
// assembly, the 64-column POTRF / TRSM chain with recursive inner updates and
// lookahead outer updates, and the CB SYRK (K = w, the children's CB entries
// gathered per tile).  Multi-rank handles add the comm steps of the plan (dist.cpp)
// and the distributed panels' slab schedule.  Task pointers are final device
// addresses, so the whole schedule can be captured once into a hipGraph.
// ScheduleBuilder holds what the emission paths share; tests/test_schedule_digest.py pins
// what they emit.
#include "numeric_impl.hpp"

namespace sc {

void append_tiles(std::vector<int2>& out, int task, int M, int N, int bt, int G) {
    const int TM = (M + bt - 1) / bt, TN = (N + bt - 1) / bt;
    for (int sj = 0; sj < TN; sj += G)
        for (int si = sj; si < TM; si += G)
            for (int tj = sj; tj < std::min(TN, sj + G); ++tj)
                for (int ti = std::max(si, tj); ti < std::min(TM, si + G); ++ti)
                    out.push_back(make_int2(task, (ti << 16) | tj));
}

void xcd_order(int2* tiles, int64_t n) {
    if (n <= 8) return;
    std::vector<int2> src(tiles, tiles + n);
    const int64_t q = n / 8, r = n % 8;
    for (int64_t b = 0; b < n; ++b) {
        const int64_t x = b % 8, j = b / 8;
        tiles[b] = src[x * q + std::min(x, r) + j];
    }
}

// Work-balanced XCD order of a multi-task launch (workgroup b runs on XCD b % 8,
// each XCD has its own L2).  The tiles arrive task-contiguous, each task in
// supertile order.  Every task is cut into 8 contiguous chunks, one per XCD, with
// the remainders dealt round robin across tasks so that each XCD receives exactly
// its ceil((n - x) / 8) tiles; an XCD walks its chunks in decreasing K (longest
// tiles first).  With one task this is xcd_order.
void xcd_order_tasks(int2* tiles, int64_t n, const GemmTask* tasks, int ntasks) {
    if (n <= 8) return;
    std::vector<int64_t> beg((size_t)ntasks + 1, 0);
    for (int64_t i = 0; i < n; ++i) beg[(size_t)tiles[i].x + 1]++;
    for (int t = 0; t < ntasks; ++t) beg[t + 1] += beg[t];
    std::vector<int> ord((size_t)ntasks);
    for (int t = 0; t < ntasks; ++t) ord[t] = t;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return tasks[a].K > tasks[b].K; });
    std::vector<std::vector<int2>> per(8);
    int p = 0;
    for (int t : ord) {
        const int64_t nt = beg[t + 1] - beg[t], base = nt / 8, rem = nt % 8;
        int64_t off = beg[t];
        for (int x = 0; x < 8; ++x) {
            const int64_t cnt = base + (((x - p + 8) % 8) < rem ? 1 : 0);
            per[x].insert(per[x].end(), tiles + off, tiles + off + cnt);
            off += cnt;
        }
        p = (int)((p + rem) % 8);
    }
    for (int x = 0; x < 8; ++x)
        if ((int64_t)per[x].size() != (n - x + 7) / 8) return xcd_order(tiles, n);  // cannot happen
    for (int64_t b = 0; b < n; ++b) tiles[b] = per[b % 8][b / 8];
}

bool gather_segments_front(int w, int mb, const int32_t* kids, int nkids, const int64_t* rel_ptr,
                           const int32_t* relind, const int32_t* d_relind, const double* const* cb,
                           std::vector<int64_t>& gblk, std::vector<GSeg>& gseg) {
    const int nb = (mb + 63) / 64;
    bool resident = true;
    for (int rb = 0; rb < nb; ++rb)
        for (int cbk = 0; cbk <= rb; ++cbk) {
            gblk.push_back((int64_t)gseg.size());
            for (int q = 0; q < nkids; ++q) {
                const int32_t c = kids[q];
                const int32_t* rel = relind + rel_ptr[c];
                const int mbc = (int)(rel_ptr[c + 1] - rel_ptr[c]);
                auto at = [&](int x) { return (int)(std::lower_bound(rel, rel + mbc, w + x) - rel); };
                GSeg g {};
                g.ilo = at(64 * rb);
                g.ihi = at(std::min(mb, 64 * rb + 64));
                g.jlo = at(64 * cbk);
                g.jhi = at(std::min(mb, 64 * cbk + 64));
                if (g.ilo >= g.ihi || g.jlo >= g.jhi) continue;
                if (!cb[q]) {
                    resident = false;
                    continue;
                }
                g.cb = cb[q];
                g.rel = d_relind + rel_ptr[c];
                g.mbc = mbc;
                gseg.push_back(g);
            }
        }
    gblk.push_back((int64_t)gseg.size());
    return resident;
}

void asm_block_tasks(std::vector<int2>& out, int32_t s, int cb, int m, bool tiled) {
    if (!tiled) return out.push_back(make_int2(s, cb));
    for (int k = cb * ASM_COLS / ASM_ROWS; k * ASM_ROWS < m; ++k) out.push_back(make_int2(s, (k << 16) | cb));
}

namespace {

// LDS edge of a small front's launch.  88: the widest front whose 4 x 4 tiles fit one
// per thread (KT = 1, 124 VGPRs, 4 workgroups per CU; 96 needs KT = 2 at 2 per CU)
int bucket_of(int m) {
    if (m <= 32) return 32;
    if (m <= 64) return 64;
    if (m <= 88) return 88;
    if (m <= 96) return 96;
    return 128;
}

Launch make_launch(int kind, int level, int vr = 0, int var = 0) {
    Launch L {};
    L.kind = kind;
    L.level = level;
    L.vr = vr;
    L.var = var;
    return L;
}

// One SYRK task, C (an M x N lower trapezoid) -= A A^T over K columns, appended to vec
// with its flops 2 K (N M - N (N - 1) / 2) added to fl.  Empty updates are dropped
// (nullptr).
GemmTask* syrk_task(std::vector<GemmTask>& vec, double& fl, double* C, int64_t ldc, const double* A, int64_t lda,
                    int M, int Nn, int K) {
    if (M <= 0 || Nn <= 0 || K <= 0) return nullptr;
    const GemmTask t {C, A, ldc, lda, M, Nn, K};
    vec.push_back(t);
    fl += 2.0 * t.K * ((double)t.N * t.M - (double)t.N * (t.N - 1) / 2.0);
    return &vec.back();
}

// A distributed panel while it is being emitted (ScheduleBuilder::emit_dist_front)
struct DistFront {
    int32_t lev, s;
    int w, m, mb, nsl, own, nbo;
    const std::vector<int32_t>& sr;  // slab -> rank
    std::vector<int> vs;             // hosted holders
    // per hosted rank and slab k: the event after the lookahead-stream launch of step k
    std::vector<std::vector<int>> ev1;
    int c0(int k) const { return k * nbo; }
    int c1(int k) const { return std::min(w, (k + 1) * nbo); }
    int last_ev1(int v, int kmax) const {  // latest lookahead event of steps <= kmax
        for (int k = std::min(kmax, nsl - 1); k >= 0; --k)
            if (ev1[v][k] >= 0) return ev1[v][k];
        return -1;
    }
};

struct ScheduleBuilder {
    Numeric& N;
    SchedBuild& B;
    const Symbolic& S;
    const DistPlan& D;
    const bool multi;
    const int NBO;  // slab width of the panels one rank factors
    std::vector<std::vector<int32_t>> by_level;
    std::vector<int32_t> hosted_of;  // rank -> index into N.R
    // step lookup tables of the plan
    std::vector<int32_t> init_step, deliver_step;
    // early children: early_step[c][g] = the DELIVER step of column group g (-1: none; a
    // group whose columns all stay on the producer has no messages and no step)
    std::vector<std::vector<int32_t>> early_step;
    // split fronts / distributed panels: slab_step[s][k] = the steps of slab k's pieces (dist_pieces)
    std::vector<std::vector<std::vector<int32_t>>> slab_step;
    std::vector<std::vector<int>> early_ev;  // sender: event after each CB column group
    std::vector<int64_t> step_beg;
    std::vector<char> emitted;

    ScheduleBuilder(Numeric& N_, SchedBuild& B_)
        : N(N_), B(B_), S(*N_.S), D(N_.D), multi(!N_.owner.empty()),
          NBO(std::max(PNB, (S.opt.panel_nb_outer / PNB) * PNB)), by_level((size_t)S.nlevels),
          hosted_of((size_t)std::max(N_.nranks, 1), -1), deliver_step((size_t)S.nlevels, -1), early_ev((size_t)S.ns) {
        for (int32_t s = 0; s < S.ns; ++s) by_level[S.level[s]].push_back(s);
        for (size_t v = 0; v < N.R.size(); ++v) hosted_of[N.R[v].rank] = (int32_t)v;
        if (!multi) return;
        init_step.assign((size_t)S.ns, -1);
        slab_step.assign((size_t)S.ns, {});
        early_step.assign((size_t)S.ns, {});
        for (int32_t id = 0; id < (int32_t)D.steps.size(); ++id) {
            const DistStep& t = D.steps[id];
            if (t.kind == STEP_INIT) init_step[t.s] = id;
            if (t.kind == STEP_SLAB) {
                auto& ks = slab_step[t.s];
                if ((int)ks.size() <= t.k) ks.resize((size_t)t.k + 1);
                if ((int)ks[t.k].size() <= t.p) ks[t.k].resize((size_t)t.p + 1, -1);
                ks[t.k][t.p] = id;
            }
            if (t.kind == STEP_DELIVER && t.s < 0) deliver_step[t.level] = id;
            if (t.kind == STEP_DELIVER && t.s >= 0) {
                auto& es = early_step[t.s];
                if ((int)es.size() <= t.k) es.resize((size_t)t.k + 1, -1);
                es[t.k] = id;
            }
        }
        step_beg.assign(D.steps.size() + 1, 0);
        for (const DistMsg& g : D.msgs) step_beg[g.step + 1]++;
        for (size_t i = 0; i < D.steps.size(); ++i) step_beg[i + 1] += step_beg[i];
        emitted.assign(D.steps.size(), 0);
    }

    bool is_split(int32_t s) const { return multi && D.split[s] >= 0; }
    bool is_dpanel(int32_t s) const { return multi && D.pd[s] >= 0; }
    bool is_dasm(int32_t s) const { return multi && D.dasm[s]; }
    bool is_early_sender(int32_t s, int v) const { return multi && D.early[s] && D.owner[s] == N.R[v].rank; }
    // fronts whose CB SYRK gathers the children's CB entries itself (one CB launch
    // task covering the whole CB): their assembly stops at the panel columns
    bool gathers(int32_t s, int v) const {
        return S.opt.cb_gather && S.mb(s) > 0 && !is_split(s) && !is_early_sender(s, v);
    }
    bool asm_tiled(int m) const { return m >= (S.opt.asm_tile_min_m > 0 ? S.opt.asm_tile_min_m : ASM_TILE_MIN_M); }
    double* panel_of(int v, int32_t s) const { return N.R[v].P.panel_pool + N.R[v].panel_off[s]; }
    // device address of logical element (row, col) of a region on hosted rank v
    double* region_ptr(int v, int kind, int s, int row, int col, int64_t& ld) const {
        int arena = 0;
        int64_t off = 0;
        if (!region_addr(S, multi ? &D : nullptr, N.R[v], kind, s, row, col, arena, off, ld)) return nullptr;
        return (arena == 0 ? N.R[v].P.panel_pool : N.R[v].P.cb_pool) + off;
    }

    // ---- cross-stream dependencies: record an event on a stream / make a stream wait on it
    int push_sync(int kind, int strm, int ev) {
        Launch L = make_launch(kind, 0);
        L.strm = strm;
        L.count = ev;
        N.sched.push_back(L);
        return ev;
    }
    int push_record(int strm) { return push_sync(L_RECORD, strm, N.n_sync_events++); }
    void push_wait(int strm, int ev) { push_sync(L_WAIT, strm, ev); }
    // a launch over the tasks pushed to its kind's array since `off` (end: the array's size); none: no launch
    void push_range_launch(int kind, int var, int32_t lev, int v, int64_t off, size_t end) {
        Launch L = make_launch(kind, lev, v, var);
        L.off = off;
        L.count = (int32_t)((int64_t)end - off);
        if (L.count > 0) N.sched.push_back(L);
    }

    // ---- SYRK launches ----
    // algorithmic HBM bytes of one SYRK task: its operand rows once, C written once when
    // the children are gathered (plus every child's CB entries read once), else C read
    // and written
    double task_bytes(const GemmTask& t) const {
        const double pairs = (double)t.N * t.M - (double)t.N * (t.N - 1) / 2.0;
        double b = 8.0 * t.M * (double)t.K;
        if (t.gs < 0) return b + 16.0 * pairs;
        b += 8.0 * pairs;
        for (int32_t ci = S.child_ptr[t.gs]; ci < S.child_ptr[t.gs + 1]; ++ci) {
            const double mbc = S.mb(S.child_list[ci]);
            b += 8.0 * mbc * (mbc + 1.0) / 2.0;
        }
        return b;
    }

    void push_syrk_launch(int kind, int level, const std::vector<GemmTask>& tasks, int big, double flops,
                          int strm = 0) {
        if (tasks.empty()) return;
        std::vector<int2>& tiles = B.tiles;
        Launch L = make_launch(kind, level);
        L.strm = strm;
        L.off = (int64_t)B.gemm.size();
        // 128x128 tiles on 8 waves when every task is at least 256 wide (random data,
        // 16384 x 4096: 61 vs 52 TF/s for 64x64); 64x64 on 4 waves for narrow updates
        int minN = INT32_MAX, maxK = 0;
        for (auto& t : tasks) {
            minN = std::min(minN, (int)t.N);
            maxK = std::max(maxK, (int)t.K);
        }
        const bool wide = minN >= 256;
        L.bt = (S.opt.syrk_tile == 128 || (S.opt.syrk_tile == 0 && wide)) ? SYRK_BT_LARGE : SYRK_BT_SMALL;
        // CB launches of 64 < K <= syrk_lean_kmax (level 7 at 128^3) on the lean 64-tile
        // instance even when wide: 2.44 -> 2.24 ms (64-tiles up to K = 256 / 512 made levels
        // 8-10 slower, profiles/r06/ab_cb64.txt)
        if (kind == L_CB && S.opt.syrk_tile == 0 && maxK > 64 && maxK <= S.opt.syrk_lean_kmax) L.bt = SYRK_BT_SMALL;
        // instance tag (profiles): the critical path (main-stream panel updates) and the
        // short-K CB launches (levels 4-7 at 128^3) apart from the deep-K CB and the
        // lookahead stream -- the epilogue choice it used to make went with round 6's
        // staged epilogues (kernels.hip)
        L.epi = (kind == L_PANEL && strm == 0) || (kind == L_CB && maxK < SC_EPI_KMAX);
        // (CB launches with K <= 64 -- levels 4-6 at 128^3 -- are gather-bound and lose
        // more to the lean instance's smaller gather batches than they gain in occupancy)
        L.lean = L.bt == SYRK_BT_SMALL && S.opt.syrk_lean_kmax > 0 && maxK <= S.opt.syrk_lean_kmax &&
                 (kind == L_PANEL || maxK > 64);
        // panel-chain lookahead: a task whose pre-factor workgroup forms and factors the next
        // step's diagonal block (tile (0, 0), marker y = -1) -- 64 x 64 tiles, tagged epi
        for (auto& t : tasks) L.pf |= t.pf >= 0 ? 1 : 0;
        if (L.pf) {
            L.bt = SYRK_BT_SMALL;
            L.lean = 0;
            L.epi = 1;
        }
        L.toff = (int64_t)tiles.size();
        L.bytes = 0.0;
        for (size_t q = 0; q < tasks.size(); ++q) {
            const size_t first = tiles.size();
            append_tiles(tiles, (int)q, tasks[q].M, tasks[q].N, L.bt);
            if (tasks[q].pf >= 0) tiles[first].y = -1;  // append_tiles emits tile (0, 0) first
            B.gemm.push_back(tasks[q]);
            L.bytes += task_bytes(tasks[q]);
        }
        L.count = (int32_t)((int64_t)tiles.size() - L.toff);
        xcd_order_tasks(tiles.data() + L.toff, L.count, tasks.data(), (int)tasks.size());
        if (L.pf)  // the pre-factor workgroups (the longest, on the chain) are dispatched first
            std::stable_partition(tiles.begin() + L.toff, tiles.end(), [](const int2& t) { return t.y < 0; });
        L.ntasks = (int32_t)tasks.size();
        L.big = big;
        L.flops = flops;
        if (!recut_cb_tail(L, tasks)) N.sched.push_back(L);
    }

    // Deep-K CB launch on 128-tiles: every tile takes about the same time and 512 run
    // at once (two per CU), so a last partial round leaves most CUs idle for one whole
    // tile time (~2 ms at K = 8192).  Its tiles -- the last ones dispatched -- are re-cut
    // into 64 x 64 tiles in a launch of their own (up to 1024 at once, each ~1/4 of
    // the work): the tail shrinks to about a third (cb_tail_split).  Pushes L without
    // its last round and the tail launch after it; false: L is not such a launch.
    bool recut_cb_tail(Launch L, const std::vector<GemmTask>& tasks) {
        std::vector<int2>& tiles = B.tiles;
        constexpr int64_t SLOTS = 512;
        const int64_t rem = L.count % SLOTS;
        if (L.kind != L_CB || L.bt != SYRK_BT_LARGE || !S.opt.cb_tail_split || L.epi || L.count <= SLOTS || rem <= 0 ||
            rem * 4 > SLOTS * 3)
            return false;
        std::vector<int2> tail(tiles.end() - rem, tiles.end());
        tiles.resize(tiles.size() - (size_t)rem);
        L.count -= (int32_t)rem;
        std::stable_sort(tail.begin(), tail.end(), [](const int2& a, const int2& b) { return a.x < b.x; });
        Launch T = L;
        T.bt = SYRK_BT_SMALL;
        T.tail = 1;
        T.off = (int64_t)B.gemm.size();
        T.toff = (int64_t)tiles.size();
        B.gemm.insert(B.gemm.end(), tasks.begin(), tasks.end());
        double tfl = 0.0;
        for (const int2& t : tail) {
            const GemmTask& g = tasks[t.x];
            const int ti = t.y >> 16, tj = t.y & 0xffff;
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b) {
                    const int si = 2 * ti + a, sj = 2 * tj + b;
                    if (si < sj || si * SYRK_BT_SMALL >= g.M || sj * SYRK_BT_SMALL >= g.N) continue;
                    tiles.push_back(make_int2(t.x, (si << 16) | sj));
                    // lower-triangle pairs of the sub-tile, 2 K flops each
                    const int64_t i0 = (int64_t)si * SYRK_BT_SMALL, i1 = std::min<int64_t>(i0 + SYRK_BT_SMALL, g.M);
                    const int64_t j0 = (int64_t)sj * SYRK_BT_SMALL, j1 = std::min<int64_t>(j0 + SYRK_BT_SMALL, g.N);
                    int64_t pairs = 0;
                    for (int64_t j = j0; j < j1; ++j) pairs += std::max<int64_t>(0, i1 - std::max(i0, j));
                    tfl += 2.0 * g.K * (double)pairs;
                }
        }
        T.count = (int32_t)((int64_t)tiles.size() - T.toff);
        xcd_order_tasks(tiles.data() + T.toff, T.count, tasks.data(), (int)tasks.size());
        T.bytes = L.flops > 0.0 ? L.bytes * tfl / L.flops : 0.0;
        L.bytes -= T.bytes;
        T.flops = tfl;
        L.flops -= tfl;
        N.sched.push_back(L);
        N.sched.push_back(T);
        return true;
    }

    // ---- comm steps ----
    // The hosted ranks' part of comm step `id` on the comm stream (strm 2), emitted
    // once, at the first call (the sender's point in an emulated schedule).  Sends
    // wait for the main stream's work so far (their data); the main stream waits
    // for the step when it receives.  Messages keep the plan order, so every peer
    // pair posts its matching sends and receives in the same order.
    // recv_strm: the stream that consumes what the step receives (it waits for the step;
    // the main stream by default)
    void emit_comm_step(int32_t id, int send_ev = -1, int recv_strm = 0) {
        if (!multi || id < 0 || emitted[id]) return;
        emitted[id] = 1;
        CommBuild& cbld = B.cb;
        Launch L = make_launch(L_COMM, D.steps[id].level);
        L.strm = 2;
        L.step = id;
        L.off = (int64_t)N.msgs.size();
        bool any_send = false, any_recv = false;
        std::vector<int32_t> pack_d, unpack_d;  // copy descriptors of the sends / receives
        // (buffer, staging slot) of one end: the region itself when contiguous
        auto end_of = [&](int v, int kind, int s, int row, int col, int rows, int cols, bool pack, double*& buf,
                          int64_t& slot) {
            int64_t ld = 0;
            double* a = region_ptr(v, kind, s, row, col, ld);
            if (!a) return false;
            if (ld == rows || cols == 1) {
                buf = a;
                slot = -1;
                return true;
            }
            buf = nullptr;
            slot = cbld.stage_total;
            // copy tiles pack the column offset in 16 bits and the row chunk above it
            // (j | rc << 16, copy2d_kernel): a block wider than COPY_MAX_COLS goes as several
            // descriptors, each staging its columns at their packed position in the slot
            if ((int64_t)rows > (int64_t)COPY_ROWS * 32767) {
                N.err = "comm plan: block too tall for the copy tiles";
                return false;
            }
            for (int c0 = 0; c0 < cols; c0 += COPY_MAX_COLS) {
                (pack ? pack_d : unpack_d).push_back((int32_t)cbld.copies.size());
                cbld.copies.push_back(Copy2D {a + (int64_t)c0 * ld, nullptr, ld, rows, std::min(COPY_MAX_COLS, cols - c0)});
                cbld.copy_slot.push_back(slot + (int64_t)c0 * rows);
            }
            cbld.stage_total += (int64_t)rows * cols;
            return true;
        };
        for (int64_t q = step_beg[id]; q < step_beg[id + 1]; ++q) {
            const DistMsg& g = D.msgs[q];
            const int vs = hosted_of[g.src], vd = hosted_of[g.dst];
            if (vs < 0 && vd < 0) continue;
            const int64_t cnt = (int64_t)g.rows * g.cols;
            double *sb = nullptr, *db = nullptr;
            int64_t ss = -1, ds = -1;
            if (vs >= 0 && !end_of(vs, g.skind, g.s, g.srow, g.scol, g.rows, g.cols, true, sb, ss)) {
                N.err = "comm plan: send region missing";
                return;
            }
            if (vd >= 0 && !end_of(vd, g.dkind, g.s, g.drow, g.dcol, g.rows, g.cols, false, db, ds)) {
                N.err = "comm plan: receive region missing";
                return;
            }
            any_send |= vs >= 0;
            any_recv |= vd >= 0;
            auto push = [&](double* b, int64_t slot, double* src, int64_t src_slot, int peer, int op) {
                N.msgs.push_back(Msg {b, src, cnt, peer, op});
                cbld.msg_slot.push_back(slot);
                cbld.msg_src_slot.push_back(src_slot);
            };
            if (vs >= 0 && vd >= 0) {  // both ends in this process (emulated ranks)
                if (N.emul_rccl) {
                    push(sb, ss, nullptr, -1, 0, MSG_SEND);
                    push(db, ds, nullptr, -1, 0, MSG_RECV);
                } else {
                    push(db, ds, sb, ss, 0, MSG_COPY);
                }
            } else if (vs >= 0) {
                push(sb, ss, nullptr, -1, g.dst, MSG_SEND);
            } else {
                push(db, ds, nullptr, -1, g.src, MSG_RECV);
            }
        }
        L.count = (int32_t)((int64_t)N.msgs.size() - L.off);
        if (L.count == 0) return;
        auto add_tiles = [&](const std::vector<int32_t>& ds) {
            for (int32_t d : ds)
                for (int j = 0; j < cbld.copies[d].cols; j += COPY_COLS)
                    for (int rc = 0; rc * COPY_ROWS < cbld.copies[d].rows; ++rc)
                        cbld.ctiles.push_back(make_int2(d, j | (rc << 16)));
        };
        L.poff = (int64_t)cbld.ctiles.size();
        add_tiles(pack_d);
        L.pcount = (int32_t)((int64_t)cbld.ctiles.size() - L.poff);
        L.uoff = (int64_t)cbld.ctiles.size();
        add_tiles(unpack_d);
        L.ucount = (int32_t)((int64_t)cbld.ctiles.size() - L.uoff);
        // sends wait for the data (default: everything the main stream has so far);
        // receive-only steps post as soon as the main stream has finished the previous
        // level (the per-level guard below)
        if (any_send) push_wait(2, send_ev >= 0 ? send_ev : push_record(0));
        N.sched.push_back(L);
        if (any_recv) push_wait(recv_strm, push_record(2));
    }
    // the step of piece p of slab k of front s (-1: none), and all pieces of slab k
    int32_t slab_piece(int32_t s, int k, int p) const {
        if (!multi || k >= (int)slab_step[s].size() || p >= (int)slab_step[s][k].size()) return -1;
        return slab_step[s][k][p];
    }
    void emit_slab(int32_t s, int k, int recv_strm = 0) {
        if (!multi || k >= (int)slab_step[s].size()) return;
        for (int32_t id : slab_step[s][k]) emit_comm_step(id, -1, recv_strm);
    }

    // the extend-add gather's segment table of front s on hosted rank v (GSeg): per 64 x 64
    // block of its CB, every child with CB rows and columns in the block, in child order
    // (the order the entries are added in); returns the task's offset in B.gblk
    int64_t gather_segments(int32_t s, int v) {
        const int64_t gb = (int64_t)B.gblk.size();
        const RankMem& R = N.R[v];
        const int32_t* kids = S.child_list.data() + S.child_ptr[s];
        const int nkids = S.child_ptr[s + 1] - S.child_ptr[s];
        std::vector<const double*> cb((size_t)nkids);  // null: not resident on this rank
        for (int q = 0; q < nkids; ++q)
            cb[(size_t)q] = R.cb_off[kids[q]] < 0 ? nullptr : R.P.cb_pool + R.cb_base(S, kids[q]);
        // the memory plan keeps every gathered child's CB here
        if (!gather_segments_front(S.w(s), S.mb(s), kids, nkids, S.rel_ptr.data(), S.relind.data(), R.P.relind,
                                   cb.data(), B.gblk, B.gseg))
            N.err = "schedule: gathered child CB not resident on its parent's rank";
        return gb;
    }

    // ---- assembly ----
    // The assembly tasks of 16-column block cb of front s: one task (column-streaming),
    // or one per 256-row tile from the block's diagonal tile down (write-once tiles).
    void asm_block_tasks(int32_t s, int cb, bool tiled) { sc::asm_block_tasks(B.asmv, s, cb, S.sn_m[s], tiled); }
    void front_asm_tasks(int32_t s, int ncol, bool tiled) {
        for (int cb = 0; cb * ASM_COLS < ncol; ++cb) asm_block_tasks(s, cb, tiled);
    }
    // distributed assembly: one write-once tile-assembly launch of the front columns of
    // s that hosted rank v owns (its panel slabs and CB column blocks, D.col_owner), in
    // 16-column blocks; a block straddling another rank's columns computes those too,
    // into this rank's private copy, where nothing reads them
    void emit_region_asm(int32_t lev, int32_t s, int v) {
        const int who = N.R[v].rank, m = S.sn_m[s];
        const int64_t off = (int64_t)B.asmv.size();
        for (int cb = 0; cb * ASM_COLS < m; ++cb) {
            const int c1 = std::min(m, (cb + 1) * ASM_COLS);
            for (int a = cb * ASM_COLS; a < c1;) {  // each run of owned columns of the block
                if (D.col_owner(S, s, a) != who) {
                    ++a;
                    continue;
                }
                int b = a + 1;
                while (b < c1 && D.col_owner(S, s, b) == who) ++b;
                B.asml.resize(B.asmv.size(), make_int2(0, INT32_MAX));
                asm_block_tasks(s, cb, true);
                B.asml.resize(B.asmv.size(), make_int2(a, b));  // the run's tasks carry its column limits
                a = b;
            }
        }
        push_range_launch(L_ASM, ASM_TILED_LIM, lev, v, off, B.asmv.size());
    }
    // a level's large fronts on hosted rank v: fronts with m >= ASM_TILE_MIN_M one
    // workgroup per (front, 16 columns, 256-row tile), write-once; smaller fronts one
    // workgroup per (front, 16 columns) streaming child columns (measured faster below
    // ~8k rows)
    void emit_assembly(int32_t lev, const std::vector<int32_t>& large, int v) {
        for (int tiled = 1; tiled >= 0; --tiled) {
            const int64_t off = (int64_t)B.asmv.size();
            for (int32_t s : large)
                if (asm_tiled(S.sn_m[s]) == (tiled == 1) && !is_dasm(s)) {
                    front_asm_tasks(s, gathers(s, v) ? S.w(s) : S.sn_m[s], tiled == 1);
                    if (gathers(s, v)) {  // the block that straddles column w stops there
                        if (N.R[v].asm_end.empty()) N.R[v].asm_end = S.sn_m;
                        N.R[v].asm_end[s] = S.w(s);
                    }
                }
            push_range_launch(L_ASM, tiled ? ASM_TILED : ASM_BY_COLS, lev, v, off, B.asmv.size());
        }
        // distributed assembly of a split front: the owner assembles its panel columns,
        // the CB ranks their blocks (emit_cb_rank)
        for (int32_t s : large)
            if (is_dasm(s)) emit_region_asm(lev, s, v);
    }

    // ---- the 64-column chain ----
    // The TRSM tasks of block [k0, k1) of front s, TRSM_ROWS rows each from row k1 down.
    // ctr > 0: the POTRF is fused (ctr - 1: the block's arrival counter), and a block
    // with no rows below keeps one task for it.
    void trsm_tasks(std::vector<TrsmTask>& out, int32_t s, int k0, int k1, int ctr) const {
        const int m = S.sn_m[s];
        for (int r0 = k1; r0 < (ctr ? std::max(m, k1 + 1) : m); r0 += TRSM_ROWS) out.push_back(TrsmTask {s, k0, r0, m, ctr});
    }
    void push_trsm_launch(int32_t lev, int v, int var, const std::vector<TrsmTask>& tasks) {
        if (tasks.empty()) return;
        Launch L = make_launch(L_TRSM, lev, v, var);
        L.off = (int64_t)B.trsm.size();
        L.count = (int32_t)tasks.size();
        B.trsm.insert(B.trsm.end(), tasks.begin(), tasks.end());
        N.sched.push_back(L);
    }
    // The inner update after block [k0, k1) of slab [slab0, slab1) of front s (panel pan):
    // the slab's columns right of k1, or in recursive order (block b of the slab closes a
    // run of 2^t blocks, t = trailing zeros of b + 1; that run updates the next 2^t blocks,
    // K = 64 * 2^t: same flops and dependencies as right-looking, 768 instead of 1792 C
    // columns rewritten per slab).  panel_prefactor: the update also factors the next
    // step's diagonal block when that block is a full 64-column block of the same slab and
    // the update runs on 64 x 64 tiles (span <= 128; K = 64 or 128); true then, and the
    // next TRSM of s is the prefactored instance.
    bool inner_update(std::vector<GemmTask>& upd, double& fl, int32_t s, double* pan, int k0, int k1, int slab0,
                      int slab1) const {
        if (k1 >= slab1) return false;
        const int64_t m = S.sn_m[s];
        int ka = k0, c_hi = slab1;
        if (S.opt.inner_order == 1) {
            const int span = PNB << __builtin_ctz((unsigned)((k0 - slab0) / PNB + 1));
            ka = k1 - span;
            c_hi = std::min(slab1, k1 + span);
        }
        GemmTask* t = syrk_task(upd, fl, pan + k1 * m + k1, m, pan + ka * m + k1, m, (int)m - k1, c_hi - k1, k1 - ka);
        const bool pf = t && S.opt.panel_prefactor && S.opt.inner_order == 1 && S.opt.syrk_tile != 128 &&
                        k1 - ka <= 2 * PNB && k1 + PNB <= slab1;
        if (pf) t->pf = S.sn_start[s] + k1;
        return pf;
    }

    // The panel steps of a level's large fronts on hosted rank v, batched per k0.
    // Lookahead: at a slab end the outer rank-NBO update is split into the next
    // slab's columns (stream 0, needed by the next POTRF/TRSM) and the rest
    // (stream 1), which overlaps the next slab's factorization.  A later outer
    // update of overlapping columns waits for the stream-1 work first.
    void emit_panel_steps(int32_t lev, const std::vector<int32_t>& large, int v) {
        int maxw = 0;
        for (int32_t s : large) maxw = std::max(maxw, S.w(s));
        int b_pending = -1;
        // fronts whose block at the current step was pre-factored by the previous step's
        // inner update (panel_prefactor): their TRSM loads L11 (trsm_panel_g_kernel<2>)
        std::vector<char> pre((size_t)S.ns, 0);
        for (int k0 = 0; k0 < maxw; k0 += PNB) {
            const int64_t poff = (int64_t)B.potrf.size();
            std::vector<GemmTask> upd, outer_a, outer_b;
            // fused POTRF + TRSM; partial last blocks; full blocks factored by the POTRF launch
            // or by the previous inner update (each its own launch)
            std::vector<TrsmTask> fused, part, split;
            // a step whose fused launch would exceed trsm_split_wg workgroups (more than the GPU
            // holds at once) factors each diagonal block once, in the POTRF launch, instead of
            // in every workgroup of every round
            int64_t step_wg = 0;
            for (int32_t s : large) {
                if (S.w(s) < k0 + PNB) continue;
                step_wg += (std::max(S.sn_m[s], k0 + PNB + 1) - (k0 + PNB) + TRSM_ROWS - 1) / TRSM_ROWS;
            }
            const bool split_step = S.opt.trsm_split_wg > 0 && step_wg > S.opt.trsm_split_wg;
            double uflops = 0.0, afl = 0.0, bfl = 0.0;
            for (int32_t s : large) {
                const int w = S.w(s);
                const int64_t m = S.sn_m[s];
                if (w <= k0) continue;
                const int k1 = k0 + std::min(PNB, w - k0);
                const int slab0 = (k0 / NBO) * NBO;
                const int slab1 = std::min(w, slab0 + NBO);
                if (k1 - k0 < PNB) {
                    B.potrf.push_back(make_int2(s, k0));
                    trsm_tasks(part, s, k0, k1, 0);
                } else if (pre[s]) {  // L11 in place: the rows below only
                    trsm_tasks(split, s, k0, k1, 0);
                } else if (split_step) {
                    B.potrf.push_back(make_int2(s, k0));
                    trsm_tasks(split, s, k0, k1, 0);
                } else {
                    trsm_tasks(fused, s, k0, k1, (int)(B.trsm.size() + fused.size()) + 1);
                }
                double* pan = panel_of(v, s);
                pre[s] = inner_update(upd, uflops, s, pan, k0, k1, slab0, slab1);
                if (k1 == slab1 && slab1 < w) {
                    // outer_a is the last update of block slab1: a pending stream-1 outer
                    // update of those columns is waited for before outer_a runs
                    const int nxt = S.opt.lookahead ? std::min(w, slab1 + NBO) : w;
                    const double* A = pan + slab0 * m;  // column slab0, row 0
                    syrk_task(outer_a, afl, pan + slab1 * m + slab1, m, A + slab1, m, (int)m - slab1, nxt - slab1,
                              slab1 - slab0);
                    syrk_task(outer_b, bfl, pan + nxt * m + nxt, m, A + nxt, m, (int)m - nxt, w - nxt, slab1 - slab0);
                }
            }
            push_range_launch(L_POTRF, 0, lev, v, poff, B.potrf.size());
            push_trsm_launch(lev, v, TRSM_FUSED, fused);
            push_trsm_launch(lev, v, TRSM_PRE, split);
            push_trsm_launch(lev, v, TRSM_PARTIAL, part);
            push_syrk_launch(L_PANEL, lev, upd, 0, uflops);
            // split fronts: a slab is final after the TRSM of its last block; at a slab end
            // no inner update is pending
            for (int32_t s : large) {
                const int w = S.w(s);
                if (!is_split(s) || w <= k0) continue;
                const int k1 = std::min(w, k0 + PNB);
                if (k1 == w || k1 % D.nbo == 0) emit_slab(s, k0 / D.nbo);
            }
            int e_trsm = -1;
            if (!outer_b.empty()) e_trsm = push_record(0);
            if (!outer_a.empty()) {
                if (b_pending >= 0) {
                    push_wait(0, b_pending);
                    b_pending = -1;
                }
                push_syrk_launch(L_PANEL, lev, outer_a, 0, afl);
            }
            if (!outer_b.empty()) {
                push_wait(1, e_trsm);
                push_syrk_launch(L_PANEL, lev, outer_b, 0, bfl, 1);
                b_pending = push_record(1);
            }
        }
        if (b_pending >= 0) push_wait(0, b_pending);
    }

    // ---- contribution blocks ----
    // early-delivery children: the CB SYRK in column groups, an event after each
    // (the group's comm sub-step waits for exactly that event)
    void emit_early_groups(int32_t lev, const std::vector<int32_t>& large, int v) {
        for (int32_t s : large) {
            if (!is_early_sender(s, v)) continue;
            const int w = S.w(s), m = S.sn_m[s], mb = m - w;
            for (int j0 = 0; j0 < mb; j0 += D.early_gw) {
                std::vector<GemmTask> t;
                double fl = 0.0;
                syrk_task(t, fl, N.R[v].P.cb_pool + N.R[v].cb_base(S, s) + (int64_t)j0 * mb + j0, mb,
                          panel_of(v, s) + w + j0, m, mb - j0, std::min(D.early_gw, mb - j0), w);
                push_syrk_launch(L_CB, lev, t, w >= 256 ? 1 : 0, fl);
                early_ev[s].push_back(push_record(0));
            }
        }
    }
    // contribution-block SYRK, K = w; fronts with w >= 256 in their own launch
    void emit_cb_launches(int32_t lev, const std::vector<int32_t>& large, int v) {
        for (int big = 1; big >= 0; --big) {
            std::vector<GemmTask> cbt;
            double fl = 0.0;
            for (int32_t s : large) {
                const int w = S.w(s), m = S.sn_m[s], mb = m - w;
                if (mb <= 0 || (w >= 256) != (big == 1) || is_split(s) || is_early_sender(s, v)) continue;
                GemmTask* t = syrk_task(cbt, fl, N.R[v].P.cb_pool + N.R[v].cb_base(S, s), mb, panel_of(v, s) + w, m, mb,
                                        mb, w);
                if (gathers(s, v)) {
                    t->gs = s;
                    t->gv = v;
                    t->gb = gather_segments(s, v);
                    t->gw = w;
                }
            }
            push_syrk_launch(L_CB, lev, cbt, big, fl);
        }
    }
    // CB rank (hosted index v) of split front s: per final panel slab, CB -= L21_k
    // L21_k^T on the column blocks it owns (K = slab width), from its R_LAND copy
    void emit_cb_rank(int32_t lev, int32_t s, int v) {
        const int who = N.R[v].rank;
        const std::vector<int32_t>& cbr = D.cb_rank[D.split[s]];
        const int w = S.w(s), mb = S.sn_m[s] - w;
        if (is_dasm(s))
            emit_region_asm(lev, s, v);  // its own CB blocks, from the children's columns it received
        else
            emit_comm_step(init_step[s]);
        for (int k0 = 0, k = 0; k0 < w; k0 += D.nbo, ++k) {
            const int k1 = std::min(w, k0 + D.nbo);
            emit_slab(s, k);
            std::vector<GemmTask> cbt;
            double fl = 0.0;
            for (int jb = 0; jb < (int)cbr.size(); ++jb) {
                if (cbr[jb] != who) continue;
                const int r0 = jb * D.cbb;
                int64_t ldc = 0, lda = 0;
                double* C = region_ptr(v, R_CB, s, r0, r0, ldc);
                const double* A = region_ptr(v, R_LAND, s, r0, k0, lda);
                syrk_task(cbt, fl, C, ldc, A, lda, mb - r0, std::min(D.cbb, mb - r0), k1 - k0);
            }
            push_syrk_launch(L_CB, lev, cbt, w >= 256 ? 1 : 0, fl);
        }
    }

    // ---- small fronts ----
    // one launch sized for the level's largest front when the level fits one workgroup per
    // CU (fewer dependent launches on thin levels), else one launch per LDS bucket (small
    // fronts keep their occupancy on wide levels)
    void emit_small_fronts(int32_t lev, const std::vector<int32_t>& nodes, int v) {
        int nsmall = 0, bmax = 0;
        for (int32_t s : nodes)
            if (S.fclass[s] == FRONT_SMALL) {
                ++nsmall;
                bmax = std::max(bmax, bucket_of(S.sn_m[s]));
            }
        for (int b : {32, 64, 88, 96, 128}) {
            if (nsmall <= 256 && b != bmax) continue;
            Launch L = make_launch(L_SMALL, lev, v, SMALL_FRONTS);
            L.off = (int64_t)B.small.size();
            L.maxm = b;
            for (int32_t s : nodes)
                if (S.fclass[s] == FRONT_SMALL && (nsmall <= 256 || bucket_of(S.sn_m[s]) == b)) B.small.push_back(s);
            L.count = (int32_t)((int64_t)B.small.size() - L.off);
            if (L.count > 0) N.sched.push_back(L);
        }
    }

    // one level's fronts of hosted rank v
    void emit_level(int32_t lev, const std::vector<int32_t>& nodes, int v) {
        emit_small_fronts(lev, nodes, v);
        std::vector<int32_t> large;
        for (int32_t s : nodes)
            if (S.fclass[s] == FRONT_LARGE) large.push_back(s);
        if (large.empty()) return;
        emit_assembly(lev, large, v);
        for (int32_t s : large)
            if (is_split(s)) emit_comm_step(init_step[s]);
        emit_panel_steps(lev, large, v);
        emit_early_groups(lev, large, v);
        emit_cb_launches(lev, large, v);
    }

    // ---- distributed panels ----
    // slab k's update of slab k + 1 by the slab's columns [c0, c0 + pw) on stream strm
    void push_piece_update(const DistFront& F, double* pan, int k, int c0, int strm) {
        const int64_t m = F.m;
        const int j0 = F.c0(k + 1), j1 = F.c1(k + 1);
        std::vector<GemmTask> t0;
        double fl = 0.0;
        syrk_task(t0, fl, pan + j0 * m + j0, m, pan + c0 * m + j0, m, F.m - j0, j1 - j0,
                  std::min(F.c1(k), c0 + D.pw) - c0);
        push_syrk_launch(L_PANEL, F.lev, t0, 0, fl, strm);
    }
    // Hosted rank vk factors slab k: per 64 columns POTRF, TRSM of the rows below, and the
    // inner update (as emit_panel_steps, one front, no trsm_split_wg); a finished piece of
    // the slab leaves at once (dist_pieces).  Returns the event after the last local piece
    // update (dist_local_pieces), or -1.
    int factor_dist_slab(DistFront& F, int k, int vk) {
        const int32_t s = F.s, lev = F.lev;
        const int k0s = F.c0(k), k1s = F.c1(k);
        const int e = F.last_ev1(vk, k - 2);
        if (e >= 0) push_wait(0, e);
        double* pan = panel_of(vk, s);
        bool pre_blk = false;  // this block was pre-factored by the previous inner update
        // dist_local_pieces: when this rank also owns the next slab, its update by each
        // finished piece of this slab goes on the lookahead stream while the chain goes on
        const bool local_next = S.opt.dist_local_pieces && k + 1 < F.nsl && F.sr[k + 1] == F.sr[k];
        int local_ev = -1;
        for (int k0 = k0s; k0 < k1s; k0 += PNB) {
            const int k1 = std::min(k0 + PNB, k1s);
            const bool partial = k1 - k0 < PNB;
            if (partial) {  // full blocks: POTRF fused into the TRSM
                B.potrf.push_back(make_int2(s, k0));
                push_range_launch(L_POTRF, 0, lev, vk, (int64_t)B.potrf.size() - 1, B.potrf.size());
            }
            std::vector<TrsmTask> tt;
            trsm_tasks(tt, s, k0, k1, (partial || pre_blk) ? 0 : (int)B.trsm.size() + 1);
            push_trsm_launch(lev, vk, partial ? TRSM_PARTIAL : pre_blk ? TRSM_PRE : TRSM_FUSED, tt);
            // a finished piece of the slab leaves now (dist_pieces)
            if (k1 == k1s || (k1 - k0s) % D.pw == 0) {
                const int pc = (k1 - 1 - k0s) / D.pw;
                emit_comm_step(slab_piece(s, k, pc));
                if (local_next) {  // dist_local_pieces: this rank's next slab, by this piece, now
                    push_wait(1, push_record(0));
                    push_piece_update(F, pan, k, k0s + pc * D.pw, 1);
                    local_ev = push_record(1);
                }
            }
            std::vector<GemmTask> upd;
            double fl = 0.0;
            pre_blk = inner_update(upd, fl, s, pan, k0, k1, k0s, k1s);
            push_syrk_launch(L_PANEL, lev, upd, 0, fl);
        }
        return local_ev;
    }
    // Slab k's update on hosted rank v (which needs it): its own next slab on the main
    // stream (critical path, piece by piece), its other later slabs and CB blocks on the
    // lookahead stream.
    void apply_dist_slab(DistFront& F, int k, int v, bool chained, int local_ev) {
        const int32_t s = F.s;
        const int r = N.R[v].rank, k0s = F.c0(k), k1s = F.c1(k), K = k1s - k0s;
        const int64_t m = F.m;
        double* pan = panel_of(v, s);
        const double* Lk = pan + k0s * m;  // column k0s of the slab, row 0
        if (k + 1 < F.nsl && F.sr[k + 1] == r && chained && local_ev >= 0) {  // done during the chain
            push_wait(0, local_ev);
        } else if (k + 1 < F.nsl && F.sr[k + 1] == r) {  // the next slab: critical path, piece by piece
            const int e = F.last_ev1(v, k - 1);
            if (e >= 0) push_wait(0, e);
            for (int p = 0, c0 = k0s; c0 < k1s; ++p, c0 += D.pw) {
                emit_comm_step(slab_piece(s, k, p));
                push_piece_update(F, pan, k, c0, 0);
            }
        }
        // the rest of slab k feeds only the lookahead stream's updates here: that
        // stream waits for it, the main stream (this rank's chain) does not
        emit_slab(s, k, 1);
        std::vector<GemmTask> t1;
        double fl = 0.0;
        for (int j = k + 2; j < F.nsl; ++j) {
            if (F.sr[j] != r) continue;
            const int j0 = F.c0(j), j1 = F.c1(j);
            syrk_task(t1, fl, pan + j0 * m + j0, m, Lk + j0, m, F.m - j0, j1 - j0, K);
        }
        if (is_split(s)) {  // CB blocks: CB -= L21_k L21_k^T
            const std::vector<int32_t>& cbr = D.cb_rank[D.split[s]];
            for (int jb = 0; jb < (int)cbr.size(); ++jb) {
                if (cbr[jb] != r) continue;
                const int r0 = jb * D.cbb;
                int64_t ldc = 0;
                double* C = region_ptr(v, R_CB, s, r0, r0, ldc);
                syrk_task(t1, fl, C, ldc, Lk + F.w + r0, m, F.mb - r0, std::min(D.cbb, F.mb - r0), K);
            }
        } else if (F.mb > 0 && r == F.own) {  // unsplit: the owner's whole CB
            int64_t ldc = 0;
            double* C = region_ptr(v, R_CB, s, 0, 0, ldc);
            syrk_task(t1, fl, C, ldc, Lk + F.w, m, F.mb, F.mb, K);
        }
        if (t1.empty()) return;
        push_wait(1, push_record(0));
        push_syrk_launch(L_PANEL, F.lev, t1, 0, fl, 1);
        F.ev1[v][k] = push_record(1);
    }
    // Distributed panel of front s (dist.cpp): every hosted rank of its holders.  Per
    // slab k: its owner factors it (the 64-column POTRF / TRSM / inner-update chain
    // on the main stream), the SLAB step moves it, then every rank that needs it
    // updates its own next slab on the main stream (critical path) and its other
    // later slabs and CB blocks on the lookahead stream.  A lookahead-stream update
    // of slab j (from slab k <= j - 2) is waited for before the main stream touches
    // slab j (event after the lookahead launch of step j - 2, covering all earlier
    // ones: the stream is in order).
    void emit_dist_front(int32_t lev, int32_t s) {
        const int q = D.pd[s];
        DistFront F {lev, s, S.w(s), S.sn_m[s], S.mb(s), (int)D.slab_rank[q].size(), D.owner[s], D.nbo, D.slab_rank[q],
                     {}, {}};
        for (int32_t r : D.holders[q])
            if (hosted_of[r] >= 0) F.vs.push_back(hosted_of[r]);
        const int vo = hosted_of[F.own];
        if (vo >= 0 && std::find(F.vs.begin(), F.vs.end(), vo) == F.vs.end()) F.vs.push_back(vo);
        if (F.vs.empty()) return;
        if (is_dasm(s)) {  // every holder assembles its own slabs and CB blocks
            for (int v : F.vs) emit_region_asm(lev, s, v);
        } else if (vo >= 0) {  // the owner assembles the whole front (tiled or column-streaming)
            const int64_t off = (int64_t)B.asmv.size();
            front_asm_tasks(s, F.m, asm_tiled(F.m));
            push_range_launch(L_ASM, asm_tiled(F.m) ? ASM_TILED : ASM_BY_COLS, lev, vo, off, B.asmv.size());
        }
        emit_comm_step(init_step[s]);
        F.ev1.assign(N.R.size(), std::vector<int>((size_t)F.nsl, -1));
        for (int k = 0; k < F.nsl; ++k) {
            const int vk = hosted_of[F.sr[k]];
            const int local_ev = vk >= 0 ? factor_dist_slab(F, k, vk) : -1;
            for (int v : F.vs)
                if (D.need_row(S, s, k, N.R[v].rank) < F.m) apply_dist_slab(F, k, v, v == vk, local_ev);
        }
        for (int v : F.vs) {  // join the lookahead stream before the level's deliveries
            const int e = F.last_ev1(v, F.nsl - 1);
            if (e >= 0) push_wait(0, e);
        }
    }

    // ---- single device: whole-factorization launches ----
    // n <= TINY_DENSE_N (and the tiny_dense option): the whole matrix as one dense lower
    // triangle in one wave (kernels.hip tiny_dense_kernel); the plan is one (Ax index,
    // panel position) pair per dense entry (column c, row r) at c * 64 + r, -1 where the
    // entry has no A value / is not stored (internal numbering: the factor of the
    // postordered matrix is the postordered factor, so the dense image is the
    // multifrontal result).  A value and panel byte offsets stay inside the kernel's
    // 32-bit buffer ranges.
    bool emit_tiny_dense() {
        if (multi || !S.opt.tiny_dense || S.n <= 0 || S.n > TINY_DENSE_N || S.nnzA_in >= (1 << 27)) return false;
        for (int32_t s = 0; s < S.ns; ++s) {
            const int m = S.sn_m[s], w = S.w(s), c0 = S.sn_start[s];
            const int32_t* rows = S.rows.data() + S.rows_ptr[s];
            if (B.ta.empty()) B.ta.assign((size_t)tiny_dense_np((int)S.n) * 64, make_int2(-1, -1));
            for (int lc = 0; lc < w; ++lc)
                for (int64_t q = S.a_ptr[c0 + lc]; q < S.a_ptr[c0 + lc + 1]; ++q)
                    B.ta[(size_t)(c0 + lc) * 64 + rows[S.a_pos[q]]].x = (int32_t)S.a_src[q];
            const int64_t off = N.R[0].panel_off[s];
            for (int j = 0; j < w; ++j)
                for (int i = j; i < m; ++i) B.ta[(size_t)(c0 + j) * 64 + rows[i]].y = (int32_t)(off + (int64_t)j * m + i);
        }
        Launch L = make_launch(L_SMALL, 0, 0, SMALL_TINY_DENSE);
        L.maxm = (int32_t)S.n;
        L.count = 1;
        N.sched.push_back(L);
        return true;
    }
    // a tiny tree (at most TINY_MAX_FRONTS fronts, all small with m <= 64, every image and
    // CB fitting LDS): the whole factorization as one single-workgroup launch, postorder
    // (the internal numbering), everything in LDS
    bool emit_tiny_tree() {
        bool tiny = !multi && S.ns > 1 && S.ns <= TINY_MAX_FRONTS;
        int64_t lds = 0;
        for (int32_t s = 0; tiny && s < S.ns; ++s) {
            const int64_t m = S.sn_m[s], mb = S.mb(s);
            tiny = S.fclass[s] == FRONT_SMALL && m <= 64;
            lds += m * (m + 1) / 2 + mb * (mb + 1) / 2;
        }
        if (!tiny || lds > TINY_MAX_LDS) return false;
        auto pk = [](int64_t m, int64_t j) { return j * m - j * (j - 1) / 2; };
        std::vector<int32_t> img((size_t)S.ns), cbo((size_t)S.ns);
        int32_t off = 0;
        for (int32_t s = 0; s < S.ns; ++s) {
            img[s] = off;
            off += S.sn_m[s] * (S.sn_m[s] + 1) / 2;
            cbo[s] = off;
            off += S.mb(s) * (S.mb(s) + 1) / 2;
        }
        B.tiny_lds = off;
        for (int32_t s = 0; s < S.ns; ++s) {
            const int m = S.sn_m[s], w = S.w(s), c0 = S.sn_start[s];
            TinyFront f {s, c0, w, m, img[s], cbo[s], (int32_t)B.tph.size(), 0, N.R[0].panel_off[s]};
            for (int lc = 0; lc < w; ++lc)
                for (int64_t q = S.a_ptr[c0 + lc]; q < S.a_ptr[c0 + lc + 1]; ++q)
                    B.ta.push_back(make_int2((int32_t)S.a_src[q], img[s] + (int32_t)(pk(m, lc) + S.a_pos[q] - lc)));
            for (int32_t ci = S.child_ptr[s]; ci < S.child_ptr[s + 1]; ++ci) {
                const int32_t c = S.child_list[ci];
                const int mbc = S.mb(c);
                const int32_t* rel = S.relind.data() + S.rel_ptr[c];
                const int32_t beg = (int32_t)B.tpr.size();
                for (int jc = 0; jc < mbc; ++jc)
                    for (int ic = jc; ic < mbc; ++ic)
                        B.tpr.push_back(make_int2(cbo[c] + (int32_t)(pk(mbc, jc) + ic - jc),
                                                  img[s] + (int32_t)(pk(m, rel[jc]) + rel[ic] - rel[jc])));
                B.tph.push_back(make_int2(beg, (int32_t)B.tpr.size()));
            }
            f.np = (int32_t)B.tph.size() - f.e0;
            B.tfr.push_back(f);
        }
        Launch L = make_launch(L_SMALL, 0, 0, SMALL_TINY_TREE);
        L.maxm = 64;
        L.count = 1;
        N.sched.push_back(L);
        return true;
    }
    // a run of >= 2 levels holding one small front each (a chain: each front the parent of
    // the one before) runs as one single-workgroup launch
    bool chain_front(int32_t lev) const {
        return !multi && lev < S.nlevels && by_level[lev].size() == 1 && S.fclass[by_level[lev][0]] == FRONT_SMALL;
    }
    // the chain from level lev on; returns the first level after it
    int32_t emit_chain(int32_t lev) {
        Launch L = make_launch(L_SMALL, lev, 0, SMALL_CHAIN);
        L.off = (int64_t)B.cdesc.size();
        L.maxm = 32;
        int32_t sp = -1;
        for (; chain_front(lev) && (int64_t)B.cdesc.size() - L.off < CHAIN_MAXF; ++lev) {
            const int32_t s = by_level[lev][0];
            const int w = S.w(s), m = S.sn_m[s];
            L.maxm = std::max(L.maxm, bucket_of(m));
            const ChainDesc d {s, S.sn_start[s], w, m, sp, 0, N.R[0].panel_off[s], std::max<int64_t>(N.R[0].cb_off[s], 0),
                               B.chain_init, (int64_t)B.crelp.size()};
            for (int t0 = 0; t0 < m; t0 += 4) {  // parent rows of CB rows, packed per tile row
                uint32_t wd = 0;
                for (int t = 0; t < 4; ++t) {
                    const int i = t0 + t;
                    const int32_t pr = (i >= w && i < m) ? S.relind[(size_t)S.rel_ptr[s] + (i - w)] : 0;
                    wd |= (uint32_t)(pr & 255) << (8 * t);
                }
                B.crelp.push_back(wd);
            }
            B.chain_init += ((int64_t)m * (m + 1) / 2 + 63) / 64 * 64;
            B.cdesc.push_back(d);
            sp = s;
        }
        L.count = (int32_t)((int64_t)B.cdesc.size() - L.off);
        N.sched.push_back(L);
        return lev;
    }

    // ---- the levels ----
    // multi-rank: what follows the hosted ranks' own fronts of level lev -- distributed
    // panels, the CB ranks of split fronts, and the level's deliveries
    void emit_level_shared(int32_t lev) {
        for (int32_t s : by_level[lev])
            if (is_dpanel(s)) emit_dist_front(lev, s);
        // contribution-block ranks of this level's split fronts (emulated: after the
        // owners' panels, whose steps already moved the data)
        for (int32_t s : by_level[lev]) {
            if (!is_split(s) || is_dpanel(s)) continue;
            const std::vector<int32_t>& cbr = D.cb_rank[D.split[s]];
            for (size_t v = 0; v < N.R.size(); ++v) {
                const int who = N.R[v].rank;
                if (who != D.owner[s] && std::find(cbr.begin(), cbr.end(), who) != cbr.end())
                    emit_cb_rank(lev, s, (int)v);
            }
        }
        // contribution blocks that leave / enter the hosted ranks after this level:
        // early children's column groups first, then the rest
        for (int32_t c : by_level[lev]) {
            if (!D.early[c] || early_step[c].empty()) continue;
            const int ng = (S.mb(c) + D.early_gw - 1) / D.early_gw;
            const int vs = hosted_of[D.owner[c]];
            for (int g = 0; g < ng; ++g)
                if (g < (int)early_step[c].size())
                    emit_comm_step(early_step[c][g], vs >= 0 && !early_ev[c].empty() ? early_ev[c][g] : -1);
        }
        emit_comm_step(deliver_step[lev]);
    }

    int64_t run() {
        if (multi) push_wait(2, push_record(0));  // previous factorization's reads are done
        // multi-rank work-arena reuse guard (memplan.cpp): the comm steps of level L run
        // after the main stream has finished level L - 1, and the main stream starts level
        // L + 2 only after the comm steps of level L, so a region a step of level L touches
        // is never reused before level L + 2
        std::vector<int> comm_done((size_t)S.nlevels, -1);
        const bool whole = emit_tiny_dense() || emit_tiny_tree();
        for (int32_t lev = whole ? S.nlevels : 0; lev < S.nlevels; ++lev) {
            if (chain_front(lev) && chain_front(lev + 1)) {
                lev = emit_chain(lev) - 1;
                continue;
            }
            if (multi) {
                if (lev >= 2 && comm_done[lev - 2] >= 0) push_wait(0, comm_done[lev - 2]);
                push_wait(2, push_record(0));
            }
            for (size_t v = 0; v < N.R.size(); ++v) {
                if (!multi) {
                    emit_level(lev, by_level[lev], (int)v);
                    continue;
                }
                std::vector<int32_t> mine;
                for (int32_t s : by_level[lev])
                    if (D.owner[s] == N.R[v].rank && !is_dpanel(s)) mine.push_back(s);
                if (!mine.empty()) emit_level(lev, mine, (int)v);
            }
            if (!multi) continue;
            emit_level_shared(lev);
            comm_done[lev] = push_record(2);
        }
        if (multi) push_wait(0, push_record(2));  // join the comm stream (its last sends)
        return N.err.empty() ? SC_OK : SC_ERR_ARG;
    }
};

}  // namespace

int64_t build_schedule(Numeric& N, SchedBuild& B) { return ScheduleBuilder(N, B).run(); }

}  // namespace sc
