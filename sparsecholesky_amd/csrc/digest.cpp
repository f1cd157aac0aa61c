// Schedule digest (host): one 64-bit hash over every decoded schedule entry and every
// task array a handle uploads, plus counters of what a factorization issues.  Two
// handles with equal digests issue the same calls on the same streams in the same order
// with the same arguments.  Pointers enter as (arena, offset), so the digest does not
// depend on where the pools live: it can be computed with no device (placeholder pool
// bases, schedule_digest_host) and from a live handle (numeric_init) and must agree.
// Everything is hashed field by field: the structs have padding.
#include "numeric_impl.hpp"

namespace sc {

namespace {

struct Hasher {
    uint64_t h = 0xcbf29ce484222325ull;
    void u64(uint64_t v) {
        h = (h ^ v) * 0x100000001b3ull;
        h ^= h >> 29;
    }
    void i(int64_t v) { u64((uint64_t)v); }
    void f(double d) {
        uint64_t b;
        std::memcpy(&b, &d, sizeof b);
        u64(b);
    }
    void i2(const std::vector<int2>& v) {
        i((int64_t)v.size());
        for (const int2& t : v) u64((uint64_t)(uint32_t)t.x << 32 | (uint32_t)t.y);
    }
    template <class T>
    void ints(const std::vector<T>& v) {
        i((int64_t)v.size());
        for (T t : v) i((int64_t)t);
    }
};

// The pools of the hosted ranks: each kind is one allocation, the ranks back to back.
enum Arena : int { A_NONE = 0, A_PANEL = 1, A_WORK = 2, A_STAGING = 3, A_RELIND = 4 };
struct Arenas {
    const double *panel, *work, *staging;
    int64_t npanel, nstaging;
    const int32_t* relind;
    // a region or staging address; a CB's virtual origin (RankMem::cb_base) may lie
    // outside the work arena, so whatever is in no other arena is a work address
    void ptr(Hasher& H, const double* p) const {
        if (!p) {
            H.i(A_NONE);
            H.i(0);
        } else if (p >= panel && p < panel + npanel) {
            H.i(A_PANEL);
            H.i(p - panel);
        } else if (staging && p >= staging && p < staging + nstaging) {
            H.i(A_STAGING);
            H.i(p - staging);
        } else {
            H.i(A_WORK);
            H.i(p - work);
        }
    }
};

void hash_launch(Hasher& H, const Launch& L, CallKind c) {
    H.i(c);
    H.i(L.level);
    H.i(L.strm);
    H.i(L.vr);
    H.i(L.off);    // first task; comm: first message
    H.i(L.count);  // grid / tiles / messages; record and wait: the event index
    switch (c) {
        case C_FRONT_SMALL:
        case C_CHAIN:
        case C_TINY_TREE:
        case C_TINY_DENSE:
            H.i(L.maxm);
            break;
        case C_SYRK_PANEL:
        case C_SYRK_CB:
            H.i(L.toff);
            H.i(L.ntasks);
            H.i(L.bt);
            H.i(L.epi);
            H.i(L.lean);
            H.i(L.pf);
            H.i(L.big);
            H.f(L.flops);
            H.f(L.bytes);
            break;
        case C_COMM:
            H.i(L.step);
            H.i(L.poff);
            H.i(L.pcount);
            H.i(L.uoff);
            H.i(L.ucount);
            break;
        default:
            break;
    }
}

}  // namespace

SchedDigest schedule_digest(const Numeric& N, const SchedBuild& B) {
    SchedDigest D;
    Hasher H;
    Arenas A {};
    A.panel = N.R[0].P.panel_pool;
    A.work = N.R[0].P.cb_pool;
    A.relind = N.R[0].P.relind;
    A.staging = N.staging;
    A.nstaging = B.cb.stage_total;
    for (const RankMem& R : N.R) A.npanel += R.panel_total;

    H.i((int64_t)N.sched.size());
    for (const Launch& L : N.sched) {
        const CallKind c = decode_call(L);
        hash_launch(H, L, c);
        D.calls[c]++;
        D.tail_split += L.tail != 0;
        D.pf += (c == C_SYRK_PANEL || c == C_SYRK_CB) && L.pf;
    }
    D.comm_steps = D.calls[C_COMM];
    D.events = N.n_sync_events;
    D.msgs = (int64_t)N.msgs.size();
    D.gsegs = (int64_t)B.gseg.size();
    H.i(D.events);

    H.ints(B.small);
    H.i2(B.asmv);
    H.i2(B.asml);
    H.i2(B.potrf);
    H.i((int64_t)B.trsm.size());
    for (const TrsmTask& t : B.trsm) {
        H.i(t.s);
        H.i(t.k0);
        H.i(t.r0);
        H.i(t.r1);
        H.i(t.ctr);
    }
    H.i((int64_t)B.gemm.size());
    for (const GemmTask& t : B.gemm) {
        A.ptr(H, t.C);
        A.ptr(H, t.A);
        H.i(t.ldc);
        H.i(t.lda);
        H.i(t.M);
        H.i(t.N);
        H.i(t.K);
        H.i(t.gs);
        H.i(t.gv);
        H.i(t.gb);
        H.i(t.gw);
        H.i(t.pf);
    }
    H.i2(B.tiles);
    H.ints(B.gblk);
    H.i((int64_t)B.gseg.size());
    for (const GSeg& g : B.gseg) {
        H.i(g.cb - A.work);  // always a work address (the child's CB origin)
        H.i(g.rel - A.relind);
        H.i(g.mbc);
        H.i(g.ilo);
        H.i(g.ihi);
        H.i(g.jlo);
        H.i(g.jhi);
    }
    H.i((int64_t)B.cdesc.size());
    for (const ChainDesc& d : B.cdesc) {
        H.i(d.s);
        H.i(d.c0);
        H.i(d.w);
        H.i(d.m);
        H.i(d.sp);
        H.i(d.panel_off);
        H.i(d.cb_off);
        H.i(d.init_off);
        H.i(d.relp_off);
    }
    H.ints(B.crelp);
    H.i(B.chain_init);
    H.i((int64_t)B.tfr.size());
    for (const TinyFront& f : B.tfr) {
        H.i(f.s);
        H.i(f.c0);
        H.i(f.w);
        H.i(f.m);
        H.i(f.img);
        H.i(f.cb);
        H.i(f.e0);
        H.i(f.np);
        H.i(f.panel_off);
    }
    H.i2(B.ta);
    H.i2(B.tph);
    H.i2(B.tpr);
    H.i(B.tiny_lds);

    H.i((int64_t)N.msgs.size());
    for (const Msg& m : N.msgs) {
        A.ptr(H, m.buf);
        A.ptr(H, m.src_buf);
        H.i(m.count);
        H.i(m.peer);
        H.i(m.op);
    }
    H.i((int64_t)B.cb.copies.size());
    for (const Copy2D& c : B.cb.copies) {
        A.ptr(H, c.a);
        A.ptr(H, c.b);
        H.i(c.lda);
        H.i(c.rows);
        H.i(c.cols);
    }
    H.i2(B.cb.ctiles);
    H.ints(B.cb.copy_slot);
    H.ints(B.cb.msg_slot);
    H.ints(B.cb.msg_src_slot);
    H.i(B.cb.stage_total);
    D.hash = H.h;
    return D;
}

namespace {

// The schedule of a handle planned on the host (placeholder pool bases): N.sched and B.
int64_t plan_schedule_host(const Symbolic& S, int nranks, int rank, int emulate, Numeric& N, SchedBuild& B,
                           std::string& err) {
    if (nranks < 1 || rank < 0 || rank >= nranks || emulate < 0 || emulate > 2) return SC_ERR_ARG;
    N.rank = emulate ? 0 : rank;
    N.nranks = nranks;
    N.emulated = emulate != 0;
    N.emul_rccl = emulate == 2 ? 1 : 0;
    int64_t rc = SC_OK;
    if (nranks > 1 || emulate) {  // as numeric_create_dist
        if ((rc = dist_plan(S, nranks, N.D)) != SC_OK) return rc;
        N.owner = N.D.owner;
    }
    // pool bases that are never dereferenced, far enough apart that no offset crosses
    auto base = [](int arena) { return (uintptr_t)arena << 44; };
    if ((rc = numeric_plan_host(N, S)) == SC_OK) {
        for (RankMem& R : N.R) R.P.relind = (const int32_t*)base(A_RELIND);
        set_pool_bases(N, (double*)base(A_PANEL), (double*)base(A_WORK));
        rc = build_schedule(N, B);
    }
    if (rc != SC_OK) {
        err = N.err;
        return rc;
    }
    finish_build(N, B, (double*)base(A_STAGING));
    return SC_OK;
}

}  // namespace

int64_t schedule_digest_host(const Symbolic& S, int nranks, int rank, int emulate, SchedDigest& out,
                             std::string& err) {
    Numeric N;
    SchedBuild B;
    const int64_t rc = plan_schedule_host(S, nranks, rank, emulate, N, B, err);
    if (rc != SC_OK) return rc;
    out = schedule_digest(N, B);
    return SC_OK;
}

int64_t schedule_syrk_host(const Symbolic& S, int nranks, int rank, int emulate, std::vector<int64_t>& out,
                           std::string& err) {
    Numeric N;
    SchedBuild B;
    const int64_t rc = plan_schedule_host(S, nranks, rank, emulate, N, B, err);
    if (rc != SC_OK) return rc;
    out.clear();
    for (const Launch& L : N.sched) {
        if (L.kind != L_PANEL && L.kind != L_CB) continue;
        int64_t gathers = 0;
        for (int64_t q = L.off; q < L.off + L.ntasks; ++q) gathers |= B.gemm[(size_t)q].gs >= 0;
        const int64_t v[8] = {L.kind == L_CB, L.bt, L.lean, L.epi, L.pf, L.tail, L.count, gathers};
        out.insert(out.end(), v, v + 8);
    }
    return SC_OK;
}

}  // namespace sc
