// Device numeric factorization driver: memory plan, level schedule, launches, export.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "kernels.hpp"
#include "symbolic.hpp"

namespace sc {

enum LaunchKind : int32_t {
    L_SMALL = 0,
    L_ASM = 1,
    L_POTRF = 2,
    L_TRSM = 3,
    L_PANEL = 4,
    L_CB = 5,
    L_COMM = 6,    // one comm step of the hosted ranks (pack, transfer group, unpack)
    L_RECORD = 11, // record sync event `count` on stream `strm`
    L_WAIT = 12,   // stream `strm` waits for sync event `count`
    L_KINDS = 13
};

// ---------------- multi-GPU plan (dist.cpp) ----------------
// Comm steps, in one global order every rank follows (each rank posts exactly its
// part of every step it takes part in, as one transfer group, on its comm stream):
//   STEP_INIT(s)    split front s: the owner sends the assembled CB column blocks to
//                   the ranks that compute them
//   STEP_SLAB(s,k)  split front s: the owner sends rows [w, m) of panel slab k (final)
//                   to every CB rank
//   STEP_DELIVER(l) after level l: every contribution block (column block) whose
//                   producer is not the executing rank of the parent goes there; one
//                   sub-step (s = child, k = group) per column group of an early child
//                   first, then one (s = -1) with the rest
enum StepKind : int32_t { STEP_INIT = 0, STEP_SLAB = 1, STEP_DELIVER = 2 };
struct DistStep {
    int32_t kind, level, s, k;
    int32_t p = 0;  // STEP_SLAB of a distributed panel: the column piece of slab k (dist_pieces)
};

// Device memory regions of a rank (memplan.cpp).  Messages and tasks name a region
// by kind, supernode and LOGICAL coordinates; every rank maps them to its own
// physical layout, so sender and receiver may store a block differently.
//   R_PANEL  the L panel of s: m x w, row = front row (owner only; permanent)
//   R_CB     the contribution block of s: mb x mb, row/col = front row - w, held as a
//            full square (ld = mb) on every rank that computes or receives part of it
//            (only those parts are valid there)
//   R_LAND   a split front's L21 (rows [w, m) of its panel) on a CB rank: mb x w
enum RegionKind : int32_t { R_PANEL = 0, R_CB = 1, R_LAND = 2 };

// One 2D block transfer: rows x cols doubles from (skind, s, srow, scol) on src to
// (dkind, s, drow, dcol) on dst, moved packed (column-contiguous) through staging.
struct DistMsg {
    int32_t step;
    int32_t src, dst;
    int32_t skind, dkind;
    int32_t s;
    int32_t srow, scol, drow, dcol;
    int32_t rows, cols;
};
struct DistPlan {
    int nranks = 1;
    int cbb = 1024;  // CB column-block width
    int nbo = 1024;  // panel slab width (panel_nb_outer)
    int pw = 1024;   // distributed panels: columns per STEP_SLAB piece (nbo / dist_pieces, 64-aligned)
    std::vector<int32_t> owner;    // rank executing each supernode's assembly + panel
    std::vector<int32_t> gsize;    // rank-group size of each supernode (1 = inside a subtree)
    std::vector<int32_t> split;    // index into split_s / cb_rank, or -1
    std::vector<int32_t> split_s;
    std::vector<std::vector<int32_t>> cb_rank;  // per split front: rank of CB column block jb
    // distributed panels (dist_panel): a shared front wider than one slab has panel slab
    // k (columns [k nbo, (k+1) nbo)) factored by slab_rank[pd[s]][k] (slab 0 on the
    // owner, the rest cyclic over the group); every rank in holders[pd[s]] (slab owners
    // and CB ranks, ascending) keeps a full m x w panel copy
    std::vector<int32_t> pd;       // per supernode: index into pd_s / slab_rank / holders, or -1
    std::vector<int32_t> pd_s;
    std::vector<std::vector<int32_t>> slab_rank;
    std::vector<std::vector<int32_t>> holders;
    // first front row rank r needs of final slab k of distributed front s: the start of
    // its first own slab after k, or w for a CB rank; m = not needed
    int need_row(const Symbolic& S, int32_t s, int k, int r) const;
    bool holds(int32_t s, int r) const;  // r keeps a panel copy of s (owner included)
    // distributed assembly (dist_asm): a shared front with a distributed panel or a split
    // CB is assembled where its columns live -- every rank assembles the panel slabs and
    // CB column blocks it owns, and each child's CB columns go straight to the rank
    // owning the parent columns they map into (no STEP_INIT)
    std::vector<char> dasm;
    int col_owner(const Symbolic& S, int32_t p, int col) const;  // rank assembling front column col of p
    // rank r assembles a parent column that child c's CB maps into (holds CB(c) until then)
    bool receives(const Symbolic& S, int32_t c, int r) const;
    // rank r computes column blocks of s's CB (holds the full-square CB(s) from level(s))
    bool produces_cb(const Symbolic& S, int32_t s, int r) const;
    // early delivery: a large, unsplit child whose parent runs on another rank has its
    // CB SYRK in column groups of early_gw, each group sent as soon as it is computed
    int early_gw = 4096;
    std::vector<char> early;
    std::vector<DistStep> steps;
    std::vector<DistMsg> msgs;     // ascending step
    std::vector<double> work;      // estimated flops per rank
};
int64_t dist_plan(const Symbolic& S, int nranks, DistPlan& D);

// Memory of one rank (a process hosts one rank, or every rank when emulated).
//   panel arena  the L panels of the supernodes this rank owns, back to back
//   work arena   transient regions (contribution blocks, landing slabs), each live
//                over a closed interval of assembly-tree levels; offsets from an
//                interval plan (memplan.cpp), so a region is reused once dead
struct RankMem {
    int32_t rank = 0;
    std::vector<int64_t> panel_off;  // per supernode: doubles into the panel arena, -1 = not here
    std::vector<int64_t> cb_off;     // per supernode: the CB region in the work arena, -1 = not here
    // per supernode: first CB column the region holds (columns [cb_col0, ...) of the mb x mb
    // square, ld = mb): a rank computing or receiving only some column blocks of a shared
    // front's CB keeps just their column range; cb_base() is the square's (virtual) origin
    std::vector<int32_t> cb_col0;
    int64_t cb_base(const Symbolic& S, int32_t s) const { return cb_off[s] - (int64_t)cb_col0[s] * S.mb(s); }
    std::vector<int64_t> land_off;   // per supernode: R_LAND slab (ld = mb) in the work arena, -1
    int64_t panel_total = 0;     // doubles (incl. the PNB tail the TRSM reads past)
    int64_t work_total = 0;      // doubles: high-water mark of the interval plan
    int64_t work_live_max = 0;   // doubles: max over levels of the live region sizes (lower bound)
    // per supernode, or empty (every front whole): the front columns [0, asm_end) this rank's
    // large-front assembly fills (schedule.cpp emit_assembly; DevPlan.asm_end)
    std::vector<int32_t> asm_end;
    DevPlan P {};                // pools + device copies of panel_off / cb_off / asm_end
};
// Plan rank `rank`'s regions (D == nullptr: single device, every front here);
// `placed` (optional) receives every work-arena region with its lifetime.
struct PlacedRegion {
    int64_t off, size;
    int32_t t0, t1;
};
int64_t plan_rank_memory(const Symbolic& S, const DistPlan* D, int rank, RankMem& R,
                         std::vector<PlacedRegion>* placed = nullptr);
// Panel arena of `rank` alone: panel_off per supernode (-1 = no copy here); returns
// the arena size in doubles (incl. the PNB tail the TRSM reads past)
int64_t plan_rank_panels(const Symbolic& S, const DistPlan* D, int rank, std::vector<int64_t>& panel_off);
int64_t plan_check(const Symbolic& S, int nranks);
// Physical location of logical element (row, col) of region (kind, s) on R: arena
// (0 panel, 1 work), offset in doubles and leading dimension.  false: not on R.
bool region_addr(const Symbolic& S, const DistPlan* D, const RankMem& R, int kind, int s, int row, int col,
                 int& arena, int64_t& off, int64_t& ld);
// Region lifetimes of the plan, in assembly-tree levels (exposed for tests):
// fills the peak and the lower bound of the work arena of every rank.
int64_t plan_memory_stats(const Symbolic& S, int nranks, int64_t* panel_doubles, int64_t* work_doubles,
                          int64_t* work_lower_bound);

// transport argument of numeric_create_dist selecting the dry mode
#define DIST_DRY ((int32_t(*)(void*, int32_t, int32_t, void*, int64_t))1)

// One transfer of a comm step, device addresses resolved.
enum MsgOp : int32_t { MSG_SEND = 0, MSG_RECV = 1, MSG_COPY = 2 };
struct Msg {
    double* buf;      // staging slot (packed rows x cols), or the region itself when contiguous
    double* src_buf;  // MSG_COPY (both ends hosted, device-copy transport): the sender's slot
    int64_t count;    // doubles
    int32_t peer;     // communicator rank of the other end
    int32_t op;       // MsgOp
};

// Which kernel instance a launch of its kind uses (Launch::var), in CallKind order.
enum SmallVar : int32_t { SMALL_FRONTS = 0, SMALL_CHAIN, SMALL_TINY_TREE, SMALL_TINY_DENSE };
enum AsmVar : int32_t { ASM_BY_COLS = 0, ASM_TILED, ASM_TILED_LIM };
enum TrsmVar : int32_t { TRSM_FUSED = 0, TRSM_PRE, TRSM_PARTIAL };

struct Launch {
    int32_t kind;
    int32_t var;      // L_SMALL: SmallVar, L_ASM: AsmVar, L_TRSM: TrsmVar; 0 for the other kinds
    int32_t level;
    int64_t off;      // first task in the kind's task array
    int64_t toff;     // first tile in the SYRK tile list
    int32_t count;    // grid size (tiles for SYRK launches; the event of L_RECORD / L_WAIT)
    int32_t ntasks;   // tasks (SYRK launches)
    int32_t maxm;     // L_SMALL: LDS edge (tiny dense: n)
    int32_t big;      // CB launch covering fronts with w >= 256
    int32_t bt;       // SYRK tile edge (64 or 128)
    int32_t epi;      // SYRK instance tag: critical-path panel updates and short-K CB launches (profiles)
    int32_t lean;     // SYRK on 64 x 64 tiles with half the LDS (deepest K <= syrk_lean_kmax)
    int32_t pf;       // panel update carrying pre-factor workgroups (GemmTask.pf; 64 x 64 tiles)
    int32_t strm;     // 0 = main stream, 1 = lookahead stream, 2 = comm stream
    int32_t vr;       // hosted rank whose DevPlan the kernel uses
    double flops;     // algorithmic SYRK flops, 2 K per lower-trapezoid entry
    double bytes;     // algorithmic HBM bytes of a SYRK launch (numeric_syrk_bytes)
    // L_COMM: copy tiles [poff, poff + pcount) pack the sends, [uoff, uoff + ucount)
    // unpack the receives (Numeric::d_ctiles)
    int64_t poff, uoff;
    int32_t pcount, ucount;
    int32_t step;
    int32_t tail;     // CB launch holding the re-cut last round of the launch before it (cb_tail_split)
};

// The call a schedule entry stands for: the launcher and the kernel instance it picks.
// launch_one (numeric.cpp) dispatches on it and the schedule digest (digest.cpp) hashes
// it, so the two cannot disagree.
enum CallKind : int32_t {
    C_FRONT_SMALL = 0,  // one workgroup per small front
    C_CHAIN,            // a run of single-front levels in one workgroup
    C_TINY_TREE,        // the whole tree in one workgroup
    C_TINY_DENSE,       // the whole matrix in one wave
    C_ASM_COLS,         // column-streaming assembly
    C_ASM_TILED,        // write-once tile assembly
    C_ASM_TILED_LIM,    // tile assembly with per-task column limits (distributed assembly)
    C_POTRF,
    C_TRSM_FUSED,       // full 64-column blocks, POTRF fused
    C_TRSM_PRE,         // full blocks whose L11 is already in place
    C_TRSM_PARTIAL,     // partial last blocks (nb < 64)
    C_SYRK_PANEL,
    C_SYRK_CB,
    C_COMM,
    C_RECORD,
    C_WAIT,
    C_KINDS
};
inline CallKind decode_call(const Launch& L) {
    switch (L.kind) {
        case L_SMALL: return CallKind(C_FRONT_SMALL + L.var);
        case L_ASM: return CallKind(C_ASM_COLS + L.var);
        case L_POTRF: return C_POTRF;
        case L_TRSM: return CallKind(C_TRSM_FUSED + L.var);
        case L_PANEL: return C_SYRK_PANEL;
        case L_CB: return C_SYRK_CB;
        case L_COMM: return C_COMM;
        case L_RECORD: return C_RECORD;
        case L_WAIT: return C_WAIT;
    }
    return C_KINDS;
}

// Digest of a schedule (digest.cpp): one hash over every decoded entry and every uploaded
// task array (pointers as arena + offset), plus counters of what it issues.
struct SchedDigest {
    uint64_t hash = 0;
    int64_t calls[C_KINDS] = {0};  // entries per CallKind
    int64_t tail_split = 0;        // re-cut CB tail launches
    int64_t pf = 0;                // panel updates carrying pre-factor workgroups
    int64_t comm_steps = 0, events = 0, msgs = 0, gsegs = 0;
    static constexpr int NVALS = 1 + C_KINDS + 6;
};

struct Numeric {
    const Symbolic* S = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // trailing panel updates overlapped with the next slab
    hipStream_t stream3 = nullptr;  // multi-rank: comm stream (pack, transfer group, unpack), strm == 2
    std::vector<hipEvent_t> sync_ev;
    int32_t n_sync_events = 0;
    std::vector<RankMem> R;          // hosted ranks
    std::vector<int64_t> rank_base;  // gathered panel layout: first double of each rank's arena
    std::vector<void*> allocs;
    int64_t dev_bytes = 0;           // device memory held (pools, plan, staging)
    std::vector<Launch> sched;
    SchedDigest digest;              // of sched and the uploaded task arrays
    int32_t* d_small = nullptr;
    ChainPlan CP {};                 // chain launches (runs of single small-front levels)
    TinyPlan TP {};                  // tiny trees: the whole factorization in one workgroup
    int64_t n_chain = 0;             // chained fronts (descriptors)
    int2* d_asm = nullptr;
    int2* d_asml = nullptr;  // per assembly task: owned front columns (distributed-assembly launches)
    int2* d_potrf = nullptr;
    TrsmTask* d_trsm = nullptr;
    int32_t* d_arrive = nullptr;  // fused POTRF + TRSM: per-block arrival counters
    GemmTask* d_gemm = nullptr;
    int2* d_tiles = nullptr;
    GatherTab gtab;              // the CB SYRK extend-add gather's segment tables (schedule.cpp)
    int32_t* d_info = nullptr;       // shared by the hosted ranks' DevPlans
    int32_t* h_info = nullptr;       // pinned host copy, written at the end of each factorization
    static constexpr int32_t STATUS_PENDING = -2;  // h_info before the status kernel's store
    // single-rank handles: device view of h_info; the last launch of a factorization stores
    // the status word there (and re-arms d_info), the host polls it (no memset / copy)
    int32_t* status_dp = nullptr;
    double* d_Ax_owned = nullptr;
    const double* last_Ax = nullptr;
    bool factored = false;
    int64_t factor_gen = 0;          // factorizations enqueued
    int64_t status = 0;
    bool status_valid = false;

    // profiling: 1 = HIP events around every launch (eager runs); 2 = timestamp
    // kernels around the CB SYRK launches only (works inside hipGraph replay)
    int profile = 0;
    uint64_t* d_stamps = nullptr;
    std::vector<int32_t> stamp_of;  // launch -> stamp pair index, -1 = none
    std::vector<hipEvent_t> ev;
    double phase_ms[8] = {0};
    // hipGraph replay
    bool use_graph = false;
    hipGraphExec_t gexec = nullptr;
    hipGraph_t graph = nullptr;
    const double* graph_Ax = nullptr;
    int graph_profiled = 0;

    // multi-rank: this process hosts R (one rank of nranks, or all of them when
    // emulated on one device with private per-rank memory)
    int rank = 0, nranks = 1;
    bool emulated = false;
    int emul_rccl = 0;  // emulated: 1 = hosted-to-hosted transfers as RCCL self send/recv
    std::vector<int32_t> owner;  // empty = single device
    DistPlan D;
    std::vector<Msg> msgs;
    Copy2D* d_copy = nullptr;     // pack / unpack descriptors
    int2* d_ctiles = nullptr;     // (descriptor, first column) per copy workgroup
    double* staging = nullptr;    // packed slots of the hosted ranks' messages
    void* comm = nullptr;  // ncclComm_t
    // host-staged transport (tests: several processes on one GPU, no RCCL):
    // op 0 post send, 1 post recv, 2 complete everything posted
    int32_t (*xport)(void* ctx, int32_t op, int32_t peer, void* buf, int64_t bytes) = nullptr;
    void* xport_ctx = nullptr;
    bool dry_comm = false;  // comm steps pack / unpack but move nothing (one-rank timing projection)

    // gathered factor (every supernode's panel in the rank_base layout): the panel
    // arena itself for single-device and emulated handles, else gathered on demand
    double* gpanel = nullptr;
    bool gpanel_owned = false;
    int64_t gather_gen = -1;         // factor_gen the gathered copy belongs to
    std::vector<int64_t> gpo;        // per supernode: offset in gpanel
    int64_t* d_gpo = nullptr;
    struct SlabFix {                 // gathered copy of a slab another rank factored
        int64_t src, dst, ld;        // doubles into gpanel
        int32_t rows, cols;
    };
    std::vector<SlabFix> fix;

    // triangular solves (built at the first solve)
    struct SolveStep {
        int64_t doff, goff, foff, gaoff;
        int32_t dcount, gcount, fcount, gacount;  // gacount: forward-gather fronts (level's first step)
    };
    std::vector<SolveStep> solve_steps;  // forward order (levels up, k0 up)
    bool solve_ready = false;
    SolvePlan SP {};
    int4* d_sdiag = nullptr;         // 128-column diagonal blocks (s, k0, first GEMV task, GEMV tasks)
    int32_t* d_sgather = nullptr;    // forward gather: fronts with children, per level
    int64_t u_total = 0;             // doubles of SP.u (sum of the fronts' mb)
    int2* d_sinv = nullptr;          // 64-column blocks (s, k0): inverse preparation
    int2* d_sinv2 = nullptr;         // 128-column blocks wider than 64: off-diagonal inverse quadrant
    int32_t n_sinv = 0, n_sinv2 = 0;
    int64_t inv_gen = -1;            // factor_gen whose diagonal-block inverses are in place
    int4* d_sgemv = nullptr;         // backward GEMV tasks (s, k0, r0)
    int4* d_sfwd = nullptr;  // fused forward steps (s, k0, r0, writer)
    int32_t* d_post = nullptr;
    double* d_sbuf = nullptr;  // host-interface staging (b in, x out)
    bool solve_eager = false;  // debug: launch the sweeps directly instead of the graphs
    // panel family (SOLVE_RHS right-hand sides): the plan's 16-wide buffers, allocated at
    // the first panel sweep
    bool multi_ready = false;
    SolvePlan SPM {};
    int64_t solve_max_g = 1;           // most GEMV workgroups in one backward step
    double* d_mbuf = nullptr;          // io (n x SOLVE_RHS column-major), c, y (SOLVE_RHS-wide rows)
    // the solves and the factor operators (numeric_apply_*): the etree postorder alone
    // (d_post itself when no fill-reducing permutation is in effect), uploaded at the first
    // L-level op, and one lazily captured graph per family (0 single vector, in and out
    // through d_sbuf; 1 panel, through d_mbuf's io) and op (sc_factor_op; the solves are
    // SC_OP_SOLVE_A)
    static constexpr int APPLY_OPS = 7;
    int32_t* d_etpost = nullptr;
    hipGraph_t apply_graph[2][APPLY_OPS] = {};
    hipGraphExec_t apply_gexec[2][APPLY_OPS] = {};

    // selected inversion (selinv.cpp; single-device handles): the Z panel arena (gpanel's
    // layout, allocated at the first call, kept), the W scratch of the largest step and the
    // task lists, in execution order: levels down, 128-column steps down
    struct SelStep {
        int64_t toff, koff, roff, poff;  // first W / Z_RK tile, Z_KK task, Z_KK reduction, push task
        int32_t tcount, kcount, rcount, pcount;  // pcount > 0 only after a level's last block (k0 = 0)
    };
    std::vector<SelStep> sel_steps;
    bool sel_ready = false;
    SelPlan SEL {};
    int2* d_seltile = nullptr;
    int4* d_selkk = nullptr;
    int4* d_selred = nullptr;
    int4* d_selpush = nullptr;
    int64_t sel_gen = -1;              // factor_gen the Z panel belongs to
    bool sel_profile = false;          // HIP events around every launch of the next calls
    double sel_ms[4] = {0, 0, 0, 0};   // last profiled call: W, Z_RK, Z_KK, push (ms)

    // rank-k update / downdate (updown.cpp; single-device handles): the n x UPD_W workspace,
    // the T scratch, the sweep's own status word and the staging of one chunk's entries
    // (UPD_W columns of at most the longest column of L each), allocated at the first call, kept
    bool upd_ready = false;
    UpdPlan UPD {};
    int64_t* d_uidx = nullptr;
    double* d_uval = nullptr;
    int64_t upd_cap = 0;               // entries d_uidx / d_uval hold

    // Schur complement (schur.cpp; single-device handles of a Schur analysis): D = L_SS
    // (ns x ns, ld = ns), gathered once per generation of the factor, the per-column
    // (supernode, local column) table and the index set, allocated at the first use; the
    // n x SCHUR_RHS panel of the partial solves at the first of those
    bool sch_ready = false;
    SchurPlan SCH {};
    double* d_schD = nullptr;
    int32_t* d_schidx = nullptr;
    int64_t sch_gen = -1;              // factor_gen the gathered D belongs to
    double* d_schW = nullptr;

    // products with A and iterative refinement (refine.cpp; single-device handles): A as a
    // gather structure with its task lists and partial slots, the transposed X panel, the
    // R / D panel (n x SOLVE_RHS, ld = n) and the norm scratch, allocated at the first use, kept
    bool spmv_ready = false;
    SpmvPlan SPMV {};
    double* d_rfxt = nullptr;
    double* d_rfR = nullptr;
    double* d_rfnorm = nullptr;        // SPMV_NQ + 1 rows of SOLVE_RHS norms, then the increment norm's partials

    // preconditioned conjugate gradients (pcg.cpp; single-device handles), besides the above:
    // the z, p and q panels (n x SOLVE_RHS, ld = n), the partials of the sums (PCG_NQ x
    // SOLVE_RHS doubles per PCG_ROWS rows) and the scalar block (two results of PCG_NQ x
    // SOLVE_RHS doubles), allocated at the first use, kept
    bool pcg_ready = false;
    double* d_pcgZ = nullptr;
    double* d_pcgP = nullptr;
    double* d_pcgQ = nullptr;
    double* d_pcgpart = nullptr;
    double* d_pcgscal = nullptr;

    // block Lanczos eigensolver (eigs.cpp; single-device handles), besides the product's buffers:
    // the basis of eigs_blocks + 1 panels (n x SOLVE_RHS, ld = n), the Gram partials
    // (eigs_groups(n) x eigs_blocks tiles), the coefficient buffer (2 eigs_blocks tiles) -- all
    // three replaced by larger ones when a call asks for more blocks -- and the residual panel
    int32_t eigs_blocks = 0;
    double* d_egV = nullptr;
    double* d_egpart = nullptr;
    double* d_egC = nullptr;
    double* d_egY = nullptr;

    // gradients on A's pattern (grad.cpp; single-device handles): the effective entries (row,
    // column, slot) in slot order, the ignored slots, the two transposed panels of the outer
    // product (SOLVE_RHS-wide rows) and the dot's partials with its result behind them,
    // allocated at the first use, kept
    bool grad_ready = false;
    GradEntry* d_gent = nullptr;
    int64_t* d_gign = nullptr;
    int64_t grad_ne = 0, grad_nign = 0;
    double* d_gut = nullptr;
    double* d_gvt = nullptr;
    double* d_gpart = nullptr;

    std::string err;
};

// Host-only planning of a handle (no device needed): the hosted ranks (N.R), their
// memory plans and the gathered panel layout.  N.rank / nranks / emulated / owner / D
// are set by the caller.
int64_t numeric_plan_host(Numeric& N, const Symbolic& S);
// Builds the memory plan, pools and schedule of the hosted ranks.
int64_t numeric_init(Numeric& N, const Symbolic& S, int device);
// The digest of the schedule a handle created as numeric_create (nranks == 1, emulate ==
// 0) or numeric_create_dist (emulate: 0 one real rank, 1 device copies, 2 RCCL to self)
// would build, planned on the host with placeholder pool bases.  No HIP call.
int64_t schedule_digest_host(const Symbolic& S, int nranks, int rank, int emulate, SchedDigest& out,
                             std::string& err);
// The SYRK launches of the same host-planned schedule, in schedule order, eight values
// each: kind (0 panel, 1 CB), bt, lean, epi, pf, tail, tiles, any task gathers (gs >= 0).
int64_t schedule_syrk_host(const Symbolic& S, int nranks, int rank, int emulate, std::vector<int64_t>& out,
                           std::string& err);

int64_t numeric_create(const Symbolic& S, int device, Numeric*& out, std::string& err);
int64_t numeric_factor(Numeric& N, const double* d_Ax, bool sync);
int64_t numeric_status(Numeric& N);
// Makes gpanel / gpo hold the whole factor of the last factorization (multi-rank
// handles: a collective exchange of every rank's panel arena; all ranks call it).
int64_t numeric_gather(Numeric& N);
int64_t numeric_export(Numeric& N, int64_t* Lp, int32_t* Li, double* Lx);
// Natural columns [j0, j1) in front-row form (count only when ri == NULL): column j
// holds the rows of its supernode's front from its own position down (natural
// numbering, front order; relaxed zeros included) with their values.  cp[j1-j0+1].
// pool: another arena in gpanel's layout to read the values from (the Z panel), or null.
int64_t numeric_export_cols(Numeric& N, int64_t j0, int64_t j1, int64_t* cp, int32_t* ri, double* rx,
                            const double* pool = nullptr);
int64_t numeric_timing(Numeric& N, double* t, int nt);
int64_t numeric_level_times(Numeric& N, double* ms, int nl);
int64_t numeric_launch_trace(Numeric& N, int32_t* kind, int32_t* level, int32_t* strm, double* ms, double* flops,
                             int64_t cap);
int64_t numeric_syrk_stats(Numeric& N, int wmin, double* flops, double* ms, int64_t* launches);
int64_t numeric_syrk_bytes(Numeric& N, int wmin, double* bytes);
int64_t numeric_launch_times(Numeric& N, double* t0, double* t1, int32_t* kind, int32_t* step, int32_t* strm,
                             int64_t cap);
void numeric_free(Numeric* N);
// x = A^{-1} b with the factor: device vectors of length n (may alias), on the
// library stream, synchronous.  Multi-rank handles gather the factor first
// (collective) and every rank solves with the whole factor.
int64_t numeric_solve_device(Numeric& N, const double* d_b, double* d_x);
int64_t numeric_solve_host(Numeric& N, const double* b, double* x);
// X = A^{-1} B for nrhs right-hand sides, column-major (ldb, ldx >= n), in panels of
// SOLVE_RHS columns through the panel kernels (also for nrhs == 1); a partial last panel
// is padded with zero columns in the handle's own buffers.  d_X may be d_B when ldx ==
// ldb.  Status, ordering and collective rules of numeric_solve_device.
int64_t numeric_solve_device_multi(Numeric& N, int32_t nrhs, const double* d_B, int64_t ldb, double* d_X,
                                   int64_t ldx);
int64_t numeric_solve_host_multi(Numeric& N, int32_t nrhs, const double* B, int64_t ldb, double* X, int64_t ldx);
// Factor operators (op: sc_factor_op; L in the numbering of numeric_export, the order of
// P A P^T): X = op(B).  The single-vector entry points run the single-vector kernels for
// the half solves; the products have panel kernels only, so a single vector travels as a
// panel of one column.  numeric_solve_* are SC_OP_SOLVE_A.  Buffers, status, ordering and
// collective rules of the solves; x may be b.
int64_t numeric_apply_device(Numeric& N, int32_t op, const double* d_b, double* d_x);
int64_t numeric_apply_host(Numeric& N, int32_t op, const double* b, double* x);
int64_t numeric_apply_device_multi(Numeric& N, int32_t op, int32_t nrhs, const double* d_B, int64_t ldb, double* d_X,
                                   int64_t ldx);
int64_t numeric_apply_host_multi(Numeric& N, int32_t op, int32_t nrhs, const double* B, int64_t ldb, double* X,
                                 int64_t ldx);
// log det A = 2 sum_j log L(j, j), reduced on the device in a fixed order.
int64_t numeric_logdet(Numeric& N, double* logdet);
// Selected inversion: Z = (P A P^T)^-1 on the pattern of L into the handle's Z panel
// (synchronous).  Status rules of the solves; multi-rank and emulated handles:
// SC_ERR_NOTIMPL.  The accessors compute first when the Z panel does not belong to the
// current factorization: diag in A's own order, the export in numeric_export's layout.
int64_t numeric_selinv(Numeric& N);
int64_t numeric_selinv_diag_device(Numeric& N, double* d_d);
int64_t numeric_selinv_diag_host(Numeric& N, double* d);
int64_t numeric_selinv_export(Numeric& N, int64_t* Lp, int32_t* Li, double* Zx);
// numeric_export_cols of the Z panel (for factors too large for numeric_selinv_export)
int64_t numeric_selinv_export_cols(Numeric& N, int64_t j0, int64_t j1, int64_t* cp, int32_t* ri, double* rx);
// Dense flops of the sweep from the symbolic structure (the formula of sc_selinv_flops).
double selinv_flops(const Symbolic& S);
// Rank-k update / downdate (updown.cpp).  updown_check: host only.  W (n x k, CSC, rows in
// A's own numbering) is admissible when every column w, permuted to the order of P A P^T,
// has struct(w) within struct(L(:, j0)), j0 its smallest row (tested entry by entry with the
// row-subtree walk of ereach, the pattern of L is never formed).  first_col[k] (may be
// null): j0 per column, -1 for an empty one; path[3] (may be null): touched supernodes,
// their 64-column blocks, their panel entries.  SC_ERR_ARG with `err` = who + ": " + reason.
int64_t updown_check(const Symbolic& S, int32_t k, const int64_t* Wp, const int32_t* Wi, int32_t* first_col,
                     int64_t* path, const char* who, std::string& err);
// L <- factor of P (A + sign W W^T) P^T in place, in chunks of UPD_W columns, synchronous
// on the handle's stream.  Returns SC_OK, or the first failing column + 1 of a downdate
// that leaves the matrix not positive definite (L partly modified; that becomes the
// handle's status until the next factorization).
int64_t numeric_updown_host(Numeric& N, int32_t sign, int32_t k, const int64_t* Wp, const int32_t* Wi,
                            const double* Wx);
// Schur complement of the index set a Schur analysis ordered last (schur.cpp, DESIGN.md
// section 9.4): D = L_SS and S_c = D D^T, ns x ns column-major in the caller's numbering
// (row / column q is schur_idx[q]), and the two partial solves around S_c (B, X: n x nrhs in
// A's order; G, XS: ns x nrhs).  Synchronous on the handle's stream; status rules of the
// selected inversion; a handle without a Schur set: SC_OK, nothing touched (expand: the solve).
int64_t numeric_schur_factor(Numeric& N, double* D, int64_t ldd, bool host);
int64_t numeric_schur_matrix(Numeric& N, double* S, int64_t lds, bool host);
int64_t numeric_schur_condense(Numeric& N, int32_t nrhs, const double* B, int64_t ldb, double* G, int64_t ldg,
                               bool host);
int64_t numeric_schur_expand(Numeric& N, int32_t nrhs, const double* B, int64_t ldb, const double* XS, int64_t ldxs,
                             double* X, int64_t ldx, bool host);
// Products with A, residuals and iterative refinement (refine.cpp),
// in panels of SOLVE_RHS columns; all arrays column-major in A's own order, device or host
// memory by `host` (the host forms stage their arrays for the length of the call).  Ax: the
// values in the order of the analysed pattern, or null for the copy sc_factor made (SC_ERR_ARG
// when the last factorization was not an sc_factor).  Synchronous on the handle's stream.
// The product and the residual never look at the factor.  mode: SC_RESIDUAL_*.
int64_t numeric_spmv(Numeric& N, int32_t nrhs, const double* Ax, const double* X, int64_t ldx, double* Y, int64_t ldy,
                     bool host, const char* who);
int64_t numeric_residual(Numeric& N, int32_t mode, int32_t nrhs, const double* Ax, const double* B, int64_t ldb,
                         const double* X, int64_t ldx, double* R, int64_t ldr, double* berr_norm, double* berr_comp,
                         bool host, const char* who);
// X = A^-1 B by the panel solve plus refinement steps against Ax; status rules of the solves,
// multi-rank and emulated handles SC_ERR_NOTIMPL.  opt: validated by the caller.
int64_t numeric_solve_refine(Numeric& N, const sc_refine_options& opt, int32_t nrhs, const double* Ax, const double* B,
                             int64_t ldb, double* X, int64_t ldx, sc_refine_info* info, bool host, const char* who);
// X = A'^-1 B by conjugate gradients on the values Ax, preconditioned with the factor (pcg.cpp,
// DESIGN.md section 9.6); arguments, values and status rules as numeric_solve_refine.  opt:
// validated by the caller; with opt.use_x0 X holds the starting vectors on entry.
int64_t numeric_solve_pcg(Numeric& N, const sc_pcg_options& opt, int32_t nrhs, const double* Ax, const double* B,
                          int64_t ldb, double* X, int64_t ldx, sc_pcg_info* info, bool host, const char* who);
// One vector kernel of the conjugate gradients alone on caller panels (device), synchronous;
// include/sparsecholesky_debug.h has the contract.
int64_t debug_pcg_vec(int32_t which, int32_t n, int32_t nrhs, uint32_t mask, const double* coef, double* dA,
                      int64_t lda, double* dB, int64_t ldb, const double* dC, int64_t ldc, const double* dD, int64_t ldd,
                      double* dT, double* out, std::string& err);
// The nev eigenpairs of the factored matrix nearest zero by block shift-invert Lanczos (eigs.cpp,
// DESIGN.md section 9.7); values and status rules as numeric_solve_refine.  opt and the
// arguments: validated by the caller.  lambda and info are host arrays in both forms.
int64_t numeric_eigs(Numeric& N, const sc_eigs_options& opt, int32_t nev, const double* Ax, const double* X0,
                     int64_t ldx0, double* lambda, double* X, int64_t ldx, sc_eigs_info* info, bool host,
                     const char* who);
// Gradients on A's pattern (grad.cpp).  G, H: arrays of the length and
// order of the analysed pattern's values; an effective entry is a slot the analysis uses (the
// set of spmv_structure's sp), every other slot of an output is written +0.0.  U, V, X, Xbar,
// Bbar: n x nrhs column-major in A's own order.  Device or host memory by `host`; synchronous
// on the handle's stream; multi-rank and emulated handles SC_ERR_NOTIMPL.  Arguments are
// validated by the caller.
//   pattern_outer  G_k = beta G_k + alpha sum_c (U[i,c] V[j,c] + [i != j] U[j,c] V[i,c]); never
//                  looks at the factor
//   pattern_dot    *out (host) = sum over the effective entries of G_k H_k
//   logdet_grad    G_k = c_k inv(A)[i_k, j_k] from the Z panel (computed first when it does
//                  not belong to the current factorization); status rules of the selected inversion
//   solve_grad     Bbar = the panel solve of Xbar, G = pattern_outer(-1, Bbar, X, 0)
int64_t numeric_pattern_outer(Numeric& N, double alpha, int32_t nrhs, const double* U, int64_t ldu, const double* V,
                              int64_t ldv, double beta, double* G, bool host, const char* who);
int64_t numeric_pattern_dot(Numeric& N, const double* G, const double* H, double* out, bool host, const char* who);
int64_t numeric_logdet_grad(Numeric& N, double* G, bool host, const char* who);
int64_t numeric_solve_grad(Numeric& N, int32_t nrhs, const double* Xbar, int64_t ldxb, const double* X, int64_t ldx,
                           double* Bbar, int64_t ldbb, double* G, bool host, const char* who);
// eigs.cpp's host dense algebra (include/sparsecholesky_debug.h: sc_debug_eigs_dense)
bool eigs_sym_eig(int m, double* a, double* d);
int eigs_chol_inv(const double* G, int b, double thr, double* rinv);
// The Gram and the block-update kernel alone on caller panels (device), synchronous;
// include/sparsecholesky_debug.h has the contracts.
int64_t debug_eigs_gram(int32_t n, int32_t b, int32_t nb, const double* dV, int64_t ldv, int64_t vstride,
                        const double* dW, int64_t ldw, double* out, std::string& err);
int64_t debug_eigs_update(int32_t n, int32_t b, int32_t bc, int32_t nb, double beta, double* dOut, int64_t ldo,
                          const double* dW, int64_t ldw, const double* dV, int64_t ldv, int64_t vstride,
                          const double* C, std::string& err);
// The kernels alone on a caller's structure (host arrays, validated: rp ascending from 0, ci
// in [0, n), sp in [0, nval)) and values and panels (device pointers), synchronous: mode
// SpmvMode; X, B, R, W column-major n x nrhs (nrhs <= SOLVE_RHS); W and norms (SPMV_NQ x
// SOLVE_RHS, device) may be null.
int64_t debug_spmv(int32_t mode, int32_t n, const int64_t* rp, const int32_t* ci, const int64_t* sp, int64_t nval,
                   const double* d_Ax, int32_t nrhs, const double* d_X, int64_t ldx, const double* d_B, int64_t ldb,
                   double* d_R, int64_t ldr, double* d_W, int64_t ldw, double* d_norms, std::string& err);
// The product kernel alone on caller data (device), synchronous.
int64_t debug_schur_llt(const double* dD, int32_t ns, int64_t ldd, double* dS, int64_t lds);
// The two kernels of one block step on block k0 of a caller's m x w panel and m x UPD_W
// workspace (device; dW row-major, row = front row), through a one-front plan.
int64_t debug_updown_block(double* dF, int m, int w, int k0, double* dW, int sign, int32_t* info);
// One 128-column step of the solve family on block k0 of a caller's m x w panel through a
// one-front plan whose row list is the identity (op 0 inverses, 1 forward, 2 backward, 3 L Z,
// 4 L^T Z; width 1 or SOLVE_RHS), and the forward gather of one parent front from nchild
// children (rel_ptr, relind: host).  include/sparsecholesky_debug.h has the contracts.
int64_t debug_solve_step(double* dF, int m, int w, int k0, int op, int width, double* dC, double* dY, double* dU);
int64_t debug_solve_gather(int width, int w, int mb, int nchild, const int64_t* rel_ptr, const int32_t* relind,
                           const double* dUc, double* dC, double* dU);
// One step of the selected inversion on block k0 of a caller's m x w L and Z panels through a
// one-front plan whose row list is the identity (op 0 W = L_RK X, 1 Z_RK = -Z_RR W with its
// mirror, 2 Z_KK), cut by selinv_cut_block; returns the workgroups launched.  And the push of
// one child's Z_II (mbc rows at the parent positions relind, host) out of a parent front (m,
// w).  include/sparsecholesky_debug.h has the contracts; err: the reason of an SC_ERR_ARG.
int64_t debug_selinv_step(const double* dL, double* dZ, int m, int w, int k0, int op, const double* dZii, double* dW,
                          std::string& err);
int64_t debug_selinv_push(int m, int w, const double* dZ, const double* dZii, int mbc, const int32_t* relind,
                          double* dOut, std::string& err);
// One of the four extend-add implementations on one parent front (m, w) with prescribed
// children and A entries (host index arrays, validated; device values), through a one-parent
// plan whose bounds, gather table and tasks come from block_bounds, gather_segments_front and
// asm_block_tasks: op 0 assemble_cols_kernel (p0 = ncol), 1 assemble_tile_kernel (p0 = ncol,
// [p1, p2) = the tasks' column limits or both < 0), 2 front_small_kernel (p0 = the bucket), 3
// the gathering CB SYRK (p0 = bt, p1 = lean, p2 = epi).  *info: the status word (failing panel
// column + 1, or 0).  include/sparsecholesky_debug.h has the contract.
int64_t debug_extend_add(int op, int m, int w, int nchild, const int64_t* rel_ptr, const int32_t* relind,
                         const int64_t* a_ptr, const int32_t* a_pos, const int64_t* a_src, int64_t nval,
                         const double* dAx, const double* dKids, double* dPanel, double* dCb, int p0, int p1, int p2,
                         int32_t* info, std::string& err);
// Destroys the captured graphs of the solves and operators (they point at one panel pool).
void numeric_drop_solve_graphs(Numeric& N);
int64_t debug_syrk(double* dC, int ldc, const double* dA, int lda, int M, int N, int K);
// debug_syrk on the instance the caller names: bt 64 / 128, lean (64 only), tag, epi; no
// gather, no pre-factor.  SC_ERR_ARG on an inconsistent combination, before any HIP call.
int64_t debug_syrk_ex(double* dC, int ldc, const double* dA, int lda, int M, int N, int K, int bt, int lean, int tag,
                      int epi);
// The panel kernels on block k0 of a caller's m x w front panel (device, column-major, ld =
// m) through a one-front plan with an identity post table; mode 0 POTRF alone, 1 the fused
// TRSM, 2 POTRF then the prefactored TRSM, 3 (partial blocks) POTRF then the partial TRSM.
// *info: the status word (first failing column + 1, or 0).
int64_t debug_panel(double* dF, int m, int w, int k0, int mode, int32_t* info);
int64_t numeric_chain_stamps(Numeric& N, int enable, uint64_t* out, int64_t cap);
int64_t debug_bench(int which, int M, int K, int reps, int arg, double* tflops);
int64_t debug_contention(int M, int K, int chain_rows, int nchain, int mode, int mask_stride, double* out);

}  // namespace sc
