// extern "C" boundary (include/sparsecholesky.h).  Every entry point runs under the guard of
// capi_guard.hpp: validators say why with fail(), the guard adds the entry point's name, copies
// the handle's message and keeps exceptions inside.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/sparsecholesky.h"
#include "../../include/sparsecholesky_debug.h"
#include "capi_guard.hpp"
#include "normal_ops.hpp"
#include "numeric.hpp"
#include "symbolic.hpp"

namespace sc {
i64 triplet_to_csc(i64 n, i64 nt, const i32* ti, const i32* tj, const double* tx, i64* Ap, i32* Ai,
                   double* Ax);
i64 read_mtx(const char* path, i64* n_out, i64* Ap, i32* Ai, double* Ax);
i64 compute_supernodes_ref(i64 n, const i32* parent, const i64* cp, i32* sn_id, i64* supernodes);
i64 atree_ref(i64 n, const i64* Lp, const i32* Li, const i32* sn_id, const i64* supernodes, i64 ns,
              i32* super_parent);
i64 laplacian3d(i64 k, int nd, i64* Ap, i32* Ai, double* Ax, i32* perm_out);
i64 dist_owner_map(const Symbolic& S, int nranks, i32* owner, double* work);
i64 dist_schedule(const Symbolic& S, int nranks, int rank, i32* level, i32* peer, i64* bytes, i32* is_send,
                  i64 cap);
i64 numeric_create_dist(const Symbolic& S, int device, int rank, int nranks, const void* id128,
                        int32_t (*xport)(void*, int32_t, int32_t, void*, int64_t), void* xport_ctx, int emulate,
                        Numeric*& out, std::string& err);
i64 dist_unique_id(void* id128);
}  // namespace sc

struct sc_symbolic {
    sc::Symbolic S;
};
struct sc_numeric {
    sc::Numeric* N = nullptr;
    const sc_symbolic* sym = nullptr;
};
struct sc_normal {
    sc::Normal* N = nullptr;
};

using sc::fail;
using sc::guarded;
using sc::guarded_or;

// The guard for an entry point whose first parameter is a handle: a null handle is SC_ERR_ARG
// "null handle", and a numeric or normal handle's own message is carried over.
template <class F>
static int64_t entry(const char* who, const sc_symbolic* sym, F&& f) {
    return guarded(who, [&]() -> int64_t { return sym ? f() : fail("null handle"); });
}
template <class F>
static int64_t entry(const char* who, const sc_numeric* num, F&& f) {
    if (!num || !num->N) return guarded(who, [] { return fail("null handle"); });
    return guarded(who, *num->N, f);
}
template <class F>
static int64_t entry(const char* who, const sc_normal* normal, F&& f) {
    if (!normal) return guarded(who, [] { return fail("null handle"); });
    return guarded(who, *normal->N, f);
}

// An options argument: null stands for the defaults, a struct_size of another header is refused.
template <class O>
static int64_t options_arg(const O* opt, void (*defaults)(O*), const char* type, const char* init, O& o) {
    defaults(&o);
    if (!opt) return SC_OK;
    if (opt->struct_size != (int32_t)sizeof(O))
        return fail(std::string(type) + ".struct_size does not match this library's sizeof(" + type +
                    "): initialise the options with " + init);
    o = *opt;
    return SC_OK;
}

// The arrays of nrhs columns: a leading dimension below the row count, or a null array that
// would be read or written.  rows < 0 stands for n.
struct PanelArg {
    const void* p;
    int64_t ld;
    const char* name;
    int64_t rows = -1;
    const char* rows_name = "n";
};
static int64_t panel_args(int64_t n, int32_t nrhs, std::initializer_list<PanelArg> arrays) {
    if (nrhs < 0) return fail("nrhs < 0");
    for (const PanelArg& a : arrays) {
        const int64_t rows = a.rows < 0 ? n : a.rows;
        if (a.ld < rows) return fail(std::string("leading dimension of ") + a.name + " below " + a.rows_name);
        if (nrhs > 0 && rows > 0 && !a.p) return fail(std::string("null ") + a.name);
    }
    return SC_OK;
}

// A numeric handle on sym: make() is the sc:: creator, bad says that another argument is wrong.
template <class F>
static int64_t numeric_create(const char* who, const sc_symbolic* sym, bool bad, sc_numeric** out, F&& make) {
    return sc::guarded_create(who, out, [&](sc_numeric& h) -> int64_t {
        if (!sym) return fail("null handle");
        if (bad) return SC_ERR_ARG;
        h.sym = sym;
        return make(h.N, sc::last_error());
    });
}

extern "C" {

int32_t sc_version(void) { return SC_VERSION; }

const char* sc_status_string(int64_t st) { return sc::status_string(st); }

const char* sc_last_error(void) { return sc::last_error().c_str(); }

void sc_default_options(sc_options* opt) {
    if (!opt) return;
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(sc_options);
    opt->relax = 1;
    opt->nrelax[0] = 4;
    opt->nrelax[1] = 16;
    opt->nrelax[2] = 48;
    opt->zrelax[0] = 0.8;
    opt->zrelax[1] = 0.1;
    opt->zrelax[2] = 0.05;
    opt->small_front_max = 128;
    opt->panel_nb = 64;
    opt->panel_nb_outer = 1024;
    opt->use_graph = 0;
    opt->relax_wmax = 1;
    opt->syrk_tile = 0;
    opt->lookahead = 1;
    opt->inner_order = 1;
    opt->asm_tile_min_m = 0;
    opt->dist_split = 1;
    opt->dist_cbb = 1024;
    opt->dist_early = 1;
    opt->dist_panel = 1;
    opt->cb_gather = 1;
    opt->dist_slab_block = 2;
    opt->trsm_split_wg = 1024;
    opt->syrk_lean_kmax = 128;
    opt->cb_tail_split = 1;
    opt->tiny_dense = 1;
    opt->dist_asm = 1;
    opt->dist_pieces = 4;
    opt->dist_local_pieces = 1;
    opt->panel_prefactor = 1;
}

// sc_analyze (ns == 0) and sc_analyze_schur (the list validated, ns > 0): the latter
// factors P A P^T with the interior ordered by opt->ordering and schur_idx last.
static int64_t analyze_into(sc_symbolic& h, int64_t n, const int64_t* Ap, const int32_t* Ai, const sc_options* opt,
                            int32_t ns, const int32_t* schur_idx) {
    sc_options o;
    int64_t rc = options_arg(opt, sc_default_options, "sc_options", "sc_default_options() from the matching header", o);
    if (rc != SC_OK) return rc;
    if (o.small_front_max > 128) o.small_front_max = 128;
    if (o.small_front_max < 0) o.small_front_max = 0;
    if (o.lookahead != 0 && o.lookahead != 1) return fail("sc_options.lookahead must be 0 or 1");
    if (o.inner_order != 0 && o.inner_order != 1) return fail("sc_options.inner_order must be 0 or 1");
    if (o.ordering != SC_ORDER_NATURAL && o.ordering != SC_ORDER_ND && o.ordering != SC_ORDER_AMD)
        return fail("sc_options.ordering must be SC_ORDER_NATURAL, SC_ORDER_ND or SC_ORDER_AMD");
    std::string& err = sc::last_error();
    if (!((o.ordering != SC_ORDER_NATURAL || ns > 0) && n > 0 && Ap && (Ai || Ap[n] == 0)))
        return sc::analyze(n, Ap, Ai, o, h.S, err);
    // factor B = P A P^T; numeric values still come from A's arrays (a_src remapped)
    std::vector<int32_t> perm((size_t)n);
    std::vector<int64_t> Bp, src;
    std::vector<int32_t> Bi;
    // the CSC checks analyze() makes, before the ordering walks the arrays
    rc = Ap[0] == 0 ? SC_OK : SC_ERR_ARG;
    for (int64_t j = 0; rc == SC_OK && j < n; ++j)
        if (Ap[j + 1] < Ap[j]) rc = SC_ERR_ARG;
    for (int64_t p = 0; rc == SC_OK && p < Ap[n]; ++p)
        if (Ai[p] < 0 || Ai[p] >= n) rc = SC_ERR_ARG;
    if (rc != SC_OK) return fail("malformed CSC");
    rc = ns > 0 ? sc::schur_order(n, Ap, Ai, o.ordering, ns, schur_idx, perm.data())
         : o.ordering == SC_ORDER_AMD ? sc::amd_order(n, Ap, Ai, perm.data())
                                      : sc::nd_order(n, Ap, Ai, perm.data());
    if (rc != SC_OK) return fail("ordering failed", rc);
    sc::permute_upper(n, Ap, Ai, perm.data(), Bp, Bi, src);
    rc = sc::analyze(n, Bp.data(), Bi.data(), o, h.S, err);
    if (rc != SC_OK) return rc;
    auto& S = h.S;
    for (int64_t q = 0; q < S.nnzA_used; ++q) S.a_src[q] = src[S.a_src[q]];
    S.nnzA_in = Ap[n];
    S.Ap_in.assign(Ap, Ap + n + 1);
    S.Ai_in.assign(Ai, Ai + Ap[n]);
    S.perm = std::move(perm);
    S.n_schur = ns;
    return SC_OK;
}

int64_t sc_analyze(int64_t n, const int64_t* Ap, const int32_t* Ai, const sc_options* opt,
                   sc_symbolic** out) {
    return sc::guarded_create(__func__, out,
                              [&](sc_symbolic& h) { return analyze_into(h, n, Ap, Ai, opt, 0, nullptr); });
}

// ns in 0..n and ns distinct indices in 0..n-1
static int64_t schur_list_arg(int64_t n, int32_t ns, const int32_t* schur_idx) {
    if (ns < 0) return fail("ns = " + std::to_string(ns) + " < 0");
    if (ns > n) return fail("ns = " + std::to_string(ns) + " exceeds n = " + std::to_string(n));
    if (ns > 0 && !schur_idx) return fail("null schur_idx with ns = " + std::to_string(ns));
    std::vector<int32_t> at((size_t)std::max<int64_t>(n, 0), -1);  // position of an index in the list
    for (int32_t q = 0; q < ns; ++q) {
        const int32_t v = schur_idx[q];
        const std::string name = "schur_idx[" + std::to_string(q) + "] = " + std::to_string(v);
        if (v < 0 || v >= n) return fail(name + " is out of range [0, " + std::to_string(n) + ")");
        if (at[v] >= 0) return fail(name + " appears twice (first as schur_idx[" + std::to_string(at[v]) + "])");
        at[v] = q;
    }
    return SC_OK;
}

int64_t sc_analyze_schur(int64_t n, const int64_t* Ap, const int32_t* Ai, const sc_options* opt, int32_t ns,
                         const int32_t* schur_idx, sc_symbolic** out) {
    return sc::guarded_create(__func__, out, [&](sc_symbolic& h) {
        const int64_t rc = schur_list_arg(n, ns, schur_idx);
        return rc != SC_OK ? rc : analyze_into(h, n, Ap, Ai, opt, ns, schur_idx);
    });
}

int64_t sc_symbolic_schur(const sc_symbolic* sym, int32_t* schur_idx) {
    return entry(__func__, sym, [&]() -> int64_t {
        const auto& S = sym->S;
        if (schur_idx && S.n_schur > 0)
            std::memcpy(schur_idx, S.perm.data() + (S.n - S.n_schur), sizeof(int32_t) * (size_t)S.n_schur);
        return S.n_schur;
    });
}

int64_t sc_symbolic_get_stats(const sc_symbolic* sym, sc_symbolic_stats* st) {
    return entry(__func__, sym, [&]() -> int64_t {
        if (!st) return fail("null st");
        *st = sym->S.stats;
        return SC_OK;
    });
}

int64_t sc_nnz_L(const sc_symbolic* sym) {
    return entry(__func__, sym, [&]() -> int64_t { return sym->S.nnzL; });
}
double sc_flops(const sc_symbolic* sym) {
    return guarded_or(-1.0, [&] { return sym ? sym->S.flops : -1.0; });
}

int64_t sc_symbolic_pattern(const sc_symbolic* sym, int64_t* Lp, int32_t* Li) {
    return entry(__func__, sym, [&]() -> int64_t {
        if (!Lp) return fail("null Lp");
        sc::pattern_L(sym->S, Lp, Li);
        return SC_OK;
    });
}

int64_t sc_symbolic_etree(const sc_symbolic* sym, int32_t* parent, int32_t* post) {
    return entry(__func__, sym, [&]() -> int64_t {
        const auto& S = sym->S;
        if (parent) std::memcpy(parent, S.parent.data(), sizeof(int32_t) * (size_t)S.n);
        if (post) std::memcpy(post, S.post.data(), sizeof(int32_t) * (size_t)S.n);
        return SC_OK;
    });
}

int64_t sc_symbolic_supernodes(const sc_symbolic* sym, int32_t* sn_start, int32_t* sn_m, int32_t* sn_parent,
                               int32_t* level) {
    return entry(__func__, sym, [&]() -> int64_t {
        const auto& S = sym->S;
        const size_t ns = (size_t)S.ns;
        if (sn_start) std::memcpy(sn_start, S.sn_start.data(), sizeof(int32_t) * (ns + 1));
        if (sn_m && ns) std::memcpy(sn_m, S.sn_m.data(), sizeof(int32_t) * ns);
        if (sn_parent && ns) std::memcpy(sn_parent, S.sn_parent.data(), sizeof(int32_t) * ns);
        if (level && ns) std::memcpy(level, S.level.data(), sizeof(int32_t) * ns);
        return S.ns;
    });
}

int64_t sc_symbolic_perm(const sc_symbolic* sym, int32_t* perm) {
    return entry(__func__, sym, [&]() -> int64_t {
        const auto& S = sym->S;
        if (perm) {
            if (S.perm.empty())
                for (int64_t i = 0; i < S.n; ++i) perm[i] = (int32_t)i;
            else
                std::memcpy(perm, S.perm.data(), sizeof(int32_t) * (size_t)S.n);
        }
        return S.perm.empty() ? 0 : 1;
    });
}

void sc_free_symbolic(sc_symbolic* sym) {
    guarded_or(0, [&] { return delete sym, 0; });
}

int64_t sc_numeric_create(const sc_symbolic* sym, int32_t device, sc_numeric** out) {
    return numeric_create(__func__, sym, false, out, [&](sc::Numeric*& N, std::string& err) {
        return sc::numeric_create(sym->S, device, N, err);
    });
}

int64_t sc_factor_device(sc_numeric* num, const double* d_Ax, int32_t sync) {
    return entry(__func__, num, [&]() -> int64_t {
        if (!d_Ax && num->sym->S.nnzA_in > 0) return fail("null d_Ax");
        return sc::numeric_factor(*num->N, d_Ax, sync != 0);
    });
}

int64_t sc_debug_time_factor(sc_numeric* num, const double* d_Ax, int32_t reps, double* best_ms) {
    return entry(__func__, num, [&]() -> int64_t {
        if (reps < 1 || !best_ms) return SC_ERR_ARG;
        double best = 1e30;
        for (int r = 0; r <= reps; ++r) {  // the first call captures / warms up
            const auto t0 = std::chrono::steady_clock::now();
            const int64_t rc = sc::numeric_factor(*num->N, d_Ax, true);
            const auto t1 = std::chrono::steady_clock::now();
            if (rc < 0) return rc;
            if (r > 0) best = std::min(best, std::chrono::duration<double, std::milli>(t1 - t0).count());
        }
        *best_ms = best;
        return SC_OK;
    });
}

int64_t sc_debug_solve_eager(sc_numeric* num, int32_t eager) {
    return entry(__func__, num, [&]() -> int64_t {
        num->N->solve_eager = eager != 0;
        return SC_OK;
    });
}

int64_t sc_factor(sc_numeric* num, const double* Ax) {
    return entry(__func__, num, [&]() -> int64_t {
        sc::Numeric& N = *num->N;
        const int64_t nnz = num->sym->S.nnzA_in;
        if (nnz > 0 && !Ax) return fail("null Ax");
        if (hipSetDevice(N.device) != hipSuccess) return SC_ERR_HIP;
        if (!N.d_Ax_owned) {
            if (hipMalloc(&N.d_Ax_owned, (size_t)std::max<int64_t>(nnz, 1) * sizeof(double)) != hipSuccess) {
                N.d_Ax_owned = nullptr;
                return SC_ERR_DEVMEM;
            }
        }
        if (nnz > 0 && hipMemcpyAsync(N.d_Ax_owned, Ax, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice,
                                      N.stream) != hipSuccess)
            return SC_ERR_HIP;
        return sc::numeric_factor(N, N.d_Ax_owned, true);
    });
}

int64_t sc_numeric_status(sc_numeric* num) {
    return entry(__func__, num, [&]() -> int64_t { return sc::numeric_status(*num->N); });
}

int64_t sc_export_L(sc_numeric* num, int64_t* Lp, int32_t* Li, double* Lx) {
    return entry(__func__, num, [&]() -> int64_t { return sc::numeric_export(*num->N, Lp, Li, Lx); });
}

int64_t sc_export_L_cols(sc_numeric* num, int64_t j0, int64_t j1, int64_t* cp, int32_t* ri, double* rx) {
    return entry(__func__, num, [&]() -> int64_t {
        if (!cp) return fail("null cp");
        return sc::numeric_export_cols(*num->N, j0, j1, cp, ri, rx);
    });
}

void* sc_numeric_stream(sc_numeric* num) {
    return guarded_or((void*)nullptr, [&] { return (num && num->N) ? (void*)num->N->stream : nullptr; });
}

int64_t sc_numeric_set_profile(sc_numeric* num, int32_t on) {
    return entry(__func__, num, [&]() -> int64_t {
        num->N->profile = (on == 1 || on == 2) ? on : 0;
        return SC_OK;
    });
}

int64_t sc_numeric_timing(sc_numeric* num, double* t, int32_t nt) {
    return entry(__func__, num, [&]() -> int64_t {
        if (!t) return fail("null t");
        return sc::numeric_timing(*num->N, t, nt);
    });
}

int64_t sc_numeric_level_times(sc_numeric* num, double* ms, int32_t nl) {
    return entry(__func__, num, [&]() -> int64_t {
        if (!ms) return fail("null ms");
        return sc::numeric_level_times(*num->N, ms, nl);
    });
}

int64_t sc_numeric_launch_trace(sc_numeric* num, int32_t* kind, int32_t* level, int32_t* strm, double* ms,
                                double* flops, int64_t cap) {
    return entry(__func__, num, [&]() -> int64_t {
        return sc::numeric_launch_trace(*num->N, kind, level, strm, ms, flops, cap);
    });
}

int64_t sc_numeric_syrk_stats(sc_numeric* num, int32_t wmin, double* flops, double* ms, int64_t* launches) {
    return entry(__func__, num, [&]() -> int64_t {
        return sc::numeric_syrk_stats(*num->N, wmin, flops, ms, launches);
    });
}

int64_t sc_numeric_launch_times(sc_numeric* num, double* t0, double* t1, int32_t* kind, int32_t* step,
                                int32_t* stream, int64_t cap) {
    return entry(__func__, num, [&]() -> int64_t {
        if (t0 && (!t1 || !kind || !step || !stream)) return fail("t0 given without t1, kind, step and stream");
        return sc::numeric_launch_times(*num->N, t0, t1, kind, step, stream, cap);
    });
}

int64_t sc_numeric_syrk_bytes(sc_numeric* num, int32_t wmin, double* bytes) {
    return entry(__func__, num, [&]() -> int64_t {
        if (!bytes) return fail("null bytes");
        return sc::numeric_syrk_bytes(*num->N, wmin, bytes);
    });
}

int64_t sc_debug_chain_stamps(sc_numeric* num, int32_t enable, uint64_t* out, int64_t cap) {
    return entry(__func__, num, [&]() -> int64_t { return sc::numeric_chain_stamps(*num->N, enable, out, cap); });
}

static int64_t digest_out(const sc::SchedDigest& d, int64_t* out, int64_t cap) {
    int64_t v[sc::SchedDigest::NVALS] = {(int64_t)d.hash};
    for (int c = 0; c < sc::C_KINDS; ++c) v[1 + c] = d.calls[c];
    const int64_t rest[6] = {d.tail_split, d.pf, d.comm_steps, d.events, d.msgs, d.gsegs};
    std::copy(rest, rest + 6, v + 1 + sc::C_KINDS);
    if (out) std::copy(v, v + std::min<int64_t>(cap, sc::SchedDigest::NVALS), out);
    return sc::SchedDigest::NVALS;
}

int64_t sc_debug_schedule_digest(const sc_symbolic* sym, int32_t nranks, int32_t rank, int32_t emulate, int64_t* out,
                                 int64_t cap) {
    return entry(__func__, sym, [&]() -> int64_t {
        if (cap < 0) return fail("cap < 0");
        sc::SchedDigest d;
        const int64_t rc = sc::schedule_digest_host(sym->S, nranks, rank, emulate, d, sc::last_error());
        return rc != SC_OK ? rc : digest_out(d, out, cap);
    });
}

int64_t sc_debug_schedule_syrk(const sc_symbolic* sym, int32_t nranks, int32_t rank, int32_t emulate, int64_t* out,
                               int64_t cap) {
    return entry(__func__, sym, [&]() -> int64_t {
        if (cap < 0 || (cap > 0 && !out)) return fail("cap < 0, or null out with cap > 0");
        std::vector<int64_t> v;
        const int64_t rc = sc::schedule_syrk_host(sym->S, nranks, rank, emulate, v, sc::last_error());
        if (rc != SC_OK) return rc;
        if (out) std::copy(v.begin(), v.begin() + std::min<int64_t>(cap, (int64_t)v.size()), out);
        return (int64_t)v.size();
    });
}

int64_t sc_debug_numeric_digest(const sc_numeric* num, int64_t* out, int64_t cap) {
    return entry(__func__, num, [&]() -> int64_t {
        if (cap < 0) return fail("cap < 0");
        return digest_out(num->N->digest, out, cap);
    });
}

void sc_free_numeric(sc_numeric* num) {
    guarded_or(0, [&] {
        if (num) sc::numeric_free(num->N);
        return delete num, 0;
    });
}

int64_t sc_solve_host(sc_numeric* num, const double* b, double* x) {
    return entry(__func__, num, [&]() -> int64_t {
        if (!b || !x) return fail("null b or x");
        return sc::numeric_solve_host(*num->N, b, x);
    });
}

int64_t sc_solve_device(sc_numeric* num, const double* d_b, double* d_x) {
    return entry(__func__, num, [&]() -> int64_t {
        if (!d_b || !d_x) return fail("null b or x");
        return sc::numeric_solve_device(*num->N, d_b, d_x);
    });
}

// B and X of a solve: X may be B itself, with the same leading dimension
static int64_t solve_multi_args(const sc::Numeric& N, int32_t nrhs, const double* B, int64_t ldb, double* X,
                                int64_t ldx) {
    const int64_t rc = panel_args(N.S->n, nrhs, {{B, ldb, "B"}, {X, ldx, "X"}});
    if (rc != SC_OK) return rc;
    if (nrhs > 0 && (const double*)X == B && ldx != ldb) return fail("X aliases B with ldx != ldb");
    return SC_OK;
}

int64_t sc_solve_host_multi(sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb, double* X, int64_t ldx) {
    return entry(__func__, num, [&]() -> int64_t {
        const int64_t rc = solve_multi_args(*num->N, nrhs, B, ldb, X, ldx);
        return rc != SC_OK ? rc : sc::numeric_solve_host_multi(*num->N, nrhs, B, ldb, X, ldx);
    });
}

int64_t sc_solve_device_multi(sc_numeric* num, int32_t nrhs, const double* d_B, int64_t ldb, double* d_X,
                              int64_t ldx) {
    return entry(__func__, num, [&]() -> int64_t {
        const int64_t rc = solve_multi_args(*num->N, nrhs, d_B, ldb, d_X, ldx);
        return rc != SC_OK ? rc : sc::numeric_solve_device_multi(*num->N, nrhs, d_B, ldb, d_X, ldx);
    });
}

// ---- factor operators ----
static int64_t apply_op_arg(int32_t op) {
    return (op >= SC_OP_SOLVE_A && op <= SC_OP_PERM_T) ? SC_OK : fail("op is not an sc_factor_op");
}

static int64_t apply_vec(const char* who, sc_numeric* num, int32_t op, const double* b, double* x, bool host) {
    return entry(who, num, [&]() -> int64_t {
        if (!b || !x) return fail("null b or x");
        const int64_t rc = apply_op_arg(op);
        if (rc != SC_OK) return rc;
        return host ? sc::numeric_apply_host(*num->N, op, b, x) : sc::numeric_apply_device(*num->N, op, b, x);
    });
}

int64_t sc_apply_device(sc_numeric* num, int32_t op, const double* d_b, double* d_x) {
    return apply_vec(__func__, num, op, d_b, d_x, false);
}
int64_t sc_apply_host(sc_numeric* num, int32_t op, const double* b, double* x) {
    return apply_vec(__func__, num, op, b, x, true);
}

static int64_t apply_multi(const char* who, sc_numeric* num, int32_t op, int32_t nrhs, const double* B, int64_t ldb,
                           double* X, int64_t ldx, bool host) {
    return entry(who, num, [&]() -> int64_t {
        int64_t rc = solve_multi_args(*num->N, nrhs, B, ldb, X, ldx);
        if (rc == SC_OK) rc = apply_op_arg(op);
        if (rc != SC_OK) return rc;
        return host ? sc::numeric_apply_host_multi(*num->N, op, nrhs, B, ldb, X, ldx)
                    : sc::numeric_apply_device_multi(*num->N, op, nrhs, B, ldb, X, ldx);
    });
}

int64_t sc_apply_device_multi(sc_numeric* num, int32_t op, int32_t nrhs, const double* d_B, int64_t ldb, double* d_X,
                              int64_t ldx) {
    return apply_multi(__func__, num, op, nrhs, d_B, ldb, d_X, ldx, false);
}
int64_t sc_apply_host_multi(sc_numeric* num, int32_t op, int32_t nrhs, const double* B, int64_t ldb, double* X,
                            int64_t ldx) {
    return apply_multi(__func__, num, op, nrhs, B, ldb, X, ldx, true);
}

int64_t sc_logdet(sc_numeric* num, double* logdet) {
    return entry(__func__, num, [&]() -> int64_t {
        if (!logdet) return fail("null logdet");
        return sc::numeric_logdet(*num->N, logdet);
    });
}

// ---- selected inversion ----
int64_t sc_selinv(sc_numeric* num) {
    return entry(__func__, num, [&]() -> int64_t { return sc::numeric_selinv(*num->N); });
}

int64_t sc_selinv_diag_host(sc_numeric* num, double* d) {
    return entry(__func__, num, [&]() -> int64_t {
        if (!d) return fail("null d");
        return sc::numeric_selinv_diag_host(*num->N, d);
    });
}

int64_t sc_selinv_diag_device(sc_numeric* num, double* d_d) {
    return entry(__func__, num, [&]() -> int64_t {
        if (!d_d) return fail("null d_d");
        return sc::numeric_selinv_diag_device(*num->N, d_d);
    });
}

int64_t sc_selinv_export(sc_numeric* num, int64_t* Lp, int32_t* Li, double* Zx) {
    return entry(__func__, num, [&]() -> int64_t { return sc::numeric_selinv_export(*num->N, Lp, Li, Zx); });
}

int64_t sc_selinv_flops(const sc_symbolic* sym, double* flops) {
    return entry(__func__, sym, [&]() -> int64_t {
        if (!flops) return fail("null flops");
        *flops = sc::selinv_flops(sym->S);
        return SC_OK;
    });
}

int64_t sc_debug_selinv_times(sc_numeric* num, int32_t profile, double* ms) {
    return entry(__func__, num, [&]() -> int64_t {
        num->N->sel_profile = profile != 0;
        if (ms)
            for (int i = 0; i < 4; ++i) ms[i] = num->N->sel_ms[i];
        return SC_OK;
    });
}

int64_t sc_debug_selinv_cols(sc_numeric* num, int64_t j0, int64_t j1, int64_t* cp, int32_t* ri, double* rx) {
    return entry(__func__, num, [&]() -> int64_t {
        return sc::numeric_selinv_export_cols(*num->N, j0, j1, cp, ri, rx);
    });
}

// ---- rank-k update / downdate ----
static int64_t updown_args(int32_t k, const int64_t* Wp, const int32_t* Wi) {
    if (k < 0) return fail("k < 0");
    if (k > 0 && !Wp) return fail("null Wp");
    if (k > 0 && !Wi && Wp[k] > 0) return fail("null Wi");
    return SC_OK;
}

int64_t sc_updown_check(const sc_symbolic* sym, int32_t k, const int64_t* Wp, const int32_t* Wi, int32_t* first_col,
                        int64_t* path) {
    return entry(__func__, sym, [&]() -> int64_t {
        const int64_t rc = updown_args(k, Wp, Wi);
        if (rc != SC_OK) return rc;
        if (path) path[0] = path[1] = path[2] = 0;
        if (k == 0 || sym->S.n == 0) {
            for (int32_t c = 0; first_col && c < k; ++c) first_col[c] = -1;
            return SC_OK;
        }
        return sc::updown_check(sym->S, k, Wp, Wi, first_col, path, "sc_updown_check", sc::last_error());
    });
}

int64_t sc_updown_host(sc_numeric* num, int32_t sign, int32_t k, const int64_t* Wp, const int32_t* Wi,
                       const double* Wx) {
    return entry(__func__, num, [&]() -> int64_t {
        const int64_t rc = updown_args(k, Wp, Wi);
        if (rc != SC_OK) return rc;
        if (sign != 1 && sign != -1) return fail("sign must be +1 (update) or -1 (downdate)");
        if (k > 0 && !Wx && Wp[k] > 0) return fail("null Wx");
        return sc::numeric_updown_host(*num->N, sign, k, Wp, Wi, Wx);
    });
}

// ---- Schur complement ----
static int64_t schur_dense(const char* who, sc_numeric* num, double* out, int64_t ld, bool matrix, bool host) {
    return entry(who, num, [&]() -> int64_t {
        if (!out) return fail("null output");
        if (ld < num->N->S->n_schur) return fail("leading dimension below ns");
        return matrix ? sc::numeric_schur_matrix(*num->N, out, ld, host)
                      : sc::numeric_schur_factor(*num->N, out, ld, host);
    });
}

int64_t sc_schur_factor_device(sc_numeric* num, double* d_D, int64_t ldd) {
    return schur_dense(__func__, num, d_D, ldd, false, false);
}
int64_t sc_schur_factor_host(sc_numeric* num, double* D, int64_t ldd) {
    return schur_dense(__func__, num, D, ldd, false, true);
}
int64_t sc_schur_matrix_device(sc_numeric* num, double* d_S, int64_t lds) {
    return schur_dense(__func__, num, d_S, lds, true, false);
}
int64_t sc_schur_matrix_host(sc_numeric* num, double* S, int64_t lds) {
    return schur_dense(__func__, num, S, lds, true, true);
}

static int64_t schur_condense(const char* who, sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb, double* G,
                              int64_t ldg, bool host) {
    return entry(who, num, [&]() -> int64_t {
        const sc::Symbolic& S = *num->N->S;
        const int64_t rc = panel_args(S.n, nrhs, {{B, ldb, "B"}, {G, ldg, "G", S.n_schur, "ns"}});
        return rc != SC_OK ? rc : sc::numeric_schur_condense(*num->N, nrhs, B, ldb, G, ldg, host);
    });
}

// B / X by the rules of sc_apply_device_multi, plus the ns-row array
static int64_t schur_expand(const char* who, sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb,
                            const double* XS, int64_t ldxs, double* X, int64_t ldx, bool host) {
    return entry(who, num, [&]() -> int64_t {
        int64_t rc = solve_multi_args(*num->N, nrhs, B, ldb, X, ldx);
        if (rc == SC_OK) rc = panel_args(0, nrhs, {{XS, ldxs, "XS", num->N->S->n_schur, "ns"}});
        return rc != SC_OK ? rc : sc::numeric_schur_expand(*num->N, nrhs, B, ldb, XS, ldxs, X, ldx, host);
    });
}

int64_t sc_schur_condense_device_multi(sc_numeric* num, int32_t nrhs, const double* d_B, int64_t ldb, double* d_G,
                                       int64_t ldg) {
    return schur_condense(__func__, num, nrhs, d_B, ldb, d_G, ldg, false);
}
int64_t sc_schur_condense_host_multi(sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb, double* G,
                                     int64_t ldg) {
    return schur_condense(__func__, num, nrhs, B, ldb, G, ldg, true);
}
int64_t sc_schur_expand_device_multi(sc_numeric* num, int32_t nrhs, const double* d_B, int64_t ldb,
                                     const double* d_XS, int64_t ldxs, double* d_X, int64_t ldx) {
    return schur_expand(__func__, num, nrhs, d_B, ldb, d_XS, ldxs, d_X, ldx, false);
}
int64_t sc_schur_expand_host_multi(sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb, const double* XS,
                                   int64_t ldxs, double* X, int64_t ldx) {
    return schur_expand(__func__, num, nrhs, B, ldb, XS, ldxs, X, ldx, true);
}

int64_t sc_debug_schur_llt(const double* dD, int32_t ns, int64_t ldd, double* dS, int64_t lds) {
    return guarded(__func__, [&]() -> int64_t {
        if (ns < 0 || ldd < ns || lds < ns || (ns > 0 && (!dD || !dS))) return SC_ERR_ARG;
        return sc::debug_schur_llt(dD, ns, ldd, dS, lds);
    });
}

// ---- products with A, residuals, iterative refinement ----
void sc_default_refine_options(sc_refine_options* opt) {
    if (!opt) return;
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(sc_refine_options);
    opt->max_iter = 10;
    opt->residual = SC_RESIDUAL_DD;
    opt->rho_max = 0.5;
}

int64_t sc_spmv_structure(const sc_symbolic* sym, int64_t* rp, int32_t* ci, int64_t* sp) {
    return entry(__func__, sym, [&]() -> int64_t {
        if ((ci == nullptr) != (sp == nullptr)) return fail("only one of ci and sp given");
        return sc::spmv_structure(sym->S, rp, ci, sp);
    });
}

static int64_t spmv_multi(const char* who, sc_numeric* num, int32_t nrhs, const double* Ax, const double* X,
                          int64_t ldx, double* Y, int64_t ldy, bool host) {
    return entry(who, num, [&]() -> int64_t {
        const int64_t n = num->N->S->n;
        const int64_t rc = panel_args(n, nrhs, {{X, ldx, "X"}, {Y, ldy, "Y"}});
        if (rc != SC_OK) return rc;
        if (nrhs > 0 && n > 0 && (const double*)Y == X) return fail("Y aliases X");
        return sc::numeric_spmv(*num->N, nrhs, Ax, X, ldx, Y, ldy, host, who);
    });
}

int64_t sc_spmv_host_multi(sc_numeric* num, int32_t nrhs, const double* Ax, const double* X, int64_t ldx, double* Y,
                           int64_t ldy) {
    return spmv_multi(__func__, num, nrhs, Ax, X, ldx, Y, ldy, true);
}
int64_t sc_spmv_device_multi(sc_numeric* num, int32_t nrhs, const double* d_Ax, const double* d_X, int64_t ldx,
                             double* d_Y, int64_t ldy) {
    return spmv_multi(__func__, num, nrhs, d_Ax, d_X, ldx, d_Y, ldy, false);
}

static int64_t residual_mode_arg(int32_t residual) {
    if (residual == SC_RESIDUAL_FP64 || residual == SC_RESIDUAL_DD) return SC_OK;
    return fail("residual is neither SC_RESIDUAL_FP64 nor SC_RESIDUAL_DD");
}

static int64_t residual_multi(const char* who, sc_numeric* num, int32_t residual, int32_t nrhs, const double* Ax,
                              const double* B, int64_t ldb, const double* X, int64_t ldx, double* R, int64_t ldr,
                              double* berr_norm, double* berr_comp, bool host) {
    return entry(who, num, [&]() -> int64_t {
        const int64_t n = num->N->S->n;
        int64_t rc = panel_args(n, nrhs, {{B, ldb, "B"}, {X, ldx, "X"}, {R, ldr, "R"}});
        if (rc == SC_OK) rc = residual_mode_arg(residual);
        if (rc != SC_OK) return rc;
        if (nrhs > 0 && n > 0 && ((const double*)R == X || (const double*)R == B)) return fail("R aliases B or X");
        return sc::numeric_residual(*num->N, residual, nrhs, Ax, B, ldb, X, ldx, R, ldr, berr_norm, berr_comp, host,
                                    who);
    });
}

int64_t sc_residual_host_multi(sc_numeric* num, int32_t residual, int32_t nrhs, const double* Ax, const double* B,
                               int64_t ldb, const double* X, int64_t ldx, double* R, int64_t ldr, double* berr_norm,
                               double* berr_comp) {
    return residual_multi(__func__, num, residual, nrhs, Ax, B, ldb, X, ldx, R, ldr, berr_norm, berr_comp, true);
}
int64_t sc_residual_device_multi(sc_numeric* num, int32_t residual, int32_t nrhs, const double* d_Ax,
                                 const double* d_B, int64_t ldb, const double* d_X, int64_t ldx, double* d_R,
                                 int64_t ldr, double* berr_norm, double* berr_comp) {
    return residual_multi(__func__, num, residual, nrhs, d_Ax, d_B, ldb, d_X, ldx, d_R, ldr, berr_norm, berr_comp,
                          false);
}

// the refinement options of sc_solve_refine_*_multi and sc_normal_lstsq_*_multi
static int64_t refine_options_arg(const sc_refine_options* opt, sc_refine_options& o) {
    const int64_t rc =
        options_arg(opt, sc_default_refine_options, "sc_refine_options", "sc_default_refine_options()", o);
    if (rc != SC_OK) return rc;
    if (o.max_iter < 0) return fail("max_iter < 0");
    if (!(o.rho_max > 0.0 && o.rho_max < 1.0)) return fail("rho_max outside (0, 1)");
    return residual_mode_arg(o.residual);
}

static int64_t refine_multi(const char* who, sc_numeric* num, const sc_refine_options* opt, int32_t nrhs,
                            const double* Ax, const double* B, int64_t ldb, double* X, int64_t ldx,
                            sc_refine_info* info, bool host) {
    return entry(who, num, [&]() -> int64_t {
        const int64_t n = num->N->S->n;
        sc_refine_options o;
        int64_t rc = panel_args(n, nrhs, {{B, ldb, "B"}, {X, ldx, "X"}});
        if (rc == SC_OK) rc = refine_options_arg(opt, o);
        if (rc != SC_OK) return rc;
        if (nrhs > 0 && n > 0 && (const double*)X == B) return fail("X aliases B (refinement needs B after X exists)");
        return sc::numeric_solve_refine(*num->N, o, nrhs, Ax, B, ldb, X, ldx, info, host, who);
    });
}

int64_t sc_solve_refine_host_multi(sc_numeric* num, const sc_refine_options* opt, int32_t nrhs, const double* Ax,
                                   const double* B, int64_t ldb, double* X, int64_t ldx, sc_refine_info* info) {
    return refine_multi(__func__, num, opt, nrhs, Ax, B, ldb, X, ldx, info, true);
}
int64_t sc_solve_refine_device_multi(sc_numeric* num, const sc_refine_options* opt, int32_t nrhs, const double* d_Ax,
                                     const double* d_B, int64_t ldb, double* d_X, int64_t ldx, sc_refine_info* info) {
    return refine_multi(__func__, num, opt, nrhs, d_Ax, d_B, ldb, d_X, ldx, info, false);
}

// ---- conjugate gradients preconditioned with the factor ----
void sc_default_pcg_options(sc_pcg_options* opt) {
    if (!opt) return;
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(sc_pcg_options);
    opt->max_iter = 100;
    opt->use_x0 = 0;
    opt->tol = 1e-10;
}

static int64_t pcg_multi(const char* who, sc_numeric* num, const sc_pcg_options* opt, int32_t nrhs, const double* Ax,
                         const double* B, int64_t ldb, double* X, int64_t ldx, sc_pcg_info* info, bool host) {
    return entry(who, num, [&]() -> int64_t {
        const int64_t n = num->N->S->n;
        sc_pcg_options o;
        int64_t rc = panel_args(n, nrhs, {{B, ldb, "B"}, {X, ldx, "X"}});
        if (rc == SC_OK) rc = options_arg(opt, sc_default_pcg_options, "sc_pcg_options", "sc_default_pcg_options()", o);
        if (rc != SC_OK) return rc;
        if (o.max_iter < 0) return fail("max_iter < 0");
        if (!(o.tol >= 0.0 && o.tol < 1.0)) return fail("tol outside [0, 1)");
        if (o.use_x0 != 0 && o.use_x0 != 1) return fail("use_x0 is neither 0 nor 1");
        if (nrhs > 0 && n > 0 && (const double*)X == B) return fail("X aliases B (the iteration needs B after X exists)");
        return sc::numeric_solve_pcg(*num->N, o, nrhs, Ax, B, ldb, X, ldx, info, host, who);
    });
}

int64_t sc_solve_pcg_host_multi(sc_numeric* num, const sc_pcg_options* opt, int32_t nrhs, const double* Ax,
                                const double* B, int64_t ldb, double* X, int64_t ldx, sc_pcg_info* info) {
    return pcg_multi(__func__, num, opt, nrhs, Ax, B, ldb, X, ldx, info, true);
}
int64_t sc_solve_pcg_device_multi(sc_numeric* num, const sc_pcg_options* opt, int32_t nrhs, const double* d_Ax,
                                  const double* d_B, int64_t ldb, double* d_X, int64_t ldx, sc_pcg_info* info) {
    return pcg_multi(__func__, num, opt, nrhs, d_Ax, d_B, ldb, d_X, ldx, info, false);
}

// ---- eigenpairs nearest zero by block shift-invert Lanczos ----
void sc_default_eigs_options(sc_eigs_options* opt) {
    if (!opt) return;
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(sc_eigs_options);
    opt->max_blocks = 32;
    opt->use_x0 = 0;
    opt->seed = 1;
    opt->tol = 1e-10;
    opt->sigma = 0.0;
}

static int64_t eigs_entry(const char* who, sc_numeric* num, const sc_eigs_options* opt, int32_t nev, const double* Ax,
                          const double* X0, int64_t ldx0, double* lambda, double* X, int64_t ldx, sc_eigs_info* info,
                          bool host) {
    return entry(who, num, [&]() -> int64_t {
        const int64_t n = num->N->S->n;
        sc_eigs_options o;
        int64_t rc = options_arg(opt, sc_default_eigs_options, "sc_eigs_options", "sc_default_eigs_options()", o);
        if (rc != SC_OK) return rc;
        if (o.max_blocks < 1 || o.max_blocks > 32) return fail("max_blocks outside 1..32");
        if (!(o.tol >= 0.0 && o.tol < 1.0)) return fail("tol outside [0, 1)");
        if (o.use_x0 != 0 && o.use_x0 != 1) return fail("use_x0 is neither 0 nor 1");
        if (!std::isfinite(o.sigma)) return fail("sigma is not finite");
        if (nev < 0) return fail("nev < 0");
        if (nev > std::min<int64_t>(n, (int64_t)16 * o.max_blocks)) return fail("nev > min(n, 16 max_blocks)");
        rc = panel_args(n, nev, {{X, ldx, "X"}});
        if (rc == SC_OK && o.use_x0) rc = panel_args(n, nev, {{X0, ldx0, "X0"}});  // not looked at otherwise
        if (rc != SC_OK) return rc;
        if (nev > 0 && !lambda) return fail("null lambda");
        return sc::numeric_eigs(*num->N, o, nev, Ax, X0, ldx0, lambda, X, ldx, info, host, who);
    });
}

int64_t sc_eigs_host(sc_numeric* num, const sc_eigs_options* opt, int32_t nev, const double* Ax, const double* X0,
                     int64_t ldx0, double* lambda, double* X, int64_t ldx, sc_eigs_info* info) {
    return eigs_entry(__func__, num, opt, nev, Ax, X0, ldx0, lambda, X, ldx, info, true);
}
int64_t sc_eigs_device(sc_numeric* num, const sc_eigs_options* opt, int32_t nev, const double* d_Ax, const double* d_X0,
                       int64_t ldx0, double* lambda, double* d_X, int64_t ldx, sc_eigs_info* info) {
    return eigs_entry(__func__, num, opt, nev, d_Ax, d_X0, ldx0, lambda, d_X, ldx, info, false);
}

// ---- gradients on A's pattern ----
int64_t sc_value_entries(const sc_symbolic* sym, int32_t* row, int32_t* col, int32_t* effective) {
    return entry(__func__, sym, [&]() -> int64_t { return sc::value_entries(sym->S, row, col, effective); });
}

// a value-length array may be null only when the value array is empty
static int64_t grad_value_arg(const sc::Numeric& N, const void* a, const char* name) {
    return (a || N.S->nnzA_in == 0) ? SC_OK : fail(std::string("null ") + name);
}

static int64_t pattern_outer(const char* who, sc_numeric* num, double alpha, int32_t nrhs, const double* U, int64_t ldu,
                             const double* V, int64_t ldv, double beta, double* G, bool host) {
    return entry(who, num, [&]() -> int64_t {
        int64_t rc = panel_args(num->N->S->n, nrhs, {{U, ldu, "U"}, {V, ldv, "V"}});
        if (rc == SC_OK) rc = grad_value_arg(*num->N, G, "G");
        if (rc != SC_OK) return rc;
        if (G && ((const double*)G == U || (const double*)G == V)) return fail("G aliases U or V");
        return sc::numeric_pattern_outer(*num->N, alpha, nrhs, U, ldu, V, ldv, beta, G, host, who);
    });
}

int64_t sc_pattern_outer_host(sc_numeric* num, double alpha, int32_t nrhs, const double* U, int64_t ldu,
                              const double* V, int64_t ldv, double beta, double* G) {
    return pattern_outer(__func__, num, alpha, nrhs, U, ldu, V, ldv, beta, G, true);
}
int64_t sc_pattern_outer_device(sc_numeric* num, double alpha, int32_t nrhs, const double* d_U, int64_t ldu,
                                const double* d_V, int64_t ldv, double beta, double* d_G) {
    return pattern_outer(__func__, num, alpha, nrhs, d_U, ldu, d_V, ldv, beta, d_G, false);
}

static int64_t pattern_dot(const char* who, sc_numeric* num, const double* G, const double* H, double* out, bool host) {
    return entry(who, num, [&]() -> int64_t {
        if (!out) return fail("null out");
        int64_t rc = grad_value_arg(*num->N, G, "G");
        if (rc == SC_OK) rc = grad_value_arg(*num->N, H, "H");
        return rc != SC_OK ? rc : sc::numeric_pattern_dot(*num->N, G, H, out, host, who);
    });
}

int64_t sc_pattern_dot_host(sc_numeric* num, const double* G, const double* H, double* out) {
    return pattern_dot(__func__, num, G, H, out, true);
}
int64_t sc_pattern_dot_device(sc_numeric* num, const double* d_G, const double* d_H, double* out) {
    return pattern_dot(__func__, num, d_G, d_H, out, false);
}

static int64_t logdet_grad(const char* who, sc_numeric* num, double* G, bool host) {
    return entry(who, num, [&]() -> int64_t {
        const int64_t rc = grad_value_arg(*num->N, G, "G");
        return rc != SC_OK ? rc : sc::numeric_logdet_grad(*num->N, G, host, who);
    });
}

int64_t sc_logdet_grad_host(sc_numeric* num, double* G) { return logdet_grad(__func__, num, G, true); }
int64_t sc_logdet_grad_device(sc_numeric* num, double* d_G) { return logdet_grad(__func__, num, d_G, false); }

static int64_t solve_grad(const char* who, sc_numeric* num, int32_t nrhs, const double* Xbar, int64_t ldxb,
                          const double* X, int64_t ldx, double* Bbar, int64_t ldbb, double* G, bool host) {
    return entry(who, num, [&]() -> int64_t {
        const int64_t n = num->N->S->n;
        int64_t rc = panel_args(n, nrhs, {{Xbar, ldxb, "Xbar"}, {X, ldx, "X"}, {Bbar, ldbb, "Bbar"}});
        if (rc == SC_OK) rc = grad_value_arg(*num->N, G, "G");
        if (rc != SC_OK) return rc;
        if (G && ((const double*)G == Xbar || (const double*)G == X || G == Bbar))
            return fail("G aliases Xbar, X or Bbar");
        if (nrhs > 0 && n > 0 && (const double*)Bbar == X) return fail("Bbar aliases X");
        return sc::numeric_solve_grad(*num->N, nrhs, Xbar, ldxb, X, ldx, Bbar, ldbb, G, host, who);
    });
}

int64_t sc_solve_grad_host(sc_numeric* num, int32_t nrhs, const double* Xbar, int64_t ldxb, const double* X,
                           int64_t ldx, double* Bbar, int64_t ldbb, double* G) {
    return solve_grad(__func__, num, nrhs, Xbar, ldxb, X, ldx, Bbar, ldbb, G, true);
}
int64_t sc_solve_grad_device(sc_numeric* num, int32_t nrhs, const double* d_Xbar, int64_t ldxb, const double* d_X,
                             int64_t ldx, double* d_Bbar, int64_t ldbb, double* d_G) {
    return solve_grad(__func__, num, nrhs, d_Xbar, ldxb, d_X, ldx, d_Bbar, ldbb, d_G, false);
}

int64_t sc_debug_eigs_gram(int32_t n, int32_t b, int32_t nb, const double* d_V, int64_t ldv, int64_t vstride,
                           const double* d_W, int64_t ldw, double* out) {
    return guarded(__func__, [&]() -> int64_t {
        return sc::debug_eigs_gram(n, b, nb, d_V, ldv, vstride, d_W, ldw, out, sc::last_error());
    });
}
int64_t sc_debug_eigs_update(int32_t n, int32_t b, int32_t bc, int32_t nb, double beta, double* d_Out, int64_t ldo,
                             const double* d_W, int64_t ldw, const double* d_V, int64_t ldv, int64_t vstride,
                             const double* C) {
    return guarded(__func__, [&]() -> int64_t {
        return sc::debug_eigs_update(n, b, bc, nb, beta, d_Out, ldo, d_W, ldw, d_V, ldv, vstride, C,
                                     sc::last_error());
    });
}
int64_t sc_debug_eigs_dense(int32_t which, int32_t m, double* A, double* d) {
    return guarded(__func__, [&]() -> int64_t {
        if (m < 0 || (m > 0 && (!A || !d)) || which < 0 || which > 1 || (which == 0 && m > 512) ||
            (which == 1 && m > 16))
            return fail("unknown operation, m out of range or a null array");
        if (which == 0) return sc::eigs_sym_eig(m, A, d) ? 0 : 1;
        return sc::eigs_chol_inv(A, m, d[0], d);
    });
}

int64_t sc_debug_pcg_vec(int32_t which, int32_t n, int32_t nrhs, uint32_t mask, const double* coef, double* d_A,
                         int64_t lda, double* d_B, int64_t ldb, const double* d_C, int64_t ldc, const double* d_D,
                         int64_t ldd, double* d_T, double* out) {
    return guarded(__func__, [&]() -> int64_t {
        return sc::debug_pcg_vec(which, n, nrhs, mask, coef, d_A, lda, d_B, ldb, d_C, ldc, d_D, ldd, d_T, out,
                                 sc::last_error());
    });
}

int64_t sc_debug_spmv(int32_t mode, int32_t n, const int64_t* rp, const int32_t* ci, const int64_t* sp, int64_t nval,
                      const double* d_Ax, int32_t nrhs, const double* d_X, int64_t ldx, const double* d_B, int64_t ldb,
                      double* d_R, int64_t ldr, double* d_W, int64_t ldw, double* d_norms) {
    return guarded(__func__, [&]() -> int64_t {
        return sc::debug_spmv(mode, n, rp, ci, sp, nval, d_Ax, nrhs, d_X, ldx, d_B, ldb, d_R, ldr, d_W, ldw, d_norms,
                              sc::last_error());
    });
}

// ---- weighted normal equations ----
int64_t sc_normal_create(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const int64_t* Cp,
                         const int32_t* Ci, int32_t device, sc_normal** out) {
    return sc::guarded_create(__func__, out, [&](sc_normal& h) {
        return sc::normal_create(m, n, Jp, Ji, Cp, Ci, device, h.N, sc::last_error());
    });
}

void sc_normal_free(sc_normal* normal) {
    guarded_or(0, [&] {
        if (normal) sc::normal_free(normal->N);
        return delete normal, 0;
    });
}

int64_t sc_normal_pattern(const sc_normal* normal, int64_t* Sp, int32_t* Si) {
    return entry(__func__, normal, [&]() -> int64_t {
        const sc::NormalStruct& H = normal->N->H;
        if (Sp) std::copy(H.Sp.begin(), H.Sp.end(), Sp);
        if (Si) std::copy(H.Si.begin(), H.Si.end(), Si);
        return (int64_t)H.Si.size();
    });
}

int64_t sc_normal_terms(const sc_normal* normal) {
    return entry(__func__, normal, [&]() -> int64_t { return normal->N->H.T; });
}

int64_t sc_normal_term_lists(const sc_normal* normal, int64_t* tp, int32_t* pa, int32_t* pb, int32_t* r,
                             int64_t* cpos) {
    return entry(__func__, normal, [&]() -> int64_t {
        const sc::NormalStruct& H = normal->N->H;
        if (tp) std::copy(H.tp.begin(), H.tp.end(), tp);
        if (pa) std::copy(H.ta.begin(), H.ta.end(), pa);
        if (pb) std::copy(H.tb.begin(), H.tb.end(), pb);
        if (r) std::copy(H.tr.begin(), H.tr.end(), r);
        if (cpos) std::copy(H.cpos.begin(), H.cpos.end(), cpos);
        return H.T;
    });
}

int64_t sc_normal_rows(const sc_normal* normal, int64_t* rp, int32_t* ci, int64_t* sp) {
    return entry(__func__, normal, [&]() -> int64_t {
        const sc::NormalStruct& H = normal->N->H;
        if (rp) std::copy(H.rp.begin(), H.rp.end(), rp);
        if (ci) std::copy(H.ci.begin(), H.ci.end(), ci);
        if (sp) std::copy(H.sp.begin(), H.sp.end(), sp);
        return H.nnzJ;
    });
}

int64_t sc_normal_memory(const sc_normal* normal, int64_t* out, int32_t cap) {
    return entry(__func__, normal, [&]() -> int64_t {
        if ((!out && cap > 0) || cap < 0) return fail("null array");
        return sc::normal_memory(*normal->N, out, cap);
    });
}

int64_t sc_normal_constants(int32_t* out, int32_t cap) {
    return guarded(__func__, [&]() -> int64_t {
        const int32_t v[4] = {sc::NORMAL_SHORT, sc::NORMAL_LANES, sc::NORMAL_CH, sc::NORMAL_PCH};
        if ((!out && cap > 0) || cap < 0) return fail("null array");
        for (int32_t k = 0; k < cap && k < 4; ++k) out[k] = v[k];
        return 4;
    });
}

// the value arrays of a form call: Jx, and Cx where the handle has base entries
static int64_t normal_value_args(const sc::NormalStruct& H, const double* Jx, const double* Cx) {
    if (H.nnzJ > 0 && !Jx) return fail("null Jx");
    if (Cx && !H.has_base) return fail("base values given, but the handle was created without a base pattern");
    return SC_OK;
}

static int64_t normal_values(const char* who, sc_normal* h, const double* Jx, const double* w, const double* Cx,
                             const double* d, double lambda, double* Sx, bool host) {
    return entry(who, h, [&]() -> int64_t {
        const int64_t rc = normal_value_args(h->N->H, Jx, Cx);
        if (rc != SC_OK) return rc;
        if (!Sx && !h->N->H.Si.empty()) return fail("null Sx");
        return sc::normal_values(*h->N, Jx, w, Cx, d, lambda, Sx, host, who);
    });
}

int64_t sc_normal_values_host(sc_normal* normal, const double* Jx, const double* w, const double* Cx,
                              const double* d, double lambda, double* Sx) {
    return normal_values(__func__, normal, Jx, w, Cx, d, lambda, Sx, true);
}
int64_t sc_normal_values_device(sc_normal* normal, const double* d_Jx, const double* d_w, const double* d_Cx,
                                const double* d_d, double lambda, double* d_Sx) {
    return normal_values(__func__, normal, d_Jx, d_w, d_Cx, d_d, lambda, d_Sx, false);
}

static int64_t normal_factor(const char* who, sc_normal* h, sc_numeric* num, const double* Jx, const double* w,
                             const double* Cx, const double* d, double lambda, bool host) {
    return entry(who, h, [&]() -> int64_t {
        const int64_t rc = normal_value_args(h->N->H, Jx, Cx);
        if (rc != SC_OK) return rc;
        if (!num || !num->N) return fail("null numeric handle");
        return sc::normal_factor(*h->N, *num->N, Jx, w, Cx, d, lambda, host, who);
    });
}

int64_t sc_normal_factor_host(sc_normal* normal, sc_numeric* num, const double* Jx, const double* w,
                              const double* Cx, const double* d, double lambda) {
    return normal_factor(__func__, normal, num, Jx, w, Cx, d, lambda, true);
}
int64_t sc_normal_factor_device(sc_normal* normal, sc_numeric* num, const double* d_Jx, const double* d_w,
                                const double* d_Cx, const double* d_d, double lambda) {
    return normal_factor(__func__, normal, num, d_Jx, d_w, d_Cx, d_d, lambda, false);
}

const double* sc_normal_values_ptr(const sc_normal* normal) {
    return guarded_or((const double*)nullptr,
                      [&] { return (normal && normal->N->values_valid) ? (const double*)normal->N->Sbuf : nullptr; });
}

// Y = J X (in: n rows, out: m rows) or G = J^T W Y (transposed: in m rows, out n rows)
static int64_t normal_product(const char* who, sc_normal* h, bool transposed, int32_t nrhs, const double* Jx,
                              const double* w, const PanelArg& in, const PanelArg& out, bool host) {
    return entry(who, h, [&]() -> int64_t {
        const int64_t rc = panel_args(0, nrhs, {in, out});
        if (rc != SC_OK) return rc;
        if (nrhs > 0 && out.rows > 0) {
            if (h->N->H.nnzJ > 0 && !Jx) return fail("null Jx");
            if (out.p == in.p) return fail("the output aliases the input");
        }
        return sc::normal_product(*h->N, transposed, nrhs, Jx, w, (const double*)in.p, in.ld, (double*)out.p, out.ld,
                                  host, who);
    });
}

// the row counts of a null handle are never looked at
static int64_t normal_m(const sc_normal* h) { return h ? h->N->H.m : 0; }
static int64_t normal_n(const sc_normal* h) { return h ? h->N->H.n : 0; }

int64_t sc_normal_mul_host_multi(sc_normal* normal, int32_t nrhs, const double* Jx, const double* X, int64_t ldx,
                                 double* Y, int64_t ldy) {
    return normal_product(__func__, normal, false, nrhs, Jx, nullptr, {X, ldx, "X", normal_n(normal), "n"},
                          {Y, ldy, "Y", normal_m(normal), "m"}, true);
}
int64_t sc_normal_mul_device_multi(sc_normal* normal, int32_t nrhs, const double* d_Jx, const double* d_X,
                                   int64_t ldx, double* d_Y, int64_t ldy) {
    return normal_product(__func__, normal, false, nrhs, d_Jx, nullptr, {d_X, ldx, "X", normal_n(normal), "n"},
                          {d_Y, ldy, "Y", normal_m(normal), "m"}, false);
}
int64_t sc_normal_mult_host_multi(sc_normal* normal, int32_t nrhs, const double* Jx, const double* w,
                                  const double* Y, int64_t ldy, double* G, int64_t ldg) {
    return normal_product(__func__, normal, true, nrhs, Jx, w, {Y, ldy, "Y", normal_m(normal), "m"},
                          {G, ldg, "G", normal_n(normal), "n"}, true);
}
int64_t sc_normal_mult_device_multi(sc_normal* normal, int32_t nrhs, const double* d_Jx, const double* d_w,
                                    const double* d_Y, int64_t ldy, double* d_G, int64_t ldg) {
    return normal_product(__func__, normal, true, nrhs, d_Jx, d_w, {d_Y, ldy, "Y", normal_m(normal), "m"},
                          {d_G, ldg, "G", normal_n(normal), "n"}, false);
}

static int64_t normal_lstsq(const char* who, sc_normal* h, sc_numeric* num, const sc_refine_options* opt, int32_t nrhs,
                            const double* Jx, const double* w, const double* B, int64_t ldb, double* X, int64_t ldx,
                            sc_lstsq_info* info, bool host) {
    return entry(who, h, [&]() -> int64_t {
        if (!num || !num->N) return fail("null numeric handle");
        const sc::NormalStruct& H = h->N->H;
        int64_t rc = panel_args(H.n, nrhs, {{B, ldb, "B", H.m, "m"}, {X, ldx, "X"}});
        if (rc != SC_OK) return rc;
        if (nrhs > 0 && H.n > 0) {
            if (H.nnzJ > 0 && !Jx) return fail("null Jx");
            if ((const double*)X == B) return fail("X aliases B (the steps need B after X exists)");
        }
        sc_refine_options o;
        rc = refine_options_arg(opt, o);
        if (rc != SC_OK) return rc;
        return sc::normal_lstsq(*h->N, *num->N, o, nrhs, Jx, w, B, ldb, X, ldx, info, host, who);
    });
}

int64_t sc_normal_lstsq_host_multi(sc_normal* normal, sc_numeric* num, const sc_refine_options* opt, int32_t nrhs,
                                   const double* Jx, const double* w, const double* B, int64_t ldb, double* X,
                                   int64_t ldx, sc_lstsq_info* info) {
    return normal_lstsq(__func__, normal, num, opt, nrhs, Jx, w, B, ldb, X, ldx, info, true);
}
int64_t sc_normal_lstsq_device_multi(sc_normal* normal, sc_numeric* num, const sc_refine_options* opt, int32_t nrhs,
                                     const double* d_Jx, const double* d_w, const double* d_B, int64_t ldb,
                                     double* d_X, int64_t ldx, sc_lstsq_info* info) {
    return normal_lstsq(__func__, normal, num, opt, nrhs, d_Jx, d_w, d_B, ldb, d_X, ldx, info, false);
}

int64_t sc_debug_normal_form(int64_t ne, const int64_t* tp, const int32_t* ta, const int32_t* tb, const int32_t* tr,
                             const int64_t* cpos, const int32_t* dcol, int64_t nJ, int64_t nw, int64_t nC, int64_t nd,
                             const double* d_Jx, const double* d_w, const double* d_Cx, const double* d_d,
                             double lambda, double* d_Sx) {
    return guarded(__func__, [&]() -> int64_t {
        return sc::debug_normal_form(ne, tp, ta, tb, tr, cpos, dcol, nJ, nw, nC, nd, d_Jx, d_w, d_Cx, d_d, lambda,
                                     d_Sx, sc::last_error());
    });
}

int64_t sc_debug_normal_mul(int32_t mode, int64_t m, int64_t n, const int64_t* rp, const int32_t* ci,
                            const int64_t* sp, int64_t nval, const double* d_Jx, int32_t nrhs, const double* d_X,
                            int64_t ldx, const double* d_B, int64_t ldb, double* d_R, int64_t ldr) {
    return guarded(__func__, [&]() -> int64_t {
        if (!sp) return fail("null sp");
        return sc::debug_normal_prod(false, mode, m, n, rp, ci, sp, nval, d_Jx, nullptr, nrhs, d_X, ldx, d_B, ldb, d_R,
                                     ldr, sc::last_error());
    });
}

int64_t sc_debug_normal_mult(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const double* d_Jx,
                             const double* d_w, int32_t nrhs, const double* d_Y, int64_t ldy, double* d_G,
                             int64_t ldg) {
    return guarded(__func__, [&]() -> int64_t {
        const int64_t nval = (Jp && n > 0) ? Jp[n] : 0;
        return sc::debug_normal_prod(true, 0, n, m, Jp, Ji, nullptr, nval, d_Jx, d_w, nrhs, d_Y, ldy, nullptr, 0, d_G,
                                     ldg, sc::last_error());
    });
}

int64_t sc_debug_normal_pair(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const int64_t* rp,
                             const int32_t* ci, const int64_t* sp, const double* d_Jx, const double* d_w, int32_t nrhs,
                             const double* d_X, int64_t ldx, const double* d_B, int64_t ldb, double* d_R, double* d_Rl,
                             int64_t ldr, double* d_G, double* d_Gl, int64_t ldg) {
    return guarded(__func__, [&]() -> int64_t {
        return sc::debug_normal_pair(m, n, Jp, Ji, rp, ci, sp, d_Jx, d_w, nrhs, d_X, ldx, d_B, ldb, d_R, d_Rl, ldr, d_G,
                                     d_Gl, ldg, sc::last_error());
    });
}

// ---- reference-API helpers ----
int64_t sc_etree(int64_t n, const int64_t* Ap, const int32_t* Ai, int32_t* parent) {
    return guarded(__func__, [&]() -> int64_t {
        if (n < 0 || !Ap || !parent) return SC_ERR_ARG;
        sc::etree(n, Ap, Ai, parent);
        return SC_OK;
    });
}

int64_t sc_post_order(int64_t n, const int32_t* parent, int32_t* post) {
    return guarded(__func__, [&]() -> int64_t {
        if (n < 0 || !parent || !post) return SC_ERR_ARG;
        sc::post_order(n, parent, post);
        return SC_OK;
    });
}

int64_t sc_col_count(int64_t n, const int64_t* Ap, const int32_t* Ai, const int32_t* parent,
                     const int32_t* post, int64_t* colcount) {
    return guarded(__func__, [&]() -> int64_t {
        if (n < 0 || !Ap || !parent || !post || !colcount) return SC_ERR_ARG;
        sc::col_count(n, Ap, Ai, parent, post, colcount);
        return SC_OK;
    });
}

int64_t sc_ereach(int64_t n, const int64_t* Ap, const int32_t* Ai, const double* Ax, int64_t k,
                  const int32_t* parent, int32_t* s, int32_t* w, double* x) {
    return guarded(__func__, [&]() -> int64_t {
        if (n < 0 || k < 0 || k >= n || !Ap || !parent || !s || !w) return SC_ERR_ARG;
        std::vector<int32_t> path((size_t)n);
        return sc::ereach(n, Ap, Ai, Ax, k, parent, s, w, x, path);
    });
}

int64_t sc_compute_levels(int64_t n, const int32_t* parent, int32_t* level_of) {
    return guarded(__func__, [&]() -> int64_t {
        if (n < 0 || !parent) return SC_ERR_ARG;
        return sc::compute_levels(n, parent, level_of);
    });
}

int64_t sc_compute_supernodes(int64_t n, const int32_t* parent, const int64_t* Lp, int32_t* sn_id,
                              int64_t* supernodes) {
    return guarded(__func__, [&]() -> int64_t {
        if (n < 0 || !parent || !Lp) return SC_ERR_ARG;
        return sc::compute_supernodes_ref(n, parent, Lp, sn_id, supernodes);
    });
}

int64_t sc_atree(int64_t n, const int64_t* Lp, const int32_t* Li, const int32_t* sn_id,
                 const int64_t* supernodes, int64_t ns, int32_t* super_parent) {
    return guarded(__func__, [&]() -> int64_t {
        if (n < 0 || !Lp || !Li || !sn_id || !supernodes || !super_parent) return SC_ERR_ARG;
        return sc::atree_ref(n, Lp, Li, sn_id, supernodes, ns, super_parent);
    });
}

int64_t sc_triplet_to_csc(int64_t n, int64_t nt, const int32_t* ti, const int32_t* tj, const double* tx,
                          int64_t* Ap, int32_t* Ai, double* Ax) {
    return guarded(__func__, [&]() -> int64_t {
        if (n < 0 || nt < 0 || (nt > 0 && (!ti || !tj))) return SC_ERR_ARG;
        return sc::triplet_to_csc(n, nt, ti, tj, tx, Ap, Ai, Ax);
    });
}

int64_t sc_read_mtx(const char* path, int64_t* n, int64_t* Ap, int32_t* Ai, double* Ax) {
    return guarded(__func__, [&]() -> int64_t {
        if (!path || !n) return SC_ERR_ARG;
        return sc::read_mtx(path, n, Ap, Ai, Ax);
    });
}

int64_t sc_laplacian3d(int64_t k, int32_t nd_order, int64_t* Ap, int32_t* Ai, double* Ax, int32_t* perm) {
    return guarded(__func__, [&]() -> int64_t { return sc::laplacian3d(k, nd_order, Ap, Ai, Ax, perm); });
}

// ---- multi-GPU ----
int64_t sc_dist_unique_id(void* id128) {
    return guarded(__func__, [&]() -> int64_t { return sc::dist_unique_id(id128); });
}

int64_t sc_dist_owner_map(const sc_symbolic* sym, int32_t nranks, int32_t* owner, double* work) {
    return entry(__func__, sym, [&]() -> int64_t {
        if (nranks <= 0) return fail("nranks <= 0");
        return sc::dist_owner_map(sym->S, nranks, owner, work);
    });
}

static bool bad_rank(int32_t nranks, int32_t rank) { return nranks <= 0 || rank < 0 || rank >= nranks; }

int64_t sc_dist_schedule(const sc_symbolic* sym, int32_t nranks, int32_t rank, int32_t* level, int32_t* peer,
                         int64_t* bytes, int32_t* is_send, int64_t cap) {
    return entry(__func__, sym, [&]() -> int64_t {
        if (bad_rank(nranks, rank)) return fail("nranks <= 0, or rank outside 0..nranks-1");
        return sc::dist_schedule(sym->S, nranks, rank, level, peer, bytes, is_send, cap);
    });
}

int64_t sc_numeric_create_dist(const sc_symbolic* sym, int32_t device, int32_t rank, int32_t nranks,
                               const void* id128, sc_numeric** out) {
    return numeric_create(__func__, sym, bad_rank(nranks, rank), out,
                          [&](sc::Numeric*& N, std::string& err) {
                              return sc::numeric_create_dist(sym->S, device, rank, nranks, id128, nullptr, nullptr,
                                                             id128 ? 0 : 1, N, err);
                          });
}

int64_t sc_numeric_create_dist_host(const sc_symbolic* sym, int32_t device, int32_t rank, int32_t nranks,
                                    sc_transport_fn fn, void* ctx, sc_numeric** out) {
    return numeric_create(__func__, sym, !fn || bad_rank(nranks, rank), out,
                          [&](sc::Numeric*& N, std::string& err) {
                              return sc::numeric_create_dist(sym->S, device, rank, nranks, nullptr, fn, ctx, 0, N, err);
                          });
}

int64_t sc_numeric_create_dist_dry(const sc_symbolic* sym, int32_t device, int32_t rank, int32_t nranks,
                                   sc_numeric** out) {
    return numeric_create(__func__, sym, bad_rank(nranks, rank), out,
                          [&](sc::Numeric*& N, std::string& err) {
                              return sc::numeric_create_dist(sym->S, device, rank, nranks, nullptr, DIST_DRY, nullptr,
                                                             0, N, err);
                          });
}

int64_t sc_numeric_create_dist_emulated(const sc_symbolic* sym, int32_t device, int32_t nranks, int32_t use_rccl,
                                        sc_numeric** out) {
    return numeric_create(__func__, sym, nranks <= 0, out, [&](sc::Numeric*& N, std::string& err) {
        return sc::numeric_create_dist(sym->S, device, 0, nranks, nullptr, nullptr, nullptr, use_rccl ? 2 : 1, N, err);
    });
}

int64_t sc_memory_plan(const sc_symbolic* sym, int32_t nranks, int64_t* panel_bytes, int64_t* work_bytes,
                       int64_t* work_lower_bound_bytes) {
    return entry(__func__, sym, [&]() -> int64_t {
        if (nranks <= 0) return fail("nranks <= 0");
        std::vector<int64_t> p((size_t)nranks), w((size_t)nranks), l((size_t)nranks);
        const int64_t rc = sc::plan_memory_stats(sym->S, nranks, p.data(), w.data(), l.data());
        if (rc != SC_OK) return rc;
        for (int32_t r = 0; r < nranks; ++r) {
            if (panel_bytes) panel_bytes[r] = p[r] * (int64_t)sizeof(double);
            if (work_bytes) work_bytes[r] = w[r] * (int64_t)sizeof(double);
            if (work_lower_bound_bytes) work_lower_bound_bytes[r] = l[r] * (int64_t)sizeof(double);
        }
        return SC_OK;
    });
}

int64_t sc_memory_plan_check(const sc_symbolic* sym, int32_t nranks) {
    return entry(__func__, sym, [&]() -> int64_t {
        if (nranks <= 0) return fail("nranks <= 0");
        return sc::plan_check(sym->S, nranks);
    });
}

int64_t sc_numeric_memory(sc_numeric* num, int64_t* info, int32_t n) {
    return entry(__func__, num, [&]() -> int64_t {
        if (!info) return fail("null info");
        const sc::Numeric& N = *num->N;
        int64_t v[4] = {N.dev_bytes, 0, 0, 0};
        for (const sc::RankMem& R : N.R) {
            v[1] += R.panel_total * (int64_t)sizeof(double);
            v[2] += R.work_total * (int64_t)sizeof(double);
            v[3] += R.work_live_max * (int64_t)sizeof(double);
        }
        for (int32_t i = 0; i < n && i < 4; ++i) info[i] = v[i];
        return SC_OK;
    });
}

int64_t sc_dist_steps(const sc_symbolic* sym, int32_t nranks, int32_t* kind, int32_t* level, int32_t* front,
                      int32_t* k, int32_t* p, int64_t cap) {
    return entry(__func__, sym, [&]() -> int64_t {
        if (nranks <= 0) return fail("nranks <= 0");
        sc::DistPlan D;
        int64_t rc = sc::dist_plan(sym->S, nranks, D);
        if (rc != SC_OK) return rc;
        for (size_t i = 0; i < D.steps.size() && (int64_t)i < cap; ++i) {
            if (kind) kind[i] = D.steps[i].kind;
            if (level) level[i] = D.steps[i].level;
            if (front) front[i] = D.steps[i].s;
            if (k) k[i] = D.steps[i].k;
            if (p) p[i] = D.steps[i].p;
        }
        return (int64_t)D.steps.size();
    });
}

// the number of distinct ranks in a list
static int32_t distinct_ranks(std::vector<int32_t> r) {
    std::sort(r.begin(), r.end());
    return (int32_t)(std::unique(r.begin(), r.end()) - r.begin());
}

int64_t sc_dist_plan_info(const sc_symbolic* sym, int32_t nranks, int32_t* gsize, int32_t* split_cb_ranks,
                          int32_t* slab_ranks, int64_t* n_steps) {
    return entry(__func__, sym, [&]() -> int64_t {
        if (nranks <= 0) return fail("nranks <= 0");
        sc::DistPlan D;
        int64_t rc = sc::dist_plan(sym->S, nranks, D);
        if (rc != SC_OK) return rc;
        for (int32_t s = 0; s < sym->S.ns; ++s) {
            if (gsize) gsize[s] = D.gsize[s];
            if (split_cb_ranks) split_cb_ranks[s] = D.split[s] >= 0 ? distinct_ranks(D.cb_rank[D.split[s]]) : 0;
            if (slab_ranks) slab_ranks[s] = D.pd[s] >= 0 ? distinct_ranks(D.slab_rank[D.pd[s]]) : 0;
        }
        if (n_steps) *n_steps = (int64_t)D.steps.size();
        return (int64_t)D.msgs.size();
    });
}

// ---- debug hooks ----
int64_t sc_debug_syrk(double* dC, int32_t ldc, const double* dA, int32_t lda, int32_t M, int32_t N,
                      int32_t K) {
    return guarded(__func__, [&]() -> int64_t {
        if (!dC || !dA || M < 0 || N < 0 || K < 0 || N > M) return SC_ERR_ARG;
        return sc::debug_syrk(dC, ldc, dA, lda, M, N, K);
    });
}

int64_t sc_debug_syrk_ex(double* dC, int32_t ldc, const double* dA, int32_t lda, int32_t M, int32_t N, int32_t K,
                         int32_t bt, int32_t lean, int32_t tag, int32_t epi) {
    return guarded(__func__, [&]() -> int64_t {
        if (!dC || !dA) return SC_ERR_ARG;
        return sc::debug_syrk_ex(dC, ldc, dA, lda, M, N, K, bt, lean, tag, epi);
    });
}

int64_t sc_debug_panel(double* dF, int32_t m, int32_t w, int32_t k0, int32_t mode, int32_t* info) {
    return guarded(__func__, [&]() -> int64_t {
        if (!dF || !info) return SC_ERR_ARG;
        return sc::debug_panel(dF, m, w, k0, mode, info);
    });
}

int64_t sc_debug_updown_block(double* dF, int32_t m, int32_t w, int32_t k0, double* dW, int32_t sign,
                              int32_t* info) {
    return guarded(__func__, [&]() -> int64_t {
        if (!dF || !dW || !info) return SC_ERR_ARG;
        return sc::debug_updown_block(dF, m, w, k0, dW, sign, info);
    });
}

int64_t sc_debug_solve_step(double* dF, int32_t m, int32_t w, int32_t k0, int32_t op, int32_t width, double* dC,
                            double* dY, double* dU) {
    return guarded(__func__, [&]() -> int64_t {
        if (!dF || !dC || !dY) return SC_ERR_ARG;
        return sc::debug_solve_step(dF, m, w, k0, op, width, dC, dY, dU);
    });
}

int64_t sc_debug_solve_gather(int32_t width, int32_t w, int32_t mb, int32_t nchild, const int64_t* rel_ptr,
                              const int32_t* relind, const double* dUc, double* dC, double* dU) {
    return guarded(__func__, [&]() -> int64_t {
        if (!rel_ptr || !dC) return SC_ERR_ARG;
        return sc::debug_solve_gather(width, w, mb, nchild, rel_ptr, relind, dUc, dC, dU);
    });
}

int64_t sc_debug_selinv_step(const double* dL, double* dZ, int32_t m, int32_t w, int32_t k0, int32_t op,
                             const double* dZii, double* dW) {
    return guarded(__func__, [&]() -> int64_t {
        return sc::debug_selinv_step(dL, dZ, m, w, k0, op, dZii, dW, sc::last_error());
    });
}

int64_t sc_debug_selinv_push(int32_t m, int32_t w, const double* dZ, const double* dZii, int32_t mbc,
                             const int32_t* relind, double* dOut) {
    return guarded(__func__, [&]() -> int64_t {
        return sc::debug_selinv_push(m, w, dZ, dZii, mbc, relind, dOut, sc::last_error());
    });
}

int64_t sc_debug_extend_add(int32_t op, int32_t m, int32_t w, int32_t nchild, const int64_t* rel_ptr,
                            const int32_t* relind, const int64_t* a_ptr, const int32_t* a_pos, const int64_t* a_src,
                            int64_t nval, const double* d_Ax, const double* d_child_cb, double* d_panel, double* d_cb,
                            int32_t p0, int32_t p1, int32_t p2, int32_t* info) {
    return guarded(__func__, [&]() -> int64_t {
        return sc::debug_extend_add(op, m, w, nchild, rel_ptr, relind, a_ptr, a_pos, a_src, nval, d_Ax, d_child_cb, d_panel,
                                    d_cb, p0, p1, p2, info, sc::last_error());
    });
}

int64_t sc_debug_bench(int32_t which, int32_t M, int32_t K, int32_t reps, int32_t arg, double* tflops) {
    return guarded(__func__, [&]() -> int64_t {
        if (!tflops || M <= 0 || K <= 0 || reps <= 0) return SC_ERR_ARG;
        return sc::debug_bench(which, M, K, reps, arg, tflops);
    });
}

int64_t sc_debug_contention(int32_t M, int32_t K, int32_t chain_rows, int32_t nchain, int32_t mode,
                            int32_t mask_stride, double* out) {
    return guarded(__func__, [&]() -> int64_t {
        if (!out) return SC_ERR_ARG;
        return sc::debug_contention(M, K, chain_rows, nchain, mode, mask_stride, out);
    });
}

int64_t sc_debug_hwid(int32_t nwg, int32_t threads, int32_t spin_ticks, uint32_t* out) {
    return guarded(__func__, [&]() -> int64_t {
        // spin_ticks is compared unsigned in the kernel: a negative value would spin ~forever,
        // and more than ~1 s (1e8 ticks of the 100 MHz clock) is never a placement probe
        if (!out || nwg <= 0 || threads <= 0 || threads > 1024 || spin_ticks < 0 || spin_ticks > 100000000)
            return SC_ERR_ARG;
        void* d = nullptr;
        if (hipMalloc(&d, (size_t)nwg * 8) != hipSuccess) return SC_ERR_DEVMEM;
        hipError_t e = sc::launch_hwid((uint32_t*)d, nwg, threads, spin_ticks, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(out, d, (size_t)nwg * 8, hipMemcpyDeviceToHost);
        (void)hipFree(d);
        return e == hipSuccess ? SC_OK : SC_ERR_HIP;
    });
}

int64_t sc_device_count(void) {
    return guarded(__func__, [&]() -> int64_t {
        int n = 0;
        return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
    });
}

}  // extern "C"
