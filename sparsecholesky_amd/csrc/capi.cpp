// extern "C" boundary (include/sparsecholesky.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "../../include/sparsecholesky.h"
#include "../../include/sparsecholesky_debug.h"
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

static thread_local std::string g_last_error;

extern "C" {

int32_t sc_version(void) { return SC_VERSION; }

const char* sc_status_string(int64_t st) {
    if (st > 0) return "A is not positive definite.";  // chol.hpp:850
    switch (st) {
        case SC_OK: return "ok";
        case SC_ERR_ARG: return "invalid argument";
        case SC_ERR_NOMEM: return "host allocation failed";
        case SC_ERR_HIP: return "HIP runtime error";
        case SC_ERR_DEVMEM: return "device allocation failed";
        case SC_ERR_STATE: return "call out of order";
        case SC_ERR_COMM: return "communication error";
        case SC_ERR_NOTIMPL: return "not implemented";
        case SC_ERR_NOTSYM: return "matrix is not symmetric";
        case SC_ERR_IO: return "file could not be opened";
    }
    return "unknown status";
}

const char* sc_last_error(void) { return g_last_error.c_str(); }

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
static int64_t analyze_impl(int64_t n, const int64_t* Ap, const int32_t* Ai, const sc_options* opt, int32_t ns,
                            const int32_t* schur_idx, sc_symbolic** out) {
    if (!out) return SC_ERR_ARG;
    *out = nullptr;
    sc_options o;
    if (opt) {
        if (opt->struct_size != (int32_t)sizeof(sc_options)) {
            g_last_error = "sc_options.struct_size does not match this library's sizeof(sc_options): "
                           "initialise the options with sc_default_options() from the matching header";
            return SC_ERR_ARG;
        }
        o = *opt;
    } else {
        sc_default_options(&o);
    }
    if (o.small_front_max > 128) o.small_front_max = 128;
    if (o.small_front_max < 0) o.small_front_max = 0;
    if (o.lookahead != 0 && o.lookahead != 1) {
        g_last_error = "sc_options.lookahead must be 0 or 1";
        return SC_ERR_ARG;
    }
    if (o.inner_order != 0 && o.inner_order != 1) {
        g_last_error = "sc_options.inner_order must be 0 or 1";
        return SC_ERR_ARG;
    }
    sc_symbolic* h = new (std::nothrow) sc_symbolic();
    if (!h) return SC_ERR_NOMEM;
    std::string err;
    int64_t rc;
    try {
        if (o.ordering != SC_ORDER_NATURAL && o.ordering != SC_ORDER_ND && o.ordering != SC_ORDER_AMD) {
            rc = SC_ERR_ARG;
            err = "sc_options.ordering must be SC_ORDER_NATURAL, SC_ORDER_ND or SC_ORDER_AMD";
        } else if ((o.ordering != SC_ORDER_NATURAL || ns > 0) && n > 0 && Ap && (Ai || Ap[n] == 0)) {
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
            if (rc != SC_OK) err = "malformed CSC";
            if (rc == SC_OK) {
                rc = ns > 0 ? sc::schur_order(n, Ap, Ai, o.ordering, ns, schur_idx, perm.data())
                     : o.ordering == SC_ORDER_AMD ? sc::amd_order(n, Ap, Ai, perm.data())
                                                  : sc::nd_order(n, Ap, Ai, perm.data());
                if (rc != SC_OK) err = "ordering failed";
            }
            if (rc == SC_OK) {
                sc::permute_upper(n, Ap, Ai, perm.data(), Bp, Bi, src);
                rc = sc::analyze(n, Bp.data(), Bi.data(), o, h->S, err);
            }
            if (rc == SC_OK) {
                auto& S = h->S;
                for (int64_t q = 0; q < S.nnzA_used; ++q) S.a_src[q] = src[S.a_src[q]];
                S.nnzA_in = Ap[n];
                S.Ap_in.assign(Ap, Ap + n + 1);
                S.Ai_in.assign(Ai, Ai + Ap[n]);
                S.perm = std::move(perm);
                S.n_schur = ns;
            }
        } else {
            rc = sc::analyze(n, Ap, Ai, o, h->S, err);
        }
    } catch (const std::bad_alloc&) {
        rc = SC_ERR_NOMEM;
        err = "out of host memory";
    }
    if (rc != SC_OK) {
        g_last_error = err;
        delete h;
        return rc;
    }
    *out = h;
    return SC_OK;
}

int64_t sc_analyze(int64_t n, const int64_t* Ap, const int32_t* Ai, const sc_options* opt,
                   sc_symbolic** out) {
    return analyze_impl(n, Ap, Ai, opt, 0, nullptr, out);
}

int64_t sc_analyze_schur(int64_t n, const int64_t* Ap, const int32_t* Ai, const sc_options* opt, int32_t ns,
                         const int32_t* schur_idx, sc_symbolic** out) {
    if (out) *out = nullptr;
    auto fail = [&](const std::string& what) {
        g_last_error = "sc_analyze_schur: " + what;
        return (int64_t)SC_ERR_ARG;
    };
    if (ns < 0) return fail("ns = " + std::to_string(ns) + " < 0");
    if (ns > n) return fail("ns = " + std::to_string(ns) + " exceeds n = " + std::to_string(n));
    if (ns > 0 && !schur_idx) return fail("null schur_idx with ns = " + std::to_string(ns));
    try {
        std::vector<int32_t> at((size_t)std::max<int64_t>(n, 0), -1);  // position of an index in the list
        for (int32_t q = 0; q < ns; ++q) {
            const int32_t v = schur_idx[q];
            const std::string name = "schur_idx[" + std::to_string(q) + "] = " + std::to_string(v);
            if (v < 0 || v >= n) return fail(name + " is out of range [0, " + std::to_string(n) + ")");
            if (at[v] >= 0) return fail(name + " appears twice (first as schur_idx[" + std::to_string(at[v]) + "])");
            at[v] = q;
        }
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
    return analyze_impl(n, Ap, Ai, opt, ns, schur_idx, out);
}

int64_t sc_symbolic_schur(const sc_symbolic* sym, int32_t* schur_idx) {
    if (!sym) return SC_ERR_ARG;
    const auto& S = sym->S;
    if (schur_idx && S.n_schur > 0)
        std::memcpy(schur_idx, S.perm.data() + (S.n - S.n_schur), sizeof(int32_t) * (size_t)S.n_schur);
    return S.n_schur;
}

int64_t sc_symbolic_get_stats(const sc_symbolic* sym, sc_symbolic_stats* st) {
    if (!sym || !st) return SC_ERR_ARG;
    *st = sym->S.stats;
    return SC_OK;
}

int64_t sc_nnz_L(const sc_symbolic* sym) { return sym ? sym->S.nnzL : SC_ERR_ARG; }
double sc_flops(const sc_symbolic* sym) { return sym ? sym->S.flops : -1.0; }

int64_t sc_symbolic_pattern(const sc_symbolic* sym, int64_t* Lp, int32_t* Li) {
    if (!sym || !Lp) return SC_ERR_ARG;
    sc::pattern_L(sym->S, Lp, Li);
    return SC_OK;
}

int64_t sc_symbolic_etree(const sc_symbolic* sym, int32_t* parent, int32_t* post) {
    if (!sym) return SC_ERR_ARG;
    const auto& S = sym->S;
    if (parent) std::memcpy(parent, S.parent.data(), sizeof(int32_t) * (size_t)S.n);
    if (post) std::memcpy(post, S.post.data(), sizeof(int32_t) * (size_t)S.n);
    return SC_OK;
}

int64_t sc_symbolic_supernodes(const sc_symbolic* sym, int32_t* sn_start, int32_t* sn_m, int32_t* sn_parent,
                               int32_t* level) {
    if (!sym) return SC_ERR_ARG;
    const auto& S = sym->S;
    const size_t ns = (size_t)S.ns;
    if (sn_start) std::memcpy(sn_start, S.sn_start.data(), sizeof(int32_t) * (ns + 1));
    if (sn_m && ns) std::memcpy(sn_m, S.sn_m.data(), sizeof(int32_t) * ns);
    if (sn_parent && ns) std::memcpy(sn_parent, S.sn_parent.data(), sizeof(int32_t) * ns);
    if (level && ns) std::memcpy(level, S.level.data(), sizeof(int32_t) * ns);
    return S.ns;
}

int64_t sc_symbolic_perm(const sc_symbolic* sym, int32_t* perm) {
    if (!sym) return SC_ERR_ARG;
    const auto& S = sym->S;
    if (perm) {
        if (S.perm.empty())
            for (int64_t i = 0; i < S.n; ++i) perm[i] = (int32_t)i;
        else
            std::memcpy(perm, S.perm.data(), sizeof(int32_t) * (size_t)S.n);
    }
    return S.perm.empty() ? 0 : 1;
}

void sc_free_symbolic(sc_symbolic* sym) { delete sym; }

int64_t sc_numeric_create(const sc_symbolic* sym, int32_t device, sc_numeric** out) {
    if (!sym || !out) return SC_ERR_ARG;
    *out = nullptr;
    sc_numeric* h = new (std::nothrow) sc_numeric();
    if (!h) return SC_ERR_NOMEM;
    std::string err;
    int64_t rc = sc::numeric_create(sym->S, device, h->N, err);
    if (rc != SC_OK) {
        g_last_error = err;
        delete h;
        return rc;
    }
    h->sym = sym;
    *out = h;
    return SC_OK;
}

int64_t sc_factor_device(sc_numeric* num, const double* d_Ax, int32_t sync) {
    if (!num || !num->N || (!d_Ax && num->sym->S.nnzA_in > 0)) return SC_ERR_ARG;
    int64_t rc = sc::numeric_factor(*num->N, d_Ax, sync != 0);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_debug_time_factor(sc_numeric* num, const double* d_Ax, int32_t reps, double* best_ms) {
    if (!num || !num->N || reps < 1 || !best_ms) return SC_ERR_ARG;
    double best = 1e30;
    for (int r = 0; r <= reps; ++r) {  // the first call captures / warms up
        const auto t0 = std::chrono::steady_clock::now();
        const int64_t rc = sc::numeric_factor(*num->N, d_Ax, true);
        const auto t1 = std::chrono::steady_clock::now();
        if (rc < 0) {
            g_last_error = num->N->err;
            return rc;
        }
        if (r > 0) best = std::min(best, std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    *best_ms = best;
    return SC_OK;
}

int64_t sc_debug_solve_eager(sc_numeric* num, int32_t eager) {
    if (!num || !num->N) return SC_ERR_ARG;
    num->N->solve_eager = eager != 0;
    return SC_OK;
}

int64_t sc_factor(sc_numeric* num, const double* Ax) {
    if (!num || !num->N) return SC_ERR_ARG;
    sc::Numeric& N = *num->N;
    const int64_t nnz = num->sym->S.nnzA_in;
    if (nnz > 0 && !Ax) return SC_ERR_ARG;
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
    return sc_factor_device(num, N.d_Ax_owned, 1);
}

int64_t sc_numeric_status(sc_numeric* num) {
    if (!num || !num->N) return SC_ERR_ARG;
    return sc::numeric_status(*num->N);
}

int64_t sc_export_L(sc_numeric* num, int64_t* Lp, int32_t* Li, double* Lx) {
    if (!num || !num->N) return SC_ERR_ARG;
    try {
        return sc::numeric_export(*num->N, Lp, Li, Lx);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
}

int64_t sc_export_L_cols(sc_numeric* num, int64_t j0, int64_t j1, int64_t* cp, int32_t* ri, double* rx) {
    if (!num || !num->N || !cp) return SC_ERR_ARG;
    try {
        const int64_t rc = sc::numeric_export_cols(*num->N, j0, j1, cp, ri, rx);
        if (rc < 0) g_last_error = num->N->err;
        return rc;
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
}

void* sc_numeric_stream(sc_numeric* num) { return (num && num->N) ? (void*)num->N->stream : nullptr; }

int64_t sc_numeric_set_profile(sc_numeric* num, int32_t on) {
    if (!num || !num->N) return SC_ERR_ARG;
    num->N->profile = (on == 1 || on == 2) ? on : 0;
    return SC_OK;
}

int64_t sc_numeric_timing(sc_numeric* num, double* t, int32_t nt) {
    if (!num || !num->N || !t) return SC_ERR_ARG;
    return sc::numeric_timing(*num->N, t, nt);
}

int64_t sc_numeric_level_times(sc_numeric* num, double* ms, int32_t nl) {
    if (!num || !num->N || !ms) return SC_ERR_ARG;
    return sc::numeric_level_times(*num->N, ms, nl);
}

int64_t sc_numeric_launch_trace(sc_numeric* num, int32_t* kind, int32_t* level, int32_t* strm, double* ms,
                                double* flops, int64_t cap) {
    if (!num || !num->N) return SC_ERR_ARG;
    return sc::numeric_launch_trace(*num->N, kind, level, strm, ms, flops, cap);
}

int64_t sc_numeric_syrk_stats(sc_numeric* num, int32_t wmin, double* flops, double* ms, int64_t* launches) {
    if (!num || !num->N) return SC_ERR_ARG;
    return sc::numeric_syrk_stats(*num->N, wmin, flops, ms, launches);
}

int64_t sc_numeric_launch_times(sc_numeric* num, double* t0, double* t1, int32_t* kind, int32_t* step,
                                int32_t* stream, int64_t cap) {
    if (!num || !num->N) return SC_ERR_ARG;
    if (t0 && (!t1 || !kind || !step || !stream)) return SC_ERR_ARG;
    return sc::numeric_launch_times(*num->N, t0, t1, kind, step, stream, cap);
}

int64_t sc_numeric_syrk_bytes(sc_numeric* num, int32_t wmin, double* bytes) {
    if (!num || !num->N || !bytes) return SC_ERR_ARG;
    return sc::numeric_syrk_bytes(*num->N, wmin, bytes);
}

int64_t sc_debug_chain_stamps(sc_numeric* num, int32_t enable, uint64_t* out, int64_t cap) {
    if (!num || !num->N) return SC_ERR_ARG;
    return sc::numeric_chain_stamps(*num->N, enable, out, cap);
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
    if (!sym || cap < 0) return SC_ERR_ARG;
    sc::SchedDigest d;
    const int64_t rc = sc::schedule_digest_host(sym->S, nranks, rank, emulate, d, g_last_error);
    return rc != SC_OK ? rc : digest_out(d, out, cap);
}

int64_t sc_debug_schedule_syrk(const sc_symbolic* sym, int32_t nranks, int32_t rank, int32_t emulate, int64_t* out,
                               int64_t cap) {
    if (!sym || cap < 0 || (cap > 0 && !out)) return SC_ERR_ARG;
    std::vector<int64_t> v;
    const int64_t rc = sc::schedule_syrk_host(sym->S, nranks, rank, emulate, v, g_last_error);
    if (rc != SC_OK) return rc;
    if (out) std::copy(v.begin(), v.begin() + std::min<int64_t>(cap, (int64_t)v.size()), out);
    return (int64_t)v.size();
}

int64_t sc_debug_numeric_digest(const sc_numeric* num, int64_t* out, int64_t cap) {
    if (!num || !num->N || cap < 0) return SC_ERR_ARG;
    return digest_out(num->N->digest, out, cap);
}

void sc_free_numeric(sc_numeric* num) {
    if (!num) return;
    sc::numeric_free(num->N);
    delete num;
}

int64_t sc_solve_host(sc_numeric* num, const double* b, double* x) {
    if (!num || !num->N || !b || !x) return SC_ERR_ARG;
    int64_t rc = sc::numeric_solve_host(*num->N, b, x);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_solve_device(sc_numeric* num, const double* d_b, double* d_x) {
    if (!num || !num->N || !d_b || !d_x) return SC_ERR_ARG;
    int64_t rc = sc::numeric_solve_device(*num->N, d_b, d_x);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

static int64_t solve_multi_args(sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb, double* X,
                                int64_t ldx, const char* what) {
    const char* bad = nullptr;
    const int64_t n = (num && num->N) ? num->N->S->n : 0;
    if (!num || !num->N)
        bad = "null handle";
    else if (nrhs < 0)
        bad = "nrhs < 0";
    else if (ldb < n || ldx < n)
        bad = "leading dimension below n";
    else if (nrhs > 0 && (!B || !X))
        bad = "null B or X";
    else if (nrhs > 0 && (const double*)X == B && ldx != ldb)
        bad = "X aliases B with ldx != ldb";
    if (!bad) return SC_OK;
    g_last_error = std::string(what) + ": " + bad;
    return SC_ERR_ARG;
}

int64_t sc_solve_host_multi(sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb, double* X, int64_t ldx) {
    int64_t rc = solve_multi_args(num, nrhs, B, ldb, X, ldx, "sc_solve_host_multi");
    if (rc != SC_OK) return rc;
    rc = sc::numeric_solve_host_multi(*num->N, nrhs, B, ldb, X, ldx);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_solve_device_multi(sc_numeric* num, int32_t nrhs, const double* d_B, int64_t ldb, double* d_X,
                              int64_t ldx) {
    int64_t rc = solve_multi_args(num, nrhs, d_B, ldb, d_X, ldx, "sc_solve_device_multi");
    if (rc != SC_OK) return rc;
    rc = sc::numeric_solve_device_multi(*num->N, nrhs, d_B, ldb, d_X, ldx);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

// ---- factor operators ----
static int64_t apply_op_arg(int32_t op, const char* what) {
    if (op >= SC_OP_SOLVE_A && op <= SC_OP_PERM_T) return SC_OK;
    g_last_error = std::string(what) + ": op is not an sc_factor_op";
    return SC_ERR_ARG;
}

static int64_t apply_vec_args(sc_numeric* num, int32_t op, const double* b, double* x, const char* what) {
    if (!num || !num->N || !b || !x) {
        g_last_error = std::string(what) + ((!num || !num->N) ? ": null handle" : ": null b or x");
        return SC_ERR_ARG;
    }
    return apply_op_arg(op, what);
}

int64_t sc_apply_device(sc_numeric* num, int32_t op, const double* d_b, double* d_x) {
    int64_t rc = apply_vec_args(num, op, d_b, d_x, "sc_apply_device");
    if (rc != SC_OK) return rc;
    rc = sc::numeric_apply_device(*num->N, op, d_b, d_x);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_apply_host(sc_numeric* num, int32_t op, const double* b, double* x) {
    int64_t rc = apply_vec_args(num, op, b, x, "sc_apply_host");
    if (rc != SC_OK) return rc;
    rc = sc::numeric_apply_host(*num->N, op, b, x);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_apply_device_multi(sc_numeric* num, int32_t op, int32_t nrhs, const double* d_B, int64_t ldb, double* d_X,
                              int64_t ldx) {
    int64_t rc = solve_multi_args(num, nrhs, d_B, ldb, d_X, ldx, "sc_apply_device_multi");
    if (rc == SC_OK) rc = apply_op_arg(op, "sc_apply_device_multi");
    if (rc != SC_OK) return rc;
    rc = sc::numeric_apply_device_multi(*num->N, op, nrhs, d_B, ldb, d_X, ldx);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_apply_host_multi(sc_numeric* num, int32_t op, int32_t nrhs, const double* B, int64_t ldb, double* X,
                            int64_t ldx) {
    int64_t rc = solve_multi_args(num, nrhs, B, ldb, X, ldx, "sc_apply_host_multi");
    if (rc == SC_OK) rc = apply_op_arg(op, "sc_apply_host_multi");
    if (rc != SC_OK) return rc;
    rc = sc::numeric_apply_host_multi(*num->N, op, nrhs, B, ldb, X, ldx);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_logdet(sc_numeric* num, double* logdet) {
    if (!num || !num->N || !logdet) {
        g_last_error = (!num || !num->N) ? "sc_logdet: null handle" : "sc_logdet: null logdet";
        return SC_ERR_ARG;
    }
    const int64_t rc = sc::numeric_logdet(*num->N, logdet);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

// ---- selected inversion ----
static int64_t selinv_args(sc_numeric* num, const void* out, const char* who, const char* what) {
    if (!num || !num->N) {
        g_last_error = std::string(who) + ": null handle";
        return SC_ERR_ARG;
    }
    if (!out) {
        g_last_error = std::string(who) + ": null " + what;
        return SC_ERR_ARG;
    }
    return SC_OK;
}

int64_t sc_selinv(sc_numeric* num) {
    int64_t rc = selinv_args(num, num, "sc_selinv", "handle");
    if (rc != SC_OK) return rc;
    rc = sc::numeric_selinv(*num->N);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_selinv_diag_host(sc_numeric* num, double* d) {
    int64_t rc = selinv_args(num, d, "sc_selinv_diag_host", "d");
    if (rc != SC_OK) return rc;
    rc = sc::numeric_selinv_diag_host(*num->N, d);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_selinv_diag_device(sc_numeric* num, double* d_d) {
    int64_t rc = selinv_args(num, d_d, "sc_selinv_diag_device", "d_d");
    if (rc != SC_OK) return rc;
    rc = sc::numeric_selinv_diag_device(*num->N, d_d);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_selinv_export(sc_numeric* num, int64_t* Lp, int32_t* Li, double* Zx) {
    int64_t rc = selinv_args(num, num, "sc_selinv_export", "handle");
    if (rc != SC_OK) return rc;
    rc = sc::numeric_selinv_export(*num->N, Lp, Li, Zx);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_selinv_flops(const sc_symbolic* sym, double* flops) {
    if (!sym || !flops) {
        g_last_error = !sym ? "sc_selinv_flops: null symbolic" : "sc_selinv_flops: null flops";
        return SC_ERR_ARG;
    }
    *flops = sc::selinv_flops(sym->S);
    return SC_OK;
}

int64_t sc_debug_selinv_times(sc_numeric* num, int32_t profile, double* ms) {
    if (!num || !num->N) return SC_ERR_ARG;
    num->N->sel_profile = profile != 0;
    if (ms)
        for (int i = 0; i < 4; ++i) ms[i] = num->N->sel_ms[i];
    return SC_OK;
}

int64_t sc_debug_selinv_cols(sc_numeric* num, int64_t j0, int64_t j1, int64_t* cp, int32_t* ri, double* rx) {
    if (!num || !num->N) return SC_ERR_ARG;
    const int64_t rc = sc::numeric_selinv_export_cols(*num->N, j0, j1, cp, ri, rx);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

// ---- rank-k update / downdate ----
static int64_t updown_args(const void* handle, int32_t k, const int64_t* Wp, const int32_t* Wi, const char* who) {
    const char* bad = nullptr;
    if (!handle)
        bad = "null handle";
    else if (k < 0)
        bad = "k < 0";
    else if (k > 0 && !Wp)
        bad = "null Wp";
    else if (k > 0 && !Wi && Wp[k] > 0)
        bad = "null Wi";
    if (!bad) return SC_OK;
    g_last_error = std::string(who) + ": " + bad;
    return SC_ERR_ARG;
}

int64_t sc_updown_check(const sc_symbolic* sym, int32_t k, const int64_t* Wp, const int32_t* Wi, int32_t* first_col,
                        int64_t* path) {
    int64_t rc = updown_args(sym, k, Wp, Wi, "sc_updown_check");
    if (rc != SC_OK) return rc;
    if (path) path[0] = path[1] = path[2] = 0;
    if (k == 0 || sym->S.n == 0) {
        for (int32_t c = 0; first_col && c < k; ++c) first_col[c] = -1;
        return SC_OK;
    }
    try {
        std::string err;
        rc = sc::updown_check(sym->S, k, Wp, Wi, first_col, path, "sc_updown_check", err);
        if (rc < 0) g_last_error = err;
        return rc;
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
}

int64_t sc_updown_host(sc_numeric* num, int32_t sign, int32_t k, const int64_t* Wp, const int32_t* Wi,
                       const double* Wx) {
    int64_t rc = updown_args((num && num->N) ? num : nullptr, k, Wp, Wi, "sc_updown_host");
    if (rc != SC_OK) return rc;
    if (sign != 1 && sign != -1) {
        g_last_error = "sc_updown_host: sign must be +1 (update) or -1 (downdate)";
        return SC_ERR_ARG;
    }
    if (k > 0 && !Wx && Wp[k] > 0) {
        g_last_error = "sc_updown_host: null Wx";
        return SC_ERR_ARG;
    }
    try {
        rc = sc::numeric_updown_host(*num->N, sign, k, Wp, Wi, Wx);
        if (rc < 0) g_last_error = num->N->err;
        return rc;
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
}

// ---- Schur complement ----
static int64_t schur_out_args(sc_numeric* num, const void* out, int64_t ld, const char* who) {
    const char* bad = nullptr;
    if (!num || !num->N)
        bad = "null handle";
    else if (!out)
        bad = "null output";
    else if (ld < num->N->S->n_schur)
        bad = "leading dimension below ns";
    if (!bad) return SC_OK;
    g_last_error = std::string(who) + ": " + bad;
    return SC_ERR_ARG;
}

static int64_t schur_dense(sc_numeric* num, double* out, int64_t ld, bool matrix, bool host, const char* who) {
    int64_t rc = schur_out_args(num, out, ld, who);
    if (rc != SC_OK) return rc;
    rc = matrix ? sc::numeric_schur_matrix(*num->N, out, ld, host) : sc::numeric_schur_factor(*num->N, out, ld, host);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_schur_factor_device(sc_numeric* num, double* d_D, int64_t ldd) {
    return schur_dense(num, d_D, ldd, false, false, "sc_schur_factor_device");
}
int64_t sc_schur_factor_host(sc_numeric* num, double* D, int64_t ldd) {
    return schur_dense(num, D, ldd, false, true, "sc_schur_factor_host");
}
int64_t sc_schur_matrix_device(sc_numeric* num, double* d_S, int64_t lds) {
    return schur_dense(num, d_S, lds, true, false, "sc_schur_matrix_device");
}
int64_t sc_schur_matrix_host(sc_numeric* num, double* S, int64_t lds) {
    return schur_dense(num, S, lds, true, true, "sc_schur_matrix_host");
}

// B / X by the rules of sc_apply_device_multi (has_x false: B alone), plus the ns-row array
static int64_t schur_solve_args(sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb, bool has_x, double* X,
                                int64_t ldx, const double* GS, int64_t ldgs, const char* what, const char* who) {
    int64_t rc = solve_multi_args(num, nrhs, B, ldb, has_x ? X : const_cast<double*>(B), has_x ? ldx : ldb, who);
    if (rc != SC_OK) return rc;
    const int64_t ns = num->N->S->n_schur;
    const char* bad = nullptr;
    if (ldgs < ns)
        bad = " below ns";
    else if (nrhs > 0 && ns > 0 && !GS)
        bad = ": null array";
    if (!bad) return SC_OK;
    g_last_error = std::string(who) + ": " + what + bad;
    return SC_ERR_ARG;
}

static int64_t schur_condense(sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb, double* G, int64_t ldg,
                              bool host, const char* who) {
    int64_t rc = schur_solve_args(num, nrhs, B, ldb, false, nullptr, 0, G, ldg, "ldg / G", who);
    if (rc != SC_OK) return rc;
    rc = sc::numeric_schur_condense(*num->N, nrhs, B, ldb, G, ldg, host);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

static int64_t schur_expand(sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb, const double* XS,
                            int64_t ldxs, double* X, int64_t ldx, bool host, const char* who) {
    int64_t rc = schur_solve_args(num, nrhs, B, ldb, true, X, ldx, XS, ldxs, "ldxs / XS", who);
    if (rc != SC_OK) return rc;
    rc = sc::numeric_schur_expand(*num->N, nrhs, B, ldb, XS, ldxs, X, ldx, host);
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_schur_condense_device_multi(sc_numeric* num, int32_t nrhs, const double* d_B, int64_t ldb, double* d_G,
                                       int64_t ldg) {
    return schur_condense(num, nrhs, d_B, ldb, d_G, ldg, false, "sc_schur_condense_device_multi");
}
int64_t sc_schur_condense_host_multi(sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb, double* G,
                                     int64_t ldg) {
    return schur_condense(num, nrhs, B, ldb, G, ldg, true, "sc_schur_condense_host_multi");
}
int64_t sc_schur_expand_device_multi(sc_numeric* num, int32_t nrhs, const double* d_B, int64_t ldb,
                                     const double* d_XS, int64_t ldxs, double* d_X, int64_t ldx) {
    return schur_expand(num, nrhs, d_B, ldb, d_XS, ldxs, d_X, ldx, false, "sc_schur_expand_device_multi");
}
int64_t sc_schur_expand_host_multi(sc_numeric* num, int32_t nrhs, const double* B, int64_t ldb, const double* XS,
                                   int64_t ldxs, double* X, int64_t ldx) {
    return schur_expand(num, nrhs, B, ldb, XS, ldxs, X, ldx, true, "sc_schur_expand_host_multi");
}

int64_t sc_debug_schur_llt(const double* dD, int32_t ns, int64_t ldd, double* dS, int64_t lds) {
    if (ns < 0 || ldd < ns || lds < ns || (ns > 0 && (!dD || !dS))) return SC_ERR_ARG;
    return sc::debug_schur_llt(dD, ns, ldd, dS, lds);
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
    if (!sym || ((ci == nullptr) != (sp == nullptr))) {
        g_last_error = "sc_spmv_structure: null handle, or only one of ci and sp given";
        return SC_ERR_ARG;
    }
    try {
        return sc::spmv_structure(sym->S, rp, ci, sp);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
}

// the handle, nrhs and up to three n x nrhs arrays with their leading dimensions
struct PanelArg {
    const void* p;
    int64_t ld;
    const char* name;
};
static int64_t panel_args(sc_numeric* num, int32_t nrhs, std::initializer_list<PanelArg> arrays, const char* who) {
    std::string bad;
    if (!num || !num->N)
        bad = "null handle";
    else if (nrhs < 0)
        bad = "nrhs < 0";
    else
        for (const PanelArg& a : arrays) {
            if (a.ld < num->N->S->n)
                bad = std::string("leading dimension of ") + a.name + " below n";
            else if (nrhs > 0 && num->N->S->n > 0 && !a.p)
                bad = std::string("null ") + a.name;
            if (!bad.empty()) break;
        }
    if (bad.empty()) return SC_OK;
    g_last_error = std::string(who) + ": " + bad;
    return SC_ERR_ARG;
}

static int64_t spmv_multi(sc_numeric* num, int32_t nrhs, const double* Ax, const double* X, int64_t ldx, double* Y,
                          int64_t ldy, bool host, const char* who) {
    int64_t rc = panel_args(num, nrhs, {{X, ldx, "X"}, {Y, ldy, "Y"}}, who);
    if (rc != SC_OK) return rc;
    if (nrhs > 0 && num->N->S->n > 0 && (const double*)Y == X) {
        g_last_error = std::string(who) + ": Y aliases X";
        return SC_ERR_ARG;
    }
    try {
        rc = sc::numeric_spmv(*num->N, nrhs, Ax, X, ldx, Y, ldy, host, who);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_spmv_host_multi(sc_numeric* num, int32_t nrhs, const double* Ax, const double* X, int64_t ldx, double* Y,
                           int64_t ldy) {
    return spmv_multi(num, nrhs, Ax, X, ldx, Y, ldy, true, "sc_spmv_host_multi");
}
int64_t sc_spmv_device_multi(sc_numeric* num, int32_t nrhs, const double* d_Ax, const double* d_X, int64_t ldx,
                             double* d_Y, int64_t ldy) {
    return spmv_multi(num, nrhs, d_Ax, d_X, ldx, d_Y, ldy, false, "sc_spmv_device_multi");
}

static int64_t residual_mode_arg(int32_t residual, const char* who) {
    if (residual == SC_RESIDUAL_FP64 || residual == SC_RESIDUAL_DD) return SC_OK;
    g_last_error = std::string(who) + ": residual is neither SC_RESIDUAL_FP64 nor SC_RESIDUAL_DD";
    return SC_ERR_ARG;
}

static int64_t residual_multi(sc_numeric* num, int32_t residual, int32_t nrhs, const double* Ax, const double* B,
                              int64_t ldb, const double* X, int64_t ldx, double* R, int64_t ldr, double* berr_norm,
                              double* berr_comp, bool host, const char* who) {
    int64_t rc = panel_args(num, nrhs, {{B, ldb, "B"}, {X, ldx, "X"}, {R, ldr, "R"}}, who);
    if (rc == SC_OK) rc = residual_mode_arg(residual, who);
    if (rc != SC_OK) return rc;
    if (nrhs > 0 && num->N->S->n > 0 && ((const double*)R == X || (const double*)R == B)) {
        g_last_error = std::string(who) + ": R aliases B or X";
        return SC_ERR_ARG;
    }
    try {
        rc = sc::numeric_residual(*num->N, residual, nrhs, Ax, B, ldb, X, ldx, R, ldr, berr_norm, berr_comp, host, who);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_residual_host_multi(sc_numeric* num, int32_t residual, int32_t nrhs, const double* Ax, const double* B,
                               int64_t ldb, const double* X, int64_t ldx, double* R, int64_t ldr, double* berr_norm,
                               double* berr_comp) {
    return residual_multi(num, residual, nrhs, Ax, B, ldb, X, ldx, R, ldr, berr_norm, berr_comp, true,
                          "sc_residual_host_multi");
}
int64_t sc_residual_device_multi(sc_numeric* num, int32_t residual, int32_t nrhs, const double* d_Ax,
                                 const double* d_B, int64_t ldb, const double* d_X, int64_t ldx, double* d_R,
                                 int64_t ldr, double* berr_norm, double* berr_comp) {
    return residual_multi(num, residual, nrhs, d_Ax, d_B, ldb, d_X, ldx, d_R, ldr, berr_norm, berr_comp, false,
                          "sc_residual_device_multi");
}

static int64_t refine_multi(sc_numeric* num, const sc_refine_options* opt, int32_t nrhs, const double* Ax,
                            const double* B, int64_t ldb, double* X, int64_t ldx, sc_refine_info* info, bool host,
                            const char* who) {
    int64_t rc = panel_args(num, nrhs, {{B, ldb, "B"}, {X, ldx, "X"}}, who);
    if (rc != SC_OK) return rc;
    sc_refine_options o;
    sc_default_refine_options(&o);
    const char* bad = nullptr;
    if (opt) {
        if (opt->struct_size != (int32_t)sizeof(sc_refine_options))
            bad = "sc_refine_options.struct_size does not match this library's sizeof(sc_refine_options): initialise "
                  "the options with sc_default_refine_options()";
        else
            o = *opt;
    }
    if (!bad && o.max_iter < 0) bad = "max_iter < 0";
    if (!bad && !(o.rho_max > 0.0 && o.rho_max < 1.0)) bad = "rho_max outside (0, 1)";
    if (!bad && nrhs > 0 && num->N->S->n > 0 && (const double*)X == B)
        bad = "X aliases B (refinement needs B after X exists)";
    if (bad) {
        g_last_error = std::string(who) + ": " + bad;
        return SC_ERR_ARG;
    }
    rc = residual_mode_arg(o.residual, who);
    if (rc != SC_OK) return rc;
    try {
        rc = sc::numeric_solve_refine(*num->N, o, nrhs, Ax, B, ldb, X, ldx, info, host, who);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_solve_refine_host_multi(sc_numeric* num, const sc_refine_options* opt, int32_t nrhs, const double* Ax,
                                   const double* B, int64_t ldb, double* X, int64_t ldx, sc_refine_info* info) {
    return refine_multi(num, opt, nrhs, Ax, B, ldb, X, ldx, info, true, "sc_solve_refine_host_multi");
}
int64_t sc_solve_refine_device_multi(sc_numeric* num, const sc_refine_options* opt, int32_t nrhs, const double* d_Ax,
                                     const double* d_B, int64_t ldb, double* d_X, int64_t ldx, sc_refine_info* info) {
    return refine_multi(num, opt, nrhs, d_Ax, d_B, ldb, d_X, ldx, info, false, "sc_solve_refine_device_multi");
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

static int64_t pcg_multi(sc_numeric* num, const sc_pcg_options* opt, int32_t nrhs, const double* Ax, const double* B,
                         int64_t ldb, double* X, int64_t ldx, sc_pcg_info* info, bool host, const char* who) {
    int64_t rc = panel_args(num, nrhs, {{B, ldb, "B"}, {X, ldx, "X"}}, who);
    if (rc != SC_OK) return rc;
    sc_pcg_options o;
    sc_default_pcg_options(&o);
    const char* bad = nullptr;
    if (opt) {
        if (opt->struct_size != (int32_t)sizeof(sc_pcg_options))
            bad = "sc_pcg_options.struct_size does not match this library's sizeof(sc_pcg_options): initialise the "
                  "options with sc_default_pcg_options()";
        else
            o = *opt;
    }
    if (!bad && o.max_iter < 0) bad = "max_iter < 0";
    if (!bad && !(o.tol >= 0.0 && o.tol < 1.0)) bad = "tol outside [0, 1)";
    if (!bad && o.use_x0 != 0 && o.use_x0 != 1) bad = "use_x0 is neither 0 nor 1";
    if (!bad && nrhs > 0 && num->N->S->n > 0 && (const double*)X == B)
        bad = "X aliases B (the iteration needs B after X exists)";
    if (bad) {
        g_last_error = std::string(who) + ": " + bad;
        return SC_ERR_ARG;
    }
    try {
        rc = sc::numeric_solve_pcg(*num->N, o, nrhs, Ax, B, ldb, X, ldx, info, host, who);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_solve_pcg_host_multi(sc_numeric* num, const sc_pcg_options* opt, int32_t nrhs, const double* Ax,
                                const double* B, int64_t ldb, double* X, int64_t ldx, sc_pcg_info* info) {
    return pcg_multi(num, opt, nrhs, Ax, B, ldb, X, ldx, info, true, "sc_solve_pcg_host_multi");
}
int64_t sc_solve_pcg_device_multi(sc_numeric* num, const sc_pcg_options* opt, int32_t nrhs, const double* d_Ax,
                                  const double* d_B, int64_t ldb, double* d_X, int64_t ldx, sc_pcg_info* info) {
    return pcg_multi(num, opt, nrhs, d_Ax, d_B, ldb, d_X, ldx, info, false, "sc_solve_pcg_device_multi");
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

static int64_t eigs_entry(sc_numeric* num, const sc_eigs_options* opt, int32_t nev, const double* Ax, const double* X0,
                          int64_t ldx0, double* lambda, double* X, int64_t ldx, sc_eigs_info* info, bool host,
                          const char* who) {
    sc_eigs_options o;
    sc_default_eigs_options(&o);
    std::string bad;
    if (!num || !num->N)
        bad = "null handle";
    else if (opt && opt->struct_size != (int32_t)sizeof(sc_eigs_options))
        bad = "sc_eigs_options.struct_size does not match this library's sizeof(sc_eigs_options): initialise the "
              "options with sc_default_eigs_options()";
    else {
        if (opt) o = *opt;
        const int64_t n = num->N->S->n;
        if (o.max_blocks < 1 || o.max_blocks > 32)
            bad = "max_blocks outside 1..32";
        else if (!(o.tol >= 0.0 && o.tol < 1.0))
            bad = "tol outside [0, 1)";
        else if (o.use_x0 != 0 && o.use_x0 != 1)
            bad = "use_x0 is neither 0 nor 1";
        else if (!std::isfinite(o.sigma))
            bad = "sigma is not finite";
        else if (nev < 0)
            bad = "nev < 0";
        else if (nev > std::min<int64_t>(n, (int64_t)16 * o.max_blocks))
            bad = "nev > min(n, 16 max_blocks)";
        else if (ldx < n)
            bad = "leading dimension of X below n";
        else if (o.use_x0 && ldx0 < n)
            bad = "leading dimension of X0 below n";
        else if (nev > 0 && !lambda)
            bad = "null lambda";
        else if (nev > 0 && !X)
            bad = "null X";
        else if (nev > 0 && o.use_x0 && !X0)
            bad = "null X0";
    }
    if (!bad.empty()) {
        g_last_error = std::string(who) + ": " + bad;
        return SC_ERR_ARG;
    }
    int64_t rc;
    try {
        rc = sc::numeric_eigs(*num->N, o, nev, Ax, X0, ldx0, lambda, X, ldx, info, host, who);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

int64_t sc_eigs_host(sc_numeric* num, const sc_eigs_options* opt, int32_t nev, const double* Ax, const double* X0,
                     int64_t ldx0, double* lambda, double* X, int64_t ldx, sc_eigs_info* info) {
    return eigs_entry(num, opt, nev, Ax, X0, ldx0, lambda, X, ldx, info, true, "sc_eigs_host");
}
int64_t sc_eigs_device(sc_numeric* num, const sc_eigs_options* opt, int32_t nev, const double* d_Ax, const double* d_X0,
                       int64_t ldx0, double* lambda, double* d_X, int64_t ldx, sc_eigs_info* info) {
    return eigs_entry(num, opt, nev, d_Ax, d_X0, ldx0, lambda, d_X, ldx, info, false, "sc_eigs_device");
}

// ---- gradients on A's pattern ----
int64_t sc_value_entries(const sc_symbolic* sym, int32_t* row, int32_t* col, int32_t* effective) {
    if (!sym) {
        g_last_error = "sc_value_entries: null handle";
        return SC_ERR_ARG;
    }
    return sc::value_entries(sym->S, row, col, effective);
}

// a value-length array may be null only when the value array is empty
static int64_t grad_value_arg(sc_numeric* num, const void* a, const char* name, const char* who) {
    if (a || num->N->S->nnzA_in == 0) return SC_OK;
    g_last_error = std::string(who) + ": null " + name;
    return SC_ERR_ARG;
}

static int64_t grad_finish(sc_numeric* num, int64_t rc) {
    if (rc < 0) g_last_error = num->N->err;
    return rc;
}

static int64_t pattern_outer(sc_numeric* num, double alpha, int32_t nrhs, const double* U, int64_t ldu, const double* V,
                             int64_t ldv, double beta, double* G, bool host, const char* who) {
    int64_t rc = panel_args(num, nrhs, {{U, ldu, "U"}, {V, ldv, "V"}}, who);
    if (rc == SC_OK) rc = grad_value_arg(num, G, "G", who);
    if (rc != SC_OK) return rc;
    if (G && ((const double*)G == U || (const double*)G == V)) {
        g_last_error = std::string(who) + ": G aliases U or V";
        return SC_ERR_ARG;
    }
    try {
        rc = sc::numeric_pattern_outer(*num->N, alpha, nrhs, U, ldu, V, ldv, beta, G, host, who);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
    return grad_finish(num, rc);
}

int64_t sc_pattern_outer_host(sc_numeric* num, double alpha, int32_t nrhs, const double* U, int64_t ldu,
                              const double* V, int64_t ldv, double beta, double* G) {
    return pattern_outer(num, alpha, nrhs, U, ldu, V, ldv, beta, G, true, "sc_pattern_outer_host");
}
int64_t sc_pattern_outer_device(sc_numeric* num, double alpha, int32_t nrhs, const double* d_U, int64_t ldu,
                                const double* d_V, int64_t ldv, double beta, double* d_G) {
    return pattern_outer(num, alpha, nrhs, d_U, ldu, d_V, ldv, beta, d_G, false, "sc_pattern_outer_device");
}

static int64_t pattern_dot(sc_numeric* num, const double* G, const double* H, double* out, bool host, const char* who) {
    if (!num || !num->N || !out) {
        g_last_error = std::string(who) + ((!num || !num->N) ? ": null handle" : ": null out");
        return SC_ERR_ARG;
    }
    int64_t rc = grad_value_arg(num, G, "G", who);
    if (rc == SC_OK) rc = grad_value_arg(num, H, "H", who);
    if (rc != SC_OK) return rc;
    try {
        rc = sc::numeric_pattern_dot(*num->N, G, H, out, host, who);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
    return grad_finish(num, rc);
}

int64_t sc_pattern_dot_host(sc_numeric* num, const double* G, const double* H, double* out) {
    return pattern_dot(num, G, H, out, true, "sc_pattern_dot_host");
}
int64_t sc_pattern_dot_device(sc_numeric* num, const double* d_G, const double* d_H, double* out) {
    return pattern_dot(num, d_G, d_H, out, false, "sc_pattern_dot_device");
}

static int64_t logdet_grad(sc_numeric* num, double* G, bool host, const char* who) {
    if (!num || !num->N) {
        g_last_error = std::string(who) + ": null handle";
        return SC_ERR_ARG;
    }
    int64_t rc = grad_value_arg(num, G, "G", who);
    if (rc != SC_OK) return rc;
    try {
        rc = sc::numeric_logdet_grad(*num->N, G, host, who);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
    return grad_finish(num, rc);
}

int64_t sc_logdet_grad_host(sc_numeric* num, double* G) { return logdet_grad(num, G, true, "sc_logdet_grad_host"); }
int64_t sc_logdet_grad_device(sc_numeric* num, double* d_G) {
    return logdet_grad(num, d_G, false, "sc_logdet_grad_device");
}

static int64_t solve_grad(sc_numeric* num, int32_t nrhs, const double* Xbar, int64_t ldxb, const double* X, int64_t ldx,
                          double* Bbar, int64_t ldbb, double* G, bool host, const char* who) {
    int64_t rc = panel_args(num, nrhs, {{Xbar, ldxb, "Xbar"}, {X, ldx, "X"}, {Bbar, ldbb, "Bbar"}}, who);
    if (rc == SC_OK) rc = grad_value_arg(num, G, "G", who);
    if (rc != SC_OK) return rc;
    if (G && ((const double*)G == Xbar || (const double*)G == X || G == Bbar)) {
        g_last_error = std::string(who) + ": G aliases Xbar, X or Bbar";
        return SC_ERR_ARG;
    }
    if (nrhs > 0 && num->N->S->n > 0 && (const double*)Bbar == X) {
        g_last_error = std::string(who) + ": Bbar aliases X";
        return SC_ERR_ARG;
    }
    try {
        rc = sc::numeric_solve_grad(*num->N, nrhs, Xbar, ldxb, X, ldx, Bbar, ldbb, G, host, who);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
    return grad_finish(num, rc);
}

int64_t sc_solve_grad_host(sc_numeric* num, int32_t nrhs, const double* Xbar, int64_t ldxb, const double* X,
                           int64_t ldx, double* Bbar, int64_t ldbb, double* G) {
    return solve_grad(num, nrhs, Xbar, ldxb, X, ldx, Bbar, ldbb, G, true, "sc_solve_grad_host");
}
int64_t sc_solve_grad_device(sc_numeric* num, int32_t nrhs, const double* d_Xbar, int64_t ldxb, const double* d_X,
                             int64_t ldx, double* d_Bbar, int64_t ldbb, double* d_G) {
    return solve_grad(num, nrhs, d_Xbar, ldxb, d_X, ldx, d_Bbar, ldbb, d_G, false, "sc_solve_grad_device");
}

int64_t sc_debug_eigs_gram(int32_t n, int32_t b, int32_t nb, const double* d_V, int64_t ldv, int64_t vstride,
                           const double* d_W, int64_t ldw, double* out) {
    return sc::debug_eigs_gram(n, b, nb, d_V, ldv, vstride, d_W, ldw, out, g_last_error);
}
int64_t sc_debug_eigs_update(int32_t n, int32_t b, int32_t bc, int32_t nb, double beta, double* d_Out, int64_t ldo,
                             const double* d_W, int64_t ldw, const double* d_V, int64_t ldv, int64_t vstride,
                             const double* C) {
    return sc::debug_eigs_update(n, b, bc, nb, beta, d_Out, ldo, d_W, ldw, d_V, ldv, vstride, C, g_last_error);
}
int64_t sc_debug_eigs_dense(int32_t which, int32_t m, double* A, double* d) {
    if (m < 0 || (m > 0 && (!A || !d)) || which < 0 || which > 1 || (which == 0 && m > 512) || (which == 1 && m > 16)) {
        g_last_error = "sc_debug_eigs_dense: unknown operation, m out of range or a null array";
        return SC_ERR_ARG;
    }
    try {
        if (which == 0) return sc::eigs_sym_eig(m, A, d) ? 0 : 1;
        return sc::eigs_chol_inv(A, m, d[0], d);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
}

int64_t sc_debug_pcg_vec(int32_t which, int32_t n, int32_t nrhs, uint32_t mask, const double* coef, double* d_A,
                         int64_t lda, double* d_B, int64_t ldb, const double* d_C, int64_t ldc, const double* d_D,
                         int64_t ldd, double* d_T, double* out) {
    return sc::debug_pcg_vec(which, n, nrhs, mask, coef, d_A, lda, d_B, ldb, d_C, ldc, d_D, ldd, d_T, out,
                             g_last_error);
}

int64_t sc_debug_spmv(int32_t mode, int32_t n, const int64_t* rp, const int32_t* ci, const int64_t* sp, int64_t nval,
                      const double* d_Ax, int32_t nrhs, const double* d_X, int64_t ldx, const double* d_B, int64_t ldb,
                      double* d_R, int64_t ldr, double* d_W, int64_t ldw, double* d_norms) {
    try {
        return sc::debug_spmv(mode, n, rp, ci, sp, nval, d_Ax, nrhs, d_X, ldx, d_B, ldb, d_R, ldr, d_W, ldw, d_norms,
                              g_last_error);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
}

// ---- weighted normal equations ----
static int64_t normal_fail(const char* who, const std::string& what) {
    g_last_error = std::string(who) + ": " + what;
    return SC_ERR_ARG;
}

// runs f, maps bad_alloc and carries the handle's message over
static int64_t normal_call(sc_normal* h, const std::function<int64_t()>& f) {
    int64_t rc;
    h->N->err.clear();  // a failure without a message of its own must not show an earlier one
    try {
        rc = f();
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
    if (rc < 0) g_last_error = h->N->err;
    return rc;
}

int64_t sc_normal_create(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const int64_t* Cp,
                         const int32_t* Ci, int32_t device, sc_normal** out) {
    if (!out) return normal_fail("sc_normal_create", "null out");
    *out = nullptr;
    sc_normal* h = new (std::nothrow) sc_normal();
    if (!h) return SC_ERR_NOMEM;
    int64_t rc;
    std::string err;
    try {
        rc = sc::normal_create(m, n, Jp, Ji, Cp, Ci, device, h->N, err);
    } catch (const std::bad_alloc&) {
        rc = SC_ERR_NOMEM;
    }
    if (rc != SC_OK) {
        g_last_error = err;
        delete h;
        return rc;
    }
    *out = h;
    return SC_OK;
}

void sc_normal_free(sc_normal* normal) {
    if (!normal) return;
    sc::normal_free(normal->N);
    delete normal;
}

int64_t sc_normal_pattern(const sc_normal* normal, int64_t* Sp, int32_t* Si) {
    if (!normal) return normal_fail("sc_normal_pattern", "null handle");
    const sc::NormalStruct& H = normal->N->H;
    if (Sp) std::copy(H.Sp.begin(), H.Sp.end(), Sp);
    if (Si) std::copy(H.Si.begin(), H.Si.end(), Si);
    return (int64_t)H.Si.size();
}

int64_t sc_normal_terms(const sc_normal* normal) {
    if (!normal) return normal_fail("sc_normal_terms", "null handle");
    return normal->N->H.T;
}

int64_t sc_normal_term_lists(const sc_normal* normal, int64_t* tp, int32_t* pa, int32_t* pb, int32_t* r,
                             int64_t* cpos) {
    if (!normal) return normal_fail("sc_normal_term_lists", "null handle");
    const sc::NormalStruct& H = normal->N->H;
    if (tp) std::copy(H.tp.begin(), H.tp.end(), tp);
    if (pa) std::copy(H.ta.begin(), H.ta.end(), pa);
    if (pb) std::copy(H.tb.begin(), H.tb.end(), pb);
    if (r) std::copy(H.tr.begin(), H.tr.end(), r);
    if (cpos) std::copy(H.cpos.begin(), H.cpos.end(), cpos);
    return H.T;
}

int64_t sc_normal_rows(const sc_normal* normal, int64_t* rp, int32_t* ci, int64_t* sp) {
    if (!normal) return normal_fail("sc_normal_rows", "null handle");
    const sc::NormalStruct& H = normal->N->H;
    if (rp) std::copy(H.rp.begin(), H.rp.end(), rp);
    if (ci) std::copy(H.ci.begin(), H.ci.end(), ci);
    if (sp) std::copy(H.sp.begin(), H.sp.end(), sp);
    return H.nnzJ;
}

int64_t sc_normal_memory(const sc_normal* normal, int64_t* out, int32_t cap) {
    if (!normal || (!out && cap > 0) || cap < 0) return normal_fail("sc_normal_memory", "null handle or array");
    return sc::normal_memory(*normal->N, out, cap);
}

int64_t sc_normal_constants(int32_t* out, int32_t cap) {
    const int32_t v[4] = {sc::NORMAL_SHORT, sc::NORMAL_LANES, sc::NORMAL_CH, sc::NORMAL_PCH};
    if ((!out && cap > 0) || cap < 0) return normal_fail("sc_normal_constants", "null array");
    for (int32_t k = 0; k < cap && k < 4; ++k) out[k] = v[k];
    return 4;
}

// the value arrays of a form call: Jx, and Cx where the handle has base entries
static int64_t normal_value_args(sc_normal* h, const double* Jx, const double* Cx, const char* who) {
    if (!h) return normal_fail(who, "null handle");
    const sc::NormalStruct& H = h->N->H;
    if (H.nnzJ > 0 && !Jx) return normal_fail(who, "null Jx");
    if (Cx && !H.has_base) return normal_fail(who, "base values given, but the handle was created without a base pattern");
    return SC_OK;
}

static int64_t normal_values(sc_normal* h, const double* Jx, const double* w, const double* Cx, const double* d,
                             double lambda, double* Sx, bool host, const char* who) {
    int64_t rc = normal_value_args(h, Jx, Cx, who);
    if (rc != SC_OK) return rc;
    if (!Sx && !h->N->H.Si.empty()) return normal_fail(who, "null Sx");
    return normal_call(h, [&] { return sc::normal_values(*h->N, Jx, w, Cx, d, lambda, Sx, host, who); });
}

int64_t sc_normal_values_host(sc_normal* normal, const double* Jx, const double* w, const double* Cx,
                              const double* d, double lambda, double* Sx) {
    return normal_values(normal, Jx, w, Cx, d, lambda, Sx, true, "sc_normal_values_host");
}
int64_t sc_normal_values_device(sc_normal* normal, const double* d_Jx, const double* d_w, const double* d_Cx,
                                const double* d_d, double lambda, double* d_Sx) {
    return normal_values(normal, d_Jx, d_w, d_Cx, d_d, lambda, d_Sx, false, "sc_normal_values_device");
}

static int64_t normal_factor(sc_normal* h, sc_numeric* num, const double* Jx, const double* w, const double* Cx,
                             const double* d, double lambda, bool host, const char* who) {
    int64_t rc = normal_value_args(h, Jx, Cx, who);
    if (rc != SC_OK) return rc;
    if (!num || !num->N) return normal_fail(who, "null numeric handle");
    return normal_call(h, [&] { return sc::normal_factor(*h->N, *num->N, Jx, w, Cx, d, lambda, host, who); });
}

int64_t sc_normal_factor_host(sc_normal* normal, sc_numeric* num, const double* Jx, const double* w,
                              const double* Cx, const double* d, double lambda) {
    return normal_factor(normal, num, Jx, w, Cx, d, lambda, true, "sc_normal_factor_host");
}
int64_t sc_normal_factor_device(sc_normal* normal, sc_numeric* num, const double* d_Jx, const double* d_w,
                                const double* d_Cx, const double* d_d, double lambda) {
    return normal_factor(normal, num, d_Jx, d_w, d_Cx, d_d, lambda, false, "sc_normal_factor_device");
}

const double* sc_normal_values_ptr(const sc_normal* normal) {
    return (normal && normal->N->values_valid) ? normal->N->Sbuf : nullptr;
}

static int64_t normal_product(sc_normal* h, bool transposed, int32_t nrhs, const double* Jx, const double* w,
                              const double* X, int64_t ldx, double* Y, int64_t ldy, bool host, const char* who) {
    if (!h) return normal_fail(who, "null handle");
    const sc::NormalStruct& H = h->N->H;
    const int64_t nin = transposed ? H.m : H.n, nout = transposed ? H.n : H.m;
    if (nrhs < 0) return normal_fail(who, "nrhs < 0");
    if (ldx < nin) return normal_fail(who, "leading dimension of the input below its row count");
    if (ldy < nout) return normal_fail(who, "leading dimension of the output below its row count");
    if (nrhs > 0 && nout > 0) {
        if (!Y || (nin > 0 && !X)) return normal_fail(who, "null panel");
        if (H.nnzJ > 0 && !Jx) return normal_fail(who, "null Jx");
        if ((const double*)Y == X) return normal_fail(who, "the output aliases the input");
    }
    return normal_call(h, [&] { return sc::normal_product(*h->N, transposed, nrhs, Jx, w, X, ldx, Y, ldy, host, who); });
}

int64_t sc_normal_mul_host_multi(sc_normal* normal, int32_t nrhs, const double* Jx, const double* X, int64_t ldx,
                                 double* Y, int64_t ldy) {
    return normal_product(normal, false, nrhs, Jx, nullptr, X, ldx, Y, ldy, true, "sc_normal_mul_host_multi");
}
int64_t sc_normal_mul_device_multi(sc_normal* normal, int32_t nrhs, const double* d_Jx, const double* d_X,
                                   int64_t ldx, double* d_Y, int64_t ldy) {
    return normal_product(normal, false, nrhs, d_Jx, nullptr, d_X, ldx, d_Y, ldy, false, "sc_normal_mul_device_multi");
}
int64_t sc_normal_mult_host_multi(sc_normal* normal, int32_t nrhs, const double* Jx, const double* w,
                                  const double* Y, int64_t ldy, double* G, int64_t ldg) {
    return normal_product(normal, true, nrhs, Jx, w, Y, ldy, G, ldg, true, "sc_normal_mult_host_multi");
}
int64_t sc_normal_mult_device_multi(sc_normal* normal, int32_t nrhs, const double* d_Jx, const double* d_w,
                                    const double* d_Y, int64_t ldy, double* d_G, int64_t ldg) {
    return normal_product(normal, true, nrhs, d_Jx, d_w, d_Y, ldy, d_G, ldg, false, "sc_normal_mult_device_multi");
}

static int64_t normal_lstsq(sc_normal* h, sc_numeric* num, const sc_refine_options* opt, int32_t nrhs,
                            const double* Jx, const double* w, const double* B, int64_t ldb, double* X, int64_t ldx,
                            sc_lstsq_info* info, bool host, const char* who) {
    if (!h) return normal_fail(who, "null handle");
    if (!num || !num->N) return normal_fail(who, "null numeric handle");
    const sc::NormalStruct& H = h->N->H;
    if (nrhs < 0) return normal_fail(who, "nrhs < 0");
    if (ldb < H.m) return normal_fail(who, "leading dimension of B below m");
    if (ldx < H.n) return normal_fail(who, "leading dimension of X below n");
    if (nrhs > 0 && H.n > 0) {
        if (!X || (H.m > 0 && !B)) return normal_fail(who, "null B or X");
        if (H.nnzJ > 0 && !Jx) return normal_fail(who, "null Jx");
        if ((const double*)X == B) return normal_fail(who, "X aliases B (the steps need B after X exists)");
    }
    sc_refine_options o;
    sc_default_refine_options(&o);
    if (opt) {
        if (opt->struct_size != (int32_t)sizeof(sc_refine_options))
            return normal_fail(who, "sc_refine_options.struct_size does not match this library's "
                                    "sizeof(sc_refine_options): initialise the options with sc_default_refine_options()");
        o = *opt;
    }
    if (o.max_iter < 0) return normal_fail(who, "max_iter < 0");
    if (!(o.rho_max > 0.0 && o.rho_max < 1.0)) return normal_fail(who, "rho_max outside (0, 1)");
    const int64_t rc = residual_mode_arg(o.residual, who);
    if (rc != SC_OK) return rc;
    return normal_call(
        h, [&] { return sc::normal_lstsq(*h->N, *num->N, o, nrhs, Jx, w, B, ldb, X, ldx, info, host, who); });
}

int64_t sc_normal_lstsq_host_multi(sc_normal* normal, sc_numeric* num, const sc_refine_options* opt, int32_t nrhs,
                                   const double* Jx, const double* w, const double* B, int64_t ldb, double* X,
                                   int64_t ldx, sc_lstsq_info* info) {
    return normal_lstsq(normal, num, opt, nrhs, Jx, w, B, ldb, X, ldx, info, true, "sc_normal_lstsq_host_multi");
}
int64_t sc_normal_lstsq_device_multi(sc_normal* normal, sc_numeric* num, const sc_refine_options* opt, int32_t nrhs,
                                     const double* d_Jx, const double* d_w, const double* d_B, int64_t ldb,
                                     double* d_X, int64_t ldx, sc_lstsq_info* info) {
    return normal_lstsq(normal, num, opt, nrhs, d_Jx, d_w, d_B, ldb, d_X, ldx, info, false,
                        "sc_normal_lstsq_device_multi");
}

int64_t sc_debug_normal_form(int64_t ne, const int64_t* tp, const int32_t* ta, const int32_t* tb, const int32_t* tr,
                             const int64_t* cpos, const int32_t* dcol, int64_t nJ, int64_t nw, int64_t nC, int64_t nd,
                             const double* d_Jx, const double* d_w, const double* d_Cx, const double* d_d,
                             double lambda, double* d_Sx) {
    try {
        g_last_error.clear();
        return sc::debug_normal_form(ne, tp, ta, tb, tr, cpos, dcol, nJ, nw, nC, nd, d_Jx, d_w, d_Cx, d_d, lambda,
                                     d_Sx, g_last_error);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
}

int64_t sc_debug_normal_mul(int32_t mode, int64_t m, int64_t n, const int64_t* rp, const int32_t* ci,
                            const int64_t* sp, int64_t nval, const double* d_Jx, int32_t nrhs, const double* d_X,
                            int64_t ldx, const double* d_B, int64_t ldb, double* d_R, int64_t ldr) {
    try {
        g_last_error.clear();
        if (!sp) return normal_fail("sc_debug_normal_mul", "null sp");
        return sc::debug_normal_prod(false, mode, m, n, rp, ci, sp, nval, d_Jx, nullptr, nrhs, d_X, ldx, d_B, ldb, d_R,
                                     ldr, g_last_error);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
}

int64_t sc_debug_normal_mult(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const double* d_Jx,
                             const double* d_w, int32_t nrhs, const double* d_Y, int64_t ldy, double* d_G,
                             int64_t ldg) {
    try {
        g_last_error.clear();
        const int64_t nval = (Jp && n > 0) ? Jp[n] : 0;
        return sc::debug_normal_prod(true, 0, n, m, Jp, Ji, nullptr, nval, d_Jx, d_w, nrhs, d_Y, ldy, nullptr, 0, d_G,
                                     ldg, g_last_error);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
}

int64_t sc_debug_normal_pair(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const int64_t* rp,
                             const int32_t* ci, const int64_t* sp, const double* d_Jx, const double* d_w, int32_t nrhs,
                             const double* d_X, int64_t ldx, const double* d_B, int64_t ldb, double* d_R, double* d_Rl,
                             int64_t ldr, double* d_G, double* d_Gl, int64_t ldg) {
    try {
        g_last_error.clear();
        return sc::debug_normal_pair(m, n, Jp, Ji, rp, ci, sp, d_Jx, d_w, nrhs, d_X, ldx, d_B, ldb, d_R, d_Rl, ldr, d_G,
                                     d_Gl, ldg, g_last_error);
    } catch (const std::bad_alloc&) {
        return SC_ERR_NOMEM;
    }
}

// ---- reference-API helpers ----
int64_t sc_etree(int64_t n, const int64_t* Ap, const int32_t* Ai, int32_t* parent) {
    if (n < 0 || !Ap || !parent) return SC_ERR_ARG;
    sc::etree(n, Ap, Ai, parent);
    return SC_OK;
}

int64_t sc_post_order(int64_t n, const int32_t* parent, int32_t* post) {
    if (n < 0 || !parent || !post) return SC_ERR_ARG;
    sc::post_order(n, parent, post);
    return SC_OK;
}

int64_t sc_col_count(int64_t n, const int64_t* Ap, const int32_t* Ai, const int32_t* parent,
                     const int32_t* post, int64_t* colcount) {
    if (n < 0 || !Ap || !parent || !post || !colcount) return SC_ERR_ARG;
    sc::col_count(n, Ap, Ai, parent, post, colcount);
    return SC_OK;
}

int64_t sc_ereach(int64_t n, const int64_t* Ap, const int32_t* Ai, const double* Ax, int64_t k,
                  const int32_t* parent, int32_t* s, int32_t* w, double* x) {
    if (n < 0 || k < 0 || k >= n || !Ap || !parent || !s || !w) return SC_ERR_ARG;
    std::vector<int32_t> path((size_t)n);
    return sc::ereach(n, Ap, Ai, Ax, k, parent, s, w, x, path);
}

int64_t sc_compute_levels(int64_t n, const int32_t* parent, int32_t* level_of) {
    if (n < 0 || !parent) return SC_ERR_ARG;
    return sc::compute_levels(n, parent, level_of);
}

int64_t sc_compute_supernodes(int64_t n, const int32_t* parent, const int64_t* Lp, int32_t* sn_id,
                              int64_t* supernodes) {
    if (n < 0 || !parent || !Lp) return SC_ERR_ARG;
    return sc::compute_supernodes_ref(n, parent, Lp, sn_id, supernodes);
}

int64_t sc_atree(int64_t n, const int64_t* Lp, const int32_t* Li, const int32_t* sn_id,
                 const int64_t* supernodes, int64_t ns, int32_t* super_parent) {
    if (n < 0 || !Lp || !Li || !sn_id || !supernodes || !super_parent) return SC_ERR_ARG;
    return sc::atree_ref(n, Lp, Li, sn_id, supernodes, ns, super_parent);
}

int64_t sc_triplet_to_csc(int64_t n, int64_t nt, const int32_t* ti, const int32_t* tj, const double* tx,
                          int64_t* Ap, int32_t* Ai, double* Ax) {
    if (n < 0 || nt < 0 || (nt > 0 && (!ti || !tj))) return SC_ERR_ARG;
    return sc::triplet_to_csc(n, nt, ti, tj, tx, Ap, Ai, Ax);
}

int64_t sc_read_mtx(const char* path, int64_t* n, int64_t* Ap, int32_t* Ai, double* Ax) {
    if (!path || !n) return SC_ERR_ARG;
    return sc::read_mtx(path, n, Ap, Ai, Ax);
}

int64_t sc_laplacian3d(int64_t k, int32_t nd_order, int64_t* Ap, int32_t* Ai, double* Ax, int32_t* perm) {
    return sc::laplacian3d(k, nd_order, Ap, Ai, Ax, perm);
}

// ---- multi-GPU ----
int64_t sc_dist_unique_id(void* id128) { return sc::dist_unique_id(id128); }

int64_t sc_dist_owner_map(const sc_symbolic* sym, int32_t nranks, int32_t* owner, double* work) {
    if (!sym || nranks <= 0) return SC_ERR_ARG;
    return sc::dist_owner_map(sym->S, nranks, owner, work);
}

int64_t sc_dist_schedule(const sc_symbolic* sym, int32_t nranks, int32_t rank, int32_t* level, int32_t* peer,
                         int64_t* bytes, int32_t* is_send, int64_t cap) {
    if (!sym || nranks <= 0 || rank < 0 || rank >= nranks) return SC_ERR_ARG;
    return sc::dist_schedule(sym->S, nranks, rank, level, peer, bytes, is_send, cap);
}

int64_t sc_numeric_create_dist(const sc_symbolic* sym, int32_t device, int32_t rank, int32_t nranks,
                               const void* id128, sc_numeric** out) {
    if (!sym || !out || nranks <= 0 || rank < 0 || rank >= nranks) return SC_ERR_ARG;
    *out = nullptr;
    sc_numeric* h = new (std::nothrow) sc_numeric();
    if (!h) return SC_ERR_NOMEM;
    std::string err;
    int64_t rc = sc::numeric_create_dist(sym->S, device, rank, nranks, id128, nullptr, nullptr, id128 ? 0 : 1, h->N,
                                         err);
    if (rc != SC_OK) {
        g_last_error = err;
        delete h;
        return rc;
    }
    h->sym = sym;
    *out = h;
    return SC_OK;
}

int64_t sc_numeric_create_dist_host(const sc_symbolic* sym, int32_t device, int32_t rank, int32_t nranks,
                                    sc_transport_fn fn, void* ctx, sc_numeric** out) {
    if (!sym || !out || !fn || nranks <= 0 || rank < 0 || rank >= nranks) return SC_ERR_ARG;
    *out = nullptr;
    sc_numeric* h = new (std::nothrow) sc_numeric();
    if (!h) return SC_ERR_NOMEM;
    std::string err;
    int64_t rc = sc::numeric_create_dist(sym->S, device, rank, nranks, nullptr, fn, ctx, 0, h->N, err);
    if (rc != SC_OK) {
        g_last_error = err;
        delete h;
        return rc;
    }
    h->sym = sym;
    *out = h;
    return SC_OK;
}

int64_t sc_numeric_create_dist_dry(const sc_symbolic* sym, int32_t device, int32_t rank, int32_t nranks,
                                   sc_numeric** out) {
    if (!sym || !out || nranks <= 0 || rank < 0 || rank >= nranks) return SC_ERR_ARG;
    *out = nullptr;
    sc_numeric* h = new (std::nothrow) sc_numeric();
    if (!h) return SC_ERR_NOMEM;
    std::string err;
    int64_t rc = sc::numeric_create_dist(sym->S, device, rank, nranks, nullptr, DIST_DRY, nullptr, 0, h->N, err);
    if (rc != SC_OK) {
        g_last_error = err;
        delete h;
        return rc;
    }
    h->sym = sym;
    *out = h;
    return SC_OK;
}

int64_t sc_numeric_create_dist_emulated(const sc_symbolic* sym, int32_t device, int32_t nranks, int32_t use_rccl,
                                        sc_numeric** out) {
    if (!sym || !out || nranks <= 0) return SC_ERR_ARG;
    *out = nullptr;
    sc_numeric* h = new (std::nothrow) sc_numeric();
    if (!h) return SC_ERR_NOMEM;
    std::string err;
    int64_t rc = sc::numeric_create_dist(sym->S, device, 0, nranks, nullptr, nullptr, nullptr, use_rccl ? 2 : 1, h->N,
                                         err);
    if (rc != SC_OK) {
        g_last_error = err;
        delete h;
        return rc;
    }
    h->sym = sym;
    *out = h;
    return SC_OK;
}

int64_t sc_memory_plan(const sc_symbolic* sym, int32_t nranks, int64_t* panel_bytes, int64_t* work_bytes,
                       int64_t* work_lower_bound_bytes) {
    if (!sym || nranks <= 0) return SC_ERR_ARG;
    std::vector<int64_t> p((size_t)nranks), w((size_t)nranks), l((size_t)nranks);
    const int64_t rc = sc::plan_memory_stats(sym->S, nranks, p.data(), w.data(), l.data());
    if (rc != SC_OK) return rc;
    for (int32_t r = 0; r < nranks; ++r) {
        if (panel_bytes) panel_bytes[r] = p[r] * (int64_t)sizeof(double);
        if (work_bytes) work_bytes[r] = w[r] * (int64_t)sizeof(double);
        if (work_lower_bound_bytes) work_lower_bound_bytes[r] = l[r] * (int64_t)sizeof(double);
    }
    return SC_OK;
}

int64_t sc_memory_plan_check(const sc_symbolic* sym, int32_t nranks) {
    if (!sym || nranks <= 0) return SC_ERR_ARG;
    return sc::plan_check(sym->S, nranks);
}

int64_t sc_numeric_memory(sc_numeric* num, int64_t* info, int32_t n) {
    if (!num || !num->N || !info) return SC_ERR_ARG;
    const sc::Numeric& N = *num->N;
    int64_t v[4] = {N.dev_bytes, 0, 0, 0};
    for (const sc::RankMem& R : N.R) {
        v[1] += R.panel_total * (int64_t)sizeof(double);
        v[2] += R.work_total * (int64_t)sizeof(double);
        v[3] += R.work_live_max * (int64_t)sizeof(double);
    }
    for (int32_t i = 0; i < n && i < 4; ++i) info[i] = v[i];
    return SC_OK;
}

int64_t sc_dist_steps(const sc_symbolic* sym, int32_t nranks, int32_t* kind, int32_t* level, int32_t* front,
                      int32_t* k, int32_t* p, int64_t cap) {
    if (!sym || nranks <= 0) return SC_ERR_ARG;
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
}

int64_t sc_dist_plan_info(const sc_symbolic* sym, int32_t nranks, int32_t* gsize, int32_t* split_cb_ranks,
                          int32_t* slab_ranks, int64_t* n_steps) {
    if (!sym || nranks <= 0) return SC_ERR_ARG;
    sc::DistPlan D;
    int64_t rc = sc::dist_plan(sym->S, nranks, D);
    if (rc != SC_OK) return rc;
    for (int32_t s = 0; s < sym->S.ns; ++s) {
        if (gsize) gsize[s] = D.gsize[s];
        if (split_cb_ranks) {
            int32_t v = 0;
            if (D.split[s] >= 0) {
                std::vector<int32_t> r = D.cb_rank[D.split[s]];
                std::sort(r.begin(), r.end());
                v = (int32_t)(std::unique(r.begin(), r.end()) - r.begin());
            }
            split_cb_ranks[s] = v;
        }
        if (slab_ranks) {
            int32_t v = 0;
            if (D.pd[s] >= 0) {
                std::vector<int32_t> r = D.slab_rank[D.pd[s]];
                std::sort(r.begin(), r.end());
                v = (int32_t)(std::unique(r.begin(), r.end()) - r.begin());
            }
            slab_ranks[s] = v;
        }
    }
    if (n_steps) *n_steps = (int64_t)D.steps.size();
    return (int64_t)D.msgs.size();
}

// ---- debug hooks ----
int64_t sc_debug_syrk(double* dC, int32_t ldc, const double* dA, int32_t lda, int32_t M, int32_t N,
                      int32_t K) {
    if (!dC || !dA || M < 0 || N < 0 || K < 0 || N > M) return SC_ERR_ARG;
    return sc::debug_syrk(dC, ldc, dA, lda, M, N, K);
}

int64_t sc_debug_syrk_ex(double* dC, int32_t ldc, const double* dA, int32_t lda, int32_t M, int32_t N, int32_t K,
                         int32_t bt, int32_t lean, int32_t tag, int32_t epi) {
    if (!dC || !dA) return SC_ERR_ARG;
    return sc::debug_syrk_ex(dC, ldc, dA, lda, M, N, K, bt, lean, tag, epi);
}

int64_t sc_debug_panel(double* dF, int32_t m, int32_t w, int32_t k0, int32_t mode, int32_t* info) {
    if (!dF || !info) return SC_ERR_ARG;
    return sc::debug_panel(dF, m, w, k0, mode, info);
}

int64_t sc_debug_updown_block(double* dF, int32_t m, int32_t w, int32_t k0, double* dW, int32_t sign,
                              int32_t* info) {
    if (!dF || !dW || !info) return SC_ERR_ARG;
    return sc::debug_updown_block(dF, m, w, k0, dW, sign, info);
}

int64_t sc_debug_solve_step(double* dF, int32_t m, int32_t w, int32_t k0, int32_t op, int32_t width, double* dC,
                            double* dY, double* dU) {
    if (!dF || !dC || !dY) return SC_ERR_ARG;
    return sc::debug_solve_step(dF, m, w, k0, op, width, dC, dY, dU);
}

int64_t sc_debug_solve_gather(int32_t width, int32_t w, int32_t mb, int32_t nchild, const int64_t* rel_ptr,
                              const int32_t* relind, const double* dUc, double* dC, double* dU) {
    if (!rel_ptr || !dC) return SC_ERR_ARG;
    return sc::debug_solve_gather(width, w, mb, nchild, rel_ptr, relind, dUc, dC, dU);
}

int64_t sc_debug_bench(int32_t which, int32_t M, int32_t K, int32_t reps, int32_t arg, double* tflops) {
    if (!tflops || M <= 0 || K <= 0 || reps <= 0) return SC_ERR_ARG;
    return sc::debug_bench(which, M, K, reps, arg, tflops);
}

int64_t sc_debug_contention(int32_t M, int32_t K, int32_t chain_rows, int32_t nchain, int32_t mode,
                            int32_t mask_stride, double* out) {
    if (!out) return SC_ERR_ARG;
    return sc::debug_contention(M, K, chain_rows, nchain, mode, mask_stride, out);
}

int64_t sc_debug_hwid(int32_t nwg, int32_t threads, int32_t spin_ticks, uint32_t* out) {
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
}

int64_t sc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // extern "C"
