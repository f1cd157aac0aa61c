// Rank-k update and downdate of the finished factor: given
// P A P^T = L L^T in the panel arena and a sparse n x k matrix W, L becomes the factor of
// P (A + sign W W^T) P^T in place, without a new factorization.
//
// Admissible W.  A column w (rows permuted to the order of P A P^T, j0 its smallest) must
// satisfy struct(w) within struct(L(:, j0)) -- the true pattern, not the front rows with
// their relaxed zeros.  Then the clique of w lies in the filled graph, the pattern of L
// does not grow, and the column travels up the etree path of j0 alone.  L(i, j0) != 0 iff
// j0 lies in the row subtree of i: some entry A(k, i), k <= j0, has j0 on its etree path
// towards i.  That walk (the one ereach makes) is done per entry, with the nodes below j0
// marked as reaching it or not, so a column costs its entries plus the nodes walked once.
//
// Sweep.  Internal (postorder) numbering.  A chunk of UPD_W = 16 columns is scattered into
// the zeroed workspace wd (n x 16).  The touched supernodes are the union of the
// assembly-tree paths from the supernodes of the j0 to the root; ascending supernode
// index is a topological order.  All 16 columns ride through every touched supernode: a
// column not yet active there has exact zeros on the pivot rows and the block kernel skips
// it, so its part of the transform is exactly the identity.  Per 64-column block the block
// kernel (one workgroup), then the row kernel over the front rows below; block b + 1 needs
// only what block b's row kernel wrote, so stream order is the only dependency.  The launch
// list depends on W: launched eagerly, no graph.
//
// The strict upper triangles of the diagonal blocks hold the solves' stored inverses; the
// kernels neither read nor write them.  A sweep starts a new generation of the factor
// (factor_gen), so the inverses, the Z panel of the selected inversion and a gathered copy
// are recomputed by their own mechanisms at their next use.
#include "numeric_impl.hpp"

namespace sc {

namespace {

// the columns of W in the order of P A P^T, validated: per column j0 (-1 when empty)
struct UpdCheck {
    std::vector<int32_t> iperm;  // A's row -> row of P A P^T (empty: the same)
    std::vector<int32_t> first;
};

int64_t check_columns(const Symbolic& S, int32_t k, const int64_t* Wp, const int32_t* Wi, UpdCheck& U,
                      const char* who, std::string& err) {
    const int64_t n = S.n;
    auto fail = [&](const std::string& what) {
        err = std::string(who) + ": " + what;
        return (int64_t)SC_ERR_ARG;
    };
    if (Wp[0] != 0) return fail("Wp[0] != 0");
    for (int32_t c = 0; c < k; ++c)
        if (Wp[c + 1] < Wp[c]) return fail("column pointers of W not monotone");
    if (Wp[k] > 0 && !Wi) return fail("null Wi");
    if (!S.perm.empty()) {
        U.iperm.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) U.iperm[S.perm[i]] = (int32_t)i;
    }
    U.first.assign((size_t)k, -1);
    std::vector<int32_t> seen((size_t)n, -1);   // column that last held the row
    std::vector<int32_t> mark((size_t)n, -1);   // 2 c + (reaches j0 of column c)
    for (int32_t c = 0; c < k; ++c) {
        int32_t j0 = INT32_MAX;
        for (int64_t p = Wp[c]; p < Wp[c + 1]; ++p) {
            const int32_t r = Wi[p];
            if (r < 0 || r >= n)
                return fail("column " + std::to_string(c) + " of W: row " + std::to_string(r) + " is out of range");
            if (seen[r] == c)
                return fail("column " + std::to_string(c) + " of W: row " + std::to_string(r) + " appears twice");
            seen[r] = c;
            j0 = std::min(j0, U.iperm.empty() ? r : U.iperm[r]);
        }
        if (j0 == INT32_MAX) continue;
        U.first[c] = j0;
        for (int64_t p = Wp[c]; p < Wp[c + 1]; ++p) {
            const int32_t i = U.iperm.empty() ? Wi[p] : U.iperm[Wi[p]];
            if (i == j0) continue;
            bool found = false;
            for (int64_t q = S.Ap[i]; q < S.Ap[i + 1] && !found; ++q) {
                const int32_t a = S.Ai[q];
                if (a > j0) continue;  // not in the subtree of j0 (and entries below the diagonal are ignored)
                int32_t v = a;
                while (v != -1 && v < j0 && (mark[v] >> 1) != c) v = S.parent[v];
                const bool hit = v == j0 || (v != -1 && v < j0 && mark[v] == 2 * c + 1);
                for (int32_t u = a; u != v; u = S.parent[u]) mark[u] = 2 * c + (hit ? 1 : 0);
                found = hit;
            }
            if (!found)
                return fail("column " + std::to_string(c) + " of W is not admissible: row " + std::to_string(Wi[p]) +
                            " (row " + std::to_string(i) + " of P A P^T) is outside the pattern of column " +
                            std::to_string(j0) + " of L, the column of its first row");
        }
    }
    return SC_OK;
}

// the supernodes on the assembly-tree paths of columns [c0, c1), ascending
void touched_supernodes(const Symbolic& S, const std::vector<int32_t>& first, int32_t c0, int32_t c1,
                        std::vector<char>& on, std::vector<int32_t>& list) {
    on.assign((size_t)S.ns, 0);
    list.clear();
    for (int32_t c = c0; c < c1; ++c) {
        if (first[c] < 0) continue;
        for (int32_t s = S.sn_of[S.ipost[first[c]]]; s != -1 && !on[s]; s = S.sn_parent[s]) {
            on[s] = 1;
            list.push_back(s);
        }
    }
    std::sort(list.begin(), list.end());
}

}  // namespace

int64_t updown_check(const Symbolic& S, int32_t k, const int64_t* Wp, const int32_t* Wi, int32_t* first_col,
                     int64_t* path, const char* who, std::string& err) {
    UpdCheck U;
    const int64_t rc = check_columns(S, k, Wp, Wi, U, who, err);
    if (rc != SC_OK) return rc;
    if (first_col)
        for (int32_t c = 0; c < k; ++c) first_col[c] = U.first[c];
    if (path) {
        std::vector<char> on;
        std::vector<int32_t> list;
        touched_supernodes(S, U.first, 0, k, on, list);
        path[0] = (int64_t)list.size();
        path[1] = path[2] = 0;
        for (int32_t s : list) {
            path[1] += (S.w(s) + PNB - 1) / PNB;
            path[2] += (int64_t)S.sn_m[s] * S.w(s);
        }
    }
    return SC_OK;
}

static int64_t updown_build(Numeric& N) {
    const Symbolic& S = *N.S;
    void* p = nullptr;
    TRY(dalloc(N, (size_t)S.n * UPD_W * sizeof(double), p));
    N.UPD.wd = (double*)p;
    TRY(dalloc(N, (size_t)UPD_K * UPD_K * sizeof(double), p));
    N.UPD.tbuf = (double*)p;
    TRY(dalloc(N, sizeof(int32_t), p));
    N.UPD.info = (int32_t*)p;
    int64_t maxcc = 1;
    for (int64_t j = 0; j < S.n; ++j) maxcc = std::max(maxcc, S.colcount[j]);
    N.upd_cap = maxcc * UPD_W;  // an admissible column has at most the entries of a column of L
    TRY(dalloc(N, (size_t)N.upd_cap * sizeof(int64_t), p));
    N.d_uidx = (int64_t*)p;
    TRY(dalloc(N, (size_t)N.upd_cap * sizeof(double), p));
    N.d_uval = (double*)p;
    N.UPD.sn_start = N.SP.sn_start;
    N.UPD.sn_m = N.SP.sn_m;
    N.UPD.panel_off = N.SP.panel_off;
    N.UPD.rows_ptr = N.SP.rows_ptr;
    N.UPD.rows = N.SP.rows;
    N.UPD.post = N.R[0].P.post;
    N.upd_ready = true;
    return SC_OK;
}

int64_t numeric_updown_host(Numeric& N, int32_t sign, int32_t k, const int64_t* Wp, const int32_t* Wi,
                            const double* Wx) {
    if (!N.factored) return SC_ERR_STATE;
    if (!N.owner.empty() || N.emulated || N.R.size() != 1) {
        N.err = "sc_updown_host: update and downdate run on single-device handles only (the panels of a "
                "multi-rank or emulated handle are spread over the ranks' arenas)";
        return SC_ERR_NOTIMPL;
    }
    const int64_t st = numeric_status(N);
    if (st != SC_OK) return st;
    const Symbolic& S = *N.S;
    if (k == 0 || S.n == 0) return SC_OK;
    UpdCheck U;
    TRY(check_columns(S, k, Wp, Wi, U, "sc_updown_host", N.err));
    if (Wp[k] > 0 && !Wx) {
        N.err = "sc_updown_host: null Wx";
        return SC_ERR_ARG;
    }
    TRY(solve_prepare(N));  // the front row lists and the panel offsets on the device
    if (!N.upd_ready) TRY(updown_build(N));
    N.UPD.panel_pool = N.gpanel;
    hipStream_t s0 = N.stream;
    const UpdPlan& P = N.UPD;
    std::vector<int64_t> idx;
    std::vector<double> val;
    std::vector<char> on;
    std::vector<int32_t> list;
    for (int32_t c0 = 0; c0 < k; c0 += UPD_W) {
        const int32_t c1 = std::min(k, c0 + UPD_W);  // a partial chunk: the other columns of wd stay zero
        idx.clear();
        val.clear();
        for (int32_t c = c0; c < c1; ++c)
            for (int64_t p = Wp[c]; p < Wp[c + 1]; ++p) {
                const int32_t i = U.iperm.empty() ? Wi[p] : U.iperm[Wi[p]];
                idx.push_back((int64_t)UPD_W * S.ipost[i] + (c - c0));
                val.push_back(Wx[p]);
            }
        if (idx.empty()) continue;  // empty columns: nothing to do
        if ((int64_t)idx.size() > N.upd_cap) {  // cannot happen for admissible columns
            N.err = "sc_updown_host: a chunk of W holds more entries than 16 columns of L";
            return SC_ERR_ARG;
        }
        touched_supernodes(S, U.first, c0, c1, on, list);
        HIP_TRY(hipMemsetAsync(P.wd, 0, (size_t)S.n * UPD_W * sizeof(double), s0));
        HIP_TRY(hipMemsetAsync(P.info, 0x7f, sizeof(int32_t), s0));
        HIP_TRY(hipMemcpyAsync(N.d_uidx, idx.data(), idx.size() * sizeof(int64_t), hipMemcpyHostToDevice, s0));
        HIP_TRY(hipMemcpyAsync(N.d_uval, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice, s0));
        HIP_TRY(launch_updown_scatter(P.wd, N.d_uidx, N.d_uval, (int64_t)idx.size(), s0));
        hipError_t e = hipSuccess;
        for (size_t q = 0; e == hipSuccess && q < list.size(); ++q) {
            const int32_t s = list[q];
            const int w = S.w(s), m = S.sn_m[s];
            for (int k0 = 0; e == hipSuccess && k0 < w; k0 += PNB) {
                const int nr = m - std::min(w, k0 + PNB);
                e = launch_updown_block(P, s, k0, sign, s0);
                if (e == hipSuccess) e = launch_updown_rows(P, s, k0, nr, s0);
            }
        }
        // the factor is being rewritten: whatever was derived from it is stale from here on
        N.factor_gen++;
        HIP_TRY(e);
        HIP_TRY(hipStreamSynchronize(s0));
        int32_t info = 0;
        HIP_TRY(hipMemcpy(&info, P.info, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (info != UPD_ARMED && info > 0) {
            // not positive definite: the smallest column recorded before the sweep stopped
            // becomes the handle's status until the next factorization
            N.status = info;
            N.status_valid = true;
            return info;
        }
    }
    return SC_OK;
}

}  // namespace sc
