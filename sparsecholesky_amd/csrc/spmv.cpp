// The matrix A itself as a gather structure (host only): the full
// symmetric matrix by rows, in A's own numbering, for the products and residuals of
// refine.cpp.  It is built from the entries the factorization uses -- the analysis' own
// list a_ptr / a_pos / a_src (symbolic.cpp: entries with row > column ignored, of
// duplicates of one (row, column) the last one), mapped back from the internal numbering
// through the postorder and the fill-reducing permutation -- so a product with this
// structure is a product with exactly the matrix that was factored, whatever the ordering
// or the Schur set.  A used entry (i, k), i < k, appears in row i and in row k, a diagonal
// entry once; within a row the columns ascend.  sp is the entry's index in the caller's
// value array, so the values are read where they lie.
#include <algorithm>
#include <utility>
#include <vector>

#include "symbolic.hpp"

namespace sc {

i64 spmv_structure(const Symbolic& S, i64* rp, i32* ci, i64* sp) {
    const i64 n = S.n;
    // natural (A's own) index of an internal one
    auto nat = [&](i32 v) -> i32 {
        const i32 p = S.post[v];
        return S.perm.empty() ? p : S.perm[p];
    };
    std::vector<i64> cnt((size_t)n + 1, 0);
    for (i32 s = 0; s < S.ns; ++s) {
        const i32* rows = S.rows.data() + S.rows_ptr[s];
        for (i32 c = S.sn_start[s]; c < S.sn_start[s + 1]; ++c) {
            const i32 k = nat(c);
            for (i64 q = S.a_ptr[c]; q < S.a_ptr[c + 1]; ++q) {
                const i32 i = nat(rows[S.a_pos[q]]);
                cnt[i + 1]++;
                if (i != k) cnt[k + 1]++;
            }
        }
    }
    for (i64 i = 0; i < n; ++i) cnt[i + 1] += cnt[i];
    const i64 total = n > 0 ? cnt[n] : 0;
    if (rp) std::copy(cnt.begin(), cnt.end(), rp);
    if (!ci || !sp) return total;
    std::vector<i64> nxt(cnt.begin(), cnt.end() - 1);
    for (i32 s = 0; s < S.ns; ++s) {
        const i32* rows = S.rows.data() + S.rows_ptr[s];
        for (i32 c = S.sn_start[s]; c < S.sn_start[s + 1]; ++c) {
            const i32 k = nat(c);
            for (i64 q = S.a_ptr[c]; q < S.a_ptr[c + 1]; ++q) {
                const i32 i = nat(rows[S.a_pos[q]]);
                i64 e = nxt[i]++;
                ci[e] = k;
                sp[e] = S.a_src[q];
                if (i != k) {
                    e = nxt[k]++;
                    ci[e] = i;
                    sp[e] = S.a_src[q];
                }
            }
        }
    }
    // columns ascending per row: one fixed order of every row's sum
    std::vector<std::pair<i32, i64>> tmp;
    for (i64 i = 0; i < n; ++i) {
        const i64 b = cnt[i], e = cnt[i + 1];
        tmp.clear();
        for (i64 q = b; q < e; ++q) tmp.push_back({ci[q], sp[q]});
        std::sort(tmp.begin(), tmp.end());
        for (i64 q = b; q < e; ++q) {
            ci[q] = tmp[q - b].first;
            sp[q] = tmp[q - b].second;
        }
    }
    return total;
}

i64 value_entries(const Symbolic& S, i32* row, i32* col, i32* effective) {
    const i64 n = S.n, nnz = S.nnzA_in;
    const std::vector<i64>& Ap = S.Ap_in.empty() ? S.Ap : S.Ap_in;
    const std::vector<i32>& Ai = S.Ap_in.empty() ? S.Ai : S.Ai_in;
    for (i64 k = 0; k < n; ++k)
        for (i64 p = Ap[k]; p < Ap[k + 1]; ++p) {
            if (row) row[p] = Ai[p];
            if (col) col[p] = (i32)k;
        }
    if (effective) {
        std::fill(effective, effective + nnz, 0);
        for (i64 q = 0; q < S.nnzA_used; ++q) effective[S.a_src[q]] = 1;
    }
    return nnz;
}

}  // namespace sc
