// The structure of S = C + J^T diag(w) J + diag(d) + lambda I from the structure of J (host
// only).  J by rows first (columns ascending, with the position of
// each value in J's CSC array); then, column j of S at a time, the entries (i, j), i <= j:
// the columns i <= j of every row of J's column j, the rows of C's column j and the
// diagonal.  A second walk over the same rows, which ascend down J's column, drops each
// term (position of J[r, i], position of J[r, j], r) at the end of its entry's list, so the
// rows of a list ascend.  The work is one visit per term, T = sum_r nnz_r (nnz_r + 1) / 2.
#include <algorithm>

#include "../../include/sparsecholesky.h"
#include "normal.hpp"

namespace sc {

int64_t normal_build(int64_t m, int64_t n, const int64_t* Jp, const int32_t* Ji, const int64_t* Cp, const int32_t* Ci,
                     NormalStruct& H, std::string& err) {
    auto bad = [&](const std::string& what) {
        err = "sc_normal_create: " + what;
        return (int64_t)SC_ERR_ARG;
    };
    if (m < 0 || n < 0 || m > INT32_MAX || n > INT32_MAX) return bad("m or n negative or above 2^31 - 1");
    if (!Jp) return bad("null Jp");
    if (Jp[0] != 0) return bad("Jp[0] != 0");
    for (int64_t j = 0; j < n; ++j)
        if (Jp[j + 1] < Jp[j]) return bad("Jp descends at column " + std::to_string(j));
    const int64_t nnzJ = Jp[n];
    if (nnzJ > INT32_MAX) return bad("J has more than 2^31 - 1 entries (a term holds 32-bit positions)");
    if (nnzJ > 0 && !Ji) return bad("null Ji");
    for (int64_t j = 0; j < n; ++j)
        for (int64_t p = Jp[j]; p < Jp[j + 1]; ++p) {
            if (Ji[p] < 0 || Ji[p] >= m)
                return bad("row index " + std::to_string(Ji[p]) + " of column " + std::to_string(j) + " outside [0, m)");
            if (p > Jp[j] && Ji[p] <= Ji[p - 1])
                return bad("row indices of column " + std::to_string(j) + " do not ascend strictly");
        }
    int64_t nnzC = 0;
    if (Cp) {
        if (Cp[0] != 0) return bad("Cp[0] != 0");
        for (int64_t j = 0; j < n; ++j)
            if (Cp[j + 1] < Cp[j]) return bad("Cp descends at column " + std::to_string(j));
        nnzC = Cp[n];
        if (nnzC > 0 && !Ci) return bad("null Ci");
        for (int64_t j = 0; j < n; ++j)
            for (int64_t p = Cp[j]; p < Cp[j + 1]; ++p) {
                if (Ci[p] < 0 || Ci[p] >= n)
                    return bad("base row index of column " + std::to_string(j) + " outside [0, n)");
                if (Ci[p] > j)
                    return bad("base entry (" + std::to_string(Ci[p]) + ", " + std::to_string(j) +
                               ") lies below the diagonal: the base pattern is upper triangular");
                if (p > Cp[j] && Ci[p] <= Ci[p - 1])
                    return bad("base row indices of column " + std::to_string(j) + " do not ascend strictly");
            }
    } else if (Ci) {
        return bad("Ci without Cp");
    }

    H = NormalStruct();
    H.m = m;
    H.n = n;
    H.nnzJ = nnzJ;
    H.nnzC = nnzC;
    H.has_base = Cp != nullptr;
    H.Jp.assign(Jp, Jp + n + 1);
    H.Ji.assign(Ji, Ji + nnzJ);
    if (Cp) {
        H.Cp.assign(Cp, Cp + n + 1);
        H.Ci.assign(Ci, Ci + nnzC);
    }

    // J by rows; the columns of a row ascend because the columns are visited in order
    H.rp.assign((size_t)m + 1, 0);
    for (int64_t p = 0; p < nnzJ; ++p) H.rp[Ji[p] + 1]++;
    for (int64_t r = 0; r < m; ++r) H.rp[r + 1] += H.rp[r];
    H.ci.resize((size_t)nnzJ);
    H.sp.resize((size_t)nnzJ);
    {
        std::vector<int64_t> nxt(H.rp.begin(), H.rp.end() - 1);
        for (int64_t j = 0; j < n; ++j)
            for (int64_t p = Jp[j]; p < Jp[j + 1]; ++p) {
                const int64_t q = nxt[Ji[p]]++;
                H.ci[q] = (int32_t)j;
                H.sp[q] = p;
            }
    }
    // the term count before anything of its size is allocated
    const int64_t TMAX = (int64_t)1 << 40;
    int64_t T = 0;
    for (int64_t r = 0; r < m; ++r) {
        const int64_t k = H.rp[r + 1] - H.rp[r];
        T += k * (k + 1) / 2;  // k <= n < 2^31: no overflow
        if (T > TMAX) return bad("J has more than 2^40 terms (sum over the rows of nnz (nnz + 1) / 2)");
    }
    H.T = T;
    H.ta.resize((size_t)T);
    H.tb.resize((size_t)T);
    H.tr.resize((size_t)T);

    // column j of S: mark[i] = terms of (i, j) so far (-1: not an entry); then its place
    std::vector<int64_t> mark((size_t)n, -1), cp_of((size_t)n, -1);
    std::vector<int32_t> rows;
    H.Sp.assign((size_t)n + 1, 0);
    H.tp.assign(1, 0);
    for (int64_t j = 0; j < n; ++j) {
        rows.clear();
        auto touch = [&](int32_t i) {
            if (mark[i] < 0) {
                mark[i] = 0;
                rows.push_back(i);
            }
        };
        touch((int32_t)j);
        if (Cp)
            for (int64_t p = Cp[j]; p < Cp[j + 1]; ++p) {
                touch(Ci[p]);
                cp_of[Ci[p]] = p;
            }
        for (int64_t p = Jp[j]; p < Jp[j + 1]; ++p) {
            const int64_t r = Ji[p];
            for (int64_t q = H.rp[r]; q < H.rp[r + 1] && H.ci[q] <= j; ++q) {
                touch(H.ci[q]);
                mark[H.ci[q]]++;
            }
        }
        std::sort(rows.begin(), rows.end());
        if ((int64_t)H.Si.size() + (int64_t)rows.size() > INT32_MAX)
            return bad("S has more than 2^31 - 1 entries (a task holds a 32-bit entry index)");
        for (int32_t i : rows) {
            if (mark[i] > INT32_MAX) return bad("an entry of S has more than 2^31 - 1 terms");
            H.Si.push_back(i);
            H.cpos.push_back(cp_of[i]);
            H.dcol.push_back(i == j ? (int32_t)j : -1);
            const int64_t first = H.tp.back();
            H.tp.push_back(first + mark[i]);
            mark[i] = first;  // from here on: where the entry's next term goes
        }
        for (int64_t p = Jp[j]; p < Jp[j + 1]; ++p) {
            const int64_t r = Ji[p];
            for (int64_t q = H.rp[r]; q < H.rp[r + 1] && H.ci[q] <= j; ++q) {
                const int64_t t = mark[H.ci[q]]++;
                H.ta[t] = (int32_t)H.sp[q];
                H.tb[t] = (int32_t)p;
                H.tr[t] = (int32_t)r;
            }
        }
        for (int32_t i : rows) {
            mark[i] = -1;
            cp_of[i] = -1;
        }
        H.Sp[j + 1] = (int64_t)H.Si.size();
    }
    return SC_OK;
}

void normal_base_rows(const NormalStruct& H, std::vector<int64_t>& rp, std::vector<int32_t>& ci,
                      std::vector<int64_t>& pos) {
    const int64_t n = H.n;
    rp.assign((size_t)n + 1, 0);
    for (int64_t j = 0; j < n; ++j) {
        rp[j + 1]++;  // the diagonal shift
        if (H.has_base)
            for (int64_t p = H.Cp[j]; p < H.Cp[j + 1]; ++p) {
                rp[H.Ci[p] + 1]++;
                if (H.Ci[p] != j) rp[j + 1]++;
            }
    }
    for (int64_t i = 0; i < n; ++i) rp[i + 1] += rp[i];
    ci.resize((size_t)rp[n]);
    pos.resize((size_t)rp[n]);
    std::vector<int64_t> nxt(rp.begin(), rp.end() - 1);
    auto put = [&](int64_t row, int64_t col, int64_t p) {
        const int64_t q = nxt[row]++;
        ci[q] = (int32_t)col;
        pos[q] = p;
    };
    // three passes keep a row's columns ascending: an entry (i, j), i < j, stored in column j
    // goes to row j as column i (the row's lower half, ascending in i down the column), then
    // the diagonal, then to row i as column j (its upper half, ascending as the columns are walked)
    if (H.has_base)
        for (int64_t j = 0; j < n; ++j)
            for (int64_t p = H.Cp[j]; p < H.Cp[j + 1]; ++p)
                if (H.Ci[p] < j) put(j, H.Ci[p], p);
    for (int64_t j = 0; j < n; ++j) {
        if (H.has_base)
            for (int64_t p = H.Cp[j]; p < H.Cp[j + 1]; ++p)
                if (H.Ci[p] == j) put(j, j, p);
        put(j, j, H.nnzC + j);
    }
    if (H.has_base)
        for (int64_t j = 0; j < n; ++j)
            for (int64_t p = H.Cp[j]; p < H.Cp[j + 1]; ++p)
                if (H.Ci[p] < j) put(H.Ci[p], j, p);
}

void normal_form_tasks(int64_t ne, const int64_t* tp, std::vector<NormalFormTask>& task,
                       std::vector<NormalFormLong>& lng, int64_t& nslots) {
    task.clear();
    lng.clear();
    nslots = 0;
    for (int64_t e = 0; e < ne; ++e) {
        const int64_t len = tp[e + 1] - tp[e];
        if (len <= NORMAL_SHORT) continue;
        if (len <= NORMAL_CH) {
            task.push_back({tp[e], (int32_t)e, (int32_t)len, -1, 0});
            continue;
        }
        const int64_t nch = (len + NORMAL_CH - 1) / NORMAL_CH;
        lng.push_back({(int32_t)e, (int32_t)nslots, (int32_t)nch, 0});
        for (int64_t t = tp[e]; t < tp[e + 1]; t += NORMAL_CH)
            task.push_back({t, (int32_t)e, (int32_t)std::min<int64_t>(NORMAL_CH, tp[e + 1] - t), (int32_t)nslots++, 0});
    }
}

void normal_prod_tasks(int64_t nvec, const int64_t* ptr, std::vector<NormalProdTask>& task,
                       std::vector<NormalProdLong>& lng, int64_t& nslots) {
    task.clear();
    lng.clear();
    nslots = 0;
    for (int64_t v = 0; v < nvec; ++v) {
        const int64_t len = ptr[v + 1] - ptr[v];
        if (len <= NORMAL_PCH) {
            task.push_back({ptr[v], (int32_t)v, -1});
            continue;
        }
        lng.push_back({(int32_t)v, (int32_t)nslots});
        for (int64_t e = ptr[v]; e < ptr[v + 1]; e += NORMAL_PCH) task.push_back({e, (int32_t)v, (int32_t)nslots++});
    }
}

}  // namespace sc
