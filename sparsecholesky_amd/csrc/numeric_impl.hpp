// Internal helpers shared by the numeric units (numeric.cpp: handle, plan upload,
// launch / replay; schedule.cpp: the static launch schedule; solve.cpp: export and
// triangular solves; debug.cpp: microbenchmark hooks).
#pragma once

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "numeric.hpp"

namespace sc {

// CB launches with every K below this carry the short-K instance tag (Launch::epi).  The
// tag only separates them in profiles: every SYRK instance stages its epilogue through LDS
// (it once chose a batched epilogue: K <= 121 gained, K = 226 lost).
// It also keeps them out of the CB tail re-cut.
constexpr int SC_EPI_KMAX = 192;

#define HIP_TRY(x)                                                                \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            N.err = std::string(#x) + ": " + hipGetErrorString(e_);               \
            return SC_ERR_HIP;                                                    \
        }                                                                         \
    } while (0)

template <class T>
inline int64_t upload(Numeric& N, const std::vector<T>& v, T*& dptr) {
    dptr = nullptr;
    size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        N.err = std::string("hipMalloc(plan): ") + hipGetErrorString(e);
        return SC_ERR_DEVMEM;
    }
    N.allocs.push_back(p);
    N.dev_bytes += (int64_t)bytes;
    if (!v.empty()) {
        e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            N.err = std::string("hipMemcpy(plan): ") + hipGetErrorString(e);
            return SC_ERR_HIP;
        }
    }
    dptr = (T*)p;
    return SC_OK;
}

// device allocation owned by the handle (freed by numeric_free)
int64_t dalloc(Numeric& N, size_t bytes, void*& p);

#define TRY(x)                        \
    do {                              \
        int64_t r_ = (x);             \
        if (r_ != SC_OK) return r_;   \
    } while (0)


// Staging slots of the hosted ranks' messages (patched to device addresses once
// the staging pool is allocated): slot < 0 = the buffer is the region itself.
struct CommBuild {
    std::vector<Copy2D> copies;
    std::vector<int64_t> copy_slot;
    std::vector<int2> ctiles;
    std::vector<int64_t> msg_slot, msg_src_slot;
    int64_t stage_total = 0;
};

struct SchedBuild {
    std::vector<ChainDesc> cdesc;
    std::vector<uint32_t> crelp;
    int64_t chain_init = 0;  // doubles of the chained fronts' packed images
    std::vector<TinyFront> tfr;  // tiny-tree plan
    std::vector<int2> ta, tph, tpr;
    int32_t tiny_lds = 0;
    std::vector<int32_t> small;
    std::vector<int2> asmv, potrf;
    std::vector<int2> asml;  // parallel to asmv: owned front columns [x, y) of a task
    std::vector<TrsmTask> trsm;
    std::vector<GemmTask> gemm;
    std::vector<int2> tiles;
    std::vector<int64_t> gblk;  // CB gather: per task, per 64 x 64 CB block, its first segment
    std::vector<GSeg> gseg;
    CommBuild cb;
};

// The static launch schedule of a handle (schedule.cpp): N.sched plus the task arrays
// in B, final device addresses of the hosted ranks' pools.
int64_t build_schedule(Numeric& N, SchedBuild& B);
// The hosted ranks' panel and work arenas back to back from the two pool bases.
void set_pool_bases(Numeric& N, double* pbase, double* wbase);
// What remains once the staging pool exists: staging slots to addresses, column
// limits for every assembly task.  B is then what numeric_init uploads.
void finish_build(Numeric& N, SchedBuild& B, double* staging);
SchedDigest schedule_digest(const Numeric& N, const SchedBuild& B);
// The extend-add tables of one parent front (w pivots, mb CB rows), which the schedule and
// sc_debug_extend_add build alike.  gather_segments_front: the CB SYRK's gather table -- per
// 64 x 64 block (rb, cbk <= rb) of the CB one entry of gblk (the block's first segment) and,
// in child-list order (the order the entries are added in), one GSeg per child kids[q] with CB
// rows and columns in the block, then the closing entry; rel_ptr / relind: the host's relative
// indices, d_relind their device copy, cb[q] the device CB of child q (null: not resident;
// its segments are left out and the result is false).  asm_block_tasks: the assembly tasks of
// 16-column block cb of front s (m rows): one task (column streaming), or one per 256-row
// tile from the block's diagonal tile down (write-once tiles).
bool gather_segments_front(int w, int mb, const int32_t* kids, int nkids, const int64_t* rel_ptr,
                           const int32_t* relind, const int32_t* d_relind, const double* const* cb,
                           std::vector<int64_t>& gblk, std::vector<GSeg>& gseg);
void asm_block_tasks(std::vector<int2>& out, int32_t s, int cb, int m, bool tiled);

// solve.cpp
// What every solve starts with: the whole factor in gpanel, the solve plan built.
int64_t solve_prepare(Numeric& N);
// solve_prepare plus the etree postorder alone on the device (N.d_etpost), which the factor
// operators and the Schur gather address rows of P A P^T by.
int64_t apply_prepare(Numeric& N);
// The diagonal-block inverses of the current factorization in place (launch_solve_inv,
// once per factorization; shared by the solves, the half solves and the selected inversion).
int64_t solve_inverses(Numeric& N);
// The solve task lists (launch_solve_inv's two, the diagonal kernels', the backward GEMV's,
// the forward kernels') and how one front (s: m rows, w > k0 columns) adds its tasks of the
// 128-column step k0 to them; goff: where the step's GEMV tasks start in bwd (a diagonal task
// addresses its partials relative to that).  solve_build and sc_debug_solve_step cut with it.
struct SolveCut {
    std::vector<int2> inv64, inv128;
    std::vector<int4> diag, bwd, fwd;
};
void solve_cut_front(int32_t s, int w, int m, int k0, int64_t goff, SolveCut& C);

// selinv.cpp: the Z panel of the current factorization, computed if it is not there (the
// status rules of numeric_selinv)
int64_t selinv_ensure(Numeric& N);
// The task lists of the selected inversion (the W / Z_RK tiles, the Z_KK products, their
// reductions, the pushes) and how block bi -- the 128-column step k0 of a front of m rows and
// w > k0 pivots -- adds its tasks to them: one tile per SEL_BM rows below the block; per 64 x
// 64 tile of the lower triangle of Z_KK (codes 0, 2, 3) one whole product (slot -1) or, for K
// = nb + nr > SEL_KSPLIT, selinv_kchunks(K) chunk products into consecutive partial slots
// from `slot` on (advanced) and one reduction.  selinv_cut_push: the 64 x 64 tiles of child
// c's Z_II (mbc rows) under parent s.  selinv_build, sc_debug_selinv_step and
// sc_debug_selinv_push cut with them.
struct SelCut {
    std::vector<int2> tiles;
    std::vector<int4> kk, red, push;
};
void selinv_cut_block(int bi, int w, int m, int k0, int64_t& slot, SelCut& C);
void selinv_cut_push(int32_t c, int32_t s, int mbc, SelCut& C);

// refine.cpp: what the products with A, the refinement and the conjugate gradients share
// a device buffer for the length of one host call
struct DevTemp {
    void* p = nullptr;
    ~DevTemp() {
        if (p) (void)hipFree(p);
    }
    int64_t get(Numeric& N, size_t bytes) {
        if (hipMalloc(&p, std::max<size_t>(bytes, 8)) != hipSuccess) {
            p = nullptr;
            N.err = "refinement: device allocation of a host call's staging failed";
            return SC_ERR_DEVMEM;
        }
        return SC_OK;
    }
};
// SC_OK on a single-device handle, else SC_ERR_NOTIMPL with who's name in N.err
int64_t single_device(Numeric& N, const char* who);
// single_device, the handle's device current, the gather structure of A and its panels built
int64_t spmv_ensure(Numeric& N, const char* who);
// the device values a call works with: the caller's (host ones staged), or, for null, the
// copy the last sc_factor made
int64_t device_values(Numeric& N, const double* Ax, bool host, DevTemp& stage, const double*& d_Ax,
                      const char* who);
// One pass over A for a panel of nr columns: X transposed into the handle's panel, then
// Y = A X (mode SPMV_MUL) or R = B - A X; h (SPMV_NQ x SOLVE_RHS, may be null): the norms,
// on the host when the call returns.
int64_t spmv_panel(Numeric& N, int mode, const double* d_Ax, int nr, const double* X, int64_t ldx, const double* B,
                   int64_t ldb, double* R, int64_t ldr, double* h);
// the two backward errors of column c from a pass's norms (0 / 0 = 0)
void backward_errors(const double* h, int c, double& bnorm, double& bcomp);
// n x nrhs host array (ld) into a packed device buffer (copy = false: the buffer alone), and back
int64_t stage_in(Numeric& N, DevTemp& t, const double* A, int64_t ld, int64_t n, int32_t nrhs, bool copy);
int64_t stage_out(Numeric& N, const DevTemp& t, double* A, int64_t ld, int64_t n, int32_t nrhs);

// dist.cpp
hipError_t comm_launch(Numeric& N, const Launch& L);
int64_t dist_min_info(Numeric& N, int32_t& info);
int64_t dist_gather_panels(Numeric& N);
void comm_destroy(Numeric& N);

}  // namespace sc
