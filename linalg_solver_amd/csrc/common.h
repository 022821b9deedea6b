// Internal declarations shared by the HIP sources of liblsx.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/lsx.h"

// Development build only (-DLSX_TSTAMP, tools/ts_lu.sh): device-clock stamps of kernel starts (first workgroup) and
// ends (every workgroup) without a profiler attached -- rocprofv3 stretches exactly the launch gaps one wants to see.
#ifdef LSX_TSTAMP
static __device__ long long *lsx_ts_buf;
struct TsScope {
    int id;
    __device__ static void put_at(int tag, long long t) {
        long long *b = lsx_ts_buf;
        const int i = atomicAdd((int *)b, 1);
        if (i < (1 << 20)) { b[1 + 2 * i] = tag; b[2 + 2 * i] = t; }
    }
    __device__ void put(int tag) { put_at(tag, wall_clock64()); }
    __device__ TsScope(int id_) : id(id_) { if (lsx_ts_buf && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) put(id); }
    __device__ ~TsScope() { if (lsx_ts_buf && threadIdx.x == 0) put(id | 0x100); }
};
#define LSX_TS(id) TsScope ts_scope_(id)
// a mark inside kernel `id` (workgroup 0 only, time taken earlier by the caller): tag = id | 0x200 | k << 12
#define LSX_TS_MARK(id, k, t) do { if (lsx_ts_buf && blockIdx.x == 0) TsScope::put_at((id) | 0x200 | ((k) << 12), (long long)(t)); } while (0)
#define LSX_TS_MARKS 1
#define LSX_TS_SETTER(name) extern "C" void lsx_ts_set_##name(long long *p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(lsx_ts_buf), &p, sizeof p); }
#else
#define LSX_TS(id)
#define LSX_TS_MARK(id, k, t)
#define LSX_TS_MARKS 0
#define LSX_TS_SETTER(name)
#endif

namespace lsx {

void set_error(const char *fmt, ...);

#define LSX_HIP(call)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            lsx::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                           __LINE__);                                                     \
            return LSX_ERR_HIP;                                                           \
        }                                                                                 \
    } while (0)

#define LSX_TRY(call)              \
    do {                           \
        int r_ = (call);           \
        if (r_ != LSX_OK) return r_; \
    } while (0)

#define LSX_ARG(cond)                                                     \
    do {                                                                  \
        if (!(cond)) {                                                    \
            lsx::set_error("bad argument: %s (%s:%d)", #cond, __FILE__, __LINE__); \
            return LSX_ERR_ARG;                                           \
        }                                                                 \
    } while (0)

struct ProfEvent {
    hipEvent_t a, b;
    int bucket;
};

struct Prof {
    unsigned mask = 0;  // bit b set: launches of bucket b are bracketed by events
    int sample = 1;     // bracket every sample-th launch of a bucket only (events on the look-ahead chain cost time)
    long long seen[LSX_PROF_NBUCKETS] = {0};
    std::vector<ProfEvent> pending;
    std::vector<hipEvent_t> pool;
    double ms[LSX_PROF_NBUCKETS] = {0};
    long long launches[LSX_PROF_NBUCKETS] = {0};
    double flops[LSX_PROF_NBUCKETS] = {0};
    double bytes[LSX_PROF_NBUCKETS] = {0};
};

}  // namespace lsx

// One device allocation owned by the handle: grown on demand by lsx::reserve (api.hip), never shrunk, freed by lsx_destroy.
struct DevBuf { void *p = nullptr; size_t bytes = 0; };

struct lsx_handle_s {
    // ---- resources
    int device = 0;
    int num_cu = 256;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // stream in use (own or borrowed)
    hipStream_t side_stream = nullptr;  // high-priority stream for the look-ahead panel
    hipEvent_t ev_panel = nullptr, ev_next = nullptr, ev_start = nullptr, ev_done = nullptr;
    lsx::Prof prof;
    // ---- options (lsx_set_option)
    int nb = 128;        // panel width (<= 128)
    int kblock = 1;      // panels per trailing update: update depth K = kblock * nb
    int panel_mode = 4;  // 0 = per-column launches, 3 = pipelined (device-scope exchange), 4 = XCD-scope exchange on one XCD (taller panels than an XCD holds: 3)
    int lookahead = 1;   // 0: off; 1: panel k+1 on a high-priority side stream under the update of step k (fp64 n >= 7168, fp32 n >= 10240; bit-identical)
    int lookahead_min = 0; // smallest n the look-ahead driver takes (0 = measured default: 7168 fp64, 10240 fp32)
    int panel_rt = 4;     // rows per thread in the pipelined panel (mode 3)
    int panel_nt = 0;     // threads per workgroup in the pipelined panel (0 = choose by panel height)
    int trsv_mode = 2;    // few-RHS solve: 2 = 128-row steps + helper workgroups (default), 1 = one cooperative launch per direction with 64-row steps, 0 = one launch per 128-row step
    int gemm_stagger = 0; // trailing update: start delay of every second resident workgroup, units of 8128 clocks
    int gemm_waves = 0;   // waves per workgroup in the trailing-update kernel (0 = auto; 4: 64x64 per wave, 8: 64x32)
    int getri_pairs = 1;             // inverse: two 128-row blocks per trailing update (K = 256), same bits
    int left_per_step = 1;           // XCD look-ahead driver: a panel's interchanges left of it trail its step (0: all at the end)
    int chain_fused = 1;             // 1: chain head and the next panel's block solve in one launch (option chain_fused)
    int chain_wait_limit = 1 << 21;  // polls of those waits before they give up (option chain_wait_limit: tests inject a time-out with 0)
    int x_events = 0;                // option x_events (measurements, tests): no column-0 ordering in the XCD-scope schedule
    int panel_debug = 0;  // 1: stamped diagnostic panel kernel (tools/kbench.py)
    int getri_plain = 0;     // option getri_structured=0: the inverse as a plain n-right-hand-side solve of P*I
    int rref_first_fast = 1; // 1: large fp64 inputs under LSX_PIVOT_FIRST take the blocked form (option rref_first_fast)
    int rref_blocked = 1;       // 1: large inputs with LSX_PIVOT_MAX take the blocked row reduction (option rref_blocked)
    int getrs_t_blocked_min = 64;   // transposed solve: smallest nrhs that takes the blocked (MFMA) sweeps when n > 128; 0 = never
    int gesvdj_max_sweeps = 30;   // Jacobi SVD: most sweeps of a call (1 .. 60; dgesvj's NSWEEP)
    int syevj_max_sweeps = 60;    // Jacobi eigensolver: most sweeps of a call (1 .. 100)
    int potrs_few_max = 0;   // Cholesky solve: largest nrhs (<= 8) that takes the few-column step kernels; 0 = never
    int lauum_descending = 0;   // lsx_lauum_tn_*: 1 = the k-slabs in descending order, the form lsx_potri_* always runs; 0 = k ascending
    int potri_order = 0;     // SPD inverse, V^T V tiles: 0 = deepest first (ascending tile column), 1 = the symmetric update's order
    int gemm_no_tiles32 = 0;    // option gemm_tiles32=0 (measurements)
    int gemm_queue_test = 0;    // option gemm_queue_test (measurements)
    int xrows_limit = 0;        // option xrows_limit (tests)
    int hybrid_off = 0;         // option hybrid=0 (measurements): no hand-over to the XCD-scope driver above its row limit
    int panel_spin_limit = 1 << 20;   // polls before the XCD-scope panel gives up on a neighbour (option: tests)
    int spin_limit = 1 << 20;   // polls before a cooperative solve gives up (option trsv_spin_limit: tests)
    // ---- read-only counters (lsx_get_option): what the last call of a family did
    int rref_first_used = 0; // 1 if the last LSX_PIVOT_FIRST reduction took the blocked form
    int gecon_solves = 0;    // single-right-hand-side solves of the last condition estimate
    int gerfs_steps = 0;     // most refinement steps any column of the last gerfs took
    int gerfs_solves = 0;    // single-right-hand-side estimator solves of the last gerfs
    int getrs_t_path = 0;    // 1 if the last lsx_getrs_t_* call took the blocked sweeps
    int potrs_path = 0;      // 1 if the last lsx_potrs_* call took the few-column step kernels
    int potri_tiles = 0;     // tiles of the last V^T V product (lsx_potri_*, lsx_lauum_tn_*): t (t + 1) / 2, t = ceil(n / 128)
    int pocon_solves = 0;    // single-right-hand-side solves of the last lsx_pocon_* / lsx_porcond_*
    int porfs_steps = 0;     // most refinement steps any column of the last porfs took
    int porfs_solves = 0;    // single-right-hand-side estimator solves of the last porfs
    int gesvdj_sweeps = 0;   // sweeps of the last lsx_gesvdj_* / lsx_gelss_* call
    int gesvdj_rotations = 0;   // rotations of that call, saturating at INT_MAX
    int syevj_sweeps = 0;    // sweeps of the last lsx_syevj_* call
    int syevj_rotations = 0;    // rotations of that call, saturating at INT_MAX
    int panel_fallbacks = 0;    // host-buffer factorisations redone with panel mode 0 after an exchange time-out
    // ---- buffers.  A DevBuf is sized where it is used (lsx::carve / lsx::reserve) and only grows.  Growing frees the old
    // block, so no function keeps a pointer into a buffer across a call that may grow the SAME buffer.  Who holds what
    // across which calls (a callee is listed with what it grows itself):
    //   host-buffer entry points  staging, across everything below; no driver touches it
    //   getrf_dev                 scratch (in its PanelArgs), tinv (ensure_getrf_workspace), moves_all (look-ahead);
    //                             calls no other driver, and no launcher that carves scratch
    //   getrs_dev, getrs_t_dev    rhs_work, tinv: the same pieces, so the two share what they grow; the many-column
    //                             getrs_dev is done with rhs_work before lu_solve_permuted carves tinv; xchg and scratch
    //                             (ipiv_to_perm, cooperative solve) in the launchers
    //   getri_dev                 rhs_work (permutation) and getri_work, across tinv (its own or lu_solve_permuted's)
    //   potrf_dev, potrs_dev      tinv, rhs_work
    //   potri_dev                 getri_work (V = inv(U^T)), across trtri_upper_t (tinv: block inverses, rhs_work: one
    //                             128-row strip); getri_dev and potri_dev each lay getri_work out from its start
    //   potrs_few_prepare         tinv, rhs_work, in a PotrsFew that pocon_dev / porfs_dev keep across all their
    //                             potrs_few_apply calls: they call nothing else that grows these two
    //   geqrf_dev, ormqr_dev      qr_work, each laid out from its start by carve_qr; neither keeps a piece across the other
    //   orgqr_dev                 nothing of its own: the identity, then ormqr_dev
    //   gels_dev                  tinv (block inverses of R), after geqrf_dev and ormqr_dev are done with qr_work
    //   gesvdj_dev, gelss_dev     svd_work, laid out once per call by carve_svd and held across geqrf_dev / ormqr_dev (qr_work,
    //                             which those two keep to themselves) and the products; gelss_dev's U, V^T, s and Y are
    //                             pieces of the same carve
    //   syevj_dev                 eig_work, laid out once per call by carve_eig; it calls nothing that carves
    //   gecon_dev, pocon_dev      cond, across getrs_dev / getrs_t_dev and potrs_few_*
    //   refine_loop               refine, across getrs_dev / getrs_t_dev (gerfs_dev) and potrs_few_apply (porfs_dev)
    //   gesvx_dev                 equil, across geequ_dev (equil again, never more than gesvx_dev carved), lange_dev
    //                             (scratch), getrf_dev, gecon_dev, getrs_dev / getrs_t_dev and gerfs_dev
    //   gesv_refined_dev          mixed_resid, across getrs_dev
    //   rref_blocked              rhs_work (its column block and block inverses), scratch; calls block solves and updates only
    //   rref_first_fast           rref_first, across rref_blocked, getrf_dev and getrs_dev; tinv and scratch (its PanelArgs) for
    //                             its own first-rule factorisation, begun after rref_blocked and finished before those two
    // scratch belongs to the launchers; no launch relies on what an earlier call left there.  Each user writes its layout
    // once, as Carver::take calls beside the code that uses the pieces, and placement and size both come from it.  Nobody
    // holds a piece across a launcher that carves scratch itself: launch_rref, rref_blocked, launch_rref_trace,
    // launch_ipiv_to_perm, lu_solve_few_rhs, the probes.  A panel launch runs under OnStream and never reserves: it lays out
    // inside the area its PanelArgs hands over (carve_in) and exports the counted size (panel_*_bytes); so do the LU drivers,
    // inside the scratch ensure_getrf_workspace sized as the largest layout that can run.  (*_work_bytes: ONE array by pointer.)
    DevBuf staging;      // staging of caller matrices (host-buffer entry points)
    DevBuf tinv;         // triangular block inverses of every driver and solve
    DevBuf rhs_work;     // permutation + right-hand-side / panel work copies
    DevBuf mixed_resid;  // residual / correction of the mixed-precision solve
    DevBuf getri_work;   // work matrix of the structured inverse
    DevBuf rref_first;   // first-rule row reduction: a copy of the matrix, its pivot columns, interchanges
    DevBuf cond;         // condition estimators (gecon, pocon): iteration vector, sign vector, record, identity interchanges
    DevBuf refine;       // refinement loop (gerfs, porfs): residual and bound of a group, two vectors, records, partial sums
    DevBuf equil;        // equilibration (geequ, gesvx): the drivers' records, then row maxima and partial column maxima
    DevBuf qr_work;      // Householder QR: V, V^T V, T and its transpose, the two W strips, partial-sum slots, pivot rows,
                         // and for panels of more than 4096 rows the pieces of V^T C (qr_vt_times)
    DevBuf svd_work;     // Jacobi SVD: W, Z, the row norms, the permutation, the rotation counter, tau, and gelss's U, V^T, s, Y
    DevBuf eig_work;     // Jacobi eigensolver: W, Z, the row sums of the norm, the diagonal, the permutation, the rotation
                         // counter and the round's pairs, rotations and flags
    DevBuf xchg;         // few-RHS solve (kernels_trsv.hip, third form): exchange granules validated by an epoch, never cleared
    unsigned xchg_epoch = 0;
    DevBuf moves_all;    // look-ahead driver with the XCD-scope panel: one gather list per panel
    DevBuf scratch;      // pivot search partials, exchange areas, flags, index arrays
    // gather lists (int2[256] each) emitted by the cooperative panel kernels: storage only, a launch is told which one
    void *moves_buf[2] = {nullptr, nullptr};  // the drivers' lists (the shared-CU look-ahead driver alternates); [0] owns the block
    void *moves_api = nullptr;       // list of the last lsx_panel_f64_dev call, handed out by lsx_panel_moves_dev
    bool moves_api_valid = false;    // that call emitted one (touched by those two entry points only)
    // device status words (never cleared by kernels): [0] panel exchange time-outs when the caller gave no info
    // word, [1] few-RHS solve time-outs, [2] the internal info word of a factorisation called without one
    int *dev_status = nullptr;
};

namespace lsx {

// launches inside this scope go to stream s: h->stream is the ambient "stream in use", this guard alone swaps it
struct OnStream {
    lsx_handle_t h; hipStream_t keep;
    OnStream(lsx_handle_t h_, hipStream_t s) : h(h_), keep(h_->stream) { h->stream = s; }
    ~OnStream() { h->stream = keep; }
};

// How one trailing-update launch (launch_gemm_*) is scheduled; the default is the plain static grid.
struct GemmPlan {
    int kshift = 0;               // the k index starts at this offset and wraps (pair form of the backward sweep)
    // LU drivers: updates narrower than 16 columns also take the MFMA kernel, so that a column sees the same summation
    // order whichever driver (sequential / look-ahead / multi-device) splits the trailing matrix around it
    bool mfma_only = false;
    int *col0_static = nullptr;   // static grid: finished-tile count of its first tile column (zeroed by the driver)
    // interior tiles through the work queue (look-ahead driver with the XCD-scope panel, kernels_gemm.hip)
    int *counters = nullptr;      // non-null = queue: the eight per-XCD strip counters, zeroed by the driver
    const int *avoid_word = nullptr;   // device word: 1 + XCC id whose workgroups take no tiles (the panel's XCD)
    int *pass_word = nullptr;     // incremented by every workgroup that leaves because it sits on the avoided XCD
    int *col0 = nullptr;          // {ticket, done} words of the update's tile column 0 (zeroed by the driver)
};
// What launch_gemm_* reports about the launch it made.
struct GemmDone {
    bool queued = false;          // the interior went through the queue
    bool col0_complete = false;   // the column-0 count reaching col0_tiles means that column is final
    int col0_tiles = 0;
};

// Where one panel launch writes and which form it takes.  mode / nt / rt start as the handle's options; a driver that
// needs other values (shared-CU schedule, tall panels, host fall-back) changes its own copy.
struct PanelArgs {
    int mode, nt, rt;             // effective panel mode, threads per workgroup, rows per thread
    void *list;                   // int2[256]: where a cooperative kernel writes this panel's gather list
    // Where the launch lays out its exchange area or pivot candidates: to begin with all of scratch as it stands (so a
    // PanelArgs is made AFTER scratch was sized) and the launch clears what it uses; a look-ahead driver hands over one
    // of its rotating areas and keeps it cleared itself, off the panel-to-panel chain (cleared = true).
    void *area; size_t area_bytes; bool cleared = false;
    int *xcc_word = nullptr;      // where the XCD-scope kernel records 1 + its XCC id
    bool listed = false;          // out: a cooperative kernel ran, `list` describes this panel's interchanges
    PanelArgs(lsx_handle_t h, void *list_) : mode(h->panel_mode), nt(h->panel_nt), rt(h->panel_rt), list(list_), area(h->scratch.p), area_bytes(h->scratch.bytes) {}
};

// b holds at least `need` bytes afterwards: no HIP call when it already does (a warmed-up call stays graph-capturable),
// else the stream is synchronised, the old block freed and a new one of 1 MiB steps allocated (*fresh, if given, is set).
int reserve(lsx_handle_t h, DevBuf &b, size_t need, bool *fresh = nullptr);
// Bump carving of a device block, every piece on a 256-byte boundary.  With a null base it only counts: take returns
// null and off ends as the bytes the same calls need.
struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(void *b) : base((char *)b) {}
    template <typename U> U *take(size_t count) {
        off = (off + 255) & ~(size_t)255;
        U *p = base ? (U *)(base + off) : nullptr;
        off += count * sizeof(U);
        return p;
    }
};
// Size b from its own layout and lay it out: `layout` (take calls only, pointers derived from a taken one are formed
// after carve returns) runs once to count and once on the block.
template <class F> size_t carve_bytes(F &&layout) {
    Carver count(nullptr);
    layout(count);
    return count.off;
}
template <class F> int carve(lsx_handle_t h, DevBuf &b, F &&layout, bool *fresh = nullptr) {
    LSX_TRY(reserve(h, b, carve_bytes(layout), fresh));
    Carver c(b.p);
    layout(c);
    return LSX_OK;
}
// A layout placed inside an area sized earlier: no reserve (usable under OnStream); too small is an error, never another schedule.
template <class F> int carve_in(void *area, size_t bytes, const char *who, F &&layout) {
    Carver c(area);
    layout(c);
    if (area && c.off <= bytes) return LSX_OK;
    set_error("%s: needs %zu bytes of scratch, was handed %zu", who, c.off, bytes);
    return LSX_ERR_INTERNAL;
}
// Largest bytes(height) over panel heights <= m (a taller panel may take fewer, larger row slices; slice heights and the
// thresholds between forms are multiples of 64, so m and the multiples of 64 below it cover every case).  every: 0 if some height gives 0.
template <class F> size_t max_over_heights(int m, bool every, F &&bytes) {
    size_t need = 0;
    for (int mm = m; mm > 0; mm = (mm - 1) / 64 * 64) {
        const size_t b = bytes(mm);
        if (every && !b) return 0;
        if (b > need) need = b;
    }
    return need;
}
int ensure_getrf_workspace(lsx_handle_t h, int n, size_t elem);
// XCD-scope panel under the reference's first-non-zero pivot rule (kernels_panel_x.hip); 1 = shape not served
int panel_xcd_first(lsx_handle_t h, int m, int jb, double *P, int ldp, int row0, int col0, int32_t *d_ipiv, int *d_info, double tol,
                    PanelArgs &pa);
template <typename T>
int launch_gather_pivot_cols(lsx_handle_t h, int m, int r, int row_lo, const T *src, int lds, const int32_t *d_pivots, T *dst, int ldd);
template <typename T>
int launch_rref_finish(lsx_handle_t h, int m, int bar, T *W, int ldw, const int32_t *d_pivots, int rank);
template <typename T>
int rref_blocked(lsx_handle_t h, int m, int n, int bar, T *W, int ldw, int32_t *d_pivots, int *d_rank, double tol, int pivot_rule);   // scratch + block-inverse workspace of one LU (api.hip)

// Profiling bracket of a launch group: the constructor records the start event, the destructor the end event.
struct ProfScope {
    lsx_handle_t h;
    hipStream_t st;
    int idx = -1;
    ProfScope(lsx_handle_t h_, int bucket, double flops = 0, double bytes = 0);
    ~ProfScope();
};

template <typename T>
struct Real;
template <>
struct Real<double> {
    static constexpr double eps = 2.220446049250313e-16;
};
template <>
struct Real<float> {
    static constexpr float eps = 1.1920929e-07f;
};

// 1/x for the pivot scaling of every panel kernel, through pivot_recip below (the same function everywhere so the three
// panel modes stay bit-identical): hardware reciprocal + Newton, <= 1 ulp; an IEEE division
// costs ~40 instructions on the per-column critical path.
template <typename T>
__device__ __forceinline__ T fast_recip(T x) {
    if (sizeof(T) == 8) {
        double r = __builtin_amdgcn_rcp((double)x);
        r = r * (2.0 - (double)x * r);
        r = r * (2.0 - (double)x * r);
        return (T)r;
    }
    float r = __builtin_amdgcn_rcpf((float)x);
    r = r * (2.0f - (float)x * r);
    return (T)r;
}

// a / p for the pivot scaling, as (a * c) * rinv with rinv = fast_recip(p * c): c = 1 for a normal pivot (a * 1 is
// exact: the same bits as a * fast_recip(p)), c = 2^64 (fp32: 2^32) for a subnormal one, whose reciprocal is not a
// finite number -- LAPACK's getf2 divides below sfmin for the same reason.  p * c is then normal and a * c exact
// (|a| <= |p|).  One value per column, uniform over the wave; every kernel that scales by a pivot takes it from here.
template <typename T>
struct PivotRecip {
    T c, rinv;
    __device__ __forceinline__ T apply(T a) const { return (a * c) * rinv; }
};
template <typename T>
__device__ __forceinline__ PivotRecip<T> pivot_recip(T p) {
    const T safmin = sizeof(T) == 8 ? (T)0x1p-1022 : (T)0x1p-126f;
    const T c = (p < T(0) ? -p : p) < safmin ? (sizeof(T) == 8 ? (T)0x1p64 : (T)0x1p32f) : T(1);
    return PivotRecip<T>{c, fast_recip<T>(p * c)};
}


// ---- kernel launchers (one per .hip file section); all asynchronous on h->stream ----
template <typename T>
int launch_fill(lsx_handle_t h, int kind, uint64_t seed, int m, int n, T *A, int lda, int row_off,
                int col_off);
template <typename T>
int launch_gemm_sub(lsx_handle_t h, int m, int n, int k, const T *A, int lda, const T *B, int ldb,
                    T *C, int ldc, const GemmPlan &plan = GemmPlan(), GemmDone *done = nullptr);
// C += A*B (plus = 1) or C -= A*B (plus = 0), same MFMA kernel
template <typename T>
int launch_gemm_acc(lsx_handle_t h, int plus, int m, int n, int k, const T *A, int lda, const T *B, int ldb,
                    T *C, int ldc, const GemmPlan &plan = GemmPlan(), GemmDone *done = nullptr);
// TN form on the same tile, A stored k x m: C -= A^T*B (mode 0), C += A^T*B (1), C = A^T*B (3); bucket: where the
// launch is accounted (the Cholesky strip product counts as a block solve)
template <typename T>
int launch_gemm_tn_acc(lsx_handle_t h, int mode, int m, int n, int k, const T *A, int lda, const T *B, int ldb, T *C,
                       int ldc, int bucket = LSX_PROF_GEMM);
// upper triangle of C (n x n) -= A^T*A, A stored k x n; the strictly lower triangle of C is neither read nor written
template <typename T>
int launch_syrk_tn_sub(lsx_handle_t h, int n, int k, const T *A, int lda, T *C, int ldc);
template <typename T>
int launch_gemm_tn_sub(lsx_handle_t h, int m, int n, int k, const T *A, int lda, const T *B, int ldb, T *C, int ldc);
// upper triangle of C (n x n) = V^T*V for a lower-triangular V (n x n): tile (I, J) runs over k >= 128 J only, so the
// blocks of V strictly above its diagonal 128-blocks are never read; nothing below the diagonal of C is read or written.
// order 0: tiles handed out deepest first, 1: the order of the symmetric update.  descending: every tile takes its
// k-slabs of 16 from the last one down (k ascending inside a slab) instead of k ascending throughout.  Sets h->potri_tiles.
template <typename T>
int launch_lauum_tn(lsx_handle_t h, int n, const T *V, int ldv, T *C, int ldc, int order, bool descending);
// traced reference-order row reduction (kernels_trace.hip), carves scratch; d_out = {pivots, steps, overflow}
int launch_rref_trace(lsx_handle_t h, int m, int n, int bar, double *R, int ldr, unsigned char *Tm,
                      int32_t *d_pivots, int32_t *d_steps, int max_steps, double *d_snaps,
                      unsigned char *d_snap_t, int max_snaps, int *d_out);
template <typename T>
int launch_panel(lsx_handle_t h, int m, int jb, T *P, int ldp, int row0, int32_t *d_ipiv,
                 int *d_info, PanelArgs &pa);
// Counts of the launchers' own layouts for panels of up to m rows.  panel_scratch_bytes: a self-clearing launch_panel,
// whichever form takes a height.  The other two: one exchange area of the pipelined / XCD-scope kernel; for_driver: one a
// look-ahead driver keeps cleared, 0 = these settings do not serve every height (else: the largest among those served).
size_t panel_scratch_bytes(lsx_handle_t h, int mode, int nt, int rt, int m, size_t elem);
size_t panel_pipe_area_bytes(lsx_handle_t h, int mode, int nt, int rt, int m, bool for_driver = true);
size_t panel_x_area_bytes(lsx_handle_t h, int mode, int m, size_t elem, bool for_driver = true);
template <typename T>
int launch_laswp(lsx_handle_t h, int ncols, T *A, int lda, int row0, int jb, const int32_t *d_ipiv);
// same interchanges from a gather list (written by the cooperative panel kernel)
template <typename T>
int launch_laswp_moves(lsx_handle_t h, const int2 *moves, int ncols, T *A, int lda, int row0);
template <typename T>
int launch_laswp_left_all(lsx_handle_t h, T *A, int lda, int k0, int nb, int nsteps, const void *lists);
int launch_gate(lsx_handle_t h, const int *word, int target);
// info: the factorisation's info word (a time-out makes it negative), or null
int launch_wait_count(lsx_handle_t h, const int *word, int target, int *info);
int launch_resid_mixed(lsx_handle_t h, int n, int nrhs, const float *A, int lda, const float *B, int ldb, const double *X,
                       int ldx, float *R, int ldr);
int launch_refine_apply(lsx_handle_t h, int n, int nrhs, int init, const float *D, int ldd, double *X, int ldx, float *Xf,
                        int ldf, double *d_out2);
template <typename T>
int diag_chain_head(lsx_handle_t h, int jb, const T *Tm, int ldt, T *Tinv, int ncols, T *A, int lda, int row0,
                    const void *moves);
template <typename T>
int launch_laswp_moves_around(lsx_handle_t h, const int2 *moves, int n, T *A, int lda, int row0, int hole_at, int hole_w);
// Tinv (ceil(jb/64) blocks of 64x64) <- inverses of the 64x64 diagonal blocks of the
// unit-lower (lower=1) or non-unit upper (lower=0) triangle stored at T.
template <typename T>
int launch_trtri(lsx_handle_t h, int lower, int jb, const T *Tm, int ldt, T *Tinv);
// trtri(unit lower) + gather-list interchanges on a column block in one launch; 1 = not applicable (no list: moves
// null, or shapes).  info: the factorisation's info word for the in-kernel wait (time-out -> negative), or null
template <typename T>
int launch_chain_head(lsx_handle_t h, const int2 *moves, int *info, int jb, const T *Tm, int ldt, T *Tinv, int ncols, T *A,
                      int lda, int row0, const int *wait_word = nullptr, int wait_target = 0);
// chain head + block solve of the next panel's 128 columns in one launch (kernels_misc.hip); 1 = shapes not served
template <typename T>
int launch_chain_fused(lsx_handle_t h, const int2 *moves, int *info, int jb, const T *Tm, int ldt, T *Tinv, int ncols, T *A,
                       int lda, int row0, const int *wait_word, int wait_target, int *ready);
template <typename T>
int launch_trtri_both(lsx_handle_t h, int n, const T *LU, int lda, T *invL, T *invU);
// B (jb x ncols) <- inv(Tm) * B in place; Tinv = inverses of Tm's 64x64 diagonal blocks.
template <typename T>
int launch_trsm_block(lsx_handle_t h, int lower, int jb, int ncols, const T *Tm, int ldt,
                      const T *Tinv, T *B, int ldb);
// carves scratch (two index arrays of n)
int launch_ipiv_to_perm(lsx_handle_t h, int n, const int32_t *d_ipiv, int32_t *d_perm);
template <typename T>
int launch_gather_rows(lsx_handle_t h, int n, int ncols, const int32_t *d_perm, const T *S, int lds,
                       T *D, int ldd);
template <typename T>
int launch_set_identity_perm(lsx_handle_t h, int n, const int32_t *d_perm, T *X, int ldx);
template <typename T>
int launch_scatter_cols(lsx_handle_t h, int n, const int32_t *d_perm, const T *S, int lds, T *D, int ldd);
// d_ipiv == nullptr: no interchanges (a Cholesky factor); square: the (sign, mant, exp2) triple of the product squared
template <typename T>
int launch_det(lsx_handle_t h, int n, const T *LU, int lda, const int32_t *d_ipiv, double *d_out, bool square = false);
// carves scratch: state and two rows (per-column form) or row-group candidates (blocked, which also carves rhs_work)
template <typename T>
int launch_rref(lsx_handle_t h, int m, int n, int bar, T *R, int ldr, int32_t *d_pivots,
                int *d_rank, double tol, int pivot_rule);
// d_out[0] = max|A_ij| ; d_out[1] = min_k |LU_kk|
template <typename T>
int launch_amax(lsx_handle_t h, int m, int n, const T *A, int lda, double *d_out);
template <typename T>
int launch_diag_minabs(lsx_handle_t h, int n, const T *LU, int lda, double *d_out);
// X (n x nrhs, ld = nrhs) <- U^-1 L^-1 B, nrhs <= 8, one launch per 128-row block step
template <typename T>
int lu_solve_few_rhs2(lsx_handle_t h, int n, int nrhs, int nr, const T *LU, int lda, const int32_t *d_ipiv, T *B, int ldb,
                      T *inv64L, T *inv64U, T *inv128L, T *inv128U, T *Bp, T *Y);
template <typename T>
int lu_solve_few_rhs(lsx_handle_t h, int n, int nrhs, const T *LU, int lda, T *B, int ldb, T *X, T *inv64L,
                     T *inv64U, T *inv128L, T *inv128U);
// block inverses of both triangles, 128 x 128, natural orientation (kernels_trsv.hip), and the transposed solve,
// the norms and the estimator's vector steps built on them (kernels_trsvt.hip)
template <typename T>
int launch_inv128_natural(lsx_handle_t h, int n, const T *LU, int lda, T *inv64L, T *inv64U, T *inv128L, T *inv128U);
template <typename T>
int lu_solve_transposed(lsx_handle_t h, int n, int nrhs, const T *LU, int lda, const int32_t *d_ipiv, const int32_t *perm,
                        T *B, int ldb, T *inv64L, T *inv64U, T *inv128L, T *inv128U, T *W);
// X[perm[i], 0..ncols) = W[i, 0..ncols): the row scatter that ends a transposed solve, whole rows at once
template <typename T>
int launch_scatter_rows(lsx_handle_t h, int n, int ncols, const int32_t *d_perm, const T *W, int ldw, T *X, int ldx);
size_t lange_work_bytes(int norm, int m, int n);
template <typename T>
int launch_lange(lsx_handle_t h, int norm, int m, int n, const T *A, int lda, double *d_work, double *d_out);
template <typename T>
int launch_est_fill(lsx_handle_t h, int n, int mode, T *x, int32_t *ident);
template <typename T>
int launch_est_asum_sign(lsx_handle_t h, int n, T *x, signed char *isgn, double *rec);
template <typename T>
int launch_est_amax_unit(lsx_handle_t h, int n, T *x, int jlast, double *rec);
// refined solves (kernels_refine.hip): residual + componentwise bound of up to 8 right-hand sides in one pass over A
// (trans: of A^T, two passes over partial sums in d_work), backward error / max |x| per column, and the vector steps
size_t resid_bound_work_bytes(int trans, int n);
template <typename T>
int launch_resid_bound(lsx_handle_t h, int trans, int n, int ncols, const T *A, int lda, const T *B, int ldb, const T *X,
                       int ldx, T *R, T *W, int ldr, double *d_work);
template <typename T>
int launch_berr(lsx_handle_t h, int n, int ncols, const T *R, const T *W, int ldr, const T *X, int ldx, double safe1,
                double safe2, double *rec);
template <typename T>
int launch_refine_take(lsx_handle_t h, int n, const T *Rj, int ldr, T *d);
template <typename T>
int launch_refine_add(lsx_handle_t h, int n, const T *d, T *Xj, int ldx);
template <typename T>
int launch_ferr_weight(lsx_handle_t h, int n, const T *Rj, const T *Wj, int ldr, double nu, double safe1, double safe2,
                       T *out);
template <typename T>
int launch_vec_mul(lsx_handle_t h, int n, const T *wt, T *v);
// equilibration (kernels_equil.hip): geequ's scale factors and stats = {rowcnd, colcnd, amax, info}, laqge's scaling
// (r or c null: that side unscaled; D2: a second copy of the result, or null), max |a_ij| over the first k columns
// (upper: on and above the diagonal only)
size_t geequ_work_bytes(int m, int n, size_t elem);
template <typename T>
int launch_geequ(lsx_handle_t h, int m, int n, const T *A, int lda, T *r, T *c, double *stats, void *d_work,
                 int passes = 3);
template <typename T>
int launch_laqge(lsx_handle_t h, int m, int n, T *A, int lda, const T *r, const T *c, T *D2, int ld2);
size_t maxabs_work_bytes(int m);
template <typename T>
int launch_maxabs(lsx_handle_t h, int m, int k, const T *A, int lda, int upper, double *d_work, double *d_out);
int diag_mfma_peak(lsx_handle_t h, int is_f32, int iters, int blocks_per_cu, double *tflops, double *clock_mhz);
int diag_cu_mask_probe(lsx_handle_t h, const uint32_t *mask_words, int nwords, int nblocks, unsigned *out_host);
int getrf_mg_f64(lsx_handle_t *hs, int P, int n, double *const *dA, const int *lda, int32_t *const *d_ipiv,
                 int *const *d_info);
int diag_occupy(lsx_handle_t h, int xcc, int wgs, int ms);
int diag_xchg_probe(lsx_handle_t h, int mode, int G, int stride, int wt, int epochs, double *us_per_epoch,
                    int *xcc_ids, int *nfail);
template <typename T>
int launch_copy2d(lsx_handle_t h, int m, int n, const T *S, int lds, T *D, int ldd);
// Cholesky (kernels_chol.hip).  launch_chol_diag: the jb x jb (jb <= 128) upper diagonal block at A is factored in
// place, A = U^T U, and inv(U) goes to Vinv (128 x 128, natural orientation, identity outside the block); col0 = the
// block's first column in the whole matrix, *info (never null) = 0 on entry or the launch does nothing but write the
// identity to Vinv; a pivot <= 0 or NaN at local row j sets *info = col0 + j + 1.
// launch_chol_inv: for every 128-row diagonal block of the upper factor U, inv128[blk] (natural orientation, identity
// outside the matrix) and its two 64 x 64 diagonal blocks in the layout of launch_trtri (inv64[kb / 64]).
template <typename T>
int launch_chol_diag(lsx_handle_t h, int jb, T *A, int lda, int col0, T *Vinv, int *info);
template <typename T>
int launch_chol_inv(lsx_handle_t h, int n, const T *U, int lda, T *inv64, T *inv128);
// Pieces of the SPD inverse (api.hip, potri_dev).  launch_lower_identity: X[i][j] = (i == j) for j < 128 (i / 128 + 1),
// the identity on and below the diagonal 128-blocks; the blocks above them are not written.  launch_diag_zero_info:
// *info = 0, or i + 1 for the first u_ii that is exactly zero or NaN.  launch_symmetrize_upper: a_ji = a_ij for j > i.
template <typename T>
int launch_lower_identity(lsx_handle_t h, int n, T *X, int ldx);
template <typename T>
int launch_diag_zero_info(lsx_handle_t h, int n, const T *U, int lda, int *info);
template <typename T>
int launch_symmetrize_upper(lsx_handle_t h, int n, T *A, int lda);
// Condition estimate and error bounds of the Cholesky family (kernels_posx.hip); nothing below a diagonal is loaded.
// launch_resid_bound_sym: launch_resid_bound for a symmetric A given by its upper triangle; launch_lansy: its 1-norm
// (launch_lange's contract); d_work: resid_bound_sym_work_bytes(n, ncols) bytes, ncols = 1 for the norm.
// Few right-hand sides, X <- inv(U) inv(U^T) B through W (n x nr, dense, nr in {1, 2, 4, 8} >= w): the forward half
// packs columns [c0, c0 + w) of B and solves with U^T (kernels_trsvt.hip), the backward half solves with U and
// unpacks; inv128: launch_chol_inv's.
size_t resid_bound_sym_work_bytes(int n, int ncols);
template <typename T>
int launch_resid_bound_sym(lsx_handle_t h, int n, int ncols, const T *A, int lda, const T *B, int ldb, const T *X, int ldx,
                           T *R, T *W, int ldr, double *d_work);
template <typename T>
int launch_lansy(lsx_handle_t h, int n, const T *A, int lda, double *d_work, double *d_out);
template <typename T>
int launch_trsvt_forward_upper(lsx_handle_t h, int n, int nr, int w, const T *U, int lda, const T *inv128U, const T *B,
                               int ldb, int c0, T *W);
template <typename T>
int launch_posx_backward(lsx_handle_t h, int n, int nr, int w, const T *U, int lda, const T *inv128, T *W, T *B, int ldb,
                         int c0);
// Householder QR (kernels_qr.hip).  launch_qr_panel: the jb <= 128 reflectors of a panel of mp >= jb rows, jb + 1 plain
// launches over row slabs; slots = qr_slot_elems() doubles (two sets of per-slab partial sums in turn), prow = 2 x 128
// elements (the copied pivot row, two in turn); tau receives jb entries.  launch_qr_extract_v: V (mp x 128, dense) =
// the panel's unit lower trapezoid, zero columns beyond jb.  launch_qr_larft: T (and its transpose, both 128 x 128,
// zero outside the triangle) from G = V^T V and tau.  launch_colnrm2: lsx_colnrm2_*_dev.
size_t qr_slot_elems();
template <typename T>
int launch_qr_panel(lsx_handle_t h, int mp, int jb, T *P, int ldp, T *tau, double *slots, T *prow);
template <typename T>
int launch_qr_extract_v(lsx_handle_t h, int mp, int jb, const T *P, int ldp, T *V);
template <typename T>
int launch_qr_larft(lsx_handle_t h, int jb, const T *G, const T *tau, T *Tm, T *Tt);
template <typename T>
int launch_qr_identity(lsx_handle_t h, int m, int n, T *Q, int ldq);
// out (rows x nc) = the sum of `parts` partial products, `stride` elements apart, in order, fp64, one rounding
template <typename T>
int launch_qr_sum_parts(lsx_handle_t h, int rows, int nc, int parts, const T *P, int ldp, size_t stride, T *out, int ldo);
template <typename T>
int launch_colnrm2(lsx_handle_t h, int m, int n, const T *A, int lda, double *out);
// One-sided Jacobi SVD (kernels_svd.hip).  The work arrays W (p x q) and Z (p x p) are 16-byte aligned with a leading
// dimension of svd_ld(cols) elements and zeros in the columns beyond the matrix; svd_keep_cols: the longest row the round
// kernel keeps in registers.  launch_svd_round: round r of a sweep, one workgroup per pair, *count += rotations (Z may be
// null).  launch_svd_init: D = S with the padding zeroed (upper: zeros below the diagonal too; S null: the identity).
// launch_svd_rownorm: sigma_i = ||w_i||_2.  launch_svd_gather: s, V^T (or null) and U (or null; urows >= k rows, zeros
// below row k) in the order perm.  launch_svd_scale_rows: row i of Y times 1 / s_i for i < rank, zeros below.
int svd_ld(int cols, size_t elem);
int svd_keep_cols(size_t elem);
template <typename T>
int launch_svd_round(lsx_handle_t h, int p, int q, int r, T *W, int ldw, T *Z, int ldz, double tol, int *count);
template <typename T>
int launch_svd_init(lsx_handle_t h, int rows, int cols, const T *S, int lds, int upper, T *D, int ldd);
template <typename T>
int launch_svd_rownorm(lsx_handle_t h, int p, int q, const T *W, int ldw, double *sigma);
template <typename T>
int launch_svd_gather(lsx_handle_t h, int k, int q, int urows, const T *W, int ldw, const T *Z, int ldz, const double *sigma,
                      const int *perm, double *s, T *Vt, int ldvt, T *U, int ldu);
template <typename T>
int launch_svd_scale_rows(lsx_handle_t h, int k, int nc, int rank, const double *s, T *Y, int ldy);
template <typename T>
int launch_svd_fill(lsx_handle_t h, int rows, int cols, T value, T *D, int ldd);
// Two-sided Jacobi for the symmetric eigenproblem (kernels_eig.hip).  W (n x n, both triangles) and Z (n x n) are laid out
// like the SVD's work arrays (svd_ld).  EigRound: what the decision launch of a round leaves for its rotation launch, one
// entry per position t < P / 2.  launch_eig_init: W from the upper triangle of A, mirrored, the padding zeroed.
// launch_eig_norm: *nrm = ||A||_F from the upper triangle of W (rowsq: n doubles of work).  launch_eig_decide: round r,
// *count += rotations.  launch_eig_round: W <- G W G^T in place, rows of Z (or null) alike.  launch_eig_diag: d_i = w_ii.
struct EigRound {
    int2 *pair = nullptr;      // (i, j), i < j; j >= n: the phantom player of an odd n
    double2 *rot = nullptr;    // (cs, sn), valid where flag is set
    int *flag = nullptr;       // 1: the pair is rotated in this round
};
template <typename T>
int launch_eig_init(lsx_handle_t h, int n, const T *A, int lda, T *W, int ldw);
template <typename T>
int launch_eig_norm(lsx_handle_t h, int n, const T *W, int ldw, double *rowsq, double *nrm);
template <typename T>
int launch_eig_decide(lsx_handle_t h, int n, int r, const T *W, int ldw, double thr, EigRound er, int *count);
template <typename T>
int launch_eig_round(lsx_handle_t h, int n, T *W, int ldw, T *Z, int ldz, EigRound er);
template <typename T>
int launch_eig_diag(lsx_handle_t h, int n, const T *W, int ldw, double *d);

}  // namespace lsx
