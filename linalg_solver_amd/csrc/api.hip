// C-ABI of liblsx.so (see include/lsx.h) and the host-side drivers of the
// blocked algorithms.  All device work is enqueued on the handle's stream with
// no host synchronisation inside a factorisation or solve: pivots, info and
// rank stay on the device, so a whole getrf is graph-capturable.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"

namespace lsx {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int reserve(lsx_handle_t h, DevBuf &b, size_t need, bool *fresh) {
    if (need <= b.bytes) return LSX_OK;
    if (b.p) {
        LSX_HIP(hipStreamSynchronize(h->stream));   // the old block goes: nothing queued may still use it
        LSX_HIP(hipFree(b.p));
        b = DevBuf();
    }
    need = (need + (1u << 20) - 1) & ~((size_t)(1u << 20) - 1);
    hipError_t e = hipMalloc(&b.p, need);
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu) failed: %s", need, hipGetErrorString(e));
        b.p = nullptr;
        return LSX_ERR_ALLOC;
    }
    b.bytes = need;
    if (fresh) *fresh = true;
    return LSX_OK;
}

// Every entry point runs with the handle's device current and puts the caller's back on the way out: with two
// handles in one process, or torch's current device elsewhere, workspaces and launches would land on the wrong GPU.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(lsx_handle_t h) {
        if (!h) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != h->device) switched = hipSetDevice(h->device) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};
#define LSX_DEVICE_GUARD(h) lsx::DeviceGuard device_guard_(h)

// The cooperative kernels (panel exchange, few-RHS solve) give up after a bounded spin and say so in a device word;
// a host-buffer entry point must not hand back what was computed after that.  Synchronises the handle's stream.
static int check_dev_status(lsx_handle_t h) {
    int st[3] = {0, 0, 0};
    LSX_HIP(hipStreamSynchronize(h->stream));
    LSX_HIP(hipMemcpy(st, h->dev_status, sizeof(st), hipMemcpyDeviceToHost));
    if (st[0] == 0 && st[1] == 0 && st[2] >= 0) return LSX_OK;
    LSX_HIP(hipMemset(h->dev_status, 0, sizeof(st)));
    set_error("%s timed out on the device (its workgroups were not all resident: another kernel holding the CUs?)",
              st[1] ? "the cooperative triangular solve" : "the panel exchange");
    return LSX_ERR_INTERNAL;
}

ProfScope::ProfScope(lsx_handle_t h_, int bucket, double flops, double bytes) : h(h_), st(h_->stream) {
    Prof &p = h->prof;
    if (!((p.mask >> bucket) & 1u)) return;
    if (p.sample > 1 && (p.seen[bucket]++ % p.sample) != 0) return;
    ProfEvent ev;
    ev.bucket = bucket;
    for (hipEvent_t *e : {&ev.a, &ev.b}) {
        if (!p.pool.empty()) {
            *e = p.pool.back();
            p.pool.pop_back();
        } else if (hipEventCreate(e) != hipSuccess) {
            return;
        }
    }
    (void)hipEventRecord(ev.a, st);
    p.pending.push_back(ev);
    idx = (int)p.pending.size() - 1;
    p.launches[bucket] += 1;
    p.flops[bucket] += flops;
    p.bytes[bucket] += bytes;
}

ProfScope::~ProfScope() {
    if (idx >= 0) (void)hipEventRecord(h->prof.pending[idx].b, st);
}

static size_t pad256(size_t x) { return (x + 255) & ~(size_t)255; }

// row interchanges of the panel that was just factored, applied to `ncols` columns at Acols: from its gather list,
// or (moves null: the panel emitted none) from its pivots
template <typename T>
static int apply_panel_swaps(lsx_handle_t h, const int2 *moves, int ncols, T *Acols, int lda, int row0, int jb,
                             const int32_t *d_ipiv) {
    if (moves) return launch_laswp_moves<T>(h, moves, ncols, Acols, lda, row0);
    return launch_laswp<T>(h, ncols, Acols, lda, row0, jb, d_ipiv);
}

// ---------------------------------------------------------------- look-ahead LU driver
// Right-looking LU with look-ahead depth 1.  The update of step k is split: the columns of
// the NEXT panel are updated first, then that panel is factored, all on the high-priority side
// stream, while the main stream updates the rest of the trailing matrix.  The panel chain
// (latency-bound: one cross-CU exchange per column) thus runs underneath the MFMA work.
//   side:  panel(k) | trtri(k) | record P(k) | wait N(k-1) | laswp, trsm, gemm on the next panel's columns | panel(k+1)
//   main:                         wait P(k)  | laswp, trsm, gemm on the other columns | left-hand laswp | record N(k)
// (P(k) is recorded behind the next panel's column block when both streams share the CUs.)
// Disjointness: the side stream's step k touches columns [k+jb, k+2jb); the main stream's step k writes
// columns >= k+2jb and < k and reads L21 (columns [k,k+jb)), U12 (rows [k,k+jb)) and the block inverses.
// (A third variant confined the two streams to disjoint CU sets with hipExtStreamCreateWithCUMask.  A CU mask thins
// out the CUs of EVERY XCD alike and cannot keep a kernel off an XCD, so it never separated the kernels and was
// level with this one at best: removed in round 3, history in DESIGN 6.2.)
// On an error return inside a two-stream driver, work already queued on the side stream must not outlive the
// call: the caller's stream waits for it (the next call on the handle, or the caller reading A, would race otherwise).
struct JoinSide {
    lsx_handle_t h; hipStream_t side, main_s, caller; bool armed = true;
    ~JoinSide() {
        if (!armed) return;
        if (hipEventRecord(h->ev_done, side) == hipSuccess) (void)hipStreamWaitEvent(main_s, h->ev_done, 0);
        if (caller != main_s && hipEventRecord(h->ev_start, main_s) == hipSuccess) (void)hipStreamWaitEvent(caller, h->ev_start, 0);
    }
};

// The panel settings of the shared-CU schedule for panels of up to m rows; hybrid: as the phase in front of
// getrf_lookahead_x.  One function for the driver and for ensure_getrf_workspace, which sizes the driver's areas.
static PanelArgs shared_cu_panel(PanelArgs pa, size_t elem, bool hybrid, int m) {
    // this schedule shares the CUs between the panel and the update: the XCD-scope panel (which fills an XCD) has
    // its own driver, getrf_lookahead_x; here it would stall every launch beside it
    if (pa.mode == 4) pa.mode = 3;
    // Panels taller than one XCD holds (the phase in front of getrf_lookahead_x): 256-row slices, i.e. half as many
    // workgroups of the device-scope panel.  Its time per column does not depend on the slicing (2.5-2.6 us, kbench
    // panel3tall), but every CU it holds is one the update -- the bottleneck of this phase -- does not have:
    // 16384^2 fp64 77.8 -> 74.6 ms, 12288^2 38.5 -> 37.9 ms, same bits (tools/lu_tall.py).
    if (elem == 8 && hybrid && pa.nt == 0 && m > 8192) { pa.nt = 512; pa.rt = 8; }
    return pa;
}
// Scratch of the shared-CU driver (pa: shared_cu_panel's).  Two exchange areas of the pipelined panel, used alternately
// and cleared by the DRIVER on the main stream as soon as their panel has finished -- a clear in front of every panel
// launch sits on the chain (area = 0: no such area, every launch clears its own); then the counted first tile columns' words.
struct SharedCuScratch {
    size_t area = 0; char *areas = nullptr; int *c0words = nullptr;
    void lay(Carver &c, lsx_handle_t h, const PanelArgs &pa, int m, int nwords) {
        area = panel_pipe_area_bytes(h, pa.mode, pa.nt, pa.rt, m);
        if (!area) return;
        areas = c.take<char>(2 * area);
        if (nwords) c0words = c.take<int>(nwords);
    }
};

// k0 = first column handled here (columns < k0 were factored by the sequential driver).  k_stop > 0: stop in
// front of the panel that starts at column k_stop (trailing matrix fully updated, that panel not yet factored):
// the XCD-scope driver takes over from there.
template <typename T>
static int getrf_lookahead(lsx_handle_t h, int n, T *A, int lda, int32_t *d_ipiv, int *d_info, T *Tinv, PanelArgs pa,
                           int k0, int k_stop = 0) {
    const int nb = h->nb;
    hipStream_t main_s = h->stream, side = h->side_stream;   // the handle's stream is the update stream
    JoinSide join{h, side, main_s, main_s};
    GemmPlan mfma;   // every update of an LU: see GemmPlan
    mfma.mfma_only = true;
    pa = shared_cu_panel(pa, sizeof(T), k_stop > 0, n - k0);
    // Counted first tile column of the big update (fp64, this driver as the phase in front of getrf_lookahead_x): the
    // chain of step k then waits, inside its first kernel, for update k-1 on the NEXT panel's columns only and runs
    // beside the rest of that update -- the update of step k follows update k-1 without the chain in between
    // (16384^2: the chain was ~45 us of every one of the 64 steps of this phase).
    const int nst = (n - k0 + nb - 1) / nb;
    SharedCuScratch ws;   // inside the scratch that came with pa
    const int nwords = sizeof(T) == 8 && k_stop > 0 && !h->x_events ? nst : 0;
    LSX_TRY(carve_in(pa.area, pa.area_bytes, "getrf_lookahead", [&](Carver &c) { ws.lay(c, h, pa, n - k0, nwords); }));
    const size_t area = ws.area; int *const c0words = ws.c0words;
    if (area) LSX_HIP(hipMemsetAsync(ws.areas, 0, 2 * area, main_s));
    if (c0words) LSX_HIP(hipMemsetAsync(c0words, 0, (size_t)nst * sizeof(int), main_s));
    bool prev_counted = false;
    int prev_tiles = 0;
    pa.cleared = area > 0;
    // the side stream starts after everything already queued on the main stream (info memset, fills)
    LSX_HIP(hipEventRecord(h->ev_start, main_s));
    LSX_HIP(hipStreamWaitEvent(side, h->ev_start, 0));
    // The gather list of panel p lives in moves_buf[p & 1]: panel p+1 (side stream) writes the other
    // buffer while the update stream still applies panel p's interchanges to the left-hand columns,
    // which nothing later depends on and which therefore run AFTER the big update, in its slack.
    // (A panel that took the per-column form emits no list: null here, and its interchanges come from the pivots.)
    auto list = [&](int p, bool has) { return has ? (const int2 *)h->moves_buf[p & 1] : nullptr; };
    // The whole chain panel k -> panel k+1 stays on the side stream (no cross-stream hop on the critical
    // path): inverse of panel k's diagonal blocks, then interchanges / U12 / update of the next panel's own
    // column block, then panel k+1.  The main stream follows one event behind with the other columns.  The
    // side stream must not touch the next panel's columns before the main stream's update of step k-1 has
    // written them (ev_next, recorded long before it is needed: that update runs beside panel k); the block
    // inverses alternate between two buffers because the main stream still reads step k's while the side
    // stream writes step k+1's.
    int step = 0;
    T *Tinv2[2] = {Tinv, Tinv + (size_t)((nb + 63) / 64) * 4096};
    {
        OnStream g(h, side);
        const int jb0 = (n - k0) < nb ? (n - k0) : nb;
        pa.list = h->moves_buf[0];
        if (area) pa.area = ws.areas, pa.area_bytes = area;
        LSX_TRY(launch_panel<T>(h, n - k0, jb0, A + (size_t)k0 * lda + k0, lda, k0, d_ipiv + k0, d_info, pa));
    }
    bool listed = pa.listed;    // panel k came with a gather list
    bool have_update = false;   // ev_next holds the end of the previous step's update
    for (int k = k0; k < n; k += nb, ++step) {
        const int jb = (n - k < nb) ? n - k : nb;
        T *Akk = A + (size_t)k * lda + k;
        T *Ti = Tinv2[step & 1];
        const int2 *mv = list(step, listed);   // panel k's list
        const int rest = n - k - jb;
        if (rest <= 0) {
            LSX_HIP(hipEventRecord(h->ev_panel, side));
            LSX_HIP(hipStreamWaitEvent(main_s, h->ev_panel, 0));  // the last panel is factored
            LSX_TRY(apply_panel_swaps<T>(h, mv, k, A, lda, k, jb, d_ipiv + k));
            break;
        }
        T *A12 = A + (size_t)k * lda + k + jb;
        T *L21 = A + (size_t)(k + jb) * lda + k;
        T *A22 = A + (size_t)(k + jb) * lda + k + jb;
        if (k_stop > 0 && k + jb >= k_stop) {   // last step here: no panel ahead, the whole step on the main stream
            LSX_HIP(hipEventRecord(h->ev_panel, side));
            LSX_HIP(hipStreamWaitEvent(main_s, h->ev_panel, 0));
            LSX_TRY(launch_trtri<T>(h, 1, jb, Akk, lda, Ti));
            LSX_TRY(apply_panel_swaps<T>(h, mv, rest, A + k + jb, lda, k, jb, d_ipiv + k));
            LSX_TRY(launch_trsm_block<T>(h, 1, jb, rest, Akk, lda, Ti, A12, lda));
            LSX_TRY(launch_gemm_sub<T>(h, rest, rest, jb, L21, lda, A12, lda, A22, lda, mfma));
            LSX_TRY(apply_panel_swaps<T>(h, mv, k, A, lda, k, jb, d_ipiv + k));
            break;
        }
        const int jb2 = rest < nb ? rest : nb;  // width of the next panel
        {
            OnStream g(h, side);
            // block inverses and the next block's interchanges in one launch (the main stream starts behind the
            // chain anyway: the CUs are shared)
            if (have_update && !prev_counted) LSX_HIP(hipStreamWaitEvent(side, h->ev_next, 0));
            // (no info word for the waits of this schedule: a time-out is recorded in the status word alone)
            const int fused = launch_chain_head<T>(h, mv, nullptr, jb, Akk, lda, Ti, jb2, A + k + jb, lda, k,
                                                   prev_counted ? c0words + (step - 1) : nullptr, prev_tiles);
            if (fused < 0) return fused;
            if (fused == 1 && prev_counted) LSX_TRY(launch_wait_count(h, c0words + (step - 1), prev_tiles, nullptr));
            if (fused == 1) {
                LSX_TRY(launch_trtri<T>(h, 1, jb, Akk, lda, Ti));
                LSX_TRY(apply_panel_swaps<T>(h, mv, jb2, A + k + jb, lda, k, jb, d_ipiv + k));
            }
            LSX_TRY(launch_trsm_block<T>(h, 1, jb, jb2, Akk, lda, Ti, A12, lda));
            LSX_TRY(launch_gemm_sub<T>(h, rest, jb2, jb, L21, lda, A12, lda, A22, lda, mfma));
            // Sharing the CUs, the big update would take the slots these small launches need (measured:
            // the chain doubles); the main stream therefore starts behind the chain.
            LSX_HIP(hipEventRecord(h->ev_panel, side));
            // panel k+1 writes the gather list and exchange area that step k-1 used: behind ALL of update k-1 and its
            // left-hand interchanges (with the counted column the chain above no longer waited for them)
            if (have_update && prev_counted) LSX_HIP(hipStreamWaitEvent(side, h->ev_next, 0));
            pa.list = h->moves_buf[(step + 1) & 1];
            if (area) pa.area = ws.areas + (size_t)((step + 1) & 1) * area;
            LSX_TRY(launch_panel<T>(h, rest, jb2, A22, lda, k + jb, d_ipiv + k + jb, d_info, pa));
        }
        LSX_HIP(hipStreamWaitEvent(main_s, h->ev_panel, 0));
        bool cur_counted = false;
        int cur_tiles = 0;
        // panel k is done with its exchange area; panel k+2 reuses it, behind ev_next below
        if (area) LSX_HIP(hipMemsetAsync(ws.areas + (size_t)(step & 1) * area, 0, area, main_s));
        if (rest > jb2) {
            LSX_TRY(apply_panel_swaps<T>(h, mv, rest - jb2, A + k + jb + jb2, lda, k, jb, d_ipiv + k));
            LSX_TRY(launch_trsm_block<T>(h, 1, jb, rest - jb2, Akk, lda, Ti, A12 + jb2, lda));
            GemmPlan plan = mfma;
            plan.col0_static = c0words ? c0words + step : nullptr;
            GemmDone did;
            LSX_TRY(launch_gemm_sub<T>(h, rest, rest - jb2, jb, L21, lda, A12 + jb2, lda, A22 + jb2, lda, plan, &did));
            cur_counted = c0words && did.col0_complete;
            cur_tiles = did.col0_tiles;
        }
        // panel k's interchanges on the columns left of it, in the slack after the update
        LSX_TRY(apply_panel_swaps<T>(h, mv, k, A, lda, k, jb, d_ipiv + k));
        // recorded after the last reader of panel k's gather list: panel k+2 (launched by the side stream
        // behind its wait on this event) writes the same buffer
        LSX_HIP(hipEventRecord(h->ev_next, main_s));
        have_update = true;
        listed = pa.listed;
        prev_counted = cur_counted;
        prev_tiles = cur_tiles;
    }
    join.armed = false;   // both streams were joined by the last step
    return LSX_OK;
}

// Scratch of getrf_lookahead_x: three exchange areas of the XCD panel in rotation (panel j uses area j % 3, cleared behind
// update j; each launch needs its area all zero), sized for the tallest panel; then the words the kernels count in (one memset).
struct XcdScratch {
    size_t area = 0; char *areas = nullptr;
    int *xcc_word = nullptr, *pass = nullptr, *counters = nullptr, *col0 = nullptr, *ready = nullptr;
    void lay(Carver &c, lsx_handle_t h, const PanelArgs &pa, int m, size_t elem, int nsteps) {
        area = panel_x_area_bytes(h, pa.mode, m, elem);
        if (!area) return;
        areas = c.take<char>(3 * area);
        xcc_word = c.take<int>(1);                    // 1 + XCC id of the panel's XCD (blocks = 0 mod 8 land on XCC 0)
        pass = c.take<int>(nsteps);                   // per step: update workgroups that left the panel's XCD
        counters = c.take<int>(8 * (size_t)nsteps);   // per step: the update's eight strip queues
        col0 = c.take<int>(2 * (size_t)nsteps);       // per step: {ticket, finished tiles} of the update's tile column 0
        ready = c.take<int>(nsteps);                  // per step: block inverses finished (fused chain launch)
    }
};
// ---------------------------------------------------------------- look-ahead LU driver, XCD-scope panel
// The panel of step k+1 (kernels_panel_x.hip) fills every CU of ONE XCD while it runs, and the hardware deals an
// eighth of EVERY kernel's workgroups to that XCD whatever the stream or CU mask (measured: lsx_diag_cu_mask_probe),
// so a kernel launched beside a running panel cannot finish before the panel does.  The schedule is built on that:
//   side:  [chain head k: block inverses + panel k's interchanges on the next panel's columns] -> record HEAD
//          -> U12 and update of the next panel's column block -> gate -> panel k+1
//   main:  wait HEAD -> clear panel k's exchange area -> interchanges, U12 and update of all other columns, the
//          update as ONE work-queue kernel whose workgroups on the panel's XCD leave at once and count themselves;
//          the gate in front of panel k+1 waits for that count, i.e. until the update no longer needs the XCD
//   nothing else is launched while a panel runs: the interchanges on the columns LEFT of the panels are applied
//   for the whole factorisation by one launch at the end (one gather list per panel is kept).
// Factors and pivots are bit-identical to the other drivers (same kernels per element, tests).
template <typename T>
static int getrf_lookahead_x(lsx_handle_t h, int n, T *A, int lda, int32_t *d_ipiv, int *d_info, T *Tinv, PanelArgs pa,
                             int k0) {
    const int nb = h->nb;
    const int nsteps = (n - k0 + nb - 1) / nb;
    hipStream_t main_s = h->stream, side = h->side_stream;
    GemmPlan mfma;   // every update of an LU: see GemmPlan
    mfma.mfma_only = true;
    XcdScratch ws;   // inside the scratch that came with pa
    LSX_TRY(carve_in(pa.area, pa.area_bytes, "getrf_lookahead_x", [&](Carver &c) { ws.lay(c, h, pa, n - k0, sizeof(T), nsteps); }));
    const size_t area_x = ws.area;
    if (area_x == 0) { set_error("getrf_lookahead_x: panel settings without an exchange area"); return LSX_ERR_INTERNAL; }
    LSX_TRY(reserve(h, h->moves_all, (size_t)nsteps * 2048));
    JoinSide join{h, side, main_s, main_s};
    int *const xcc_word = ws.xcc_word, *const pass = ws.pass, *const counters = ws.counters, *const col0 = ws.col0, *const ready = ws.ready;
    for (int s = 0; s < 3; ++s) LSX_HIP(hipMemsetAsync(ws.areas + (size_t)s * area_x, 0, area_x, main_s));
    LSX_HIP(hipMemsetAsync(xcc_word, 0, (char *)(ready + nsteps) - (char *)xcc_word, main_s));
    LSX_HIP(hipMemsetD32Async((hipDeviceptr_t)xcc_word, 1, 1, main_s));
    pa.area_bytes = area_x, pa.cleared = true;
    pa.xcc_word = xcc_word;
    LSX_HIP(hipEventRecord(h->ev_start, main_s));
    LSX_HIP(hipStreamWaitEvent(side, h->ev_start, 0));
    auto list = [&](int s) { return (int2 *)((char *)h->moves_all.p + (size_t)s * 2048); };   // one gather list per panel
    T *Tinv2[2] = {Tinv, Tinv + (size_t)((nb + 63) / 64) * 4096};
    {
        OnStream g(h, side);
        pa.list = list(0);
        pa.area = ws.areas;
        LSX_TRY(launch_panel<T>(h, n - k0, (n - k0) < nb ? (n - k0) : nb, A + (size_t)k0 * lda + k0, lda, k0, d_ipiv + k0, d_info, pa));
        if (!pa.listed) { set_error("getrf_lookahead_x: panel without a gather list"); return LSX_ERR_INTERNAL; }
    }
    // What the chain of step k needs from the main stream is update k-1 on the NEXT panel's columns only.  When that
    // update went through the work queue with no edge launches, its kernel does those columns (tile column 0) first
    // and counts their finished tiles; the chain then waits for the count inside a one-wave kernel: the panels run
    // ahead of a long update (the first ~15 steps of an 8192^2 LU are bound by the update, which then follows
    // back to back instead of alternating with the chain), and no gate is needed in front of a panel that leaves
    // CUs of its XCD free -- update workgroups held up behind a running panel only delay the END of the update
    // kernel, which nothing on the chain waits for any more.  Otherwise (ragged shapes): the event behind the whole
    // update, and the gate.  (What this cannot buy: the chain's small kernels overlapping a RUNNING update.  The
    // update's persistent workgroups fill every CU of seven XCDs and the hardware deals every kernel's workgroups
    // round-robin over all eight, so a chain kernel launched early waits for update workgroups to leave:
    // tools/ts_lu.py shows chain heads of 130 us in the first steps.)
    const bool use_col0 = !h->x_events;
    bool prev_col0 = false;
    int prev_tiles = 0;
    int step = 0;
    int left_done = 0;   // panels [0, left_done) have had their interchanges applied to the columns left of them
    for (int k = k0; k < n; k += nb, ++step) {
        const int jb = (n - k < nb) ? n - k : nb;
        const int rest = n - k - jb;
        if (rest <= 0) break;
        T *Akk = A + (size_t)k * lda + k;
        T *Ti = Tinv2[step & 1];
        T *A12 = A + (size_t)k * lda + k + jb;
        T *L21 = A + (size_t)(k + jb) * lda + k;
        T *A22 = A + (size_t)(k + jb) * lda + k + jb;
        const int jb2 = rest < nb ? rest : nb;  // width of the next panel
        bool fused_all = false;
        {
            OnStream g(h, side);
            // update k-1 wrote the next panel's columns: its column-0 count (waited for inside the chain head), or the
            // event behind all of it
            const bool counted = step > 0 && prev_col0;
            if (step > 0 && !counted) LSX_HIP(hipStreamWaitEvent(side, h->ev_next, 0));
            // block inverses, interchanges and U12 of the next panel's columns in one launch where the shapes allow it
            const int all = launch_chain_fused<T>(h, list(step), d_info, jb, Akk, lda, Ti, jb2, A + k + jb, lda, k,
                                                  counted ? col0 + 2 * (step - 1) + 1 : nullptr, prev_tiles, ready + step);
            if (all < 0) return all;
            if (all == 1) {
                const int fused = launch_chain_head<T>(h, list(step), d_info, jb, Akk, lda, Ti, jb2, A + k + jb, lda, k,
                                                       counted ? col0 + 2 * (step - 1) + 1 : nullptr, prev_tiles);
                if (fused < 0) return fused;
                if (fused == 1) {
                    if (counted) LSX_TRY(launch_wait_count(h, col0 + 2 * (step - 1) + 1, prev_tiles, d_info));
                    LSX_TRY(launch_trtri<T>(h, 1, jb, Akk, lda, Ti));
                    LSX_TRY(launch_laswp_moves<T>(h, list(step), jb2, A + k + jb, lda, k));
                }
            }
            // HEAD: block inverses of panel k are there.  The fused launch counts them in a device word the main stream
            // waits for in a one-wave kernel: an event record here would be a marker packet BETWEEN the chain's launches
            // (6 us on the panel-to-panel path -- what the fusion itself saved)
            fused_all = all == LSX_OK;
            if (!fused_all) {
                LSX_HIP(hipEventRecord(h->ev_panel, side));
                LSX_TRY(launch_trsm_block<T>(h, 1, jb, jb2, Akk, lda, Ti, A12, lda));
            }
            LSX_TRY(launch_gemm_sub<T>(h, rest, jb2, jb, L21, lda, A12, lda, A22, lda, mfma));
        }
        // main stream, behind HEAD.  Measured alternatives (8192^2 / 4096^2, ms): this order 18.2 / 7.6; interchanges
        // ahead of HEAD and the area cleared by the update's idle workgroups, so that the update starts earlier,
        // 18.5 / 7.9 (its resident workgroups take the CUs the next panel's small update needs: 27 instead of 17 us);
        // the update ordered behind that small update by an event 19.0 / 8.0 (a cross-stream hop on the chain).
        if (fused_all) LSX_TRY(launch_wait_count(h, ready + step, 2, d_info));
        else LSX_HIP(hipStreamWaitEvent(main_s, h->ev_panel, 0));
        GemmDone did;   // of the big update
        if (rest > jb2) {
            LSX_TRY(launch_laswp_moves<T>(h, list(step), rest - jb2, A + k + jb + jb2, lda, k));
            LSX_TRY(launch_trsm_block<T>(h, 1, jb, rest - jb2, Akk, lda, Ti, A12 + jb2, lda));
            GemmPlan plan = mfma;
            plan.counters = counters + 8 * step;
            plan.avoid_word = xcc_word;
            plan.pass_word = pass + step;
            plan.col0 = use_col0 ? col0 + 2 * step : nullptr;
            LSX_TRY(launch_gemm_sub<T>(h, rest, rest - jb2, jb, L21, lda, A12 + jb2, lda, A22 + jb2, lda, plan, &did));
        }
        const bool cur_col0 = did.queued && did.col0_complete;
        // panel k is done with its exchange area and panel k+3 reuses it: cleared behind the update, off the path
        // HEAD -> update start -> panel k+1; the chain of panel k+3 waits for (a part of) update k+1, behind this
        LSX_HIP(hipMemsetAsync(ws.areas + (size_t)(step % 3) * area_x, 0, area_x, main_s));
        LSX_HIP(hipEventRecord(h->ev_next, main_s));
        // panel k's interchanges on the columns LEFT of it: behind the update, where this stream only waits for the next
        // HEAD (one launch for all panels at the very end was 0.3 ms of an 8192^2 factorisation, on the critical path).
        // Its eighth of workgroups dealt to a busy panel XCD finishes when that panel does -- just before HEAD arrives.
        // Not in update-bound steps with a wide left-hand side, where this stream IS the critical path and the launch is not
        // small (16384^2: 8192+ columns from the first step of this driver, +0.4 ms): theirs are caught up in one launch at the
        // first step that has room.
        if (h->left_per_step && (rest <= 5632 || k <= 4096)) {
            if (left_done < step) {
                LSX_TRY(launch_laswp_left_all<T>(h, A, lda, k0 + left_done * nb, nb, step - left_done, list(left_done)));
                left_done = step;
            }
            if (k > 0) LSX_TRY(launch_laswp_moves<T>(h, list(step), k, A, lda, k));
            left_done = step + 1;
        }
        {
            OnStream g(h, side);
            // The gate (panel k+1 not before update k has started) is still wanted while the panel takes nearly every
            // CU of its XCD: launched earlier, it starves the main stream's small kernels in front of the update of
            // their eighth of workgroups dealt to that XCD (8192^2, steps 2-7: 640 instead of 455 us per step).
            // (fp32 panels above 8192 rows keep 512 rows per workgroup: 25 of 32 CUs at 12800 rows)
            const bool tall = (rest > 6400 && (sizeof(T) == 8 || rest <= 8192)) || rest > 12800;
            if (did.queued && (!cur_col0 || tall)) LSX_TRY(launch_gate(h, pass + step, 2 * h->num_cu / 8));
            pa.list = list(step + 1);
            pa.area = ws.areas + (size_t)((step + 1) % 3) * area_x;
            LSX_TRY(launch_panel<T>(h, rest, jb2, A22, lda, k + jb, d_ipiv + k + jb, d_info, pa));
            if (!pa.listed) { set_error("getrf_lookahead_x: panel without a gather list"); return LSX_ERR_INTERNAL; }
        }
        prev_col0 = cur_col0;
        prev_tiles = did.col0_tiles;
    }
    // the last panel is factored; every panel's interchanges on the columns left of it
    LSX_HIP(hipEventRecord(h->ev_panel, side));
    LSX_HIP(hipStreamWaitEvent(main_s, h->ev_panel, 0));
    join.armed = false;   // joined just above
    // what has not trailed its step: the last panel's (all of them with left_per_step = 0)
    return launch_laswp_left_all<T>(h, A, lda, k0 + left_done * nb, nb, nsteps - left_done, list(left_done));
}

// Workspaces of one factorisation of order n, sized before its first launch: tinv (block inverses, two sets: the
// look-ahead driver alternates) and scratch, which every stage lays out from its start -- so scratch is the LARGEST of
// the layouts that can run for this n, element size and options, each counted by the code that places it: a panel that clears
// its own area (sequential driver, mg.hip, first-rule row reduction) and the two look-ahead drivers from column 0 (a later start
// needs no more).  Nothing reserves scratch again until the factorisation is queued; a PanelArgs is made after this.  mg.hip sizes here too.
int ensure_getrf_workspace(lsx_handle_t h, int n, size_t elem) {
    const PanelArgs pa(h, nullptr);
    const int nsteps = (n + h->nb - 1) / h->nb;
    size_t need = panel_scratch_bytes(h, pa.mode, pa.nt, pa.rt, n, elem);
    for (const bool hybrid : {false, true})
        need = std::max(need, carve_bytes([&](Carver &c) { SharedCuScratch().lay(c, h, shared_cu_panel(pa, elem, hybrid, n), n, nsteps); }));
    need = std::max(need, carve_bytes([&](Carver &c) { XcdScratch().lay(c, h, pa, n, elem, nsteps); }));
    LSX_TRY(reserve(h, h->scratch, need));
    const size_t tinv_elems = (size_t)((h->nb * h->kblock + 63) / 64) * 64 * 64;
    return reserve(h, h->tinv, 2 * pad256(tinv_elems * elem));   // x2: the look-ahead driver alternates
}

// ---------------------------------------------------------------- blocked LU driver
// percolumn: the host fall-back after an exchange time-out -- per-column panel launches (mode 0: no workgroup waits
// for another) in the sequential driver, whatever the handle's options say.
template <typename T>
static int getrf_dev(lsx_handle_t h, int n, T *A, int lda, int32_t *d_ipiv, int *d_info, bool percolumn = false) {
    LSX_ARG(n >= 0 && lda >= n && A && d_ipiv);
    if (n == 0) return LSX_OK;
    const int nb = h->nb;
    GemmPlan mfma;   // every update of an LU: see GemmPlan
    mfma.mfma_only = true;
    LSX_TRY(ensure_getrf_workspace(h, n, sizeof(T)));
    PanelArgs pa(h, h->moves_buf[0]);
    if (percolumn) pa.mode = 0;
    T *Tinv = (T *)h->tinv.p;
    if (!d_info) d_info = h->dev_status + 2;   // a time-out must be recorded somewhere: lsx_check_status reads it
    LSX_HIP(hipMemsetAsync(d_info, 0, sizeof(int), h->stream));
    // Look-ahead (panel k+1 on a side stream under the update of step k; bit-identical factors).  Measured
    // on MI355X with the pipelined panel, lookahead=1 against the sequential driver: n = 4096 -8 %,
    // 6144 +0.5 %, 7168 +5 %, 8192 +8 %, 10240..16384 +11..12 %, 20480 +10 %.  Below ~6500 the shorter update
    // no longer hides the panel and the split update costs more than it saves (fp32: see the variant choice below).
    int LOOKAHEAD_MIN = sizeof(T) == 8 ? 7168 : 10240;   // fp32: the update is half as long, break-even higher
    // XCD-scope panel and its own schedule.  Measured against the sequential driver: fp64 1536 0 %, 2048 +2 %, 2560 +4.5 %,
    // 3072 +7 %; fp32 (short updates) 3072 -1 %, 4096 0 %, 5120 +3 %, 6144 +7 %, 7168 +12 %.
    if (pa.mode == 4) LOOKAHEAD_MIN = sizeof(T) == 8 ? 2048 : 4096;
    if (h->lookahead_min > 0) LOOKAHEAD_MIN = h->lookahead_min;                  // option (tests, tuning)
    int k_end = n;  // the sequential driver below handles columns [0, k_end)
    if (h->lookahead && !percolumn && n >= LOOKAHEAD_MIN && h->kblock == 1) k_end = 0;
    const int W = nb * h->kblock;
    for (int k = 0; k < k_end; k += W) {
        const int w = (n - k < W) ? n - k : W;  // width of this super-block
        for (int j = 0; j < w; j += nb) {
            const int c = k + j;                      // first column of this panel
            const int jb = (w - j < nb) ? w - j : nb;
            T *Acc = A + (size_t)c * lda + c;
            LSX_TRY(launch_panel<T>(h, n - c, jb, Acc, lda, c, d_ipiv + c, d_info, pa));
            if (pa.listed) {   // left and right of the panel in one launch
                LSX_TRY(launch_laswp_moves_around<T>(h, (const int2 *)pa.list, n, A, lda, c, c, jb));
            } else {
                LSX_TRY(launch_laswp<T>(h, c, A, lda, c, jb, d_ipiv + c));                      // left
                LSX_TRY(launch_laswp<T>(h, n - c - jb, A + c + jb, lda, c, jb, d_ipiv + c));  // right
            }
            const int inner = w - j - jb;  // columns of the super-block still to be factored
            if (inner > 0) {
                T *A12 = A + (size_t)c * lda + c + jb;
                LSX_TRY(launch_trtri<T>(h, 1, jb, Acc, lda, Tinv));
                LSX_TRY(launch_trsm_block<T>(h, 1, jb, inner, Acc, lda, Tinv, A12, lda));
                LSX_TRY(launch_gemm_sub<T>(h, n - c - jb, inner, jb, A + (size_t)(c + jb) * lda + c, lda, A12,
                                           lda, A + (size_t)(c + jb) * lda + c + jb, lda, mfma));
            }
        }
        const int rest = n - k - w;
        if (rest > 0) {
            T *Akk = A + (size_t)k * lda + k;
            T *A12 = A + (size_t)k * lda + k + w;
            LSX_TRY(launch_trtri<T>(h, 1, w, Akk, lda, Tinv));
            if (w > nb && nb % 64 == 0) {
                // U12 of a super-block one panel at a time: 128-row block solve, then the rows of the later
                // panels take the update of the earlier ones (a skinny MFMA update) before their own solve.
                // A single w-row block solve does the same flops inside one workgroup per 32 columns and
                // costs more than the deeper trailing update saves.
                for (int j = 0; j < w; j += nb) {
                    const int jb = (w - j < nb) ? w - j : nb;
                    if (j > 0)
                        LSX_TRY(launch_gemm_sub<T>(h, jb, rest, j, Akk + (size_t)j * lda, lda, A12, lda,
                                                   A12 + (size_t)j * lda, lda, mfma));
                    LSX_TRY(launch_trsm_block<T>(h, 1, jb, rest, Akk + (size_t)j * lda + j, lda,
                                                 Tinv + (size_t)(j / 64) * 4096, A12 + (size_t)j * lda, lda));
                }
            } else {
                LSX_TRY(launch_trsm_block<T>(h, 1, w, rest, Akk, lda, Tinv, A12, lda));
            }
            LSX_TRY(launch_gemm_sub<T>(h, rest, rest, w, A + (size_t)(k + w) * lda + k, lda, A12, lda,
                                       A + (size_t)(k + w) * lda + k + w, lda, mfma));
        }
    }
    if (k_end < n) {
        // XCD-scope panel (panel = 4): its own schedule, for the part of the matrix whose panels one XCD holds
        // (8192 rows fp64, 16384 fp32); the steps in front of that part run the shared-CU schedule with the
        // device-scope panel (12288^2 fp64: 46.4 -> see DESIGN 6).
        int xrows = 32 * 64 * (sizeof(T) == 8 ? 4 : 8);
        if (h->xrows_limit > 0 && h->xrows_limit < xrows) xrows = h->xrows_limit;   // tests: hand-over at small orders
        if (pa.mode == 4 && !h->panel_debug && nb % 32 == 0 && k_end % 32 == 0 &&
            panel_x_area_bytes(h, pa.mode, n - k_end, sizeof(T)) > 0) {
            int kx = k_end;
            if (n - kx > xrows) kx += (n - kx - xrows + nb - 1) / nb * nb;
            if (h->hybrid_off && kx > k_end) kx = n;
            if (kx < n) {
                if (kx > k_end) LSX_TRY(getrf_lookahead<T>(h, n, A, lda, d_ipiv, d_info, Tinv, pa, k_end, kx));
                return getrf_lookahead_x<T>(h, n, A, lda, d_ipiv, d_info, Tinv, pa, kx);
            }
        }
        return getrf_lookahead<T>(h, n, A, lda, d_ipiv, d_info, Tinv, pa, k_end);
    }
    return LSX_OK;
}

// Block substitution sweeps shared by the multi-right-hand-side solve and the inverse: 128-row diagonal blocks (their
// inverses in TinvL / TinvU), the rows beyond a block updated on the MFMA tile.
// pairs: TWO blocks per trailing update -- the update of the rows beyond the pair has depth 256 (the tile then runs at 0.76 of
// the MFMA pipe instead of 0.68, profiles/r03_pmc_gemm_mfma.json, and there are half as many launches), the block row in
// between gets its own 128-deep update first.  Per element the same fused multiply-adds in the same order as one block at a
// time: the accumulators start from C and take k in sequence either way; going upwards, where the block that comes second
// in memory must be applied first, the tile rotates its k index (GemmPlan::kshift).  Same bits (tools/getri_ab.py, tests).
// tri (forward sweep of the inverse): block row kb only has columns [0, kb + jb) to work on, the others are exact zeros.
template <typename T>
static int sweep_forward(lsx_handle_t h, int n, int ncols, bool tri, bool pairs, const T *LU, int lda, const T *TinvL, T *X, int ldx) {
    const int sb = 128;
    auto Lp = [&](int r, int c) { return LU + (size_t)r * lda + c; };
    auto Xp = [&](int r) { return X + (size_t)r * ldx; };
    for (int kb = 0; kb < n;) {
        const int jb = (n - kb < sb) ? n - kb : sb;
        const int nc = tri ? kb + jb : ncols;
        LSX_TRY(launch_trsm_block<T>(h, 1, jb, nc, Lp(kb, kb), lda, TinvL + (size_t)(kb / 64) * 4096, Xp(kb), ldx));
        const int below = n - kb - jb;
        if (below <= 0) break;
        if (!pairs || jb != sb) {
            LSX_TRY(launch_gemm_sub<T>(h, below, nc, jb, Lp(kb + jb, kb), lda, Xp(kb), ldx, Xp(kb + jb), ldx));
            kb += jb;
            continue;
        }
        const int jb2 = below < sb ? below : sb, nc2 = tri ? nc + jb2 : ncols;
        LSX_TRY(launch_gemm_sub<T>(h, jb2, nc, sb, Lp(kb + sb, kb), lda, Xp(kb), ldx, Xp(kb + sb), ldx));
        LSX_TRY(launch_trsm_block<T>(h, 1, jb2, nc2, Lp(kb + sb, kb + sb), lda, TinvL + (size_t)((kb + sb) / 64) * 4096, Xp(kb + sb), ldx));
        if (below > jb2)   // (tri: the first block's columns nc .. nc2 - 1 are exact zeros)
            LSX_TRY(launch_gemm_sub<T>(h, below - jb2, nc2, sb + jb2, Lp(kb + sb + jb2, kb), lda, Xp(kb), ldx, Xp(kb + sb + jb2), ldx));
        kb += sb + jb2;
    }
    return LSX_OK;
}

template <typename T>
static int sweep_backward(lsx_handle_t h, int n, int ncols, bool pairs, const T *LU, int lda, const T *TinvU, T *X, int ldx) {
    const int sb = 128;
    auto Up = [&](int r, int c) { return LU + (size_t)r * lda + c; };
    auto Xp = [&](int r) { return X + (size_t)r * ldx; };
    for (int kb = ((n - 1) / sb) * sb; kb >= 0;) {
        const int jb = (n - kb < sb) ? n - kb : sb;
        LSX_TRY(launch_trsm_block<T>(h, 0, jb, ncols, Up(kb, kb), lda, TinvU + (size_t)(kb / 64) * 4096, Xp(kb), ldx));
        if (kb == 0) break;
        const int lo = kb - sb;
        if (!pairs || jb % 16 != 0) {
            LSX_TRY(launch_gemm_sub<T>(h, kb, ncols, jb, Up(0, kb), lda, Xp(kb), ldx, X, ldx));
            kb -= sb;
            continue;
        }
        LSX_TRY(launch_gemm_sub<T>(h, sb, ncols, jb, Up(lo, kb), lda, Xp(kb), ldx, Xp(lo), ldx));   // the block row above only
        LSX_TRY(launch_trsm_block<T>(h, 0, sb, ncols, Up(lo, lo), lda, TinvU + (size_t)(lo / 64) * 4096, Xp(lo), ldx));
        if (lo > 0) {
            // rows above the pair: k runs over block kb first, then block lo -- the order of one block at a time
            GemmPlan rotated;
            rotated.kshift = sb;
            LSX_TRY(launch_gemm_sub<T>(h, lo, ncols, sb + jb, Up(0, lo), lda, Xp(lo), ldx, X, ldx, rotated));
        }
        kb = lo - sb;
    }
    return LSX_OK;
}

// two blocks per update pay where the updates are large and regular (8192^2 inverse 17.8 -> 15.7 ms, 4096^2 3.18 -> 3.05;
// ragged or small orders lose 3-12 % to the extra launches and the edge kernels)
static bool sweep_pairs(lsx_handle_t h, int n, int ncols) {
    return h->getri_pairs && ncols >= 1024 && (n >= 7168 || (n % 128 == 0 && n >= 4096));
}

// elements of the 64 x 64 (launch_trtri's layout) and of the 128 x 128 diagonal-block inverses of one triangle of order n
static size_t inv64_elems(int n) { return (size_t)((n + 63) / 64) * 64 * 64; }
static size_t inv128_elems(int n) { return (size_t)((n + 127) / 128) * 128 * 128; }
// tinv for the sweeps above: the 64 x 64 block inverses of both triangles
template <typename T>
static int carve_inv64(lsx_handle_t h, int n, T **TinvL, T **TinvU) {
    return carve(h, h->tinv, [&](Carver &c) { *TinvL = c.take<T>(inv64_elems(n)); *TinvU = c.take<T>(inv64_elems(n)); });
}
// tinv for the few-column and transposed solves: both sizes, both triangles
template <typename T> struct BlockInv { T *inv64L = nullptr, *inv64U = nullptr, *inv128L = nullptr, *inv128U = nullptr; };
template <typename T>
static int carve_block_inv(lsx_handle_t h, int n, BlockInv<T> *bi) {
    return carve(h, h->tinv, [&](Carver &c) {
        bi->inv64L = c.take<T>(inv64_elems(n)); bi->inv64U = c.take<T>(inv64_elems(n));
        bi->inv128L = c.take<T>(inv128_elems(n)); bi->inv128U = c.take<T>(inv128_elems(n));
    });
}

// X <- U^-1 L^-1 X for X already row-permuted (n x nrhs)
template <typename T>
static int lu_solve_permuted(lsx_handle_t h, int n, int nrhs, const T *LU, int lda, T *X, int ldx) {
    T *TinvL = nullptr, *TinvU = nullptr;
    LSX_TRY(carve_inv64(h, n, &TinvL, &TinvU));
    LSX_TRY(launch_trtri<T>(h, 1, n, LU, lda, TinvL));
    LSX_TRY(launch_trtri<T>(h, 0, n, LU, lda, TinvU));
    const bool pairs = sweep_pairs(h, n, nrhs);
    LSX_TRY(sweep_forward<T>(h, n, nrhs, false, pairs, LU, lda, TinvL, X, ldx));    // L y = P b   (linalg.py:587-596)
    LSX_TRY(sweep_backward<T>(h, n, nrhs, pairs, LU, lda, TinvU, X, ldx));          // U x = y     (linalg.py:611-621)
    return LSX_OK;
}

template <typename T>
static int getrs_dev(lsx_handle_t h, int n, int nrhs, const T *LU, int lda, const int32_t *d_ipiv,
                     T *B, int ldb) {
    LSX_ARG(n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs && LU && d_ipiv && B);
    if (n == 0 || nrhs == 0) return LSX_OK;
    // few right-hand sides: the solve-latency path (kernels_trsv.hip) works on 1, 2, 4 or 8 columns
    const int nr = nrhs <= 1 ? 1 : nrhs <= 2 ? 2 : nrhs <= 4 ? 4 : 8;
    if (nrhs <= 8 && n > 128) {
        int32_t *perm = nullptr; T *Bc = nullptr, *Bp = nullptr, *X = nullptr;
        LSX_TRY(carve(h, h->rhs_work, [&](Carver &c) {
            perm = c.take<int32_t>(n);
            Bc = c.take<T>((size_t)n * nr);   // copy of B, zero-padded to nr columns
            Bp = c.take<T>((size_t)n * nr);   // P * B, work space of the solve
            X = c.take<T>((size_t)n * nr);
        }));
        BlockInv<T> bi;
        LSX_TRY(carve_block_inv<T>(h, n, &bi));
        if (h->trsv_mode == 2) {   // 128-row steps, helper workgroups, interchanges + gather fused into the preparation launch
            const int r2 = lu_solve_few_rhs2<T>(h, n, nrhs, nr, LU, lda, d_ipiv, B, ldb, bi.inv64L, bi.inv64U, bi.inv128L,
                                                bi.inv128U, Bp, X);
            if (r2 != 1) return r2;
        }
        LSX_TRY(launch_ipiv_to_perm(h, n, d_ipiv, perm));
        if (nr != nrhs) LSX_HIP(hipMemsetAsync(Bc, 0, sizeof(T) * (size_t)n * nr, h->stream));
        LSX_TRY(launch_copy2d<T>(h, n, nrhs, B, ldb, Bc, nr));
        LSX_TRY(launch_gather_rows<T>(h, n, nr, perm, Bc, nr, Bp, nr));
        LSX_TRY(lu_solve_few_rhs<T>(h, n, nr, LU, lda, Bp, nr, X, bi.inv64L, bi.inv64U, bi.inv128L, bi.inv128U));
        return launch_copy2d<T>(h, n, nrhs, X, nr, B, ldb);
    }
    // perm + a copy of B for the row gather
    int32_t *perm = nullptr; T *Bc = nullptr;
    LSX_TRY(carve(h, h->rhs_work, [&](Carver &c) { perm = c.take<int32_t>(n); Bc = c.take<T>((size_t)n * nrhs); }));
    LSX_TRY(launch_ipiv_to_perm(h, n, d_ipiv, perm));
    LSX_TRY(launch_copy2d<T>(h, n, nrhs, B, ldb, Bc, nrhs));
    LSX_TRY(launch_gather_rows<T>(h, n, nrhs, perm, Bc, nrhs, B, ldb));
    return lu_solve_permuted<T>(h, n, nrhs, LU, lda, B, ldb);
}

template <typename T>
static int getri_dev(lsx_handle_t h, int n, const T *LU, int lda, const int32_t *d_ipiv, T *Inv,
                     int ldi) {
    LSX_ARG(n >= 0 && lda >= n && ldi >= n && LU && d_ipiv && Inv);
    if (n == 0) return LSX_OK;
    int32_t *perm = nullptr;
    LSX_TRY(carve(h, h->rhs_work, [&](Carver &c) { perm = c.take<int32_t>(n); }));
    LSX_TRY(launch_ipiv_to_perm(h, n, d_ipiv, perm));
    if (n >= 512 && !h->getri_plain) {
        // A^-1 = U^-1 L^-1 P with the permutation applied LAST: L^-1 of the identity is lower triangular, so the
        // forward substitution of block row kb only has columns [0, kb + jb) to work on -- n^3/3 flops instead
        // of n^3 (4/3 n^3 for the inverse, LAPACK's getri count, instead of 2 n^3).  The skipped operations are
        // multiplications by exact zeros, so every entry has the bits the plain form below gives it.
        const int ldw = (n + 15) & ~15;
        T *W = nullptr, *TinvL = nullptr, *TinvU = nullptr;
        LSX_TRY(carve(h, h->getri_work, [&](Carver &c) { W = c.take<T>((size_t)n * ldw); }));
        LSX_TRY(launch_set_identity_perm<T>(h, n, nullptr, W, ldw));
        LSX_TRY(carve_inv64(h, n, &TinvL, &TinvU));
        LSX_TRY(launch_trtri<T>(h, 1, n, LU, lda, TinvL));
        LSX_TRY(launch_trtri<T>(h, 0, n, LU, lda, TinvU));
        const bool pairs = sweep_pairs(h, n, n);
        LSX_TRY(sweep_forward<T>(h, n, n, true, pairs, LU, lda, TinvL, W, ldw));    // L Y = I on the columns that can be non-zero
        LSX_TRY(sweep_backward<T>(h, n, n, pairs, LU, lda, TinvU, W, ldw));         // U Z = Y, all columns
        return launch_scatter_cols<T>(h, n, perm, W, ldw, Inv, ldi);   // Inv[:, perm[c]] = Z[:, c]
    }
    LSX_TRY(launch_set_identity_perm<T>(h, n, perm, Inv, ldi));  // P * I
    return lu_solve_permuted<T>(h, n, n, LU, lda, Inv, ldi);
}

// ---------------------------------------------------------------- host-buffer wrappers
template <typename T>
static int h2d(lsx_handle_t h, int m, int n, const T *src, int lds, T *dst, int ldd) {
    LSX_HIP(hipMemcpy2DAsync(dst, (size_t)ldd * sizeof(T), src, (size_t)lds * sizeof(T),
                             (size_t)n * sizeof(T), m, hipMemcpyHostToDevice, h->stream));
    return LSX_OK;
}
template <typename T>
static int d2h(lsx_handle_t h, int m, int n, const T *src, int lds, T *dst, int ldd) {
    LSX_HIP(hipMemcpy2DAsync(dst, (size_t)ldd * sizeof(T), src, (size_t)lds * sizeof(T),
                             (size_t)n * sizeof(T), m, hipMemcpyDeviceToHost, h->stream));
    return LSX_OK;
}

static int ld_for(int n) { return (n + 15) & ~15; }  // device leading dimension: 128-B rows (fp64)

// Host-buffer entry points: upload, factor, read the info word -- and when the cooperative panel's exchange timed out
// (its workgroups were not all resident at once: something else held the CUs for longer than the bounded spin), upload
// again and factor with panel mode 0 (two plain launches per column, no workgroup waits for another) instead of
// failing.  hinfo < 0 on return only if that also failed.  Synchronises the handle's stream.
template <typename T>
static int factor_from_host(lsx_handle_t h, int n, const T *A, int lda, T *dA, int ld, int32_t *dp, int *dinfo,
                            int *hinfo) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        LSX_TRY(h2d<T>(h, n, n, A, lda, dA, ld));
        int rc;
        if (attempt == 0) {
            rc = getrf_dev<T>(h, n, dA, ld, dp, dinfo);
        } else {
            rc = getrf_dev<T>(h, n, dA, ld, dp, dinfo, true);
            h->panel_fallbacks += 1;
        }
        LSX_TRY(rc);
        LSX_HIP(hipMemcpyAsync(hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        LSX_HIP(hipStreamSynchronize(h->stream));
        if (*hinfo >= 0) return LSX_OK;
        // the time-out also set the status word; this call reports (or repairs) it, so it must not be left for the
        // next, unrelated call on the handle to find
        LSX_HIP(hipMemsetAsync(h->dev_status, 0, 3 * sizeof(int), h->stream));
    }
    set_error("panel exchange timed out on the device, and so did the per-column fallback");
    return LSX_ERR_INTERNAL;
}

template <typename T>
static int getrf_host(lsx_handle_t h, int n, T *A, int lda, int32_t *ipiv, int *info) {
    LSX_ARG(h && n >= 0 && lda >= n && (n == 0 || (A && ipiv)));
    if (info) *info = 0;
    if (n == 0) return LSX_OK;
    const int ld = ld_for(n);
    T *dA = nullptr; int32_t *dp = nullptr; int *dinfo = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) { dA = c.take<T>((size_t)n * ld); dp = c.take<int32_t>(n); dinfo = c.take<int>(1); }));
    int hinfo = 0;
    LSX_TRY(factor_from_host<T>(h, n, A, lda, dA, ld, dp, dinfo, &hinfo));
    LSX_TRY(d2h<T>(h, n, n, dA, ld, A, lda));
    LSX_HIP(hipMemcpyAsync(ipiv, dp, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = hinfo;
    return LSX_OK;
}

template <typename T>
static int getrs_host(lsx_handle_t h, int n, int nrhs, const T *LU, int lda, const int32_t *ipiv,
                      T *B, int ldb) {
    LSX_ARG(h && n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs);
    if (n == 0 || nrhs == 0) return LSX_OK;
    LSX_ARG(LU && ipiv && B);
    const int ld = ld_for(n), ldx = ld_for(nrhs);
    T *dA = nullptr, *dB = nullptr; int32_t *dp = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)n * ld);
        dB = c.take<T>((size_t)n * ldx);
        dp = c.take<int32_t>(n);
    }));
    LSX_TRY(h2d<T>(h, n, n, LU, lda, dA, ld));
    LSX_TRY(h2d<T>(h, n, nrhs, B, ldb, dB, ldx));
    LSX_HIP(hipMemcpyAsync(dp, ipiv, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
    LSX_TRY(getrs_dev<T>(h, n, nrhs, dA, ld, dp, dB, ldx));
    LSX_TRY(check_dev_status(h));
    LSX_TRY(d2h<T>(h, n, nrhs, dB, ldx, B, ldb));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

template <typename T>
static int gesv_host(lsx_handle_t h, int n, int nrhs, const T *A, int lda, T *B, int ldb, int *info,
                     double *pivot_ratio) {
    LSX_ARG(h && n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs);
    if (info) *info = 0;
    if (pivot_ratio) *pivot_ratio = 1.0;
    if (n == 0) return LSX_OK;
    LSX_ARG(A && (nrhs == 0 || B));
    const int ld = ld_for(n), ldx = ld_for(nrhs > 0 ? nrhs : 1);
    T *dA = nullptr, *dB = nullptr; int32_t *dp = nullptr; int *dinfo = nullptr; double *dprobe = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)n * ld);
        dB = c.take<T>((size_t)n * ldx);
        dp = c.take<int32_t>(n);
        dinfo = c.take<int>(1);
        dprobe = c.take<double>(2);
    }));
    if (nrhs > 0) LSX_TRY(h2d<T>(h, n, nrhs, B, ldb, dB, ldx));
    LSX_TRY(h2d<T>(h, n, n, A, lda, dA, ld));
    LSX_TRY(launch_amax<T>(h, n, n, dA, ld, dprobe));
    int hinfo = 0;
    LSX_TRY(factor_from_host<T>(h, n, A, lda, dA, ld, dp, dinfo, &hinfo));
    LSX_TRY(launch_diag_minabs<T>(h, n, dA, ld, dprobe));
    double probe[2] = {0, 0};
    LSX_HIP(hipMemcpyAsync(probe, dprobe, sizeof(probe), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = hinfo;
    if (pivot_ratio) *pivot_ratio = probe[0] > 0 ? probe[1] / probe[0] : 0.0;
    if (hinfo != 0 || nrhs == 0) return LSX_OK;  // singular: B is left untouched
    LSX_TRY(getrs_dev<T>(h, n, nrhs, dA, ld, dp, dB, ldx));
    LSX_TRY(check_dev_status(h));
    LSX_TRY(d2h<T>(h, n, nrhs, dB, ldx, B, ldb));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}


// ---------------------------------------------------------------- transposed solve, norms, condition estimate
// Blocked A^T X = B for many right-hand sides (n > 128): the sweeps of lu_solve_permuted for the transposed factors, every
// product on the TN form of the MFMA tile (kernels_gemm.hip), which reads the block rows of U and L as they lie in memory.
//   forward,  U^T Y = B, k ascending:   Y_k = inv(U_kk)^T W_k ;  W[k+jb:] -= U[k:k+jb, k+jb:]^T Y_k
//   backward, L^T Z = Y, k descending:  Z_k = inv(L_kk)^T Y_k ;  Y[:k]    -= L[k:k+jb, :k]^T Z_k
//   X[perm[i], :] = Z[i, :]
// inv(T_kk) are the natural-orientation 128 x 128 block inverses of the grouped path (identity outside the matrix), so
// inv^T W_k is a TN product of depth jb too; it cannot run in place, so the two n x nrhs work arrays take turns: the
// forward sweep reads W and leaves Y in the second array, the backward sweep leaves Z in the first.  W (ld = ldw, a
// multiple of 16) is an aligned copy of B: whatever ldb is, the interior tiles take the FULL form when LU allows it.
// A column's bits do not depend on the other columns of the call: every product is an MFMA tile that takes k in order.
template <typename T>
static int lu_solve_transposed_blocked(lsx_handle_t h, int n, int nrhs, const T *LU, int lda, const int32_t *perm, T *B,
                                       int ldb, const T *inv128L, const T *inv128U, T *W, T *Y, int ldw) {
    const int sb = 128;
    auto Fp = [&](int r, int c) { return LU + (size_t)r * lda + c; };
    auto Wp = [&](int r) { return W + (size_t)r * ldw; };
    auto Yp = [&](int r) { return Y + (size_t)r * ldw; };
    LSX_TRY(launch_copy2d<T>(h, n, nrhs, B, ldb, W, ldw));
    for (int kb = 0; kb < n; kb += sb) {
        const int jb = (n - kb < sb) ? n - kb : sb;
        LSX_TRY(launch_gemm_tn_acc<T>(h, 3, jb, nrhs, jb, inv128U + (size_t)(kb / sb) * sb * sb, sb, Wp(kb), ldw, Yp(kb), ldw));
        LSX_TRY(launch_gemm_tn_sub<T>(h, n - kb - jb, nrhs, jb, Fp(kb, kb + jb), lda, Yp(kb), ldw, Wp(kb + jb), ldw));
    }
    for (int kb = ((n - 1) / sb) * sb; kb >= 0; kb -= sb) {
        const int jb = (n - kb < sb) ? n - kb : sb;
        LSX_TRY(launch_gemm_tn_acc<T>(h, 3, jb, nrhs, jb, inv128L + (size_t)(kb / sb) * sb * sb, sb, Yp(kb), ldw, Wp(kb), ldw));
        LSX_TRY(launch_gemm_tn_sub<T>(h, kb, nrhs, jb, Fp(kb, 0), lda, Wp(kb), ldw, Y, ldw));
    }
    return launch_scatter_rows<T>(h, n, nrhs, perm, W, ldw, B, ldb);
}

// lsx_gemm_tn_*_dev: A is k x m (lda >= m).  A zero extent is legal and leaves C untouched, with or without pointers.
template <typename T>
static int gemm_tn_dev(lsx_handle_t h, int plus, int m, int n, int k, const T *dA, int lda, const T *dB, int ldb, T *dC,
                       int ldc) {
    LSX_ARG(h && m >= 0 && n >= 0 && k >= 0 && lda >= m && ldb >= n && ldc >= n);
    if (m == 0 || n == 0 || k == 0) return LSX_OK;
    LSX_ARG(dA && dB && dC);
    return launch_gemm_tn_acc<T>(h, plus, m, n, k, dA, lda, dB, ldb, dC, ldc);
}

// ---------------------------------------------------------------- Cholesky: A = U^T U, row-major, upper
// Right-looking over 128-row steps on one stream, no look-ahead:
//   U11, inv(U11)     <- the diagonal block, one workgroup (kernels_chol.hip)                      [PANEL]
//   U12 = inv(U11)^T A12: the TN tile in its C = A^T B mode; it cannot run in place, so A12 is copied to a
//                        jb x rest work strip and multiplied back                                   [TRSM]
//   A22(upper) -= U12^T U12: the TN tile over the tiles on and above the diagonal only               [GEMM]
// The info word lives in the work space (the caller's may be null) and is copied out at the end.  After a failed pivot
// the later diagonal launches see the word and write an identity for the strip product, which then runs on the
// untouched strip: nothing waits, nothing faults, and the leading rows stay as they were.
template <typename T>
static int potrf_dev(lsx_handle_t h, int n, T *A, int lda, int *d_info) {
    LSX_ARG(h && n >= 0 && lda >= n);
    if (n == 0) return LSX_OK;
    LSX_ARG(A);
    const int sb = 128, ldw = ld_for(n);
    int *winfo = nullptr; T *Vinv = nullptr, *W = nullptr;
    LSX_TRY(carve(h, h->tinv, [&](Carver &c) { winfo = c.take<int>(1); Vinv = c.take<T>((size_t)sb * sb); }));
    LSX_TRY(carve(h, h->rhs_work, [&](Carver &c) { W = c.take<T>((size_t)sb * ldw); }));
    LSX_HIP(hipMemsetAsync(winfo, 0, sizeof(int), h->stream));
    for (int kb = 0; kb < n; kb += sb) {
        const int jb = (n - kb < sb) ? n - kb : sb, rest = n - kb - jb;
        T *Akk = A + (size_t)kb * lda + kb, *A12 = Akk + jb, *A22 = A12 + (size_t)jb * lda;
        LSX_TRY(launch_chol_diag<T>(h, jb, Akk, lda, kb, Vinv, winfo));
        if (rest <= 0) break;
        {
            ProfScope ps(h, LSX_PROF_TRSM, 0, 2.0 * sizeof(T) * jb * (double)rest);
            LSX_TRY(launch_copy2d<T>(h, jb, rest, A12, lda, W, ldw));
        }
        LSX_TRY(launch_gemm_tn_acc<T>(h, 3, jb, rest, jb, Vinv, sb, W, ldw, A12, lda, LSX_PROF_TRSM));
        LSX_TRY(launch_syrk_tn_sub<T>(h, rest, jb, A12, lda, A22, lda));
    }
    if (d_info) LSX_HIP(hipMemcpyAsync(d_info, winfo, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    return LSX_OK;
}

// Few right-hand sides (kernels_posx.hip): one launch per 128-row block step and direction on a dense n x nr copy of
// the columns, nothing cooperative.  prepare forms the block inverses once (pocon and porfs solve many times with one
// factor); nothing else may grow tinv or rhs_work between prepare and the last apply.
template <typename T>
struct PotrsFew {
    const T *inv128 = nullptr;
    T *W = nullptr;
};
template <typename T>
static int potrs_few_prepare(lsx_handle_t h, int n, const T *U, int lda, PotrsFew<T> *pf) {
    T *inv64 = nullptr, *inv128 = nullptr;
    LSX_TRY(carve(h, h->tinv, [&](Carver &c) { inv64 = c.take<T>(inv64_elems(n)); inv128 = c.take<T>(inv128_elems(n)); }));
    LSX_TRY(carve(h, h->rhs_work, [&](Carver &c) { pf->W = c.take<T>((size_t)n * 8); }));
    pf->inv128 = inv128;
    return launch_chol_inv<T>(h, n, U, lda, inv64, inv128);
}
// B (n x nrhs, 1 <= nrhs <= 8) <- inv(U) inv(U^T) B
template <typename T>
static int potrs_few_apply(lsx_handle_t h, int n, int nrhs, const T *U, int lda, const PotrsFew<T> &pf, T *B, int ldb) {
    const int nr = nrhs <= 1 ? 1 : nrhs <= 2 ? 2 : nrhs <= 4 ? 4 : 8;
    LSX_TRY(launch_trsvt_forward_upper<T>(h, n, nr, nrhs, U, lda, pf.inv128, (const T *)B, ldb, 0, pf.W));
    return launch_posx_backward<T>(h, n, nr, nrhs, U, lda, pf.inv128, pf.W, B, ldb, 0);
}

// B <- inv(U) inv(U^T) B: the U half of lu_solve_transposed_blocked (U^T Y = B on the TN tile), then sweep_backward
// (U X = Y).  The block inverses come from the upper triangle alone (launch_chol_inv): what lies below the diagonal of
// the factor array is never loaded, it may hold anything.  Every nrhs >= 1 takes these sweeps unless the option
// potrs_few_max (default 0) sends 1 <= nrhs <= potrs_few_max through the few-column path above.
template <typename T>
static int potrs_dev(lsx_handle_t h, int n, int nrhs, const T *U, int lda, T *B, int ldb) {
    LSX_ARG(h && n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs);
    h->potrs_path = 0;
    if (n == 0 || nrhs == 0) return LSX_OK;
    LSX_ARG(U && B);
    if (nrhs <= h->potrs_few_max) {
        PotrsFew<T> pf;
        LSX_TRY(potrs_few_prepare<T>(h, n, U, lda, &pf));
        h->potrs_path = 1;
        return potrs_few_apply<T>(h, n, nrhs, U, lda, pf, B, ldb);
    }
    const int sb = 128, ldw = ld_for(nrhs);
    T *inv64 = nullptr, *inv128 = nullptr, *W = nullptr, *Y = nullptr;
    LSX_TRY(carve(h, h->tinv, [&](Carver &c) { inv64 = c.take<T>(inv64_elems(n)); inv128 = c.take<T>(inv128_elems(n)); }));
    LSX_TRY(carve(h, h->rhs_work, [&](Carver &c) { W = c.take<T>((size_t)n * ldw); Y = c.take<T>((size_t)n * ldw); }));
    auto Up = [&](int r, int c) { return U + (size_t)r * lda + c; };
    auto Wp = [&](int r) { return W + (size_t)r * ldw; };
    auto Yp = [&](int r) { return Y + (size_t)r * ldw; };
    LSX_TRY(launch_chol_inv<T>(h, n, U, lda, inv64, inv128));
    LSX_TRY(launch_copy2d<T>(h, n, nrhs, B, ldb, W, ldw));
    for (int kb = 0; kb < n; kb += sb) {
        const int jb = (n - kb < sb) ? n - kb : sb;
        LSX_TRY(launch_gemm_tn_acc<T>(h, 3, jb, nrhs, jb, inv128 + (size_t)(kb / sb) * sb * sb, sb, Wp(kb), ldw, Yp(kb), ldw));
        LSX_TRY(launch_gemm_tn_sub<T>(h, n - kb - jb, nrhs, jb, Up(kb, kb + jb), lda, Yp(kb), ldw, Wp(kb + jb), ldw));
    }
    LSX_TRY(sweep_backward<T>(h, n, nrhs, sweep_pairs(h, n, nrhs), U, lda, inv64, Y, ldw));
    return launch_copy2d<T>(h, n, nrhs, Y, ldw, B, ldb);
}

// Host <-> device traffic of the upper form: block row kb moves from its first diagonal column on, so nothing left
// of the diagonal blocks is touched on either side (inside a diagonal block the elements below the diagonal make the
// round trip unchanged; no kernel loads them).
template <typename T>
static int upper_h2d(lsx_handle_t h, int n, const T *A, int lda, T *dA, int ld) {
    for (int kb = 0; kb < n; kb += 128)
        LSX_TRY(h2d<T>(h, std::min(128, n - kb), n - kb, A + (size_t)kb * lda + kb, lda, dA + (size_t)kb * ld + kb, ld));
    return LSX_OK;
}
template <typename T>
static int upper_d2h(lsx_handle_t h, int n, const T *dA, int ld, T *A, int lda) {
    for (int kb = 0; kb < n; kb += 128)
        LSX_TRY(d2h<T>(h, std::min(128, n - kb), n - kb, dA + (size_t)kb * ld + kb, ld, A + (size_t)kb * lda + kb, lda));
    return LSX_OK;
}

template <typename T>
static int potrf_host(lsx_handle_t h, int n, T *A, int lda, int *info) {
    LSX_ARG(h && n >= 0 && lda >= n);
    if (n == 0) return LSX_OK;
    LSX_ARG(A);
    if (info) *info = 0;
    const int ld = ld_for(n);
    T *dA = nullptr; int *dinfo = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) { dA = c.take<T>((size_t)n * ld); dinfo = c.take<int>(1); }));
    int hinfo = 0;
    LSX_TRY(upper_h2d<T>(h, n, A, lda, dA, ld));
    LSX_TRY(potrf_dev<T>(h, n, dA, ld, dinfo));
    LSX_HIP(hipMemcpyAsync(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LSX_TRY(upper_d2h<T>(h, n, dA, ld, A, lda));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = hinfo;
    return LSX_OK;
}

template <typename T>
static int potrs_host(lsx_handle_t h, int n, int nrhs, const T *U, int lda, T *B, int ldb) {
    LSX_ARG(h && n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs);
    if (n == 0 || nrhs == 0) return LSX_OK;
    LSX_ARG(U && B);
    const int ld = ld_for(n), ldx = ld_for(nrhs);
    T *dU = nullptr, *dB = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) { dU = c.take<T>((size_t)n * ld); dB = c.take<T>((size_t)n * ldx); }));
    LSX_TRY(upper_h2d<T>(h, n, U, lda, dU, ld));
    LSX_TRY(h2d<T>(h, n, nrhs, B, ldb, dB, ldx));
    LSX_TRY(potrs_dev<T>(h, n, nrhs, dU, ld, dB, ldx));
    LSX_TRY(d2h<T>(h, n, nrhs, dB, ldx, B, ldb));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

template <typename T>
static int posv_host(lsx_handle_t h, int n, int nrhs, const T *A, int lda, T *B, int ldb, int *info) {
    LSX_ARG(h && n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs);
    if (n == 0 || nrhs == 0) return LSX_OK;
    LSX_ARG(A && B);
    if (info) *info = 0;
    const int ld = ld_for(n), ldx = ld_for(nrhs);
    T *dA = nullptr, *dB = nullptr; int *dinfo = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)n * ld);
        dB = c.take<T>((size_t)n * ldx);
        dinfo = c.take<int>(1);
    }));
    int hinfo = 0;
    LSX_TRY(upper_h2d<T>(h, n, A, lda, dA, ld));
    LSX_TRY(h2d<T>(h, n, nrhs, B, ldb, dB, ldx));
    LSX_TRY(potrf_dev<T>(h, n, dA, ld, dinfo));
    LSX_HIP(hipMemcpyAsync(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = hinfo;
    if (hinfo != 0) return LSX_OK;   // not positive definite: B is left untouched
    LSX_TRY(potrs_dev<T>(h, n, nrhs, dA, ld, dB, ldx));
    LSX_TRY(d2h<T>(h, n, nrhs, dB, ldx, B, ldb));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

template <typename T>
static int syrk_tn_dev(lsx_handle_t h, int n, int k, const T *dA, int lda, T *dC, int ldc) {
    LSX_ARG(h && n >= 0 && k >= 0 && lda >= n && ldc >= n);
    if (n == 0 || k == 0) return LSX_OK;
    LSX_ARG(dA && dC);
    return launch_syrk_tn_sub<T>(h, n, k, dA, lda, dC, ldc);
}

// ---------------------------------------------------------------- SPD inverse and determinant from the factor
// inv(A) = inv(U) inv(U)^T = V^T V with V = inv(U^T), lower triangular: n^3/3 flops for V, n^3/3 for the product.
//
// trtri_upper_t: V = inv(U^T) on and below the diagonal 128-blocks of V.  The forward loop of potrs_dev (U^T Y = B on
// the TN tile) applied to the identity with getri_dev's column restriction: block row kb has columns [0, kb + jb) to
// work on, the rest are exact zeros and stay unwritten.  The diagonal-block product cannot run in place, so the block
// row goes through one 128-row strip (potrf_dev's device) and back.  U is read through its diagonal blocks
// (launch_chol_inv: the upper triangle alone) and through the blocks strictly above them.  Inside a diagonal block of V
// the entries above the diagonal are exact zeros (inv128's zeros times finite numbers); the blocks of V strictly above
// the diagonal blocks are never written.
template <typename T>
static int trtri_upper_t(lsx_handle_t h, int n, const T *U, int lda, T *V, int ldv) {
    const int sb = 128, ldw = ld_for(n);
    T *inv64 = nullptr, *inv128 = nullptr, *S = nullptr;
    LSX_TRY(carve(h, h->tinv, [&](Carver &c) { inv64 = c.take<T>(inv64_elems(n)); inv128 = c.take<T>(inv128_elems(n)); }));
    LSX_TRY(carve(h, h->rhs_work, [&](Carver &c) { S = c.take<T>((size_t)sb * ldw); }));
    auto Up = [&](int r, int c) { return U + (size_t)r * lda + c; };
    auto Vp = [&](int r) { return V + (size_t)r * ldv; };
    LSX_TRY(launch_chol_inv<T>(h, n, U, lda, inv64, inv128));
    LSX_TRY(launch_lower_identity<T>(h, n, V, ldv));
    for (int kb = 0; kb < n; kb += sb) {
        const int jb = (n - kb < sb) ? n - kb : sb, nc = kb + jb;
        {
            ProfScope ps(h, LSX_PROF_TRSM, 0, 2.0 * sizeof(T) * jb * (double)nc);
            LSX_TRY(launch_copy2d<T>(h, jb, nc, Vp(kb), ldv, S, ldw));
        }
        LSX_TRY(launch_gemm_tn_acc<T>(h, 3, jb, nc, jb, inv128 + (size_t)(kb / sb) * sb * sb, sb, S, ldw, Vp(kb), ldv, LSX_PROF_TRSM));
        LSX_TRY(launch_gemm_tn_sub<T>(h, n - kb - jb, nc, jb, Up(kb, kb + jb), lda, Vp(kb), ldv, Vp(kb + jb), ldv));
    }
    return LSX_OK;
}

template <typename T>
static int trtri_upper_t_dev(lsx_handle_t h, int n, const T *dU, int lda, T *dV, int ldv) {
    LSX_ARG(h && n >= 0 && lda >= n && ldv >= n);
    if (n == 0) return LSX_OK;
    LSX_ARG(dU && dV);
    return trtri_upper_t<T>(h, n, dU, lda, dV, ldv);
}

template <typename T>
static int lauum_tn_dev(lsx_handle_t h, int n, const T *dV, int ldv, T *dC, int ldc) {
    LSX_ARG(h && n >= 0 && ldv >= n && ldc >= n);
    h->potri_tiles = 0;
    if (n == 0) return LSX_OK;
    LSX_ARG(dV && dC);
    return launch_lauum_tn<T>(h, n, dV, ldv, dC, ldc, h->potri_order, h->lauum_descending != 0);
}

// LAPACK's potri, in place: the upper triangle of the factor array receives the upper triangle of inv(A).  V lives in
// getri_work (n x ld_for(n), aligned whatever lda is); U is dead once V is formed, so the product (always in its
// descending k-slab form, which adds the dominant terms k = col last: kernels_gemm.hip) goes straight into the
// caller's array.  A zero or NaN u_ii is reported and otherwise takes its course: the launches are the same, nothing
// faults or waits, the upper triangle then holds inf / NaN.
template <typename T>
static int potri_dev(lsx_handle_t h, int n, T *U, int lda, int *d_info) {
    LSX_ARG(h && n >= 0 && lda >= n);
    h->potri_tiles = 0;
    if (n == 0) return LSX_OK;
    LSX_ARG(U);
    const int ldw = ld_for(n);
    T *V = nullptr;
    LSX_TRY(carve(h, h->getri_work, [&](Carver &c) { V = c.take<T>((size_t)n * ldw); }));
    if (d_info) LSX_TRY(launch_diag_zero_info<T>(h, n, U, lda, d_info));
    LSX_TRY(trtri_upper_t<T>(h, n, U, lda, V, ldw));
    return launch_lauum_tn<T>(h, n, V, ldw, U, lda, h->potri_order, true);
}

template <typename T>
static int symmetrize_upper_dev(lsx_handle_t h, int n, T *dA, int lda) {
    LSX_ARG(h && n >= 0 && lda >= n);
    if (n == 0) return LSX_OK;
    LSX_ARG(dA);
    return launch_symmetrize_upper<T>(h, n, dA, lda);
}

// det(A) = prod u_ii^2 as {sign, mant, exp2} (lsx_det_*_dev's format): det_kernel's frexp product, the pair squared
template <typename T>
static int podet_dev(lsx_handle_t h, int n, const T *dU, int lda, double *d_out) {
    LSX_ARG(h && n >= 0 && lda >= n && d_out && (n == 0 || dU));
    return launch_det<T>(h, n, dU, lda, nullptr, d_out, true);
}

template <typename T>
static int potri_host(lsx_handle_t h, int n, T *U, int lda, int *info) {
    LSX_ARG(h && n >= 0 && lda >= n);
    if (n == 0) return LSX_OK;
    LSX_ARG(U);
    if (info) *info = 0;
    const int ld = ld_for(n);
    T *dU = nullptr; int *dinfo = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) { dU = c.take<T>((size_t)n * ld); dinfo = c.take<int>(1); }));
    int hinfo = 0;
    LSX_TRY(upper_h2d<T>(h, n, U, lda, dU, ld));
    LSX_TRY(potri_dev<T>(h, n, dU, ld, dinfo));
    LSX_HIP(hipMemcpyAsync(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LSX_TRY(upper_d2h<T>(h, n, dU, ld, U, lda));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = hinfo;
    return LSX_OK;
}

// factor, invert, mirror: A is kept, Ainv receives both triangles
template <typename T>
static int poinv_host(lsx_handle_t h, int n, const T *A, int lda, T *Ainv, int ldi, int *info) {
    LSX_ARG(h && n >= 0 && lda >= n && ldi >= n);
    if (n == 0) return LSX_OK;
    LSX_ARG(A && Ainv);
    if (info) *info = 0;
    const int ld = ld_for(n);
    T *dA = nullptr; int *dinfo = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) { dA = c.take<T>((size_t)n * ld); dinfo = c.take<int>(1); }));
    int hinfo = 0;
    LSX_TRY(upper_h2d<T>(h, n, A, lda, dA, ld));
    LSX_TRY(potrf_dev<T>(h, n, dA, ld, dinfo));
    LSX_HIP(hipMemcpyAsync(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = hinfo;
    if (hinfo != 0) return LSX_OK;   // not positive definite: Ainv is left untouched
    LSX_TRY(potri_dev<T>(h, n, dA, ld, nullptr));   // u_ii > 0 after a clean factorisation
    LSX_TRY(launch_symmetrize_upper<T>(h, n, dA, ld));
    LSX_TRY(d2h<T>(h, n, n, dA, ld, Ainv, ldi));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

template <typename T>
static int podet_host(lsx_handle_t h, int n, const T *A, int lda, double *sign, double *mant, int64_t *exp2, int *info) {
    LSX_ARG(h && n >= 0 && lda >= n && sign && mant && exp2);
    if (info) *info = 0;
    if (n == 0) { *sign = 1; *mant = 0.5; *exp2 = 1; return LSX_OK; }   // det([]) = 1, as lsx_det_*
    LSX_ARG(A);
    const int ld = ld_for(n);
    T *dA = nullptr; int *dinfo = nullptr; double *dout = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) { dA = c.take<T>((size_t)n * ld); dinfo = c.take<int>(1); dout = c.take<double>(3); }));
    int hinfo = 0;
    LSX_TRY(upper_h2d<T>(h, n, A, lda, dA, ld));
    LSX_TRY(potrf_dev<T>(h, n, dA, ld, dinfo));
    LSX_HIP(hipMemcpyAsync(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LSX_TRY(launch_det<T>(h, n, dA, ld, nullptr, dout, true));
    double out[3];
    LSX_HIP(hipMemcpyAsync(out, dout, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = hinfo;
    if (hinfo != 0) { *sign = 0; *mant = 0; *exp2 = 0; return LSX_OK; }   // not positive definite: no value
    *sign = out[0]; *mant = out[1]; *exp2 = (int64_t)out[2];
    return LSX_OK;
}

// ---------------------------------------------------------------- Householder QR: A = Q R, row-major (kernels_qr.hip)
// Right-looking over 128-column panels on one stream, no look-ahead, nothing cooperative:
//   panel kb: columns [kb, kb + jb), rows [kb, m): jb + 1 launches over row slabs                     [PANEL]
//   V (explicit ones and zeros), G = V^T V on the TN tile, T from G and tau (dlarft)                 [TRSM]
//   block apply  W = V^T C,  W <- T^T W (Q^T) or T W (Q),  C -= V W  on the existing tiles           [GEMM]
// geqrf applies Q^T of a panel to the columns right of it; ormqr and orgqr form V and T again per block from the
// factored array and tau, as LAPACK does.  qr_work is laid out here, from its start, by whoever runs blocks.
// The products with V^T (G = V^T V, W = V^T C) run over all rows of the panel, and the TN tile adds them in one
// accumulator of the working precision.  Above QR_KSPLIT_MIN rows the depth is cut into pieces of QR_KCHUNK rows, each
// piece a product of its own, and the pieces are added in fp64 (qr_vt_times): 16386 rows as one running sum put the
// orthogonality and least-squares ratios of a 16514 x 130 U(-1, 1) matrix at 4 times LAPACK's.  Panels
// of at most QR_KSPLIT_MIN rows are computed as before, bit for bit.  The pieces take 128 / QR_KCHUNK of C's size.
constexpr int QR_KSPLIT_MIN = 4096, QR_KCHUNK = 1024;
static int qr_parts(int mp) { return mp > QR_KSPLIT_MIN ? (mp + QR_KCHUNK - 1) / QR_KCHUNK : 1; }
template <typename T>
struct QrWork {
    T *V = nullptr, *G = nullptr, *Tm = nullptr, *Tt = nullptr, *W = nullptr, *W2 = nullptr, *prow = nullptr, *parts = nullptr;
    double *slots = nullptr;
    int ldw = 0, pcols = 0;   // pcols: columns (and leading dimension) of a piece, a multiple of 128
};
template <typename T>
static int carve_qr(lsx_handle_t h, int m, int nc, QrWork<T> *w) {
    w->ldw = ld_for(nc > 0 ? nc : 1);
    const int np = qr_parts(m);
    if (np > 1) w->pcols = ((nc > 128 ? nc : 128) + 127) / 128 * 128;   // G = V^T V has 128 columns
    return carve(h, h->qr_work, [&](Carver &c) {
        w->V = c.take<T>((size_t)m * 128);
        w->G = c.take<T>((size_t)128 * 128);
        w->Tm = c.take<T>((size_t)128 * 128);
        w->Tt = c.take<T>((size_t)128 * 128);
        w->W = c.take<T>((size_t)128 * w->ldw);
        w->W2 = c.take<T>((size_t)128 * w->ldw);
        w->prow = c.take<T>((size_t)2 * 128);
        w->slots = c.take<double>(qr_slot_elems());
        if (np > 1) w->parts = c.take<T>((size_t)np * 128 * w->pcols);
    });
}
// out (jb x nc) = V^T B for the mp x 128 V of the block and B (mp x nc)
template <typename T>
static int qr_vt_times(lsx_handle_t h, int jb, int nc, int mp, const QrWork<T> &w, const T *B, int ldb, T *out, int ldo,
                       int bucket) {
    const int np = qr_parts(mp);
    if (np == 1) return launch_gemm_tn_acc<T>(h, 3, jb, nc, mp, w.V, 128, B, ldb, out, ldo, bucket);
    if (!w.parts || nc > w.pcols) {
        set_error("qr: no room for the partial products of %d rows, %d columns", mp, nc);
        return LSX_ERR_INTERNAL;
    }
    for (int p = 0; p < np; ++p) {
        const int r0 = p * QR_KCHUNK, rows = mp - r0 < QR_KCHUNK ? mp - r0 : QR_KCHUNK;
        LSX_TRY(launch_gemm_tn_acc<T>(h, 3, jb, nc, rows, w.V + (size_t)r0 * 128, 128, B + (size_t)r0 * ldb, ldb,
                                      w.parts + (size_t)p * 128 * w.pcols, w.pcols, bucket));
    }
    return launch_qr_sum_parts<T>(h, jb, nc, np, w.parts, w.pcols, (size_t)128 * w.pcols, out, ldo);
}
// V and T of the block whose reflectors lie below the diagonal of P (mp x jb) with scalars tau
template <typename T>
static int qr_block_form(lsx_handle_t h, int mp, int jb, const T *P, int ldp, const T *tau, const QrWork<T> &w) {
    LSX_TRY(launch_qr_extract_v<T>(h, mp, jb, P, ldp, w.V));
    LSX_TRY(qr_vt_times<T>(h, jb, jb, mp, w, w.V, 128, w.G, 128, LSX_PROF_TRSM));
    return launch_qr_larft<T>(h, jb, w.G, tau, w.Tm, w.Tt);
}
// C (mp x nc) <- H^T C (trans) or H C, H = I - V T V^T
template <typename T>
static int qr_block_apply(lsx_handle_t h, int trans, int mp, int jb, int nc, const QrWork<T> &w, T *C, int ldc) {
    LSX_TRY(qr_vt_times<T>(h, jb, nc, mp, w, C, ldc, w.W, w.ldw, LSX_PROF_GEMM));
    LSX_TRY(launch_gemm_tn_acc<T>(h, 3, jb, nc, jb, trans ? w.Tm : w.Tt, 128, w.W, w.ldw, w.W2, w.ldw));
    return launch_gemm_sub<T>(h, mp, nc, jb, w.V, 128, w.W2, w.ldw, C, ldc);
}

template <typename T>
static int geqrf_dev(lsx_handle_t h, int m, int n, T *A, int lda, T *d_tau) {
    LSX_ARG(h && m >= 0 && n >= 0 && lda >= n);
    const int k = m < n ? m : n;
    if (k == 0) return LSX_OK;
    LSX_ARG(A && d_tau);
    QrWork<T> w;
    LSX_TRY(carve_qr<T>(h, m, n, &w));
    for (int kb = 0; kb < k; kb += 128) {
        const int jb = (k - kb < 128) ? k - kb : 128, mp = m - kb, rest = n - kb - jb;
        T *P = A + (size_t)kb * lda + kb;
        LSX_TRY(launch_qr_panel<T>(h, mp, jb, P, lda, d_tau + kb, w.slots, w.prow));
        if (rest <= 0) continue;
        LSX_TRY(qr_block_form<T>(h, mp, jb, P, lda, d_tau + kb, w));
        LSX_TRY(qr_block_apply<T>(h, 1, mp, jb, rest, w, P + jb, lda));
    }
    return LSX_OK;
}

// C (m x ncols) <- Q^T C (trans = 1: the blocks forward) or Q C (trans = 0: backward), Q = H_0 .. H_{k-1}
template <typename T>
static int ormqr_dev(lsx_handle_t h, int trans, int m, int ncols, int k, const T *QR, int lda, const T *d_tau, T *C, int ldc) {
    LSX_ARG(h && (trans == 0 || trans == 1) && m >= 0 && ncols >= 0 && k >= 0 && k <= m && lda >= k && ldc >= ncols);
    if (m == 0 || ncols == 0 || k == 0) return LSX_OK;
    LSX_ARG(QR && d_tau && C);
    QrWork<T> w;
    LSX_TRY(carve_qr<T>(h, m, ncols, &w));
    const int last = (k - 1) / 128 * 128;
    for (int b = 0; b <= last; b += 128) {
        const int kb = trans ? b : last - b;
        const int jb = (k - kb < 128) ? k - kb : 128, mp = m - kb;
        LSX_TRY(qr_block_form<T>(h, mp, jb, QR + (size_t)kb * lda + kb, lda, d_tau + kb, w));
        LSX_TRY(qr_block_apply<T>(h, trans, mp, jb, ncols, w, C + (size_t)kb * ldc, ldc));
    }
    return LSX_OK;
}

// the thin Q (m x n, k <= n <= m), out of place: Q applied to the leading columns of the identity
template <typename T>
static int orgqr_dev(lsx_handle_t h, int m, int n, int k, const T *QR, int lda, const T *d_tau, T *Q, int ldq) {
    LSX_ARG(h && m >= 0 && n >= 0 && k >= 0 && k <= n && n <= m && lda >= k && ldq >= n);
    if (m == 0 || n == 0) return LSX_OK;
    LSX_ARG(Q && (k == 0 || (QR && d_tau)));
    LSX_TRY(launch_qr_identity<T>(h, m, n, Q, ldq));
    return ormqr_dev<T>(h, 0, m, n, k, QR, lda, d_tau, Q, ldq);
}

template <typename T>
static int colnrm2_dev(lsx_handle_t h, int m, int n, const T *dA, int lda, double *d_out) {
    LSX_ARG(h && m >= 0 && n >= 0 && lda >= n);
    if (m == 0 || n == 0) return LSX_OK;
    LSX_ARG(dA && d_out);
    return launch_colnrm2<T>(h, m, n, dA, lda, d_out);
}

// min ||b - A x||_2 for m >= n: geqrf, Q^T B, the info word (the first r_ii that is zero or NaN), then R X = (Q^T B)[0:n]
// in place on the leading rows of B: the block inverses of R come from its upper triangle alone (launch_chol_inv), and
// sweep_backward reads the blocks on and above the diagonal blocks only -- what lies below the diagonal is V.
template <typename T>
static int gels_dev(lsx_handle_t h, int m, int n, int nrhs, T *A, int lda, T *d_tau, T *B, int ldb, int *d_info) {
    LSX_ARG(h && m >= 0 && n >= 0 && nrhs >= 0 && m >= n && lda >= n && ldb >= nrhs);
    if (n == 0 || nrhs == 0) return LSX_OK;
    LSX_ARG(A && d_tau && B);
    LSX_TRY(geqrf_dev<T>(h, m, n, A, lda, d_tau));
    LSX_TRY(ormqr_dev<T>(h, 1, m, nrhs, n, A, lda, d_tau, B, ldb));
    if (d_info) LSX_TRY(launch_diag_zero_info<T>(h, n, A, lda, d_info));
    T *inv64 = nullptr, *inv128 = nullptr;
    LSX_TRY(carve(h, h->tinv, [&](Carver &c) { inv64 = c.take<T>(inv64_elems(n)); inv128 = c.take<T>(inv128_elems(n)); }));
    LSX_TRY(launch_chol_inv<T>(h, n, A, lda, inv64, inv128));
    return sweep_backward<T>(h, n, nrhs, sweep_pairs(h, n, nrhs), A, lda, inv64, B, ldb);
}

template <typename T>
static int geqrf_host(lsx_handle_t h, int m, int n, T *A, int lda, T *tau) {
    LSX_ARG(h && m >= 0 && n >= 0 && lda >= n);
    const int k = m < n ? m : n;
    if (k == 0) return LSX_OK;
    LSX_ARG(A && tau);
    const int ld = ld_for(n);
    T *dA = nullptr, *dtau = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) { dA = c.take<T>((size_t)m * ld); dtau = c.take<T>(k); }));
    LSX_TRY(h2d<T>(h, m, n, A, lda, dA, ld));
    LSX_TRY(geqrf_dev<T>(h, m, n, dA, ld, dtau));
    LSX_TRY(d2h<T>(h, m, n, dA, ld, A, lda));
    LSX_HIP(hipMemcpyAsync(tau, dtau, sizeof(T) * k, hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

template <typename T>
static int ormqr_host(lsx_handle_t h, int trans, int m, int ncols, int k, const T *QR, int lda, const T *tau, T *C, int ldc) {
    LSX_ARG(h && (trans == 0 || trans == 1) && m >= 0 && ncols >= 0 && k >= 0 && k <= m && lda >= k && ldc >= ncols);
    if (m == 0 || ncols == 0 || k == 0) return LSX_OK;
    LSX_ARG(QR && tau && C);
    const int ld = ld_for(k), ldx = ld_for(ncols);
    T *dQR = nullptr, *dtau = nullptr, *dC = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dQR = c.take<T>((size_t)m * ld);
        dtau = c.take<T>(k);
        dC = c.take<T>((size_t)m * ldx);
    }));
    LSX_TRY(h2d<T>(h, m, k, QR, lda, dQR, ld));
    LSX_HIP(hipMemcpyAsync(dtau, tau, sizeof(T) * k, hipMemcpyHostToDevice, h->stream));
    LSX_TRY(h2d<T>(h, m, ncols, C, ldc, dC, ldx));
    LSX_TRY(ormqr_dev<T>(h, trans, m, ncols, k, dQR, ld, dtau, dC, ldx));
    LSX_TRY(d2h<T>(h, m, ncols, dC, ldx, C, ldc));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

template <typename T>
static int orgqr_host(lsx_handle_t h, int m, int n, int k, const T *QR, int lda, const T *tau, T *Q, int ldq) {
    LSX_ARG(h && m >= 0 && n >= 0 && k >= 0 && k <= n && n <= m && lda >= k && ldq >= n);
    if (m == 0 || n == 0) return LSX_OK;
    LSX_ARG(Q && (k == 0 || (QR && tau)));
    const int ld = ld_for(k > 0 ? k : 1), ldx = ld_for(n);
    T *dQR = nullptr, *dtau = nullptr, *dQ = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dQR = c.take<T>((size_t)m * ld);
        dtau = c.take<T>(k > 0 ? k : 1);
        dQ = c.take<T>((size_t)m * ldx);
    }));
    if (k > 0) {
        LSX_TRY(h2d<T>(h, m, k, QR, lda, dQR, ld));
        LSX_HIP(hipMemcpyAsync(dtau, tau, sizeof(T) * k, hipMemcpyHostToDevice, h->stream));
    }
    LSX_TRY(orgqr_dev<T>(h, m, n, k, dQR, ld, dtau, dQ, ldx));
    LSX_TRY(d2h<T>(h, m, n, dQ, ldx, Q, ldq));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

// A and B are not modified; X (n x nrhs) and resid[nrhs] (may be NULL) are written only when info == 0
template <typename T>
static int gels_host(lsx_handle_t h, int m, int n, int nrhs, const T *A, int lda, const T *B, int ldb, T *X, int ldx,
                     double *resid, int *info) {
    LSX_ARG(h && m >= 0 && n >= 0 && nrhs >= 0 && m >= n && lda >= n && ldb >= nrhs && ldx >= nrhs);
    if (info) *info = 0;
    if (n == 0 || nrhs == 0) return LSX_OK;
    LSX_ARG(A && B && X);
    const int ld = ld_for(n), ldr = ld_for(nrhs);
    T *dA = nullptr, *dtau = nullptr, *dB = nullptr; int *dinfo = nullptr; double *dres = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)m * ld);
        dtau = c.take<T>(n);
        dB = c.take<T>((size_t)m * ldr);
        dinfo = c.take<int>(1);
        dres = c.take<double>(nrhs);
    }));
    int hinfo = 0;
    LSX_TRY(h2d<T>(h, m, n, A, lda, dA, ld));
    LSX_TRY(h2d<T>(h, m, nrhs, B, ldb, dB, ldr));
    LSX_TRY(gels_dev<T>(h, m, n, nrhs, dA, ld, dtau, dB, ldr, dinfo));
    LSX_HIP(hipMemcpyAsync(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = hinfo;
    if (hinfo != 0) {
        if (resid) for (int j = 0; j < nrhs; ++j) resid[j] = INFINITY;
        return LSX_OK;
    }
    LSX_TRY(d2h<T>(h, n, nrhs, dB, ldr, X, ldx));
    if (resid) {
        if (m > n) {
            LSX_TRY(colnrm2_dev<T>(h, m - n, nrhs, dB + (size_t)n * ldr, ldr, dres));
            LSX_HIP(hipMemcpyAsync(resid, dres, sizeof(double) * nrhs, hipMemcpyDeviceToHost, h->stream));
        } else {
            for (int j = 0; j < nrhs; ++j) resid[j] = 0.0;
        }
    }
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

// ---------------------------------------------------------------- one-sided Jacobi SVD: A = U diag(s) V^T (kernels_svd.hip)
// The rows of the work matrix W (p x q, p = min(m, n), q = n) are made mutually orthogonal by plane rotations, Z (p x p,
// the identity to begin with) receives the same rotations:  W = Z A (m <= n) or W = Z R with A = Q R (m > n: geqrf_dev
// first, so that the iteration runs on n x n).  Then s_i = ||w_i||_2, row i of V^T = w_i / s_i, and U = Z^T or
// Q [Z^T; 0] (ormqr_dev on the caller's U, whose rows below n the gather has zeroed).
//   a sweep = P - 1 rounds of the round-robin order, one launch each, pairs of a round disjoint           [PANEL]
//   row norms, the sorted gather of s, U, V^T, gelss's row scaling                                        [OTHER]
//   gelss: Y = U^T B and X = (V^T)^T Y on the TN tile                                                     [GEMM]
// The host reads the rotation counter once per sweep and the row norms before the first sweep (a NaN or infinity in A
// ends the call there: s all NaN, nothing iterates) and after the last one, so every form synchronises the stream.
// svd_work is laid out once per call, here; geqrf_dev and ormqr_dev keep qr_work to themselves.
template <typename T>
struct SvdWork {
    T *W = nullptr, *Z = nullptr, *tau = nullptr;
    double *sigma = nullptr;
    int *perm = nullptr, *count = nullptr;
    int ldw = 0, ldz = 0;
    // gelss only (nrhs > 0): the factors, the values in order, and Y = U^T B
    T *U = nullptr, *Vt = nullptr, *Y = nullptr;
    double *s = nullptr;
    int ldu = 0, ldvt = 0, ldy = 0;
};
template <typename T>
static int carve_svd(lsx_handle_t h, int m, int n, int jobz, int nrhs, SvdWork<T> *w) {
    const int k = m < n ? m : n;
    w->ldw = svd_ld(n, sizeof(T));
    w->ldz = svd_ld(k, sizeof(T));
    w->ldu = ld_for(k); w->ldvt = ld_for(n); w->ldy = ld_for(nrhs > 0 ? nrhs : 1);
    return carve(h, h->svd_work, [&](Carver &c) {
        w->W = c.take<T>((size_t)k * w->ldw);
        if (jobz) w->Z = c.take<T>((size_t)k * w->ldz);
        w->sigma = c.take<double>(k);
        w->perm = c.take<int>(k);
        w->count = c.take<int>(1);
        if (m > n) w->tau = c.take<T>(n);
        if (nrhs > 0) {
            w->U = c.take<T>((size_t)m * w->ldu);
            w->Vt = c.take<T>((size_t)k * w->ldvt);
            w->Y = c.take<T>((size_t)k * w->ldy);
            w->s = c.take<double>(k);
        }
    });
}

// The call on a carved work space; A (m x n, k = min(m, n) > 0) is destroyed.  s_host receives the k values in order (all
// NaN for an input that is not finite).  Synchronises the stream.
template <typename T>
static int gesvdj_run(lsx_handle_t h, const SvdWork<T> &w, int jobz, int m, int n, T *A, int lda, double *d_s, T *U, int ldu,
                      T *Vt, int ldvt, int *info, std::vector<double> *s_host) {
    const int k = m < n ? m : n, p = k, q = n;
    const bool tall = m > n;
    h->gesvdj_sweeps = 0;
    h->gesvdj_rotations = 0;
    if (tall) LSX_TRY(geqrf_dev<T>(h, m, n, A, lda, w.tau));
    LSX_TRY(launch_svd_init<T>(h, p, q, A, lda, tall ? 1 : 0, w.W, w.ldw));
    if (jobz) LSX_TRY(launch_svd_init<T>(h, p, p, (const T *)nullptr, 0, 0, w.Z, w.ldz));
    std::vector<double> sig(k);
    auto norms = [&](bool *finite) -> int {
        LSX_TRY(launch_svd_rownorm<T>(h, p, q, w.W, w.ldw, w.sigma));
        LSX_HIP(hipMemcpyAsync(sig.data(), w.sigma, sizeof(double) * k, hipMemcpyDeviceToHost, h->stream));
        LSX_HIP(hipStreamSynchronize(h->stream));
        *finite = true;
        for (double v : sig) *finite = *finite && std::isfinite(v);
        return LSX_OK;
    };
    bool finite = true;
    LSX_TRY(norms(&finite));
    int last = 0;
    if (finite) {
        const double tol = sqrt((double)q) * (0.5 * (double)Real<T>::eps);
        const int P = p + (p & 1);
        long long total = 0;
        for (int sweep = 1; sweep <= h->gesvdj_max_sweeps; ++sweep) {
            LSX_HIP(hipMemsetAsync(w.count, 0, sizeof(int), h->stream));
            for (int r = 0; r < P - 1; ++r) LSX_TRY(launch_svd_round<T>(h, p, q, r, w.W, w.ldw, jobz ? w.Z : (T *)nullptr, w.ldz, tol, w.count));
            LSX_HIP(hipMemcpyAsync(&last, w.count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
            LSX_HIP(hipStreamSynchronize(h->stream));
            h->gesvdj_sweeps = sweep;
            total += last;
            if (last == 0) break;
        }
        h->gesvdj_rotations = total > INT_MAX ? INT_MAX : (int)total;
        LSX_TRY(norms(&finite));
    }
    if (info) *info = (finite && last != 0) ? 1 : 0;
    if (!finite) {
        LSX_TRY(launch_svd_fill<double>(h, 1, k, (double)NAN, d_s, k));
        if (s_host) s_host->assign(k, (double)NAN);
        LSX_HIP(hipStreamSynchronize(h->stream));
        return LSX_OK;
    }
    std::vector<int> perm(k);
    for (int i = 0; i < k; ++i) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return sig[a] > sig[b]; });
    LSX_HIP(hipMemcpyAsync(w.perm, perm.data(), sizeof(int) * k, hipMemcpyHostToDevice, h->stream));
    LSX_TRY(launch_svd_gather<T>(h, k, q, m, w.W, w.ldw, w.Z, w.ldz, w.sigma, w.perm, d_s, jobz ? Vt : (T *)nullptr, ldvt,
                                 jobz ? U : (T *)nullptr, ldu));
    if (jobz && tall) LSX_TRY(ormqr_dev<T>(h, 0, m, k, n, A, lda, w.tau, U, ldu));
    if (s_host) {
        s_host->resize(k);
        for (int i = 0; i < k; ++i) (*s_host)[i] = sig[perm[i]];
    }
    LSX_HIP(hipStreamSynchronize(h->stream));   // perm is read by the upload
    return LSX_OK;
}

template <typename T>
static int gesvdj_dev(lsx_handle_t h, int jobz, int m, int n, T *A, int lda, double *d_s, T *U, int ldu, T *Vt, int ldvt,
                      int *info) {
    LSX_ARG(h && (jobz == 0 || jobz == 1) && m >= 0 && n >= 0 && lda >= n);
    const int k = m < n ? m : n;
    LSX_ARG(!jobz || (ldu >= k && ldvt >= n));
    if (info) *info = 0;
    if (k == 0) return LSX_OK;
    LSX_ARG(A && d_s && (!jobz || (U && Vt)));
    SvdWork<T> w;
    LSX_TRY(carve_svd<T>(h, m, n, jobz, 0, &w));
    return gesvdj_run<T>(h, w, jobz, m, n, A, lda, d_s, U, ldu, Vt, ldvt, info, nullptr);
}

// Minimum-norm least squares through the SVD: X = V diag(1 / s_i, i < rank) U^T B; A is destroyed, B is kept.
template <typename T>
static int gelss_dev(lsx_handle_t h, int m, int n, int nrhs, T *A, int lda, const T *B, int ldb, T *X, int ldx, double rcond,
                     double *d_s, int *rank, int *info) {
    LSX_ARG(h && m >= 0 && n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs && ldx >= nrhs);
    if (info) *info = 0;
    if (rank) *rank = 0;
    if (m == 0 || n == 0 || nrhs == 0) return LSX_OK;
    LSX_ARG(A && B && X);
    const int k = m < n ? m : n;
    SvdWork<T> w;
    LSX_TRY(carve_svd<T>(h, m, n, 1, nrhs, &w));
    std::vector<double> s;
    LSX_TRY(gesvdj_run<T>(h, w, 1, m, n, A, lda, w.s, w.U, w.ldu, w.Vt, w.ldvt, info, &s));
    if (d_s) LSX_HIP(hipMemcpyAsync(d_s, w.s, sizeof(double) * k, hipMemcpyDeviceToDevice, h->stream));
    if (std::isnan(s[0])) {   // an input that is not finite: no solution to speak of
        LSX_TRY(launch_svd_fill<T>(h, n, nrhs, (T)NAN, X, ldx));
        LSX_HIP(hipStreamSynchronize(h->stream));
        return LSX_OK;
    }
    const double thr = (rcond < 0.0 ? (double)(m > n ? m : n) * (0.5 * (double)Real<T>::eps) : rcond) * s[0];
    int rk = 0;
    while (rk < k && s[rk] > thr) ++rk;
    if (rank) *rank = rk;
    LSX_TRY(launch_gemm_tn_acc<T>(h, 3, k, nrhs, m, w.U, w.ldu, B, ldb, w.Y, w.ldy));
    LSX_TRY(launch_svd_scale_rows<T>(h, k, nrhs, rk, w.s, w.Y, w.ldy));
    LSX_TRY(launch_gemm_tn_acc<T>(h, 3, n, nrhs, k, w.Vt, w.ldvt, w.Y, w.ldy, X, ldx));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

template <typename T>
static int gesvdj_host(lsx_handle_t h, int jobz, int m, int n, const T *A, int lda, double *s, T *U, int ldu, T *Vt, int ldvt,
                       int *info) {
    LSX_ARG(h && (jobz == 0 || jobz == 1) && m >= 0 && n >= 0 && lda >= n);
    const int k = m < n ? m : n;
    LSX_ARG(!jobz || (ldu >= k && ldvt >= n));
    if (info) *info = 0;
    if (k == 0) return LSX_OK;
    LSX_ARG(A && s && (!jobz || (U && Vt)));
    const int ld = ld_for(n), lu = ld_for(k);
    T *dA = nullptr, *dU = nullptr, *dVt = nullptr; double *ds = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)m * ld);
        ds = c.take<double>(k);
        if (jobz) { dU = c.take<T>((size_t)m * lu); dVt = c.take<T>((size_t)k * ld); }
    }));
    LSX_TRY(h2d<T>(h, m, n, A, lda, dA, ld));
    LSX_TRY(gesvdj_dev<T>(h, jobz, m, n, dA, ld, ds, dU, lu, dVt, ld, info));
    LSX_HIP(hipMemcpyAsync(s, ds, sizeof(double) * k, hipMemcpyDeviceToHost, h->stream));
    if (jobz) {
        LSX_TRY(d2h<T>(h, m, k, dU, lu, U, ldu));
        LSX_TRY(d2h<T>(h, k, n, dVt, ld, Vt, ldvt));
    }
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

// A and B are not modified; X is n x nrhs; s (k values), resid (nrhs) may be NULL
template <typename T>
static int gelss_host(lsx_handle_t h, int m, int n, int nrhs, const T *A, int lda, const T *B, int ldb, T *X, int ldx,
                      double rcond, double *s, double *resid, int *rank, int *info) {
    LSX_ARG(h && m >= 0 && n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs && ldx >= nrhs);
    if (info) *info = 0;
    if (rank) *rank = 0;
    if (m == 0 || n == 0 || nrhs == 0) return LSX_OK;
    LSX_ARG(A && B && X);
    const int k = m < n ? m : n, ld = ld_for(n), ldr = ld_for(nrhs);
    T *dA = nullptr, *dA2 = nullptr, *dB = nullptr, *dX = nullptr; double *ds = nullptr, *dres = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)m * ld);
        if (resid) dA2 = c.take<T>((size_t)m * ld);
        dB = c.take<T>((size_t)m * ldr);
        dX = c.take<T>((size_t)n * ldr);
        ds = c.take<double>(k);
        dres = c.take<double>(nrhs);
    }));
    LSX_TRY(h2d<T>(h, m, n, A, lda, dA, ld));
    if (resid) LSX_TRY(h2d<T>(h, m, n, A, lda, dA2, ld));
    LSX_TRY(h2d<T>(h, m, nrhs, B, ldb, dB, ldr));
    LSX_TRY(gelss_dev<T>(h, m, n, nrhs, dA, ld, dB, ldr, dX, ldr, rcond, ds, rank, info));
    LSX_TRY(d2h<T>(h, n, nrhs, dX, ldr, X, ldx));
    if (s) LSX_HIP(hipMemcpyAsync(s, ds, sizeof(double) * k, hipMemcpyDeviceToHost, h->stream));
    if (resid) {   // ||b - A x||_2 on the update tile: B <- B - A X, then its column norms
        LSX_TRY(launch_gemm_sub<T>(h, m, nrhs, n, dA2, ld, dX, ldr, dB, ldr));
        LSX_TRY(colnrm2_dev<T>(h, m, nrhs, dB, ldr, dres));
        LSX_HIP(hipMemcpyAsync(resid, dres, sizeof(double) * nrhs, hipMemcpyDeviceToHost, h->stream));
    }
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

// ---------------------------------------------------------------- two-sided Jacobi: A = V diag(w) V^T (kernels_eig.hip)
// The work matrix W (n x n, both triangles, from the upper triangle of A) is driven to diagonal form by plane rotations
// W <- G W G^T; Z (the identity to begin with) receives the row rotations, so W = Z A Z^T, the eigenvalues are the
// diagonal of W and the eigenvectors the rows of Z.
//   a sweep = P - 1 rounds of the round-robin order; a round = one decision launch [OTHER] and one rotation launch [PANEL]
//   the work matrix, ||A||_F, the diagonal, the sorted gather of w and V (svd_gather_kernel)                 [OTHER]
// The host reads ||A||_F before the first sweep (a NaN or infinity ends the call there: w all NaN, nothing iterates), the
// rotation counter once per sweep and the diagonal after the last one, so every form synchronises the stream.
// eig_work is laid out once per call, here; nothing called from here carves anything.
template <typename T>
struct EigWork {
    T *W = nullptr, *Z = nullptr;
    double *rowsq = nullptr, *nrm = nullptr, *diag = nullptr;
    int *perm = nullptr, *count = nullptr;
    EigRound round;
    int ldw = 0;
};
template <typename T>
static int carve_eig(lsx_handle_t h, int n, int jobz, EigWork<T> *w) {
    const int np = (n + (n & 1)) / 2;
    w->ldw = svd_ld(n, sizeof(T));
    return carve(h, h->eig_work, [&](Carver &c) {
        w->W = c.take<T>((size_t)n * w->ldw);
        if (jobz) w->Z = c.take<T>((size_t)n * w->ldw);
        w->rowsq = c.take<double>(n);
        w->nrm = c.take<double>(1);
        w->diag = c.take<double>(n);
        w->perm = c.take<int>(n);
        w->count = c.take<int>(1);
        w->round.pair = c.take<int2>(np);
        w->round.rot = c.take<double2>(np);
        w->round.flag = c.take<int>(np);
    });
}

// dA is only read (its upper triangle); d_w: n doubles on the device, ascending; column i of V belongs to d_w[i]
template <typename T>
static int syevj_dev(lsx_handle_t h, int jobz, int n, const T *A, int lda, double *d_w, T *V, int ldv, int *info) {
    LSX_ARG(h && (jobz == 0 || jobz == 1) && n >= 0 && lda >= n && (!jobz || ldv >= n));
    if (info) *info = 0;
    if (n == 0) return LSX_OK;
    LSX_ARG(A && d_w && (!jobz || V));
    EigWork<T> w;
    LSX_TRY(carve_eig<T>(h, n, jobz, &w));
    h->syevj_sweeps = 0;
    h->syevj_rotations = 0;
    LSX_TRY(launch_eig_init<T>(h, n, A, lda, w.W, w.ldw));
    if (jobz) LSX_TRY(launch_svd_init<T>(h, n, n, (const T *)nullptr, 0, 0, w.Z, w.ldw));
    LSX_TRY(launch_eig_norm<T>(h, n, w.W, w.ldw, w.rowsq, w.nrm));
    double nrm = 0.0;
    LSX_HIP(hipMemcpyAsync(&nrm, w.nrm, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    std::vector<double> diag(n);
    bool finite = std::isfinite(nrm);
    int last = 0;
    if (finite) {
        const double thr = (0.5 * (double)Real<T>::eps) * nrm;
        const int P = n + (n & 1);
        long long total = 0;
        for (int sweep = 1; sweep <= h->syevj_max_sweeps; ++sweep) {
            LSX_HIP(hipMemsetAsync(w.count, 0, sizeof(int), h->stream));
            for (int r = 0; r < P - 1; ++r) {
                LSX_TRY(launch_eig_decide<T>(h, n, r, w.W, w.ldw, thr, w.round, w.count));
                LSX_TRY(launch_eig_round<T>(h, n, w.W, w.ldw, w.Z, w.ldw, w.round));
            }
            LSX_HIP(hipMemcpyAsync(&last, w.count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
            LSX_HIP(hipStreamSynchronize(h->stream));
            h->syevj_sweeps = sweep;
            total += last;
            if (last == 0) break;
        }
        h->syevj_rotations = total > INT_MAX ? INT_MAX : (int)total;
        LSX_TRY(launch_eig_diag<T>(h, n, w.W, w.ldw, w.diag));
        LSX_HIP(hipMemcpyAsync(diag.data(), w.diag, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
        LSX_HIP(hipStreamSynchronize(h->stream));
        for (double v : diag) finite = finite && !std::isnan(v);   // a sum that overflowed on the way
    }
    if (info) *info = (finite && last != 0) ? 1 : 0;
    if (!finite) {
        LSX_TRY(launch_svd_fill<double>(h, 1, n, (double)NAN, d_w, n));
        LSX_HIP(hipStreamSynchronize(h->stream));
        return LSX_OK;
    }
    std::vector<int> perm(n);
    for (int i = 0; i < n; ++i) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return diag[a] < diag[b]; });
    LSX_HIP(hipMemcpyAsync(w.perm, perm.data(), sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
    // w[i] = diag[perm[i]], V[r][i] = Z[perm[i]][r]: the SVD's gather with no V^T and U = V
    LSX_TRY(launch_svd_gather<T>(h, n, 0, n, w.W, w.ldw, w.Z, w.ldw, w.diag, w.perm, d_w, (T *)nullptr, 0, jobz ? V : (T *)nullptr, ldv));
    LSX_HIP(hipStreamSynchronize(h->stream));   // perm is read by the upload
    return LSX_OK;
}

// A is not modified: its upper triangle is staged (block rows from their diagonal block on)
template <typename T>
static int syevj_host(lsx_handle_t h, int jobz, int n, const T *A, int lda, double *wout, T *V, int ldv, int *info) {
    LSX_ARG(h && (jobz == 0 || jobz == 1) && n >= 0 && lda >= n && (!jobz || ldv >= n));
    if (info) *info = 0;
    if (n == 0) return LSX_OK;
    LSX_ARG(A && wout && (!jobz || V));
    const int ld = ld_for(n);
    T *dA = nullptr, *dV = nullptr; double *dw = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)n * ld);
        dw = c.take<double>(n);
        if (jobz) dV = c.take<T>((size_t)n * ld);
    }));
    LSX_TRY(upper_h2d<T>(h, n, A, lda, dA, ld));
    LSX_TRY(syevj_dev<T>(h, jobz, n, dA, ld, dw, dV, ld, info));
    LSX_HIP(hipMemcpyAsync(wout, dw, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    if (jobz) LSX_TRY(d2h<T>(h, n, n, dV, ld, V, ldv));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

// A^T X = B from the factors (kernels_trsvt.hip).  Work space as in getrs_dev, so the two share what they grow.
// may_block = false: the single-column solves inside the estimators, which keep the grouped path whatever the option says.
template <typename T>
static int getrs_t_dev(lsx_handle_t h, int n, int nrhs, const T *LU, int lda, const int32_t *d_ipiv, T *B, int ldb,
                       bool may_block = false) {
    LSX_ARG(n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs && LU && d_ipiv && B);
    if (may_block) h->getrs_t_path = 0;
    if (n == 0 || nrhs == 0) return LSX_OK;
    if (n <= 128)   // one workgroup, interchanges included: no work space
        return lu_solve_transposed<T>(h, n, nrhs, LU, lda, d_ipiv, nullptr, B, ldb, (T *)nullptr, (T *)nullptr,
                                      (T *)nullptr, (T *)nullptr, (T *)nullptr);
    // blocked path: two n x nrhs work arrays (ld = ldw) in place of the n x 8 work vector
    const bool blocked = may_block && h->getrs_t_blocked_min > 0 && nrhs >= h->getrs_t_blocked_min;
    const int ldw = ld_for(nrhs);
    int32_t *perm = nullptr; T *W = nullptr, *Y = nullptr;
    LSX_TRY(carve(h, h->rhs_work, [&](Carver &c) {
        perm = c.take<int32_t>(n);
        if (blocked) {
            W = c.take<T>((size_t)n * ldw);
            Y = c.take<T>((size_t)n * ldw);
        } else {   // all three n x 8 pieces of getrs_dev's few-column layout: the two solves grow rhs_work alike
            W = c.take<T>((size_t)n * 8);
            c.take<T>((size_t)n * 8);
            c.take<T>((size_t)n * 8);
        }
    }));
    BlockInv<T> bi;
    LSX_TRY(carve_block_inv<T>(h, n, &bi));
    LSX_TRY(launch_ipiv_to_perm(h, n, d_ipiv, perm));
    if (blocked) {
        LSX_TRY(launch_inv128_natural<T>(h, n, LU, lda, bi.inv64L, bi.inv64U, bi.inv128L, bi.inv128U));
        h->getrs_t_path = 1;
        return lu_solve_transposed_blocked<T>(h, n, nrhs, LU, lda, perm, B, ldb, (const T *)bi.inv128L,
                                              (const T *)bi.inv128U, W, Y, ldw);
    }
    return lu_solve_transposed<T>(h, n, nrhs, LU, lda, d_ipiv, perm, B, ldb, bi.inv64L, bi.inv64U, bi.inv128L, bi.inv128U, W);
}

template <typename T>
static int getrs_t_host(lsx_handle_t h, int n, int nrhs, const T *LU, int lda, const int32_t *ipiv, T *B, int ldb) {
    LSX_ARG(h && n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs);
    if (n == 0 || nrhs == 0) return LSX_OK;
    LSX_ARG(LU && ipiv && B);
    const int ld = ld_for(n), ldx = ld_for(nrhs);
    T *dA = nullptr, *dB = nullptr; int32_t *dp = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)n * ld);
        dB = c.take<T>((size_t)n * ldx);
        dp = c.take<int32_t>(n);
    }));
    LSX_TRY(h2d<T>(h, n, n, LU, lda, dA, ld));
    LSX_TRY(h2d<T>(h, n, nrhs, B, ldb, dB, ldx));
    LSX_HIP(hipMemcpyAsync(dp, ipiv, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
    LSX_TRY(getrs_t_dev<T>(h, n, nrhs, dA, ld, dp, dB, ldx, true));
    LSX_TRY(d2h<T>(h, n, nrhs, dB, ldx, B, ldb));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

template <typename T>
static int lange_dev(lsx_handle_t h, int norm, int m, int n, const T *dA, int lda, double *d_out) {
    LSX_ARG((norm == LSX_NORM_ONE || norm == LSX_NORM_INF) && m >= 0 && n >= 0 && lda >= n && d_out);
    LSX_ARG(m == 0 || n == 0 || dA);
    LSX_TRY(reserve(h, h->scratch, lange_work_bytes(norm, m, n) + 256));
    return launch_lange<T>(h, norm, m, n, dA, lda, (double *)h->scratch.p, d_out);
}

// lacn2's iteration (dlacn2.f, the states JUMP = 1..5) for the 1-norm of an operator M that is only available as
// apply(1): x <- M x and apply(2): x <- M^T x.  x holds the start vector 1/n on entry and isgn is cleared; the vector
// steps run on the device (kernels_trsvt.hip), the host reads the record (8 doubles at rec) after each and decides.
// Shared by the condition estimate (M = inv(A)) and the forward error bound of gerfs (M = diag(W) inv(op A)^T).
template <typename T, typename Apply>
static int lacn2_dev(lsx_handle_t h, int n, T *x, signed char *isgn, double *rec, Apply apply, double *est_out) {
    double r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto read = [&]() -> int {
        LSX_HIP(hipMemcpyAsync(r, rec, sizeof(r), hipMemcpyDeviceToHost, h->stream));
        LSX_HIP(hipStreamSynchronize(h->stream));
        return LSX_OK;
    };
    double est = 0;
    LSX_TRY(apply(1));
    LSX_TRY(launch_est_asum_sign<T>(h, n, x, isgn, rec));         // JUMP 1
    LSX_TRY(read());
    est = r[0];
    if (n > 1) {
        LSX_TRY(apply(2));
        LSX_TRY(launch_est_amax_unit<T>(h, n, x, -1, rec));       // JUMP 2: j, x <- e_j
        LSX_TRY(read());
        int j = (int)r[1];
        for (int iter = 2;; ++iter) {
            LSX_TRY(apply(1));
            LSX_TRY(launch_est_asum_sign<T>(h, n, x, isgn, rec)); // JUMP 3
            LSX_TRY(read());
            const double estold = est;
            est = r[0];
            if (r[4] != 0.0 || est <= estold) break;              // repeated sign vector, or no increase
            LSX_TRY(apply(2));
            LSX_TRY(launch_est_amax_unit<T>(h, n, x, j, rec));    // JUMP 4
            LSX_TRY(read());
            j = (int)r[1];
            if (!(r[3] != r[2] && iter < 5)) break;
        }
        LSX_TRY(launch_est_fill<T>(h, n, 1, x, (int32_t *)nullptr));   // the alternating vector
        LSX_TRY(apply(1));
        LSX_TRY(launch_est_asum_sign<T>(h, n, x, isgn, rec));     // JUMP 5
        LSX_TRY(read());
        const double temp = 2.0 * (r[0] / (3.0 * n));
        if (temp > est) est = temp;
    }
    *est_out = est;
    return LSX_OK;
}

// LAPACK's gecon: lacn2's iteration around single-right-hand-side solves with L U and its transpose.  Synchronises
// the handle's stream.
template <typename T>
static int gecon_dev(lsx_handle_t h, int norm, int n, const T *LU, int lda, const int32_t *d_ipiv, double anorm,
                     double *rcond) {
    LSX_ARG((norm == LSX_NORM_ONE || norm == LSX_NORM_INF) && n >= 0 && lda >= n && rcond);
    *rcond = 1.0;
    h->gecon_solves = 0;
    if (n == 0) return LSX_OK;
    LSX_ARG(LU && d_ipiv);
    if (anorm != anorm || anorm < 0) {
        set_error("bad argument: anorm must be a norm of the unfactored matrix, not NaN or negative");
        return LSX_ERR_ARG;
    }
    *rcond = 0.0;
    if (anorm == 0) return LSX_OK;
    T *x = nullptr; int32_t *ident = nullptr; signed char *isgn = nullptr; double *rec = nullptr;
    LSX_TRY(carve(h, h->cond, [&](Carver &c) {
        x = c.take<T>(n);
        ident = c.take<int32_t>(n);   // no interchange: the solves work on L U alone
        isgn = c.take<signed char>(n);
        rec = c.take<double>(8);      // rec[5] = min |U_ii|
    }));
    double r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // kase 1: x <- inv(A) x, kase 2: x <- inv(A^T) x; the infinity-norm of A is the 1-norm of A^T
    auto solve = [&](const int kase) -> int {
        h->gecon_solves += 1;
        const bool plain = (kase == 1) == (norm == LSX_NORM_ONE);
        return plain ? getrs_dev<T>(h, n, 1, LU, lda, ident, x, 1) : getrs_t_dev<T>(h, n, 1, LU, lda, ident, x, 1);
    };
    LSX_HIP(hipMemsetAsync(isgn, 0, (size_t)n, h->stream));
    LSX_TRY(launch_diag_minabs<T>(h, n, LU, lda, rec + 4));      // writes its second slot: rec[5]
    LSX_TRY(launch_est_fill<T>(h, n, 0, x, ident));
    LSX_HIP(hipMemcpyAsync(r, rec, sizeof(r), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (!(r[5] > 0)) return LSX_OK;                               // an exactly zero (or NaN) pivot: singular, rcond = 0
    double est = 0;
    LSX_TRY((lacn2_dev<T>(h, n, x, isgn, rec, solve, &est)));
    LSX_TRY(check_dev_status(h));                                 // a timed-out solve is a failure, not an estimate
    if (est > 0 && est - est == 0) *rcond = (1.0 / est) / anorm;  // non-finite estimate: 0
    return LSX_OK;
}

template <typename T> struct Lamch;
template <> struct Lamch<double> { static constexpr double u = 0x1p-53, safmin = 0x1p-1022; };
template <> struct Lamch<float> { static constexpr double u = 0x1p-24, safmin = 0x1p-126; };

// The refinement loop and forward bound of LAPACK's gerfs / porfs (dgerfs.f, dporfs.f step for step), shared by
// gerfs_dev and porfs_dev, which differ only in how a residual and a solve are made:
//   resid(g, B, X, Rg, Wg, ldr, work)  residual and componentwise bound of g <= 8 columns in one pass over the matrix
//   solve(transposed, v)               v <- inv(op A) v, or inv(op A)^T v, one vector
// F (ldf) holds the factors: an exactly zero or NaN diagonal entry means there is no solution to refine.  work_bytes:
// what resid wants behind the loop's own arrays in the refine buffer.  *steps / *solves: the read-back counters of the caller.
// Refine X until the componentwise backward error stops improving, then bound the forward error of every column with
// lacn2 on inv(op A) diag(W).  A correction is a single right-hand-side solve of the column that asked for it, so a
// column gets the same bits whatever rides along.  The host reads one record per step.  Synchronises the stream.
template <typename T, typename Resid, typename Solve>
static int refine_loop(lsx_handle_t h, int n, int nrhs, const T *F, int ldf, const T *B, int ldb, T *X, int ldx,
                       double *ferr, double *berr, bool *singular, size_t work_bytes, int *steps_max, int *solves,
                       Resid resid, Solve solve) {
    constexpr int G = 8, ITMAX = 5;
    const double u = Lamch<T>::u, safe1 = (n + 1.0) * Lamch<T>::safmin, safe2 = safe1 / u, nu = (n + 1.0) * u;
    T *Rg = nullptr, *Wg = nullptr, *v = nullptr, *wt = nullptr; signed char *isgn = nullptr; double *rec = nullptr, *part = nullptr;
    LSX_TRY(carve(h, h->refine, [&](Carver &c) {
        Rg = c.take<T>((size_t)n * G);   // residuals of the group, n x 8
        Wg = c.take<T>((size_t)n * G);   // bounds of the group
        v = c.take<T>(n);                // correction of one column / the estimator's vector
        wt = c.take<T>(n);               // the weights W of one column
        isgn = c.take<signed char>(n);
        rec = c.take<double>(64);        // [0, 16): berr[8], max|x|[8]; [16, 24): the estimator's record
        part = c.take<double>((work_bytes + 7) / 8);   // the residual pass's partial sums
    }));
    double *erec = rec + 16;
    double r[16];
    LSX_TRY(launch_diag_minabs<T>(h, n, F, ldf, rec));     // writes its second slot: rec[1]
    LSX_HIP(hipMemcpyAsync(r, rec, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (!(r[1] > 0)) {                                      // an exactly zero (or NaN) pivot: no solution to refine
        for (int j = 0; j < nrhs; ++j) ferr[j] = berr[j] = INFINITY;
        if (singular) *singular = true;
        return LSX_OK;
    }
    for (int c0 = 0; c0 < nrhs; c0 += G) {
        const int g = std::min(G, nrhs - c0);
        int steps[G] = {0, 0, 0, 0, 0, 0, 0, 0};
        double lstres[G];
        bool active[G];
        for (int j = 0; j < G; ++j) { lstres[j] = 3.0; active[j] = j < g; }
        for (;;) {
            LSX_TRY(resid(g, B + c0, X + c0, Rg, Wg, G, part));
            LSX_TRY(launch_berr<T>(h, n, g, Rg, Wg, G, X + c0, ldx, safe1, safe2, rec));
            LSX_HIP(hipMemcpyAsync(r, rec, sizeof(r), hipMemcpyDeviceToHost, h->stream));
            LSX_HIP(hipStreamSynchronize(h->stream));
            bool any = false;
            for (int j = 0; j < g; ++j) {
                if (!active[j]) continue;                   // a column that has stopped keeps its x (and its berr)
                const double be = r[j];
                berr[c0 + j] = be;
                if (be > u && 2.0 * be <= lstres[j] && steps[j] < ITMAX) {
                    LSX_TRY(launch_refine_take<T>(h, n, Rg + j, G, v));
                    LSX_TRY(solve(false, v));
                    LSX_TRY(launch_refine_add<T>(h, n, v, X + c0 + j, ldx));
                    lstres[j] = be;
                    steps[j] += 1;
                    *steps_max = std::max(*steps_max, steps[j]);
                    any = true;
                } else {
                    active[j] = false;                      // a NaN compares false: no step
                }
            }
            if (!any) break;                                // Rg, Wg and max|x| now belong to the final X
        }
        for (int j = 0; j < g; ++j) {
            if (berr[c0 + j] != berr[c0 + j]) { ferr[c0 + j] = berr[c0 + j]; continue; }   // NaN in A, B or X
            const double xmax = r[8 + j];
            LSX_TRY(launch_ferr_weight<T>(h, n, Rg + j, Wg + j, G, nu, safe1, safe2, wt));
            LSX_HIP(hipMemsetAsync(isgn, 0, (size_t)n, h->stream));
            LSX_TRY(launch_est_fill<T>(h, n, 0, v, (int32_t *)nullptr));
            // lacn2 on M = diag(W) inv(op A)^T: its 1-norm is the infinity-norm of inv(op A) diag(W)
            auto apply = [&](const int kase) -> int {
                *solves += 1;
                if (kase == 1) {
                    LSX_TRY(solve(true, v));
                    return launch_vec_mul<T>(h, n, wt, v);
                }
                LSX_TRY(launch_vec_mul<T>(h, n, wt, v));
                return solve(false, v);
            };
            double est = 0;
            LSX_TRY((lacn2_dev<T>(h, n, v, isgn, erec, apply, &est)));
            ferr[c0 + j] = xmax != 0 ? est / xmax : est;
        }
    }
    return LSX_OK;
}

// LAPACK's gerfs on device data with the caller's factors: refine_loop around the general residual pass
// (kernels_refine.hip) and single right-hand-side solves with L U and its transpose.
template <typename T>
static int gerfs_dev(lsx_handle_t h, int trans, int n, int nrhs, const T *A, int lda, const T *LU, int ldlu,
                     const int32_t *d_ipiv, const T *B, int ldb, T *X, int ldx, double *ferr, double *berr,
                     bool *singular = nullptr) {
    LSX_ARG((trans == 0 || trans == 1) && n >= 0 && nrhs >= 0 && lda >= n && ldlu >= n && ldb >= nrhs && ldx >= nrhs);
    LSX_ARG(nrhs == 0 || (ferr && berr));
    if (singular) *singular = false;
    h->gerfs_steps = 0;
    h->gerfs_solves = 0;
    for (int j = 0; j < nrhs; ++j) ferr[j] = berr[j] = 0.0;
    if (n == 0 || nrhs == 0) return LSX_OK;
    LSX_ARG(A && LU && d_ipiv && B && X);
    auto resid = [&](int g, const T *Bc, const T *Xc, T *Rg, T *Wg, int ldr, double *part) -> int {
        return launch_resid_bound<T>(h, trans, n, g, A, lda, Bc, ldb, Xc, ldx, Rg, Wg, ldr, part);
    };
    // x <- inv(op A) x (transposed: inv(op A)^T x) for one vector, with the caller's interchanges
    auto solve = [&](const bool transposed, T *v) -> int {
        return (trans != 0) != transposed ? getrs_t_dev<T>(h, n, 1, LU, ldlu, d_ipiv, v, 1)
                                          : getrs_dev<T>(h, n, 1, LU, ldlu, d_ipiv, v, 1);
    };
    bool sing = false;
    LSX_TRY((refine_loop<T>(h, n, nrhs, LU, ldlu, B, ldb, X, ldx, ferr, berr, &sing, resid_bound_work_bytes(trans, n),
                            &h->gerfs_steps, &h->gerfs_solves, resid, solve)));
    if (singular) *singular = sing;
    if (sing) return LSX_OK;
    return check_dev_status(h);                             // a timed-out solve is a failure, not a bound
}

// host buffers: stage A, the factors, B and X, refine on the device, bring X back
template <typename T>
static int gerfs_host(lsx_handle_t h, int trans, int n, int nrhs, const T *A, int lda, const T *LU, int ldlu,
                      const int32_t *ipiv, const T *B, int ldb, T *X, int ldx, double *ferr, double *berr) {
    LSX_ARG(h && (trans == 0 || trans == 1) && n >= 0 && nrhs >= 0 && lda >= n && ldlu >= n && ldb >= nrhs && ldx >= nrhs);
    LSX_ARG(nrhs == 0 || (ferr && berr));
    if (n == 0 || nrhs == 0) return gerfs_dev<T>(h, trans, n, nrhs, A, lda, LU, ldlu, ipiv, B, ldb, X, ldx, ferr, berr);
    LSX_ARG(A && LU && ipiv && B && X);
    const int ld = ld_for(n), ldr = ld_for(nrhs);
    T *dA = nullptr, *dLU = nullptr, *dB = nullptr, *dX = nullptr; int32_t *dp = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)n * ld); dLU = c.take<T>((size_t)n * ld);
        dB = c.take<T>((size_t)n * ldr); dX = c.take<T>((size_t)n * ldr);
        dp = c.take<int32_t>(n);
    }));
    LSX_TRY(h2d<T>(h, n, n, A, lda, dA, ld));
    LSX_TRY(h2d<T>(h, n, n, LU, ldlu, dLU, ld));
    LSX_TRY(h2d<T>(h, n, nrhs, B, ldb, dB, ldr));
    LSX_TRY(h2d<T>(h, n, nrhs, X, ldx, dX, ldr));
    LSX_HIP(hipMemcpyAsync(dp, ipiv, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
    bool singular = false;
    LSX_TRY(gerfs_dev<T>(h, trans, n, nrhs, dA, ld, dLU, ld, dp, dB, ldr, dX, ldr, ferr, berr, &singular));
    if (singular) return LSX_OK;                                    // X is left untouched
    LSX_TRY(d2h<T>(h, n, nrhs, dX, ldr, X, ldx));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

// factor, solve, refine, bound for a host system; A and B are kept
template <typename T>
static int gesvr_host(lsx_handle_t h, int trans, int n, int nrhs, const T *A, int lda, const T *B, int ldb, T *X, int ldx,
                      double *ferr, double *berr, int *info) {
    LSX_ARG(h && (trans == 0 || trans == 1) && n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs && ldx >= nrhs);
    LSX_ARG(nrhs == 0 || (ferr && berr));
    if (info) *info = 0;
    h->gerfs_steps = 0;
    h->gerfs_solves = 0;
    for (int j = 0; j < nrhs; ++j) ferr[j] = berr[j] = 0.0;
    if (n == 0) return LSX_OK;
    LSX_ARG(A && (nrhs == 0 || (B && X)));
    const int ld = ld_for(n), ldr = ld_for(nrhs > 0 ? nrhs : 1);
    T *dA = nullptr, *dLU = nullptr, *dB = nullptr, *dX = nullptr; int32_t *dp = nullptr; int *dinfo = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)n * ld); dLU = c.take<T>((size_t)n * ld);
        dB = c.take<T>((size_t)n * ldr); dX = c.take<T>((size_t)n * ldr);
        dp = c.take<int32_t>(n);
        dinfo = c.take<int>(1);
    }));
    int hinfo = 0;
    LSX_TRY(factor_from_host<T>(h, n, A, lda, dLU, ld, dp, dinfo, &hinfo));
    if (info) *info = hinfo;
    if (hinfo != 0) {                                               // singular: X is not written
        for (int j = 0; j < nrhs; ++j) ferr[j] = berr[j] = INFINITY;
        return LSX_OK;
    }
    if (nrhs == 0) return LSX_OK;
    LSX_TRY(h2d<T>(h, n, n, A, lda, dA, ld));
    LSX_TRY(h2d<T>(h, n, nrhs, B, ldb, dB, ldr));
    LSX_TRY(h2d<T>(h, n, nrhs, B, ldb, dX, ldr));
    if (trans) LSX_TRY(getrs_t_dev<T>(h, n, nrhs, dLU, ld, dp, dX, ldr, true));
    else LSX_TRY(getrs_dev<T>(h, n, nrhs, dLU, ld, dp, dX, ldr));
    LSX_TRY(gerfs_dev<T>(h, trans, n, nrhs, dA, ld, dLU, ld, dp, dB, ldr, dX, ldr, ferr, berr));
    LSX_TRY(d2h<T>(h, n, nrhs, dX, ldr, X, ldx));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

template <typename T>
static int gecon_host(lsx_handle_t h, int norm, int n, const T *LU, int lda, const int32_t *ipiv, double anorm,
                      double *rcond) {
    LSX_ARG(h && (norm == LSX_NORM_ONE || norm == LSX_NORM_INF) && n >= 0 && lda >= n && rcond);
    if (n == 0) { *rcond = 1.0; return LSX_OK; }
    LSX_ARG(LU && ipiv);
    const int ld = ld_for(n);
    T *dA = nullptr; int32_t *dp = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) { dA = c.take<T>((size_t)n * ld); dp = c.take<int32_t>(n); }));
    LSX_TRY(h2d<T>(h, n, n, LU, lda, dA, ld));
    LSX_HIP(hipMemcpyAsync(dp, ipiv, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
    return gecon_dev<T>(h, norm, n, dA, ld, dp, anorm, rcond);
}

template <typename T>
static int rcond_host(lsx_handle_t h, int norm, int n, const T *A, int lda, double *rcond, int *info) {
    LSX_ARG(h && (norm == LSX_NORM_ONE || norm == LSX_NORM_INF) && n >= 0 && lda >= n && rcond);
    if (info) *info = 0;
    *rcond = 1.0;
    if (n == 0) return LSX_OK;
    LSX_ARG(A);
    const int ld = ld_for(n);
    T *dA = nullptr; int32_t *dp = nullptr; int *dinfo = nullptr; double *dnorm = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)n * ld);
        dp = c.take<int32_t>(n);
        dinfo = c.take<int>(1);
        dnorm = c.take<double>(1);
    }));
    LSX_TRY(h2d<T>(h, n, n, A, lda, dA, ld));
    LSX_TRY(lange_dev<T>(h, norm, n, n, dA, ld, dnorm));
    double anorm = 0;
    LSX_HIP(hipMemcpyAsync(&anorm, dnorm, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    int hinfo = 0;
    LSX_TRY(factor_from_host<T>(h, n, A, lda, dA, ld, dp, dinfo, &hinfo));   // synchronises: anorm is there
    if (info) *info = hinfo;
    if (hinfo != 0) { *rcond = 0.0; return LSX_OK; }
    return gecon_dev<T>(h, norm, n, dA, ld, dp, anorm, rcond);
}

// ---------------------------------------------------------------- equilibration and the expert driver (gesvx)
// ---------------------------------------------------------------- Cholesky: condition estimate and error bounds
// The 1-norm (= infinity-norm) of a symmetric matrix from its upper triangle, lsx_lange_*_dev's contract otherwise.
template <typename T>
static int lansy_dev(lsx_handle_t h, int n, const T *dA, int lda, double *d_out) {
    LSX_ARG(n >= 0 && lda >= n && d_out);
    LSX_ARG(n == 0 || dA);
    LSX_TRY(reserve(h, h->scratch, resid_bound_sym_work_bytes(n, 1) + 256));
    return launch_lansy<T>(h, n, dA, lda, (double *)h->scratch.p, d_out);
}

// LAPACK's pocon: lacn2's iteration around x <- inv(U) inv(U^T) x.  The operator is symmetric, so both kase values
// apply the same solve.  Synchronises the handle's stream.
template <typename T>
static int pocon_dev(lsx_handle_t h, int n, const T *U, int lda, double anorm, double *rcond) {
    LSX_ARG(n >= 0 && lda >= n && rcond);
    *rcond = 1.0;
    h->pocon_solves = 0;
    if (n == 0) return LSX_OK;
    LSX_ARG(U);
    if (anorm != anorm || anorm < 0) {
        set_error("bad argument: anorm must be a norm of the unfactored matrix, not NaN or negative");
        return LSX_ERR_ARG;
    }
    *rcond = 0.0;
    if (anorm == 0) return LSX_OK;
    T *x = nullptr; signed char *isgn = nullptr; double *rec = nullptr;
    LSX_TRY(carve(h, h->cond, [&](Carver &c) {
        x = c.take<T>(n);
        isgn = c.take<signed char>(n);
        rec = c.take<double>(8);      // rec[5] = min |u_ii|
    }));
    double r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    LSX_HIP(hipMemsetAsync(isgn, 0, (size_t)n, h->stream));
    LSX_TRY(launch_diag_minabs<T>(h, n, U, lda, rec + 4));       // writes its second slot: rec[5]
    LSX_TRY(launch_est_fill<T>(h, n, 0, x, (int32_t *)nullptr));
    LSX_HIP(hipMemcpyAsync(r, rec, sizeof(r), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (!(r[5] > 0)) return LSX_OK;                               // an exactly zero (or NaN) u_ii: rcond = 0
    PotrsFew<T> pf;
    LSX_TRY(potrs_few_prepare<T>(h, n, U, lda, &pf));
    auto solve = [&](const int) -> int {
        h->pocon_solves += 1;
        return potrs_few_apply<T>(h, n, 1, U, lda, pf, x, 1);
    };
    double est = 0;
    LSX_TRY((lacn2_dev<T>(h, n, x, isgn, rec, solve, &est)));
    if (est > 0 && est - est == 0) *rcond = (1.0 / est) / anorm;  // non-finite estimate: 0
    return LSX_OK;
}

// LAPACK's porfs on device data: refine_loop around the symmetric residual pass and the few-column Cholesky solve.
// A and U are read from their upper triangles alone.
template <typename T>
static int porfs_dev(lsx_handle_t h, int n, int nrhs, const T *A, int lda, const T *U, int ldu, const T *B, int ldb, T *X,
                     int ldx, double *ferr, double *berr, bool *singular = nullptr) {
    LSX_ARG(n >= 0 && nrhs >= 0 && lda >= n && ldu >= n && ldb >= nrhs && ldx >= nrhs);
    LSX_ARG(nrhs == 0 || (ferr && berr));
    if (singular) *singular = false;
    h->porfs_steps = 0;
    h->porfs_solves = 0;
    for (int j = 0; j < nrhs; ++j) ferr[j] = berr[j] = 0.0;
    if (n == 0 || nrhs == 0) return LSX_OK;
    LSX_ARG(A && U && B && X);
    PotrsFew<T> pf;
    LSX_TRY(potrs_few_prepare<T>(h, n, U, ldu, &pf));          // harmless on a factor with a zero u_ii: not used then
    auto resid = [&](int g, const T *Bc, const T *Xc, T *Rg, T *Wg, int ldr, double *part) -> int {
        return launch_resid_bound_sym<T>(h, n, g, A, lda, Bc, ldb, Xc, ldx, Rg, Wg, ldr, part);
    };
    auto solve = [&](const bool, T *v) -> int { return potrs_few_apply<T>(h, n, 1, U, ldu, pf, v, 1); };
    return refine_loop<T>(h, n, nrhs, U, ldu, B, ldb, X, ldx, ferr, berr, singular,
                          resid_bound_sym_work_bytes(n, std::min(nrhs, 8)), &h->porfs_steps, &h->porfs_solves, resid, solve);
}

template <typename T>
static int pocon_host(lsx_handle_t h, int n, const T *U, int lda, double anorm, double *rcond) {
    LSX_ARG(h && n >= 0 && lda >= n && rcond);
    if (n == 0) { *rcond = 1.0; h->pocon_solves = 0; return LSX_OK; }
    LSX_ARG(U);
    const int ld = ld_for(n);
    T *dU = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) { dU = c.take<T>((size_t)n * ld); }));
    LSX_TRY(upper_h2d<T>(h, n, U, lda, dU, ld));
    return pocon_dev<T>(h, n, dU, ld, anorm, rcond);
}

// norm, factorisation and estimate of a host matrix, which is not modified; info as lsx_potrf_* (rcond = 0 then)
template <typename T>
static int porcond_host(lsx_handle_t h, int n, const T *A, int lda, double *rcond, int *info) {
    LSX_ARG(h && n >= 0 && lda >= n && rcond);
    if (info) *info = 0;
    *rcond = 1.0;
    h->pocon_solves = 0;
    if (n == 0) return LSX_OK;
    LSX_ARG(A);
    const int ld = ld_for(n);
    T *dA = nullptr; int *dinfo = nullptr; double *dnorm = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) { dA = c.take<T>((size_t)n * ld); dinfo = c.take<int>(1); dnorm = c.take<double>(1); }));
    LSX_TRY(upper_h2d<T>(h, n, A, lda, dA, ld));
    LSX_TRY(lansy_dev<T>(h, n, dA, ld, dnorm));
    double anorm = 0;
    int hinfo = 0;
    LSX_HIP(hipMemcpyAsync(&anorm, dnorm, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LSX_TRY(potrf_dev<T>(h, n, dA, ld, dinfo));
    LSX_HIP(hipMemcpyAsync(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = hinfo;
    if (hinfo != 0) { *rcond = 0.0; return LSX_OK; }
    return pocon_dev<T>(h, n, dA, ld, anorm, rcond);
}

// host buffers: stage the upper triangles of A and U, B and X, refine on the device, bring X back
template <typename T>
static int porfs_host(lsx_handle_t h, int n, int nrhs, const T *A, int lda, const T *U, int ldu, const T *B, int ldb, T *X,
                      int ldx, double *ferr, double *berr) {
    LSX_ARG(h && n >= 0 && nrhs >= 0 && lda >= n && ldu >= n && ldb >= nrhs && ldx >= nrhs);
    LSX_ARG(nrhs == 0 || (ferr && berr));
    if (n == 0 || nrhs == 0) return porfs_dev<T>(h, n, nrhs, A, lda, U, ldu, B, ldb, X, ldx, ferr, berr);
    LSX_ARG(A && U && B && X);
    const int ld = ld_for(n), ldr = ld_for(nrhs);
    T *dA = nullptr, *dU = nullptr, *dB = nullptr, *dX = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)n * ld); dU = c.take<T>((size_t)n * ld);
        dB = c.take<T>((size_t)n * ldr); dX = c.take<T>((size_t)n * ldr);
    }));
    LSX_TRY(upper_h2d<T>(h, n, A, lda, dA, ld));
    LSX_TRY(upper_h2d<T>(h, n, U, ldu, dU, ld));
    LSX_TRY(h2d<T>(h, n, nrhs, B, ldb, dB, ldr));
    LSX_TRY(h2d<T>(h, n, nrhs, X, ldx, dX, ldr));
    bool singular = false;
    LSX_TRY(porfs_dev<T>(h, n, nrhs, dA, ld, dU, ld, dB, ldr, dX, ldr, ferr, berr, &singular));
    if (singular) return LSX_OK;                                    // X is left untouched
    LSX_TRY(d2h<T>(h, n, nrhs, dX, ldr, X, ldx));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

// factor, solve, refine, bound for a host system; A and B are kept
template <typename T>
static int posvr_host(lsx_handle_t h, int n, int nrhs, const T *A, int lda, const T *B, int ldb, T *X, int ldx,
                      double *ferr, double *berr, int *info) {
    LSX_ARG(h && n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs && ldx >= nrhs);
    LSX_ARG(nrhs == 0 || (ferr && berr));
    if (info) *info = 0;
    h->porfs_steps = 0;
    h->porfs_solves = 0;
    for (int j = 0; j < nrhs; ++j) ferr[j] = berr[j] = 0.0;
    if (n == 0) return LSX_OK;
    LSX_ARG(A && (nrhs == 0 || (B && X)));
    const int ld = ld_for(n), ldr = ld_for(nrhs > 0 ? nrhs : 1);
    T *dA = nullptr, *dU = nullptr, *dB = nullptr, *dX = nullptr; int *dinfo = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)n * ld); dU = c.take<T>((size_t)n * ld);
        dB = c.take<T>((size_t)n * ldr); dX = c.take<T>((size_t)n * ldr);
        dinfo = c.take<int>(1);
    }));
    int hinfo = 0;
    LSX_TRY(upper_h2d<T>(h, n, A, lda, dU, ld));
    LSX_TRY(potrf_dev<T>(h, n, dU, ld, dinfo));
    LSX_HIP(hipMemcpyAsync(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = hinfo;
    if (hinfo != 0) {                                               // not positive definite: X is not written
        for (int j = 0; j < nrhs; ++j) ferr[j] = berr[j] = INFINITY;
        return LSX_OK;
    }
    if (nrhs == 0) return LSX_OK;
    LSX_TRY(upper_h2d<T>(h, n, A, lda, dA, ld));
    LSX_TRY(h2d<T>(h, n, nrhs, B, ldb, dB, ldr));
    LSX_TRY(h2d<T>(h, n, nrhs, B, ldb, dX, ldr));
    LSX_TRY(potrs_dev<T>(h, n, nrhs, dU, ld, dX, ldr));
    LSX_TRY(porfs_dev<T>(h, n, nrhs, dA, ld, dU, ld, dB, ldr, dX, ldr, ferr, berr));
    LSX_TRY(d2h<T>(h, n, nrhs, dX, ldr, X, ldx));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

template <typename T> struct LaqgeLim;   // dlaqge's small = safmin / prec with prec = eps * base; large = 1 / small
template <> struct LaqgeLim<double> { static constexpr double small_ = 0x1p-970, large_ = 0x1p+970; };
template <> struct LaqgeLim<float> { static constexpr double small_ = 0x1p-103, large_ = 0x1p+103; };

template <typename T>
static int d2d(lsx_handle_t h, int m, int n, const T *src, int lds, T *dst, int ldd) {
    if (m <= 0 || n <= 0) return LSX_OK;
    LSX_HIP(hipMemcpy2DAsync(dst, (size_t)ldd * sizeof(T), src, (size_t)lds * sizeof(T), (size_t)n * sizeof(T), m,
                             hipMemcpyDeviceToDevice, h->stream));
    return LSX_OK;
}

// the equil buffer: 32 doubles of records in front (the drivers'), then the work area of one reduction
static int carve_equil(lsx_handle_t h, size_t work_bytes, double **rec, double **work) {
    return carve(h, h->equil, [&](Carver &c) { *rec = c.take<double>(32); *work = c.take<double>((work_bytes + 7) / 8); });
}

// LAPACK's geequ on device data; asynchronous
template <typename T>
static int geequ_dev(lsx_handle_t h, int m, int n, const T *dA, int lda, T *d_r, T *d_c, double *d_stats, int passes = 3) {
    LSX_ARG(m >= 0 && n >= 0 && lda >= n && d_stats && passes >= 1 && passes <= 3);
    LSX_ARG(m == 0 || n == 0 || (dA && d_r && d_c));
    double *rec = nullptr, *work = nullptr;
    LSX_TRY(carve_equil(h, geequ_work_bytes(m, n, sizeof(T)), &rec, &work));
    return launch_geequ<T>(h, m, n, dA, lda, d_r, d_c, d_stats, work, passes);
}

// dlaqge's decision from the three scalars of geequ (values of the working precision held in doubles)
template <typename T>
static int laqge_decide(double rowcnd, double colcnd, double amax) {
    const double thresh = 0.1;
    const bool rows = !(rowcnd >= thresh && amax >= LaqgeLim<T>::small_ && amax <= LaqgeLim<T>::large_);
    const bool cols = !(colcnd >= thresh);
    return (rows ? LSX_EQUED_ROW : 0) | (cols ? LSX_EQUED_COL : 0);
}

// LAPACK's laqge on device data: one scaling launch or none; dCopy (may be null) receives the scaled matrix too when
// there is a launch.  Asynchronous.
template <typename T>
static int laqge_dev(lsx_handle_t h, int m, int n, T *dA, int lda, const T *d_r, const T *d_c, double rowcnd,
                     double colcnd, double amax, int *equed, T *dCopy = nullptr, int ldc = 0) {
    LSX_ARG(m >= 0 && n >= 0 && lda >= n && equed);
    *equed = LSX_EQUED_NONE;
    if (m == 0 || n == 0) return LSX_OK;
    LSX_ARG(dA && d_r && d_c);
    const int e = laqge_decide<T>(rowcnd, colcnd, amax);
    *equed = e;
    return launch_laqge<T>(h, m, n, dA, lda, (e & LSX_EQUED_ROW) ? d_r : nullptr, (e & LSX_EQUED_COL) ? d_c : nullptr,
                           dCopy, ldc);
}

// What gesvx_dev tells the host-buffer form beyond LAPACK's outputs.
struct GesvxDone {
    bool scales = false;   // d_r / d_c hold geequ's factors (equil and geequ's info == 0)
    bool solved = false;   // dX was written: a solution, or NaN throughout for a matrix with a NaN
};

// LAPACK's gesvx (dgesvx.f step for step, fact = 'N' / 'E') on device data with LAPACK's in / out contract: dA leaves
// equilibrated, dB scaled, dLU / d_ipiv hold the factors of the equilibrated matrix.  Every scalar result is a host
// variable; the host reads a small record after geequ, after the factorisation and inside gecon / gerfs, so this
// synchronises the handle's stream.
template <typename T>
static int gesvx_dev(lsx_handle_t h, int equil, int trans, int n, int nrhs, T *dA, int lda, T *dLU, int ldlu,
                     int32_t *d_ipiv, T *dB, int ldb, T *dX, int ldx, T *d_r, T *d_c, int *equed, double *rowcnd_out,
                     double *colcnd_out, double *rcond, double *ferr, double *berr, double *rpvgrw, int *info,
                     GesvxDone *done = nullptr) {
    LSX_ARG((equil == 0 || equil == 1) && (trans == 0 || trans == 1) && n >= 0 && nrhs >= 0 && lda >= n && ldlu >= n &&
            ldb >= nrhs && ldx >= nrhs);
    LSX_ARG(equed && rcond && rpvgrw && info && (nrhs == 0 || (ferr && berr)));
    *equed = LSX_EQUED_NONE;
    *rcond = 1.0;
    *rpvgrw = 1.0;
    *info = 0;
    if (rowcnd_out) *rowcnd_out = 1.0;
    if (colcnd_out) *colcnd_out = 1.0;
    h->gerfs_steps = 0;
    h->gerfs_solves = 0;
    h->gecon_solves = 0;
    for (int j = 0; j < nrhs; ++j) ferr[j] = berr[j] = 0.0;
    if (n == 0) return LSX_OK;
    LSX_ARG(dA && dLU && d_ipiv && (nrhs == 0 || (dB && dX)) && (equil == 0 || (d_r && d_c)));
    const int norm = trans ? LSX_NORM_INF : LSX_NORM_ONE;
    // records: [0..4) geequ's stats, [4] anorm, [5] max |A|, [6] max |U|, then the factorisation's info word
    double *rec = nullptr, *work = nullptr;
    LSX_TRY(carve_equil(h, std::max(geequ_work_bytes(n, n, sizeof(T)), maxabs_work_bytes(n)), &rec, &work));
    int *dinfo = (int *)(rec + 8);
    double hrec[8] = {1, 1, 0, 0, 0, 0, 0, 0};
    double rowcnd = 1.0, colcnd = 1.0;
    bool copied = false;                                             // dLU holds a copy of the (equilibrated) matrix
    if (equil) {
        LSX_TRY(geequ_dev<T>(h, n, n, dA, lda, d_r, d_c, rec));
        LSX_HIP(hipMemcpyAsync(hrec, rec, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        LSX_HIP(hipStreamSynchronize(h->stream));
        if (hrec[3] == 0.0 && done) done->scales = true;             // geequ's info == 0: r and c are handed out
        if (hrec[3] == 0.0 && hrec[2] == hrec[2]) {                  // ... and amax is no NaN: laqge decides
            rowcnd = hrec[0];
            colcnd = hrec[1];
            LSX_TRY(laqge_dev<T>(h, n, n, dA, lda, d_r, d_c, rowcnd, colcnd, hrec[2], equed, dLU, ldlu));
            copied = *equed != LSX_EQUED_NONE;
        }
    }
    if (rowcnd_out) *rowcnd_out = rowcnd;
    if (colcnd_out) *colcnd_out = colcnd;
    const bool rowequ = (*equed & LSX_EQUED_ROW) != 0, colequ = (*equed & LSX_EQUED_COL) != 0;
    if (nrhs > 0) {
        if (!trans && rowequ) LSX_TRY(launch_laqge<T>(h, n, nrhs, dB, ldb, d_r, nullptr, nullptr, 0));
        if (trans && colequ) LSX_TRY(launch_laqge<T>(h, n, nrhs, dB, ldb, d_c, nullptr, nullptr, 0));
    }
    // the norm first: a NaN in the matrix shows in it, and such a matrix is not factored at all
    LSX_TRY(lange_dev<T>(h, norm, n, n, dA, lda, rec + 4));
    LSX_HIP(hipMemcpyAsync(hrec + 4, rec + 4, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    const double anorm = hrec[4];
    if (anorm != anorm) {                                            // no output is left unwritten: X is all NaN
        *rcond = *rpvgrw = NAN;
        for (int j = 0; j < nrhs; ++j) ferr[j] = berr[j] = NAN;
        if (nrhs > 0) {
            LSX_HIP(hipMemset2DAsync(dX, (size_t)ldx * sizeof(T), 0xFF, (size_t)nrhs * sizeof(T), n, h->stream));
            if (done) done->solved = true;
        }
        LSX_HIP(hipStreamSynchronize(h->stream));
        return LSX_OK;
    }
    int hinfo = 0;
    for (int attempt = 0;; ++attempt) {                              // as factor_from_host: per-column panels after a time-out
        if (!copied) LSX_TRY(d2d<T>(h, n, n, dA, lda, dLU, ldlu));
        copied = false;
        LSX_TRY(getrf_dev<T>(h, n, dLU, ldlu, d_ipiv, dinfo, attempt == 1));
        if (attempt == 1) h->panel_fallbacks += 1;
        LSX_HIP(hipMemcpyAsync(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        LSX_HIP(hipStreamSynchronize(h->stream));
        if (hinfo >= 0) break;
        LSX_HIP(hipMemsetAsync(h->dev_status, 0, 3 * sizeof(int), h->stream));
        if (attempt == 1) {
            set_error("panel exchange timed out on the device, and so did the per-column fallback");
            return LSX_ERR_INTERNAL;
        }
    }
    // reciprocal pivot growth max |A| / max |U|, over the leading info columns when the factorisation broke down
    const int k = hinfo > 0 ? hinfo : n;
    LSX_TRY(launch_maxabs<T>(h, n, k, dA, lda, 0, work, rec + 5));
    LSX_TRY(launch_maxabs<T>(h, k, k, dLU, ldlu, 1, work, rec + 6));
    LSX_HIP(hipMemcpyAsync(hrec + 5, rec + 5, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    *rpvgrw = hrec[6] == 0.0 ? 1.0 : (double)((T)hrec[5] / (T)hrec[6]);
    *info = hinfo;
    if (hinfo > 0) {
        *rcond = 0.0;
        for (int j = 0; j < nrhs; ++j) ferr[j] = berr[j] = INFINITY;
        return LSX_OK;
    }
    LSX_TRY(gecon_dev<T>(h, norm, n, dLU, ldlu, d_ipiv, anorm, rcond));
    if (nrhs > 0) {
        LSX_TRY(d2d<T>(h, n, nrhs, dB, ldb, dX, ldx));
        if (trans) LSX_TRY(getrs_t_dev<T>(h, n, nrhs, dLU, ldlu, d_ipiv, dX, ldx, true));
        else LSX_TRY(getrs_dev<T>(h, n, nrhs, dLU, ldlu, d_ipiv, dX, ldx));
        LSX_TRY(gerfs_dev<T>(h, trans, n, nrhs, dA, lda, dLU, ldlu, d_ipiv, dB, ldb, dX, ldx, ferr, berr));
        if (!trans && colequ) {
            LSX_TRY(launch_laqge<T>(h, n, nrhs, dX, ldx, d_c, nullptr, nullptr, 0));
            for (int j = 0; j < nrhs; ++j) ferr[j] /= colcnd;
        } else if (trans && rowequ) {
            LSX_TRY(launch_laqge<T>(h, n, nrhs, dX, ldx, d_r, nullptr, nullptr, 0));
            for (int j = 0; j < nrhs; ++j) ferr[j] /= rowcnd;
        }
        if (done) done->solved = true;
    }
    if (*rcond < Lamch<T>::u) *info = n + 1;
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

// host buffers: A and B are kept, X receives the solution, r / c the scale factors geequ chose
template <typename T>
static int gesvx_host(lsx_handle_t h, int equil, int trans, int n, int nrhs, const T *A, int lda, const T *B, int ldb,
                      T *X, int ldx, int *equed, T *r, T *c, double *rcond, double *ferr, double *berr, double *rpvgrw,
                      int *info) {
    LSX_ARG(h && (equil == 0 || equil == 1) && (trans == 0 || trans == 1) && n >= 0 && nrhs >= 0 && lda >= n &&
            ldb >= nrhs && ldx >= nrhs);
    LSX_ARG(equed && rcond && rpvgrw && info && (nrhs == 0 || (ferr && berr)));
    if (n == 0)
        return gesvx_dev<T>(h, equil, trans, 0, nrhs, nullptr, lda, nullptr, lda, nullptr, nullptr, ldb, nullptr, ldx,
                            nullptr, nullptr, equed, nullptr, nullptr, rcond, ferr, berr, rpvgrw, info);
    LSX_ARG(A && (nrhs == 0 || (B && X)) && (equil == 0 || (r && c)));
    const int ld = ld_for(n), ldr = ld_for(nrhs > 0 ? nrhs : 1);
    T *dA = nullptr, *dLU = nullptr, *dB = nullptr, *dX = nullptr, *dr = nullptr, *dc = nullptr; int32_t *dp = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &cv) {
        dA = cv.take<T>((size_t)n * ld); dLU = cv.take<T>((size_t)n * ld);
        dB = cv.take<T>((size_t)n * ldr); dX = cv.take<T>((size_t)n * ldr);
        dp = cv.take<int32_t>(n);
        dr = cv.take<T>(n); dc = cv.take<T>(n);
    }));
    LSX_TRY(h2d<T>(h, n, n, A, lda, dA, ld));
    if (nrhs > 0) LSX_TRY(h2d<T>(h, n, nrhs, B, ldb, dB, ldr));
    GesvxDone done;
    LSX_TRY(gesvx_dev<T>(h, equil, trans, n, nrhs, dA, ld, dLU, ld, dp, dB, ldr, dX, ldr, dr, dc, equed, nullptr, nullptr,
                         rcond, ferr, berr, rpvgrw, info, &done));
    if (done.scales) {
        LSX_HIP(hipMemcpyAsync(r, dr, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        LSX_HIP(hipMemcpyAsync(c, dc, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    }
    if (done.solved) LSX_TRY(d2h<T>(h, n, nrhs, dX, ldr, X, ldx));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

}  // namespace lsx

using namespace lsx;

// ================================================================== extern "C"
extern "C" {

const char *lsx_last_error(void) { return g_err; }

int lsx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int lsx_create(lsx_handle_t *out, int device) {
    if (!out) { set_error("lsx_create: null out"); return LSX_ERR_ARG; }
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("no HIP device visible; liblsx has no CPU fallback");
        return LSX_ERR_NODEVICE;
    }
    LSX_ARG(device >= 0 && device < n);
    hipDeviceProp_t prop;
    LSX_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; liblsx is built for gfx950 (MI355X) only", device, prop.gcnArchName);
        return LSX_ERR_NODEVICE;
    }
    struct RestoreDevice {   // the caller's (and torch's) current device is not ours to change
        int prev = -1;
        RestoreDevice() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
        ~RestoreDevice() { if (prev >= 0) (void)hipSetDevice(prev); }
    } restore_device;
    LSX_HIP(hipSetDevice(device));
    lsx_handle_t h = new lsx_handle_s();
    h->device = device;
    h->num_cu = prop.multiProcessorCount;
    hipError_t e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
        delete h;
        return LSX_ERR_HIP;
    }
    h->stream = h->own_stream;
    {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // hi = numerically lowest = most urgent
        if (hipStreamCreateWithPriority(&h->side_stream, hipStreamNonBlocking, hi) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_panel, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_next, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_start, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming) != hipSuccess) {
            set_error("could not create the look-ahead stream / events");
            (void)hipStreamDestroy(h->own_stream);
            delete h;
            return LSX_ERR_HIP;
        }
    }
    int r = reserve(h, h->scratch, 1 << 20);
    DevBuf status, moves;   // fixed size: the handle keeps plain pointers
    if (r == LSX_OK) r = reserve(h, status, 256);
    h->dev_status = (int *)status.p;
    if (r == LSX_OK && hipMemset(status.p, 0, 256) != hipSuccess) r = LSX_ERR_HIP;
    if (r == LSX_OK) r = reserve(h, moves, 8192);
    if (r == LSX_OK) {
        h->moves_buf[0] = moves.p;
        h->moves_api = (char *)moves.p + 2048;
        h->moves_buf[1] = (char *)moves.p + 4096;
    }
    if (r != LSX_OK) { (void)hipStreamDestroy(h->own_stream); delete h; return r; }
    *out = h;
    return LSX_OK;
}

int lsx_destroy(lsx_handle_t h) {
    if (!h) return LSX_OK;
    LSX_DEVICE_GUARD(h);
    (void)hipStreamSynchronize(h->stream);
    for (auto &ev : h->prof.pending) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    for (auto &e : h->prof.pool) (void)hipEventDestroy(e);
    for (DevBuf *b : {&h->staging, &h->tinv, &h->rhs_work, &h->mixed_resid, &h->getri_work, &h->rref_first, &h->cond,
                      &h->refine, &h->equil, &h->qr_work, &h->svd_work, &h->eig_work, &h->xchg, &h->moves_all, &h->scratch})
        if (b->p) (void)hipFree(b->p);
    if (h->moves_buf[0]) (void)hipFree(h->moves_buf[0]);
    if (h->dev_status) (void)hipFree(h->dev_status);
    if (h->ev_panel) (void)hipEventDestroy(h->ev_panel);
    if (h->ev_next) (void)hipEventDestroy(h->ev_next);
    if (h->ev_start) (void)hipEventDestroy(h->ev_start);
    if (h->ev_done) (void)hipEventDestroy(h->ev_done);
    if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
    return LSX_OK;
}

int lsx_set_stream(lsx_handle_t h, void *hip_stream) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    LSX_HIP(hipStreamSynchronize(h->stream));
    h->stream = (hipStream_t)hip_stream;  // NULL = the default (null) stream
    return LSX_OK;
}

int lsx_use_own_stream(lsx_handle_t h) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    LSX_HIP(hipStreamSynchronize(h->stream));
    h->stream = h->own_stream;
    return LSX_OK;
}

int lsx_synchronize(lsx_handle_t h) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

int lsx_check_status(lsx_handle_t h) {
    LSX_ARG(h);
    LSX_DEVICE_GUARD(h);
    return check_dev_status(h);
}

int lsx_set_option(lsx_handle_t h, const char *key, int value) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && key);
    if (!strcmp(key, "nb")) {
        LSX_ARG(value >= 16 && value <= 128 && value % 16 == 0);
        h->nb = value;
    } else if (!strcmp(key, "panel")) {
        LSX_ARG(value >= 0 && value <= 4);
        if (value == 1 || value == 2) {
            set_error("panel modes 1 and 2 (superseded kernels) were removed: use 0, 3 or 4");
            return LSX_ERR_ARG;
        }
        h->panel_mode = value;
    } else if (!strcmp(key, "trsv")) {
        LSX_ARG(value >= 0 && value <= 2);
        h->trsv_mode = value;
    } else if (!strcmp(key, "gemm_tiles32")) {
        LSX_ARG(value == 0 || value == 1);
        h->gemm_no_tiles32 = !value;
    } else if (!strcmp(key, "gemm_queue_test")) {
        LSX_ARG(value >= 0 && value <= 3);
        h->gemm_queue_test = value;
    } else if (!strcmp(key, "gemm_stagger")) {
        LSX_ARG(value >= 0 && value <= 64);
        h->gemm_stagger = value;
    } else if (!strcmp(key, "gemm_waves")) {
        LSX_ARG(value == 0 || value == 4 || value == 8);
        h->gemm_waves = value;
    } else if (!strcmp(key, "kblock")) {
        LSX_ARG(value == 1 || value == 2);
        h->kblock = value;
    } else if (!strcmp(key, "panel_rt")) {
        LSX_ARG(value == 2 || value == 4 || value == 8);
        h->panel_rt = value;
    } else if (!strcmp(key, "panel_nt")) {
        LSX_ARG(value == 0 || value == 256 || value == 512 || value == 1024);
        h->panel_nt = value;
    } else if (!strcmp(key, "rref_blocked")) {
        LSX_ARG(value == 0 || value == 1);
        h->rref_blocked = value;
    } else if (!strcmp(key, "xrows_limit")) {   // tests: hand over to the XCD-scope driver below this many rows (0 = the kernel's limit)
        LSX_ARG(value >= 0);
        h->xrows_limit = value;
    } else if (!strcmp(key, "getri_structured")) {   // 0: the inverse as a plain solve of P*I (cross-check)
        LSX_ARG(value == 0 || value == 1);
        h->getri_plain = !value;
    } else if (!strcmp(key, "x_events")) {   // 1: the XCD-scope schedule orders its chain behind whole updates (events + gate)
        LSX_ARG(value == 0 || value == 1);
        h->x_events = value;
    } else if (!strcmp(key, "hybrid")) {   // 0: matrices taller than one XCD holds use the shared-CU schedule throughout
        LSX_ARG(value == 0 || value == 1);
        h->hybrid_off = !value;
    } else if (!strcmp(key, "prof_sample")) {   // bracket every value-th launch of a profiled bucket
        LSX_ARG(value >= 1);
        h->prof.sample = value;
    } else if (!strcmp(key, "panel_spin_limit")) {   // tests: a short limit turns a held-up panel into a time-out;
        LSX_ARG(value != 0);                           // negative: |value| and one participant arrives late
        h->panel_spin_limit = value;
    } else if (!strcmp(key, "trsv_spin_limit")) {   // tests: 0 makes the first unanswered poll a time-out
        LSX_ARG(value >= 0);
        h->spin_limit = value;
    } else if (!strcmp(key, "getri_pairs")) {   // 0: the inverse with one 128-row block per trailing update (cross-check: same bits)
        LSX_ARG(value == 0 || value == 1);
        h->getri_pairs = value;
    } else if (!strcmp(key, "left_per_step")) {   // 0: every panel's interchanges on the columns left of it in one launch at the end (cross-check)
        LSX_ARG(value == 0 || value == 1);
        h->left_per_step = value;
    } else if (!strcmp(key, "chain_fused")) {   // 0: chain head and the next panel's block solve as separate launches (cross-check)
        LSX_ARG(value == 0 || value == 1);
        h->chain_fused = value;
    } else if (!strcmp(key, "rref_first_fast")) {   // 0: LSX_PIVOT_FIRST always through the per-column kernels (cross-check)
        LSX_ARG(value == 0 || value == 1);
        h->rref_first_fast = value;
    } else if (!strcmp(key, "chain_wait_limit")) {   // tests: 0 makes the chain's wait for the update's first tile column a time-out
        LSX_ARG(value >= 0);
        h->chain_wait_limit = value;
    } else if (!strcmp(key, "panel_debug")) {
        h->panel_debug = value != 0;
    } else if (!strcmp(key, "lookahead")) {
        LSX_ARG(value == 0 || value == 1);
        h->lookahead = value;
    } else if (!strcmp(key, "lookahead_min")) {
        LSX_ARG(value >= 0);
        h->lookahead_min = value;
    } else if (!strcmp(key, "getrs_t_blocked_min")) {   // transposed solve: smallest nrhs on the blocked sweeps (n > 128); 0 = never
        LSX_ARG(value >= 0);
        h->getrs_t_blocked_min = value;
    } else if (!strcmp(key, "gesvdj_max_sweeps")) {   // Jacobi SVD: most sweeps of a call (dgesvj's NSWEEP = 30)
        LSX_ARG(value >= 1 && value <= 60);
        h->gesvdj_max_sweeps = value;
    } else if (!strcmp(key, "syevj_max_sweeps")) {   // Jacobi eigensolver: most sweeps of a call
        LSX_ARG(value >= 1 && value <= 100);
        h->syevj_max_sweeps = value;
    } else if (!strcmp(key, "potrs_few_max")) {   // Cholesky solve: largest nrhs on the few-column step kernels; 0 = never
        LSX_ARG(value >= 0 && value <= 8);
        h->potrs_few_max = value;
    } else if (!strcmp(key, "potri_order")) {   // SPD inverse, V^T V tiles: 0 = deepest first, 1 = the symmetric update's order (same bits)
        LSX_ARG(value == 0 || value == 1);
        h->potri_order = value;
    } else if (!strcmp(key, "lauum_descending")) {   // lsx_lauum_tn_*: 1 = the descending k-slabs lsx_potri_* runs, 0 = k ascending
        LSX_ARG(value == 0 || value == 1);
        h->lauum_descending = value;
    } else {
        set_error("unknown option '%s'", key);
        return LSX_ERR_ARG;
    }
    return LSX_OK;
}

int lsx_get_option(lsx_handle_t h, const char *key, int *value) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && key && value);
    if (!strcmp(key, "nb")) *value = h->nb;
    else if (!strcmp(key, "panel")) *value = h->panel_mode;
    else if (!strcmp(key, "lookahead")) *value = h->lookahead;
    else if (!strcmp(key, "lookahead_min")) *value = h->lookahead_min;
    else if (!strcmp(key, "panel_rt")) *value = h->panel_rt;
    else if (!strcmp(key, "kblock")) *value = h->kblock;
    else if (!strcmp(key, "gemm_waves")) *value = h->gemm_waves;
    else if (!strcmp(key, "gemm_stagger")) *value = h->gemm_stagger;
    else if (!strcmp(key, "trsv")) *value = h->trsv_mode;
    else if (!strcmp(key, "panel_nt")) *value = h->panel_nt;
    else if (!strcmp(key, "chain_wait_limit")) *value = h->chain_wait_limit;
    else if (!strcmp(key, "rref_first_fast")) *value = h->rref_first_fast;
    else if (!strcmp(key, "chain_fused")) *value = h->chain_fused;
    else if (!strcmp(key, "left_per_step")) *value = h->left_per_step;
    else if (!strcmp(key, "getri_pairs")) *value = h->getri_pairs;
    else if (!strcmp(key, "rref_first_used")) *value = h->rref_first_used;
    else if (!strcmp(key, "panel_fallbacks")) *value = h->panel_fallbacks;
    else if (!strcmp(key, "num_cu")) *value = h->num_cu;
    else if (!strcmp(key, "gecon_solves")) *value = h->gecon_solves;
    else if (!strcmp(key, "gerfs_steps")) *value = h->gerfs_steps;
    else if (!strcmp(key, "gerfs_solves")) *value = h->gerfs_solves;
    else if (!strcmp(key, "getrs_t_blocked_min")) *value = h->getrs_t_blocked_min;
    else if (!strcmp(key, "getrs_t_path")) *value = h->getrs_t_path;
    else if (!strcmp(key, "potrs_few_max")) *value = h->potrs_few_max;
    else if (!strcmp(key, "potrs_path")) *value = h->potrs_path;
    else if (!strcmp(key, "potri_order")) *value = h->potri_order;
    else if (!strcmp(key, "lauum_descending")) *value = h->lauum_descending;
    else if (!strcmp(key, "potri_tiles")) *value = h->potri_tiles;
    else if (!strcmp(key, "gesvdj_max_sweeps")) *value = h->gesvdj_max_sweeps;
    else if (!strcmp(key, "gesvdj_sweeps")) *value = h->gesvdj_sweeps;
    else if (!strcmp(key, "gesvdj_rotations")) *value = h->gesvdj_rotations;
    else if (!strcmp(key, "syevj_max_sweeps")) *value = h->syevj_max_sweeps;
    else if (!strcmp(key, "syevj_sweeps")) *value = h->syevj_sweeps;
    else if (!strcmp(key, "syevj_rotations")) *value = h->syevj_rotations;
    else if (!strcmp(key, "pocon_solves")) *value = h->pocon_solves;
    else if (!strcmp(key, "porfs_steps")) *value = h->porfs_steps;
    else if (!strcmp(key, "porfs_solves")) *value = h->porfs_solves;
    else { set_error("unknown option '%s'", key); return LSX_ERR_ARG; }
    return LSX_OK;
}

// ---- fp64 host
int lsx_getrf_f64(lsx_handle_t h, int n, double *A, int lda, int32_t *ipiv, int *info) {
    LSX_DEVICE_GUARD(h);
    return getrf_host<double>(h, n, A, lda, ipiv, info);
}
int lsx_getrs_f64(lsx_handle_t h, int n, int nrhs, const double *LU, int lda, const int32_t *ipiv,
                  double *B, int ldb) {
    LSX_DEVICE_GUARD(h);
    return getrs_host<double>(h, n, nrhs, LU, lda, ipiv, B, ldb);
}
int lsx_gesv_f64(lsx_handle_t h, int n, int nrhs, const double *A, int lda, double *B, int ldb,
                 int *info, double *pivot_ratio) {
    LSX_DEVICE_GUARD(h);
    return gesv_host<double>(h, n, nrhs, A, lda, B, ldb, info, pivot_ratio);
}
int lsx_getrf_f32(lsx_handle_t h, int n, float *A, int lda, int32_t *ipiv, int *info) {
    LSX_DEVICE_GUARD(h);
    return getrf_host<float>(h, n, A, lda, ipiv, info);
}
int lsx_getrs_f32(lsx_handle_t h, int n, int nrhs, const float *LU, int lda, const int32_t *ipiv,
                  float *B, int ldb) {
    LSX_DEVICE_GUARD(h);
    return getrs_host<float>(h, n, nrhs, LU, lda, ipiv, B, ldb);
}
int lsx_gesv_f32(lsx_handle_t h, int n, int nrhs, const float *A, int lda, float *B, int ldb,
                 int *info, double *pivot_ratio) {
    LSX_DEVICE_GUARD(h);
    return gesv_host<float>(h, n, nrhs, A, lda, B, ldb, info, pivot_ratio);
}

}  // extern "C"

namespace lsx {

template <typename T>
static int getri_host(lsx_handle_t h, int n, const T *A, int lda, T *Ainv, int ldi, int *info, double *pivot_ratio) {
    LSX_ARG(h && n >= 0 && lda >= n && ldi >= n);
    if (info) *info = 0;
    if (pivot_ratio) *pivot_ratio = 1.0;
    if (n == 0) return LSX_OK;
    LSX_ARG(A && Ainv);
    const int ld = ld_for(n);
    T *dA = nullptr, *dI = nullptr; int32_t *dp = nullptr; int *dinfo = nullptr; double *dprobe = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)n * ld); dI = c.take<T>((size_t)n * ld);
        dp = c.take<int32_t>(n);
        dinfo = c.take<int>(1);
        dprobe = c.take<double>(2);
    }));
    LSX_TRY(h2d<T>(h, n, n, A, lda, dA, ld));
    LSX_TRY(launch_amax<T>(h, n, n, dA, ld, dprobe));
    int hinfo = 0;
    LSX_TRY(factor_from_host<T>(h, n, A, lda, dA, ld, dp, dinfo, &hinfo));
    LSX_TRY(launch_diag_minabs<T>(h, n, dA, ld, dprobe));
    double probe[2] = {0, 0};
    LSX_HIP(hipMemcpyAsync(probe, dprobe, sizeof(probe), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = hinfo;
    if (pivot_ratio) *pivot_ratio = probe[0] > 0 ? probe[1] / probe[0] : 0.0;
    if (hinfo != 0) return LSX_OK;  // exactly singular: caller reports NoSolution (linalg.py:737)
    LSX_TRY(getri_dev<T>(h, n, dA, ld, dp, dI, ld));
    LSX_TRY(d2h<T>(h, n, n, dI, ld, Ainv, ldi));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

template <typename T>
static int det_host(lsx_handle_t h, int n, const T *A, int lda, double *sign, double *mant, int64_t *exp2) {
    LSX_ARG(h && n >= 0 && lda >= n && sign && mant && exp2);
    if (n == 0) { *sign = 1; *mant = 0.5; *exp2 = 1; return LSX_OK; }  // det([]) = 1 (linalg.py:197-199)
    LSX_ARG(A);
    const int ld = ld_for(n);
    T *dA = nullptr; int32_t *dp = nullptr; int *dinfo = nullptr; double *dout = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<T>((size_t)n * ld);
        dp = c.take<int32_t>(n);
        dinfo = c.take<int>(1);
        dout = c.take<double>(3);
    }));
    int hinfo = 0;   // a determinant of garbage factors must not be returned as a value: the status is read first
    LSX_TRY(factor_from_host<T>(h, n, A, lda, dA, ld, dp, dinfo, &hinfo));
    LSX_TRY(launch_det<T>(h, n, dA, ld, dp, dout));
    double out[3];
    LSX_HIP(hipMemcpyAsync(out, dout, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    *sign = out[0]; *mant = out[1]; *exp2 = (int64_t)out[2];
    return LSX_OK;
}


// ---------------------------------------------------------------- first-rule row reduction, blocked
// The reference pivots on the FIRST row whose entry is non-zero (linalg.py:548-552).  With rank < m or bar < n that
// choice shows in the result: the carried-along columns of a pivot row are a combination of exactly the original rows
// that became pivot rows, and which rows those are depends on the rule.  The per-column kernels (kernels_rref.hip)
// reproduce the rule at one read + write of the live matrix per column -- ~8 TB for an 8192^2 matrix of rank 4096.
// This form gets the same result from three pieces of the fast machinery:
//   1. rank r and the pivot columns pc from the blocked max-rule reduction of a copy (the rule does not change them);
//   2. G = A[:, pc] (m x r, full column rank) factored P G = L U by the blocked LU with the panel kernel under the FIRST
//      rule: P and the r pivot rows in order are the reference's own interchanges (a swap there is a swap here);
//   3. with P A = [A1; A2]:  top rows  A1[:, pc]^-1 A1  (the unique rows spanned by the pivot rows whose pivot columns are
//      unit vectors),  other rows  A2 - A2[:, pc] * top  (MFMA update) -- then exact unit / zero entries as above.
//      The factors of step 2 only NAME the rows: without magnitude pivoting their multipliers grow (3e-7 relative error
//      in a 520 x 300 integer case of rank 130 when they were used for the values), so A1[:, pc] is factored once more
//      with partial pivoting and the values come from that solve.
// fp64, up to 8192 rows (one XCD's panel); returns 1 for anything else and when the factorisation of G meets a column
// without a candidate above the tolerance (the two rules then disagree on the rank: the per-column pass decides).
// Synchronises the stream twice (rank and max |a| are needed on the host for the launch shapes).
static int rref_first_fast(lsx_handle_t h, int m, int n, int bar, double *R, int ldr, int32_t *d_pivots, int *d_rank, double tol) {
    typedef double T;
    h->rref_first_used = 0;
    const bool dbg = getenv("LSX_RREF_DEBUG") != nullptr;   // development: say why the blocked form was not taken
    if (!h->rref_first_fast || !h->rref_blocked || h->panel_mode != 4 || m > 8192 || (size_t)m * bar < (size_t)256 * 256) {
        if (dbg) fprintf(stderr, "rref_first_fast: not applicable (fast %d blocked %d panel %d m %d bar %d)\n", h->rref_first_fast, h->rref_blocked, h->panel_mode, m, bar);
        return 1;
    }
    const int nb = h->nb;
    const int rmax = m < bar ? m : bar;
    const int ldw = ld_for(n), ldg = ld_for(rmax);
    T *W = nullptr, *Gm = nullptr; int32_t *ipiv = nullptr, *ipiv2 = nullptr; int *ginfo = nullptr; double *amax = nullptr;
    LSX_TRY(carve(h, h->rref_first, [&](Carver &c) {
        W = c.take<T>((size_t)m * ldw);
        Gm = c.take<T>((size_t)m * ldg);
        ipiv = c.take<int32_t>(m); ipiv2 = c.take<int32_t>(m);
        ginfo = c.take<int>(2);
        amax = c.take<double>(1);
    }));
    // 1. rank and pivot columns
    LSX_TRY(launch_copy2d<T>(h, m, n, R, ldr, W, ldw));
    const int rb = rref_blocked<T>(h, m, n, bar, W, ldw, d_pivots, d_rank, tol, LSX_PIVOT_MAX);
    if (dbg && rb != LSX_OK) fprintf(stderr, "rref_first_fast: rref_blocked returned %d\n", rb);
    if (rb != LSX_OK) return rb;   // 1: not for the blocked form either
    LSX_TRY(launch_amax<T>(h, m, bar, R, ldr, amax));
    int r = 0;
    double hmax = 0.0;
    LSX_HIP(hipMemcpyAsync(&r, d_rank, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipMemcpyAsync(&hmax, amax, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (r <= 0) {   // nothing to pivot on: every entry left of the bar is at or below the tolerance and counts as zero
        h->rref_first_used = 1;
        return launch_rref_finish<T>(h, m, bar, R, ldr, d_pivots, 0);
    }
    if (r == m) {   // every row is a pivot row: the result does not depend on the rule
        h->rref_first_used = 1;
        return launch_copy2d<T>(h, m, n, W, ldw, R, ldr);
    }
    // the same threshold the row reductions use (kernels_rref.hip: 32 eps max(m, n) max|a|), fixed at the input's scale
    const double ftol = tol >= 0 ? tol : 32.0 * 2.220446049250313e-16 * (double)(m > n ? m : n) * hmax;
    // 2. P G = L U under the first-non-zero rule
    LSX_TRY(launch_gather_pivot_cols<T>(h, m, r, 0, R, ldr, d_pivots, Gm, ldg));
    LSX_TRY(ensure_getrf_workspace(h, m, sizeof(T)));
    T *Tinv = (T *)h->tinv.p;   // done with before getrf_dev / getrs_dev below carve tinv for themselves
    LSX_HIP(hipMemsetAsync(ginfo, 0, sizeof(int), h->stream));
    GemmPlan mfma;   // as in the LU drivers (the solve and the update of step 3 are no LU updates: plain)
    mfma.mfma_only = true;
    PanelArgs pa(h, h->moves_buf[0]);
    for (int k = 0; k < r; k += nb) {
        const int jb = (r - k < nb) ? r - k : nb;
        T *Gkk = Gm + (size_t)k * ldg + k;
        const int pr = panel_xcd_first(h, m - k, jb, Gkk, ldg, k, k, ipiv + k, ginfo, ftol, pa);
        if (dbg && pr != LSX_OK) fprintf(stderr, "rref_first_fast: panel at %d returned %d\n", k, pr);
        if (pr != LSX_OK) return pr;
        if (!pa.listed) { set_error("rref_first: panel without a gather list"); return LSX_ERR_INTERNAL; }
        LSX_TRY(launch_laswp_moves_around<T>(h, (const int2 *)pa.list, r, Gm, ldg, k, k, jb));         // the other columns of G
        const int rest = r - k - jb;
        if (rest > 0) {
            T *G12 = Gkk + jb;
            LSX_TRY(launch_trtri<T>(h, 1, jb, Gkk, ldg, Tinv));
            LSX_TRY(launch_trsm_block<T>(h, 1, jb, rest, Gkk, ldg, Tinv, G12, ldg));
            LSX_TRY(launch_gemm_sub<T>(h, m - k - jb, rest, jb, Gkk + (size_t)jb * ldg, ldg, G12, ldg, Gkk + (size_t)jb * ldg + jb, ldg, mfma));
        }
    }
    int hinfo = 0;
    LSX_HIP(hipMemcpyAsync(&hinfo, ginfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (dbg) fprintf(stderr, "rref_first_fast: rank %d, max|a| %g, tol %g, info of the first-rule LU %d\n", r, hmax, ftol, hinfo);
    if (hinfo != 0) {
        // a pivot column of the max rule without a first-rule candidate (or a time-out): R is still the input -- the
        // per-column pass decides
        if (hinfo < 0) (void)hipMemsetAsync(h->dev_status, 0, 3 * sizeof(int), h->stream);
        return 1;
    }
    // 3. P A, then the top rows A1[:, pc]^-1 A1 (a partial-pivot factorisation of the r x r block: the first-rule
    // factors above only named the rows) and the rest A2 - A2[:, pc] * top
    for (int k = 0; k < r; k += nb) LSX_TRY(launch_laswp<T>(h, n, R, ldr, k, (r - k < nb) ? r - k : nb, ipiv + k));
    LSX_TRY(launch_gather_pivot_cols<T>(h, r, r, 0, R, ldr, d_pivots, Gm, ldg));
    LSX_TRY(getrf_dev<T>(h, r, Gm, ldg, ipiv2, ginfo + 1));
    LSX_TRY(getrs_dev<T>(h, r, n, Gm, ldg, ipiv2, R, ldr));
    LSX_TRY(launch_gather_pivot_cols<T>(h, m, r, r, R, ldr, d_pivots, Gm, ldg));    // rows >= r of G <- (P A)[r:, pc]
    LSX_TRY(launch_gemm_sub<T>(h, m - r, n, r, Gm + (size_t)r * ldg, ldg, R, ldr, R + (size_t)r * ldr, ldr));
    LSX_TRY(launch_rref_finish<T>(h, m, bar, R, ldr, d_pivots, r));
    h->rref_first_used = 1;
    return LSX_OK;
}

// Row reduction under either rule: the blocked first-rule form where it applies, else kernels_rref.hip / _blk.hip.
template <typename T>
static int rref_any(lsx_handle_t h, int m, int n, int bar, T *R, int ldr, int32_t *d_pivots, int *d_rank, double tol, int pivot_rule) {
    if constexpr (sizeof(T) == 8) {
        if (pivot_rule == LSX_PIVOT_FIRST) {
            const int rc = rref_first_fast(h, m, n, bar, R, ldr, d_pivots, d_rank, tol);
            if (rc != 1) return rc;   // done, or a real error; 1: not applicable, R untouched
        }
    }
    return launch_rref<T>(h, m, n, bar, R, ldr, d_pivots, d_rank, tol, pivot_rule);
}

template <typename T>
static int rref_host(lsx_handle_t h, int m, int n, int bar_col, const T *A, int lda, T *R, int ldr, int32_t *pivots,
                     int *rank, double tol, int pivot_rule) {
    LSX_ARG(h && m >= 1 && n >= 1 && lda >= n && ldr >= n && A && R && pivots && rank);
    LSX_ARG(pivot_rule == LSX_PIVOT_FIRST || pivot_rule == LSX_PIVOT_MAX);
    const int bar = bar_col > 0 ? bar_col : n - 1;  // linalg.py:543
    LSX_ARG(bar <= n);
    const int ld = ld_for(n);
    const int np = m < n ? m : n;
    T *dR = nullptr; int32_t *dp = nullptr; int *drank = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dR = c.take<T>((size_t)m * ld);
        dp = c.take<int32_t>(2 * (size_t)np);
        drank = c.take<int>(1);
    }));
    LSX_TRY(h2d<T>(h, m, n, A, lda, dR, ld));
    LSX_TRY(rref_any<T>(h, m, n, bar, dR, ld, dp, drank, tol, pivot_rule));
    LSX_TRY(d2h<T>(h, m, n, dR, ld, R, ldr));
    int hr = 0;
    LSX_HIP(hipMemcpyAsync(&hr, drank, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    *rank = hr;
    if (hr > 0) LSX_HIP(hipMemcpy(pivots, dp, sizeof(int32_t) * 2 * hr, hipMemcpyDeviceToHost));
    return LSX_OK;
}

// Mixed-precision solve (BASELINE config 5, "tolerance 1e-4" against the fp64 result): fp32 factors, residuals
// b - A x accumulated in fp64, `sweeps` corrections through the same factors.  dA (unfactored) and dB are read,
// dLU (n x n, ldl) receives the factors, dX64 (n x nrhs) the solution in fp64, dX32 (may be NULL) its fp32 rounding.
// d_stats (4 doubles, may be NULL): max|d| and max|x| of the last sweep, then of the first.  Asynchronous.
static int gesv_refined_dev(lsx_handle_t h, int n, int nrhs, const float *dA, int lda, float *dLU, int ldl, int32_t *d_ipiv,
                            int *d_info, const float *dB, int ldb, double *dX64, int ldx, float *dX32, int ldf, int sweeps,
                            double *d_stats) {
    LSX_ARG(n >= 1 && nrhs >= 1 && dA && dLU && d_ipiv && d_info && dB && dX64 && sweeps >= 0 && sweeps <= 16);
    LSX_TRY(launch_copy2d<float>(h, n, n, dA, lda, dLU, ldl));
    LSX_TRY(getrf_dev<float>(h, n, dLU, ldl, d_ipiv, d_info));
    // correction / right-hand-side buffer: n x nrhs fp32 (rhs_work belongs to getrs)
    const int ldr = nrhs;
    float *dR = nullptr;
    LSX_TRY(carve(h, h->mixed_resid, [&](Carver &c) { dR = c.take<float>((size_t)n * ldr); }));
    int rc = launch_copy2d<float>(h, n, nrhs, dB, ldb, dR, ldr);
    if (rc == LSX_OK) rc = getrs_dev<float>(h, n, nrhs, dLU, ldl, d_ipiv, dR, ldr);
    if (rc == LSX_OK) rc = launch_refine_apply(h, n, nrhs, 1, dR, ldr, dX64, ldx, dX32, ldf, d_stats ? d_stats + 2 : nullptr);
    for (int s = 0; s < sweeps && rc == LSX_OK; ++s) {
        rc = launch_resid_mixed(h, n, nrhs, dA, lda, dB, ldb, dX64, ldx, dR, ldr);
        if (rc == LSX_OK) rc = getrs_dev<float>(h, n, nrhs, dLU, ldl, d_ipiv, dR, ldr);
        if (rc == LSX_OK) rc = launch_refine_apply(h, n, nrhs, 0, dR, ldr, dX64, ldx, dX32, ldf, d_stats);
    }
    return rc;
}

}  // namespace lsx

extern "C" {

int lsx_getri_f64(lsx_handle_t h, int n, const double *A, int lda, double *Ainv, int ldi, int *info,
                  double *pivot_ratio) {
    LSX_DEVICE_GUARD(h);
    return getri_host<double>(h, n, A, lda, Ainv, ldi, info, pivot_ratio);
}
int lsx_getri_f32(lsx_handle_t h, int n, const float *A, int lda, float *Ainv, int ldi, int *info,
                  double *pivot_ratio) {
    LSX_DEVICE_GUARD(h);
    return getri_host<float>(h, n, A, lda, Ainv, ldi, info, pivot_ratio);
}
int lsx_det_f64(lsx_handle_t h, int n, const double *A, int lda, double *sign, double *mant, int64_t *exp2) {
    LSX_DEVICE_GUARD(h);
    return det_host<double>(h, n, A, lda, sign, mant, exp2);
}
int lsx_det_f32(lsx_handle_t h, int n, const float *A, int lda, double *sign, double *mant, int64_t *exp2) {
    LSX_DEVICE_GUARD(h);
    return det_host<float>(h, n, A, lda, sign, mant, exp2);
}

// fp32 factors + fp64 residuals: X (fp32) and / or X64 (fp64) <- A^-1 B to well below the fp32 forward error
int lsx_gesv_f32_refined(lsx_handle_t h, int n, int nrhs, const float *A, int lda, const float *B, int ldb, float *X,
                         int ldx, double *X64, int ldx64, int sweeps, int *info, double *pivot_ratio,
                         double *last_correction) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs && sweeps >= 0 && sweeps <= 16);
    if (info) *info = 0;
    if (pivot_ratio) *pivot_ratio = 1.0;
    if (last_correction) *last_correction = 0.0;
    if (n == 0 || nrhs == 0) return LSX_OK;
    LSX_ARG(A && B && (X || X64) && (!X || ldx >= nrhs) && (!X64 || ldx64 >= nrhs));
    const int ld = ld_for(n), lr = ld_for(nrhs);
    float *dA = nullptr, *dLU = nullptr, *dB = nullptr, *dXf = nullptr; double *dX = nullptr, *dstats = nullptr;
    int32_t *dp = nullptr; int *dinfo = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<float>((size_t)n * ld); dLU = c.take<float>((size_t)n * ld);
        dB = c.take<float>((size_t)n * lr); dXf = c.take<float>((size_t)n * lr);
        dX = c.take<double>((size_t)n * lr);
        dp = c.take<int32_t>(n);
        dinfo = c.take<int>(1);
        dstats = c.take<double>(6);
    }));
    LSX_TRY(h2d<float>(h, n, n, A, lda, dA, ld));
    LSX_TRY(h2d<float>(h, n, nrhs, B, ldb, dB, lr));
    LSX_TRY(launch_amax<float>(h, n, n, dA, ld, dstats + 4));
    LSX_TRY(gesv_refined_dev(h, n, nrhs, dA, ld, dLU, ld, dp, dinfo, dB, lr, dX, lr, dXf, lr, sweeps, dstats));
    LSX_TRY(launch_diag_minabs<float>(h, n, dLU, ld, dstats + 4));
    int hinfo = 0;
    double st[6] = {0, 0, 0, 0, 0, 0};
    LSX_HIP(hipMemcpyAsync(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipMemcpyAsync(st, dstats, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    if (info) *info = hinfo;
    if (pivot_ratio) *pivot_ratio = st[4] > 0 ? st[5] / st[4] : 0.0;
    if (hinfo < 0) {
        set_error("panel exchange timed out on the device (workgroups not co-resident?)");
        return LSX_ERR_INTERNAL;
    }
    if (hinfo != 0) return LSX_OK;   // singular: X untouched
    LSX_TRY(check_dev_status(h));
    if (last_correction) *last_correction = st[1] > 0 ? st[0] / st[1] : 0.0;
    if (X) LSX_TRY(d2h<float>(h, n, nrhs, dXf, lr, X, ldx));
    if (X64) LSX_TRY(d2h<double>(h, n, nrhs, dX, lr, X64, ldx64));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}
int lsx_gesv_f32_refined_dev(lsx_handle_t h, int n, int nrhs, const float *dA, int lda, float *dLU, int ldl,
                             int32_t *d_ipiv, int *d_info, const float *dB, int ldb, double *dX64, int ldx, float *dX32,
                             int ldf, int sweeps, double *d_stats) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && lda >= n && ldl >= n && ldb >= nrhs && ldx >= nrhs && (!dX32 || ldf >= nrhs));
    return gesv_refined_dev(h, n, nrhs, dA, lda, dLU, ldl, d_ipiv, d_info, dB, ldb, dX64, ldx, dX32, ldf, sweeps, d_stats);
}

int lsx_matmul_f64(lsx_handle_t h, int m, int n, int k, const double *A, int lda, const double *B, int ldb,
                   double *C, int ldc) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && m >= 0 && n >= 0 && k >= 0 && lda >= k && ldb >= n && ldc >= n);
    if (m == 0 || n == 0) return LSX_OK;
    LSX_ARG(C && (k == 0 || (A && B)));
    const int la = ld_for(k > 0 ? k : 1), lb = ld_for(n), lc = ld_for(n);
    double *dA = nullptr, *dB = nullptr, *dC = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dA = c.take<double>((size_t)m * la);
        dB = c.take<double>((size_t)(k > 0 ? k : 1) * lb);
        dC = c.take<double>((size_t)m * lc);
    }));
    LSX_HIP(hipMemsetAsync(dC, 0, sizeof(double) * (size_t)m * lc, h->stream));
    if (k > 0) {
        LSX_TRY(h2d<double>(h, m, k, A, lda, dA, la));
        LSX_TRY(h2d<double>(h, k, n, B, ldb, dB, lb));
        LSX_TRY(launch_gemm_acc<double>(h, 1, m, n, k, dA, la, dB, lb, dC, lc));
    }
    LSX_TRY(d2h<double>(h, m, n, dC, lc, C, ldc));
    LSX_HIP(hipStreamSynchronize(h->stream));
    return LSX_OK;
}

int lsx_rref_f64(lsx_handle_t h, int m, int n, int bar_col, const double *A, int lda, double *R,
                 int ldr, int32_t *pivots, int *rank, double tol, int pivot_rule) {
    LSX_DEVICE_GUARD(h);
    return rref_host<double>(h, m, n, bar_col, A, lda, R, ldr, pivots, rank, tol, pivot_rule);
}
int lsx_rref_f32(lsx_handle_t h, int m, int n, int bar_col, const float *A, int lda, float *R,
                 int ldr, int32_t *pivots, int *rank, double tol, int pivot_rule) {
    LSX_DEVICE_GUARD(h);
    return rref_host<float>(h, m, n, bar_col, A, lda, R, ldr, pivots, rank, tol, pivot_rule);
}

// ---- transposed solves, norms, condition estimate
int lsx_getrs_t_f64(lsx_handle_t h, int n, int nrhs, const double *LU, int lda, const int32_t *ipiv, double *B, int ldb) {
    LSX_DEVICE_GUARD(h);
    return getrs_t_host<double>(h, n, nrhs, LU, lda, ipiv, B, ldb);
}
int lsx_getrs_t_f32(lsx_handle_t h, int n, int nrhs, const float *LU, int lda, const int32_t *ipiv, float *B, int ldb) {
    LSX_DEVICE_GUARD(h);
    return getrs_t_host<float>(h, n, nrhs, LU, lda, ipiv, B, ldb);
}
int lsx_getrs_t_f64_dev(lsx_handle_t h, int n, int nrhs, const double *dLU, int lda, const int32_t *d_ipiv, double *dB,
                        int ldb) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    return getrs_t_dev<double>(h, n, nrhs, dLU, lda, d_ipiv, dB, ldb, true);
}
int lsx_getrs_t_f32_dev(lsx_handle_t h, int n, int nrhs, const float *dLU, int lda, const int32_t *d_ipiv, float *dB,
                        int ldb) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    return getrs_t_dev<float>(h, n, nrhs, dLU, lda, d_ipiv, dB, ldb, true);
}
int lsx_lange_f64_dev(lsx_handle_t h, int norm, int m, int n, const double *dA, int lda, double *d_out) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    return lange_dev<double>(h, norm, m, n, dA, lda, d_out);
}
int lsx_lange_f32_dev(lsx_handle_t h, int norm, int m, int n, const float *dA, int lda, double *d_out) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    return lange_dev<float>(h, norm, m, n, dA, lda, d_out);
}
int lsx_gecon_f64(lsx_handle_t h, int norm, int n, const double *LU, int lda, const int32_t *ipiv, double anorm,
                  double *rcond) {
    LSX_DEVICE_GUARD(h);
    return gecon_host<double>(h, norm, n, LU, lda, ipiv, anorm, rcond);
}
int lsx_gecon_f32(lsx_handle_t h, int norm, int n, const float *LU, int lda, const int32_t *ipiv, double anorm,
                  double *rcond) {
    LSX_DEVICE_GUARD(h);
    return gecon_host<float>(h, norm, n, LU, lda, ipiv, anorm, rcond);
}
int lsx_gecon_f64_dev(lsx_handle_t h, int norm, int n, const double *dLU, int lda, const int32_t *d_ipiv, double anorm,
                      double *rcond) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    return gecon_dev<double>(h, norm, n, dLU, lda, d_ipiv, anorm, rcond);
}
int lsx_gecon_f32_dev(lsx_handle_t h, int norm, int n, const float *dLU, int lda, const int32_t *d_ipiv, double anorm,
                      double *rcond) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    return gecon_dev<float>(h, norm, n, dLU, lda, d_ipiv, anorm, rcond);
}

#define LSX_GERFS_ABI(sfx, T)                                                                                              \
    int lsx_gerfs_##sfx(lsx_handle_t h, int trans, int n, int nrhs, const T *A, int lda, const T *LU, int ldlu,           \
                        const int32_t *ipiv, const T *B, int ldb, T *X, int ldx, double *ferr, double *berr) {             \
        LSX_DEVICE_GUARD(h);                                                                                               \
        return gerfs_host<T>(h, trans, n, nrhs, A, lda, LU, ldlu, ipiv, B, ldb, X, ldx, ferr, berr);                       \
    }                                                                                                                      \
    int lsx_gerfs_##sfx##_dev(lsx_handle_t h, int trans, int n, int nrhs, const T *dA, int lda, const T *dLU, int ldlu,   \
                              const int32_t *d_ipiv, const T *dB, int ldb, T *dX, int ldx, double *ferr, double *berr) {   \
        LSX_DEVICE_GUARD(h);                                                                                               \
        LSX_ARG(h);                                                                                                        \
        return gerfs_dev<T>(h, trans, n, nrhs, dA, lda, dLU, ldlu, d_ipiv, dB, ldb, dX, ldx, ferr, berr);                  \
    }                                                                                                                      \
    int lsx_gesvr_##sfx(lsx_handle_t h, int trans, int n, int nrhs, const T *A, int lda, const T *B, int ldb, T *X,       \
                        int ldx, double *ferr, double *berr, int *info) {                                                  \
        LSX_DEVICE_GUARD(h);                                                                                               \
        return gesvr_host<T>(h, trans, n, nrhs, A, lda, B, ldb, X, ldx, ferr, berr, info);                                 \
    }                                                                                                                      \
    int lsx_diag_resid_bound_##sfx##_dev(lsx_handle_t h, int trans, int n, int nrhs, const T *dA, int lda, const T *dB,   \
                                         int ldb, const T *dX, int ldx, T *dR, T *dW, int ldr) {                           \
        LSX_DEVICE_GUARD(h);                                                                                               \
        LSX_ARG(h && (trans == 0 || trans == 1) && n >= 0 && nrhs >= 0 && nrhs <= 8 && lda >= n && ldb >= nrhs &&          \
                ldx >= nrhs && ldr >= nrhs);                                                                               \
        if (n == 0 || nrhs == 0) return LSX_OK;                                                                            \
        LSX_ARG(dA && dB && dX && dR && dW);                                                                               \
        LSX_TRY(reserve(h, h->scratch, resid_bound_work_bytes(trans, n) + 256));                                           \
        return launch_resid_bound<T>(h, trans, n, nrhs, dA, lda, dB, ldb, dX, ldx, dR, dW, ldr, (double *)h->scratch.p);   \
    }
LSX_GERFS_ABI(f64, double)
LSX_GERFS_ABI(f32, float)
#undef LSX_GERFS_ABI

int lsx_diag_resid_mixed_dev(lsx_handle_t h, int n, int nrhs, const float *dA, int lda, const float *dB, int ldb,
                             const double *dX, int ldx, float *dR, int ldr) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && n >= 0 && nrhs >= 0 && lda >= n && ldb >= nrhs && ldx >= nrhs && ldr >= nrhs);
    if (n == 0 || nrhs == 0) return LSX_OK;
    LSX_ARG(dA && dB && dX && dR);
    return launch_resid_mixed(h, n, nrhs, dA, lda, dB, ldb, dX, ldx, dR, ldr);
}
int lsx_rcond_f64(lsx_handle_t h, int norm, int n, const double *A, int lda, double *rcond, int *info) {
    LSX_DEVICE_GUARD(h);
    return rcond_host<double>(h, norm, n, A, lda, rcond, info);
}
int lsx_rcond_f32(lsx_handle_t h, int norm, int n, const float *A, int lda, double *rcond, int *info) {
    LSX_DEVICE_GUARD(h);
    return rcond_host<float>(h, norm, n, A, lda, rcond, info);
}

// ---- equilibration and the expert driver
#define LSX_GESVX_ABI(sfx, T)                                                                                              \
    int lsx_geequ_##sfx##_dev(lsx_handle_t h, int m, int n, const T *dA, int lda, T *d_r, T *d_c, double *d_stats) {       \
        LSX_DEVICE_GUARD(h);                                                                                               \
        LSX_ARG(h);                                                                                                        \
        return geequ_dev<T>(h, m, n, dA, lda, d_r, d_c, d_stats);                                                          \
    }                                                                                                                      \
    int lsx_diag_geequ_pass_##sfx##_dev(lsx_handle_t h, int passes, int m, int n, const T *dA, int lda, T *d_r, T *d_c,    \
                                        double *d_stats) {                                                                 \
        LSX_DEVICE_GUARD(h);                                                                                               \
        LSX_ARG(h);                                                                                                        \
        return geequ_dev<T>(h, m, n, dA, lda, d_r, d_c, d_stats, passes);                                                  \
    }                                                                                                                      \
    int lsx_laqge_##sfx##_dev(lsx_handle_t h, int m, int n, T *dA, int lda, const T *d_r, const T *d_c, double rowcnd,     \
                              double colcnd, double amax, int *equed) {                                                    \
        LSX_DEVICE_GUARD(h);                                                                                               \
        LSX_ARG(h);                                                                                                        \
        return laqge_dev<T>(h, m, n, dA, lda, d_r, d_c, rowcnd, colcnd, amax, equed);                                      \
    }                                                                                                                      \
    int lsx_gesvx_##sfx(lsx_handle_t h, int equil, int trans, int n, int nrhs, const T *A, int lda, const T *B, int ldb,   \
                        T *X, int ldx, int *equed, T *r, T *c, double *rcond, double *ferr, double *berr, double *rpvgrw,  \
                        int *info) {                                                                                       \
        LSX_DEVICE_GUARD(h);                                                                                               \
        return gesvx_host<T>(h, equil, trans, n, nrhs, A, lda, B, ldb, X, ldx, equed, r, c, rcond, ferr, berr, rpvgrw,     \
                             info);                                                                                        \
    }                                                                                                                      \
    int lsx_gesvx_##sfx##_dev(lsx_handle_t h, int equil, int trans, int n, int nrhs, T *dA, int lda, T *dLU, int ldlu,     \
                              int32_t *d_ipiv, T *dB, int ldb, T *dX, int ldx, int *equed, T *d_r, T *d_c, double *rowcnd, \
                              double *colcnd, double *rcond, double *ferr, double *berr, double *rpvgrw, int *info) {      \
        LSX_DEVICE_GUARD(h);                                                                                               \
        LSX_ARG(h);                                                                                                        \
        return gesvx_dev<T>(h, equil, trans, n, nrhs, dA, lda, dLU, ldlu, d_ipiv, dB, ldb, dX, ldx, d_r, d_c, equed,       \
                            rowcnd, colcnd, rcond, ferr, berr, rpvgrw, info);                                              \
    }
LSX_GESVX_ABI(f64, double)
LSX_GESVX_ABI(f32, float)
#undef LSX_GESVX_ABI

// ---- device-pointer entry points
int lsx_getrf_f64_dev(lsx_handle_t h, int n, double *dA, int lda, int32_t *d_ipiv, int *d_info) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    return getrf_dev<double>(h, n, dA, lda, d_ipiv, d_info);
}
int lsx_getrf_f32_dev(lsx_handle_t h, int n, float *dA, int lda, int32_t *d_ipiv, int *d_info) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    return getrf_dev<float>(h, n, dA, lda, d_ipiv, d_info);
}
int lsx_getrs_f64_dev(lsx_handle_t h, int n, int nrhs, const double *dLU, int lda,
                      const int32_t *d_ipiv, double *dB, int ldb) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    return getrs_dev<double>(h, n, nrhs, dLU, lda, d_ipiv, dB, ldb);
}
int lsx_getrs_f32_dev(lsx_handle_t h, int n, int nrhs, const float *dLU, int lda,
                      const int32_t *d_ipiv, float *dB, int ldb) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    return getrs_dev<float>(h, n, nrhs, dLU, lda, d_ipiv, dB, ldb);
}
int lsx_getri_f64_dev(lsx_handle_t h, int n, const double *dLU, int lda, const int32_t *d_ipiv,
                      double *dInv, int ldi) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    return getri_dev<double>(h, n, dLU, lda, d_ipiv, dInv, ldi);
}
int lsx_det_f64_dev(lsx_handle_t h, int n, const double *dLU, int lda, const int32_t *d_ipiv,
                    double *d_out) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && n >= 1 && dLU && d_ipiv && d_out);
    return launch_det<double>(h, n, dLU, lda, d_ipiv, d_out);
}
int lsx_getri_f32_dev(lsx_handle_t h, int n, const float *dLU, int lda, const int32_t *d_ipiv,
                      float *dInv, int ldi) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    return getri_dev<float>(h, n, dLU, lda, d_ipiv, dInv, ldi);
}
int lsx_det_f32_dev(lsx_handle_t h, int n, const float *dLU, int lda, const int32_t *d_ipiv,
                    double *d_out) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && n >= 1 && dLU && d_ipiv && d_out);
    return launch_det<float>(h, n, dLU, lda, d_ipiv, d_out);
}
int lsx_rref_trace_f64(lsx_handle_t h, int m, int n, int bar_col, const double *A, int lda, double *R, int ldr,
                       unsigned char *int_mask, int32_t *pivots, int *npivots, int32_t *steps, int max_steps,
                       int *nsteps, double *snaps, unsigned char *snap_int_mask, int max_snaps) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && m >= 1 && n >= 1 && lda >= n && ldr >= n && A && R && pivots && npivots && steps && nsteps);
    LSX_ARG(max_steps >= 1 && max_snaps >= 0 && (max_snaps == 0 || (snaps && snap_int_mask)));
    const int bar = bar_col > 0 ? bar_col : n - 1;  // linalg.py:543
    LSX_ARG(bar <= n);
    const int ld = ld_for(n);
    const int np = m < n ? m : n;
    const size_t snap_elems = (size_t)max_snaps * m * n;
    double *dR = nullptr, *dsn = nullptr; int32_t *dp = nullptr, *ds = nullptr; unsigned char *dst = nullptr, *dT = nullptr;
    int *dout = nullptr;
    LSX_TRY(carve(h, h->staging, [&](Carver &c) {
        dR = c.take<double>((size_t)m * ld);
        dp = c.take<int32_t>(2 * (size_t)np);
        ds = c.take<int32_t>(4 * (size_t)max_steps);
        dsn = snap_elems ? c.take<double>(snap_elems) : nullptr;
        dst = snap_elems ? c.take<unsigned char>(snap_elems) : nullptr;
        dT = c.take<unsigned char>((size_t)m * n);
        dout = c.take<int>(4);
    }));
    LSX_TRY(h2d<double>(h, m, n, A, lda, dR, ld));
    if (int_mask) LSX_HIP(hipMemcpyAsync(dT, int_mask, (size_t)m * n, hipMemcpyHostToDevice, h->stream));
    else LSX_HIP(hipMemsetAsync(dT, 0, (size_t)m * n, h->stream));
    LSX_TRY(launch_rref_trace(h, m, n, bar, dR, ld, dT, dp, ds, max_steps, dsn, dst, max_snaps, dout));
    LSX_TRY(d2h<double>(h, m, n, dR, ld, R, ldr));
    int out[3] = {0, 0, 0};
    LSX_HIP(hipMemcpyAsync(out, dout, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    LSX_HIP(hipStreamSynchronize(h->stream));
    *npivots = out[0];
    *nsteps = out[1];
    if (out[2]) { set_error("rref_trace: more than %d steps", max_steps); return LSX_ERR_ARG; }
    if (out[0] > 0) LSX_HIP(hipMemcpy(pivots, dp, sizeof(int32_t) * 2 * out[0], hipMemcpyDeviceToHost));
    if (out[1] > 0) LSX_HIP(hipMemcpy(steps, ds, sizeof(int32_t) * 4 * out[1], hipMemcpyDeviceToHost));
    const int ns = out[1] < max_snaps ? out[1] : max_snaps;
    if (ns > 0) LSX_HIP(hipMemcpy(snaps, dsn, sizeof(double) * (size_t)ns * m * n, hipMemcpyDeviceToHost));
    if (ns > 0) LSX_HIP(hipMemcpy(snap_int_mask, dst, (size_t)ns * m * n, hipMemcpyDeviceToHost));
    if (int_mask) LSX_HIP(hipMemcpy(int_mask, dT, (size_t)m * n, hipMemcpyDeviceToHost));
    return LSX_OK;
}
int lsx_rref_f64_dev(lsx_handle_t h, int m, int n, int bar_col, double *dR, int ldr,
                     int32_t *d_pivots, int *d_rank, double tol, int pivot_rule) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && m >= 1 && n >= 1 && ldr >= n && dR && d_pivots);
    LSX_ARG(pivot_rule == LSX_PIVOT_FIRST || pivot_rule == LSX_PIVOT_MAX);
    const int bar = bar_col > 0 ? bar_col : n - 1;
    LSX_ARG(bar <= n);
    return rref_any<double>(h, m, n, bar, dR, ldr, d_pivots, d_rank, tol, pivot_rule);
}

int lsx_panel_f64_dev(lsx_handle_t h, int m, int jb, double *dP, int ldp, int row0, int32_t *d_ipiv,
                      int *d_info) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && m >= 1 && jb >= 1 && jb <= 256 && dP && d_ipiv && ldp >= jb);
    LSX_TRY(reserve(h, h->scratch, panel_scratch_bytes(h, h->panel_mode, h->panel_nt, h->panel_rt, m, 8)));
    PanelArgs pa(h, h->moves_api);
    const int r = launch_panel<double>(h, m, jb, dP, ldp, row0, d_ipiv, d_info, pa);
    h->moves_api_valid = pa.listed;
    return r;
}
int lsx_laswp_f64_dev(lsx_handle_t h, int ncols, double *dA, int lda, int row0, int jb,
                      const int32_t *d_ipiv) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && dA && d_ipiv && jb >= 0 && jb <= 256);
    return launch_laswp<double>(h, ncols, dA, lda, row0, jb, d_ipiv);
}
int lsx_panel_moves_dev(lsx_handle_t h, int32_t *d_moves, int *valid) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && d_moves && valid);
    *valid = h->moves_api_valid ? 1 : 0;
    if (h->moves_api_valid)
        LSX_HIP(hipMemcpyAsync(d_moves, h->moves_api, 256 * 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
    return LSX_OK;
}
int lsx_laswp_moves_f64_dev(lsx_handle_t h, int ncols, double *dA, int lda, int row0, const int32_t *d_moves) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && dA && d_moves);
    return launch_laswp_moves<double>(h, (const int2 *)d_moves, ncols, dA, lda, row0);
}
int lsx_trsm_lu_f64_dev(lsx_handle_t h, int jb, int ncols, const double *dL, int ldl, double *dB,
                        int ldb) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && dL && dB && jb >= 1 && jb <= 256);
    double *Tinv = nullptr;
    LSX_TRY(carve(h, h->tinv, [&](Carver &c) { Tinv = c.take<double>(inv64_elems(jb)); }));
    LSX_TRY(launch_trtri<double>(h, 1, jb, dL, ldl, Tinv));
    return launch_trsm_block<double>(h, 1, jb, ncols, dL, ldl, Tinv, dB, ldb);
}
int lsx_gemm_sub_f64_dev(lsx_handle_t h, int m, int n, int k, const double *dA, int lda,
                         const double *dB, int ldb, double *dC, int ldc) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && dA && dB && dC && lda >= k && ldb >= n && ldc >= n);
    if (h->gemm_queue_test) {   // measurements: the work-queue form alone (1: all XCDs, 2: XCD 0 left out as beside a panel)
        int *avoid = nullptr, *pass = nullptr, *col0 = nullptr, *counters = nullptr;   // the words of XcdScratch, for one update
        LSX_TRY(carve(h, h->scratch, [&](Carver &c) { avoid = c.take<int>(1); pass = c.take<int>(1); col0 = c.take<int>(2); counters = c.take<int>(8); }));
        LSX_HIP(hipMemsetAsync(avoid, 0, (char *)(counters + 8) - (char *)avoid, h->stream));
        if (h->gemm_queue_test >= 2) LSX_HIP(hipMemsetD32Async((hipDeviceptr_t)avoid, 1, 1, h->stream));
        GemmPlan plan;
        plan.counters = counters;
        plan.avoid_word = h->gemm_queue_test >= 2 ? avoid : nullptr;
        plan.pass_word = pass;
        plan.col0 = h->gemm_queue_test == 3 ? col0 : nullptr;   // 3: with the column-0-first phase
        return launch_gemm_sub<double>(h, m, n, k, dA, lda, dB, ldb, dC, ldc, plan);
    }
    return launch_gemm_sub<double>(h, m, n, k, dA, lda, dB, ldb, dC, ldc);
}
int lsx_gemm_add_f64_dev(lsx_handle_t h, int m, int n, int k, const double *dA, int lda,
                         const double *dB, int ldb, double *dC, int ldc) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && dA && dB && dC && lda >= k && ldb >= n && ldc >= n);
    return launch_gemm_acc<double>(h, 1, m, n, k, dA, lda, dB, ldb, dC, ldc);
}
int lsx_gemm_sub_f32_dev(lsx_handle_t h, int m, int n, int k, const float *dA, int lda,
                         const float *dB, int ldb, float *dC, int ldc) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && dA && dB && dC && lda >= k && ldb >= n && ldc >= n);
    return launch_gemm_sub<float>(h, m, n, k, dA, lda, dB, ldb, dC, ldc);
}
int lsx_gemm_tn_sub_f64_dev(lsx_handle_t h, int m, int n, int k, const double *dA, int lda, const double *dB, int ldb,
                            double *dC, int ldc) {
    LSX_DEVICE_GUARD(h);
    return gemm_tn_dev<double>(h, 0, m, n, k, dA, lda, dB, ldb, dC, ldc);
}
int lsx_gemm_tn_add_f64_dev(lsx_handle_t h, int m, int n, int k, const double *dA, int lda, const double *dB, int ldb,
                            double *dC, int ldc) {
    LSX_DEVICE_GUARD(h);
    return gemm_tn_dev<double>(h, 1, m, n, k, dA, lda, dB, ldb, dC, ldc);
}
int lsx_gemm_tn_sub_f32_dev(lsx_handle_t h, int m, int n, int k, const float *dA, int lda, const float *dB, int ldb,
                            float *dC, int ldc) {
    LSX_DEVICE_GUARD(h);
    return gemm_tn_dev<float>(h, 0, m, n, k, dA, lda, dB, ldb, dC, ldc);
}

// ---- Cholesky
#define LSX_CHOL_ENTRIES(SFX, T)                                                                                          \
    int lsx_potrf_##SFX##_dev(lsx_handle_t h, int n, T *dA, int lda, int *d_info) {                                       \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return potrf_dev<T>(h, n, dA, lda, d_info);                                                                       \
    }                                                                                                                     \
    int lsx_potrs_##SFX##_dev(lsx_handle_t h, int n, int nrhs, const T *dU, int lda, T *dB, int ldb) {                    \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return potrs_dev<T>(h, n, nrhs, dU, lda, dB, ldb);                                                                \
    }                                                                                                                     \
    int lsx_syrk_tn_sub_##SFX##_dev(lsx_handle_t h, int n, int k, const T *dA, int lda, T *dC, int ldc) {                 \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return syrk_tn_dev<T>(h, n, k, dA, lda, dC, ldc);                                                                 \
    }                                                                                                                     \
    int lsx_potri_##SFX##_dev(lsx_handle_t h, int n, T *dU, int lda, int *d_info) {                                       \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return potri_dev<T>(h, n, dU, lda, d_info);                                                                       \
    }                                                                                                                     \
    int lsx_trtri_upper_t_##SFX##_dev(lsx_handle_t h, int n, const T *dU, int lda, T *dV, int ldv) {                      \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return trtri_upper_t_dev<T>(h, n, dU, lda, dV, ldv);                                                              \
    }                                                                                                                     \
    int lsx_lauum_tn_##SFX##_dev(lsx_handle_t h, int n, const T *dV, int ldv, T *dC, int ldc) {                           \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return lauum_tn_dev<T>(h, n, dV, ldv, dC, ldc);                                                                   \
    }                                                                                                                     \
    int lsx_symmetrize_upper_##SFX##_dev(lsx_handle_t h, int n, T *dA, int lda) {                                         \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return symmetrize_upper_dev<T>(h, n, dA, lda);                                                                    \
    }                                                                                                                     \
    int lsx_podet_##SFX##_dev(lsx_handle_t h, int n, const T *dU, int lda, double *d_out) {                               \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return podet_dev<T>(h, n, dU, lda, d_out);                                                                        \
    }                                                                                                                     \
    int lsx_potri_##SFX(lsx_handle_t h, int n, T *U, int lda, int *info) {                                                \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return potri_host<T>(h, n, U, lda, info);                                                                         \
    }                                                                                                                     \
    int lsx_poinv_##SFX(lsx_handle_t h, int n, const T *A, int lda, T *Ainv, int ldi, int *info) {                        \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return poinv_host<T>(h, n, A, lda, Ainv, ldi, info);                                                              \
    }                                                                                                                     \
    int lsx_podet_##SFX(lsx_handle_t h, int n, const T *A, int lda, double *sign, double *mant, int64_t *exp2, int *info) { \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return podet_host<T>(h, n, A, lda, sign, mant, exp2, info);                                                       \
    }                                                                                                                     \
    int lsx_potrf_##SFX(lsx_handle_t h, int n, T *A, int lda, int *info) {                                                \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return potrf_host<T>(h, n, A, lda, info);                                                                         \
    }                                                                                                                     \
    int lsx_potrs_##SFX(lsx_handle_t h, int n, int nrhs, const T *U, int lda, T *B, int ldb) {                            \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return potrs_host<T>(h, n, nrhs, U, lda, B, ldb);                                                                 \
    }                                                                                                                     \
    int lsx_posv_##SFX(lsx_handle_t h, int n, int nrhs, const T *A, int lda, T *B, int ldb, int *info) {                  \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return posv_host<T>(h, n, nrhs, A, lda, B, ldb, info);                                                            \
    }
#define LSX_POSX_ENTRIES(SFX, T)                                                                                          \
    int lsx_lansy_##SFX##_dev(lsx_handle_t h, int n, const T *dA, int lda, double *d_out) {                               \
        LSX_DEVICE_GUARD(h);                                                                                              \
        LSX_ARG(h);                                                                                                       \
        return lansy_dev<T>(h, n, dA, lda, d_out);                                                                        \
    }                                                                                                                     \
    int lsx_pocon_##SFX(lsx_handle_t h, int n, const T *U, int lda, double anorm, double *rcond) {                        \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return pocon_host<T>(h, n, U, lda, anorm, rcond);                                                                 \
    }                                                                                                                     \
    int lsx_pocon_##SFX##_dev(lsx_handle_t h, int n, const T *dU, int lda, double anorm, double *rcond) {                 \
        LSX_DEVICE_GUARD(h);                                                                                              \
        LSX_ARG(h);                                                                                                       \
        return pocon_dev<T>(h, n, dU, lda, anorm, rcond);                                                                 \
    }                                                                                                                     \
    int lsx_porcond_##SFX(lsx_handle_t h, int n, const T *A, int lda, double *rcond, int *info) {                         \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return porcond_host<T>(h, n, A, lda, rcond, info);                                                                \
    }                                                                                                                     \
    int lsx_porfs_##SFX(lsx_handle_t h, int n, int nrhs, const T *A, int lda, const T *U, int ldu, const T *B, int ldb,   \
                        T *X, int ldx, double *ferr, double *berr) {                                                      \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return porfs_host<T>(h, n, nrhs, A, lda, U, ldu, B, ldb, X, ldx, ferr, berr);                                     \
    }                                                                                                                     \
    int lsx_porfs_##SFX##_dev(lsx_handle_t h, int n, int nrhs, const T *dA, int lda, const T *dU, int ldu, const T *dB,   \
                              int ldb, T *dX, int ldx, double *ferr, double *berr) {                                      \
        LSX_DEVICE_GUARD(h);                                                                                              \
        LSX_ARG(h);                                                                                                       \
        return porfs_dev<T>(h, n, nrhs, dA, lda, dU, ldu, dB, ldb, dX, ldx, ferr, berr);                                  \
    }                                                                                                                     \
    int lsx_posvr_##SFX(lsx_handle_t h, int n, int nrhs, const T *A, int lda, const T *B, int ldb, T *X, int ldx,         \
                        double *ferr, double *berr, int *info) {                                                          \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return posvr_host<T>(h, n, nrhs, A, lda, B, ldb, X, ldx, ferr, berr, info);                                       \
    }                                                                                                                     \
    int lsx_diag_resid_bound_sym_##SFX##_dev(lsx_handle_t h, int n, int nrhs, const T *dA, int lda, const T *dB, int ldb, \
                                             const T *dX, int ldx, T *dR, T *dW, int ldr) {                               \
        LSX_DEVICE_GUARD(h);                                                                                              \
        LSX_ARG(h && n >= 0 && nrhs >= 0 && nrhs <= 8 && lda >= n && ldb >= nrhs && ldx >= nrhs && ldr >= nrhs);          \
        if (n == 0 || nrhs == 0) return LSX_OK;                                                                           \
        LSX_ARG(dA && dB && dX && dR && dW);                                                                              \
        LSX_TRY(reserve(h, h->scratch, resid_bound_sym_work_bytes(n, nrhs) + 256));                                       \
        return launch_resid_bound_sym<T>(h, n, nrhs, dA, lda, dB, ldb, dX, ldx, dR, dW, ldr, (double *)h->scratch.p);     \
    }
LSX_POSX_ENTRIES(f64, double)
LSX_POSX_ENTRIES(f32, float)
#undef LSX_POSX_ENTRIES
LSX_CHOL_ENTRIES(f64, double)
LSX_CHOL_ENTRIES(f32, float)
#undef LSX_CHOL_ENTRIES

// ---- Householder QR and least squares
#define LSX_QR_ENTRIES(SFX, T)                                                                                            \
    int lsx_geqrf_##SFX##_dev(lsx_handle_t h, int m, int n, T *dA, int lda, T *d_tau) {                                   \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return geqrf_dev<T>(h, m, n, dA, lda, d_tau);                                                                     \
    }                                                                                                                     \
    int lsx_ormqr_##SFX##_dev(lsx_handle_t h, int trans, int m, int ncols, int k, const T *dQR, int lda, const T *d_tau,  \
                              T *dC, int ldc) {                                                                           \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return ormqr_dev<T>(h, trans, m, ncols, k, dQR, lda, d_tau, dC, ldc);                                             \
    }                                                                                                                     \
    int lsx_orgqr_##SFX##_dev(lsx_handle_t h, int m, int n, int k, const T *dQR, int lda, const T *d_tau, T *dQ,          \
                              int ldq) {                                                                                  \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return orgqr_dev<T>(h, m, n, k, dQR, lda, d_tau, dQ, ldq);                                                        \
    }                                                                                                                     \
    int lsx_gels_##SFX##_dev(lsx_handle_t h, int m, int n, int nrhs, T *dA, int lda, T *d_tau, T *dB, int ldb,            \
                             int *d_info) {                                                                               \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return gels_dev<T>(h, m, n, nrhs, dA, lda, d_tau, dB, ldb, d_info);                                               \
    }                                                                                                                     \
    int lsx_colnrm2_##SFX##_dev(lsx_handle_t h, int m, int n, const T *dA, int lda, double *d_out) {                      \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return colnrm2_dev<T>(h, m, n, dA, lda, d_out);                                                                   \
    }                                                                                                                     \
    int lsx_geqrf_##SFX(lsx_handle_t h, int m, int n, T *A, int lda, T *tau) {                                            \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return geqrf_host<T>(h, m, n, A, lda, tau);                                                                       \
    }                                                                                                                     \
    int lsx_ormqr_##SFX(lsx_handle_t h, int trans, int m, int ncols, int k, const T *QR, int lda, const T *tau, T *C,     \
                        int ldc) {                                                                                        \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return ormqr_host<T>(h, trans, m, ncols, k, QR, lda, tau, C, ldc);                                                \
    }                                                                                                                     \
    int lsx_orgqr_##SFX(lsx_handle_t h, int m, int n, int k, const T *QR, int lda, const T *tau, T *Q, int ldq) {         \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return orgqr_host<T>(h, m, n, k, QR, lda, tau, Q, ldq);                                                           \
    }                                                                                                                     \
    int lsx_gels_##SFX(lsx_handle_t h, int m, int n, int nrhs, const T *A, int lda, const T *B, int ldb, T *X, int ldx,   \
                       double *resid, int *info) {                                                                        \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return gels_host<T>(h, m, n, nrhs, A, lda, B, ldb, X, ldx, resid, info);                                          \
    }
LSX_QR_ENTRIES(f64, double)
LSX_QR_ENTRIES(f32, float)
#undef LSX_QR_ENTRIES

// ---- Jacobi SVD and minimum-norm least squares
#define LSX_SVD_ENTRIES(SFX, T)                                                                                           \
    int lsx_gesvdj_##SFX##_dev(lsx_handle_t h, int jobz, int m, int n, T *dA, int lda, double *d_s, T *dU, int ldu,       \
                               T *dVt, int ldvt, int *info) {                                                             \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return gesvdj_dev<T>(h, jobz, m, n, dA, lda, d_s, dU, ldu, dVt, ldvt, info);                                      \
    }                                                                                                                     \
    int lsx_gesvdj_##SFX(lsx_handle_t h, int jobz, int m, int n, const T *A, int lda, double *s, T *U, int ldu, T *Vt,    \
                         int ldvt, int *info) {                                                                           \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return gesvdj_host<T>(h, jobz, m, n, A, lda, s, U, ldu, Vt, ldvt, info);                                          \
    }                                                                                                                     \
    int lsx_gelss_##SFX##_dev(lsx_handle_t h, int m, int n, int nrhs, T *dA, int lda, const T *dB, int ldb, T *dX,        \
                              int ldx, double rcond, double *d_s, int *rank, int *info) {                                 \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return gelss_dev<T>(h, m, n, nrhs, dA, lda, dB, ldb, dX, ldx, rcond, d_s, rank, info);                            \
    }                                                                                                                     \
    int lsx_gelss_##SFX(lsx_handle_t h, int m, int n, int nrhs, const T *A, int lda, const T *B, int ldb, T *X, int ldx,  \
                        double rcond, double *s, double *resid, int *rank, int *info) {                                   \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return gelss_host<T>(h, m, n, nrhs, A, lda, B, ldb, X, ldx, rcond, s, resid, rank, info);                         \
    }
LSX_SVD_ENTRIES(f64, double)
LSX_SVD_ENTRIES(f32, float)
#undef LSX_SVD_ENTRIES

// ---- symmetric eigensolver by two-sided Jacobi
#define LSX_EIG_ENTRIES(SFX, T)                                                                                           \
    int lsx_syevj_##SFX##_dev(lsx_handle_t h, int jobz, int n, T *dA, int lda, double *d_w, T *dV, int ldv, int *info) {  \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return syevj_dev<T>(h, jobz, n, dA, lda, d_w, dV, ldv, info);                                                     \
    }                                                                                                                     \
    int lsx_syevj_##SFX(lsx_handle_t h, int jobz, int n, const T *A, int lda, double *w, T *V, int ldv, int *info) {      \
        LSX_DEVICE_GUARD(h);                                                                                              \
        return syevj_host<T>(h, jobz, n, A, lda, w, V, ldv, info);                                                        \
    }
LSX_EIG_ENTRIES(f64, double)
LSX_EIG_ENTRIES(f32, float)
#undef LSX_EIG_ENTRIES

int lsx_fill_f64_dev(lsx_handle_t h, int kind, uint64_t seed, int m, int n, double *dA, int lda,
                     int row_off, int col_off) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && dA && lda >= n && (kind == LSX_FILL_INT5 || kind == LSX_FILL_U11));
    return launch_fill<double>(h, kind, seed, m, n, dA, lda, row_off, col_off);
}
int lsx_fill_f32_dev(lsx_handle_t h, int kind, uint64_t seed, int m, int n, float *dA, int lda,
                     int row_off, int col_off) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && dA && lda >= n && (kind == LSX_FILL_INT5 || kind == LSX_FILL_U11));
    return launch_fill<float>(h, kind, seed, m, n, dA, lda, row_off, col_off);
}

int lsx_diag_read_scratch(lsx_handle_t h, size_t offset, void *dst, size_t bytes) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && dst && offset + bytes <= h->scratch.bytes);
    LSX_HIP(hipStreamSynchronize(h->stream));
    LSX_HIP(hipMemcpy(dst, (char *)h->scratch.p + offset, bytes, hipMemcpyDeviceToHost));
    return LSX_OK;
}

int lsx_diag_mfma_peak(lsx_handle_t h, int is_f32, int iters, int blocks_per_cu, double *tflops,
                       double *clock_mhz) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && tflops && iters > 0 && blocks_per_cu >= 1 && blocks_per_cu <= 8);
    return diag_mfma_peak(h, is_f32, iters, blocks_per_cu, tflops, clock_mhz);
}

int lsx_diag_xchg_probe(lsx_handle_t h, int mode, int G, int stride, int write_through, int epochs,
                        double *us_per_epoch, int *xcc_ids, int *nfail) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && us_per_epoch && nfail && G >= 2 && G <= 64 && (stride == 1 || stride == 8) && epochs >= 1);
    LSX_ARG(mode >= 0 && mode <= 2 && (G - 1) * stride + 1 <= 8 * h->num_cu);
    return diag_xchg_probe(h, mode, G, stride, write_through, epochs, us_per_epoch, xcc_ids, nfail);
}

int lsx_diag_occupy(lsx_handle_t h, int xcc, int wgs, int ms) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && xcc >= 0 && xcc < 8 && wgs >= 1 && wgs <= 32 && ms >= 1 && ms <= 10000);
    return diag_occupy(h, xcc, wgs, ms);
}

int lsx_diag_cu_mask_probe(lsx_handle_t h, const uint32_t *mask_words, int nwords, int nblocks, uint32_t *out) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && out && nblocks >= 1 && nwords >= 0 && (nwords == 0 || mask_words));
    return diag_cu_mask_probe(h, mask_words, nwords, nblocks, out);
}

// fused = 1: chain_head_kernel (inverses + gather list in one launch); 0: trtri64_kernel alone.  dTinv: ceil(jb/64) blocks
// of 64 x 64.  d_moves: 256 int2 (dst, src), -1 = void.  Asynchronous on the handle's stream.
int lsx_diag_chain_head_f32(lsx_handle_t h, int fused, int jb, const float *dT, int ldt, float *dTinv, int ncols,
                            float *dA, int lda, int row0, const int32_t *d_moves) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && dT && dTinv && jb >= 1 && jb <= 128);
    if (!fused) return launch_trtri<float>(h, 1, jb, dT, ldt, dTinv);
    LSX_ARG(dA && d_moves);
    return diag_chain_head<float>(h, jb, dT, ldt, dTinv, ncols, dA, lda, row0, d_moves);
}
int lsx_diag_chain_head_f64(lsx_handle_t h, int fused, int jb, const double *dT, int ldt, double *dTinv, int ncols,
                            double *dA, int lda, int row0, const int32_t *d_moves) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && dT && dTinv && jb >= 1 && jb <= 128);
    if (!fused) return launch_trtri<double>(h, 1, jb, dT, ldt, dTinv);
    LSX_ARG(dA && d_moves);
    return diag_chain_head<double>(h, jb, dT, ldt, dTinv, ncols, dA, lda, row0, d_moves);
}

int lsx_getrf_mg_f64(lsx_handle_t *handles, int ndev, int n, double *const *dA, const int *lda,
                     int32_t *const *d_ipiv, int *const *d_info) {
    if (!handles || ndev < 1 || ndev > 64 || n < 1 || !dA || !lda || !d_ipiv || !d_info) {
        set_error("lsx_getrf_mg_f64: bad argument");
        return LSX_ERR_ARG;
    }
    for (int d = 0; d < ndev; ++d)
        if (!handles[d] || !d_ipiv[d] || !d_info[d]) { set_error("lsx_getrf_mg_f64: null handle or pointer for device %d", d); return LSX_ERR_ARG; }
    return getrf_mg_f64(handles, ndev, n, dA, lda, d_ipiv, d_info);
}

// ---- measurement
int lsx_prof_enable(lsx_handle_t h, int on) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    // 0 = off, 1 = every bucket, otherwise a bit mask (1 << LSX_PROF_*) shifted left by one:
    // e.g. 2 << LSX_PROF_GEMM brackets only the trailing-update launches
    h->prof.mask = on == 1 ? 0xffffffffu : (unsigned)on >> 1;
    return LSX_OK;
}

static int prof_drain(lsx_handle_t h) {
    LSX_HIP(hipStreamSynchronize(h->stream));
    Prof &p = h->prof;
    for (auto &ev : p.pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) p.ms[ev.bucket] += ms;
        p.pool.push_back(ev.a);
        p.pool.push_back(ev.b);
    }
    p.pending.clear();
    return LSX_OK;
}

int lsx_prof_reset(lsx_handle_t h) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h);
    LSX_TRY(prof_drain(h));
    for (int b = 0; b < LSX_PROF_NBUCKETS; ++b) {
        h->prof.ms[b] = 0; h->prof.launches[b] = 0; h->prof.flops[b] = 0; h->prof.bytes[b] = 0; h->prof.seen[b] = 0;
    }
    return LSX_OK;
}

int lsx_prof_read(lsx_handle_t h, int bucket, double *ms, long long *launches, double *flops,
                  double *bytes) {
    LSX_DEVICE_GUARD(h);
    LSX_ARG(h && bucket >= 0 && bucket < LSX_PROF_NBUCKETS);
    LSX_TRY(prof_drain(h));
    if (ms) *ms = h->prof.ms[bucket];
    if (launches) *launches = h->prof.launches[bucket];
    if (flops) *flops = h->prof.flops[bucket];
    if (bytes) *bytes = h->prof.bytes[bucket];
    return LSX_OK;
}

}  // extern "C"
