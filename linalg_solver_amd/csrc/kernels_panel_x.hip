// Panel factorisation with the pivot exchange at XCD scope ("panel = 4").
//
// Reference loops covered: pivot search, row swap, scaling and elimination below the pivot for jb
// consecutive pivots (linalg_solver/linalg.py:548-596).  Same arithmetic per element as every other panel
// mode (same multipliers from the same fast_recip, same fused multiply-adds in the same order), so the
// factors and the pivot sequence are bit-identical to theirs.
//
// What is different from kernels_panel_pipe.hip, and why (numbers: tools/kbench.py xchg / panelx):
//  * Scope.  At most 32 workgroups, dealt to ONE XCD (the launch has 8 G workgroups, those with
//    blockIdx % 8 == 0 take part; the others leave at once).  Exchange stores are plain stores that stay in
//    that XCD's L2 and the polling loads bypass L1 only: one hop is 0.26 us instead of 0.50-0.56 us through
//    the fabric.  Placement is verified by a device-scope handshake of XCC ids before column 0; a panel
//    whose participants do not share one id runs the same code with write-through stores.
//  * Cut.  A workgroup is 16 waves and wave w owns the eight panel columns [8w, 8w+8) of the workgroup's 64 RT rows
//    (lane l: rows 64 r + l; 128 registers per lane at four waves per SIMD, the tile takes 64).  PX_WC = 16 selects
//    the first form of this kernel, 8 waves x 16 columns with 256 registers per lane (measured slower).
//    The wave that owns the current column -- the owner wave -- runs the chain header -> winner ->
//    multipliers -> next candidate -> next header; the rank-1 update of the columns right of its own block belongs
//    to the other waves, which follow one barrier behind.
//  * Record.  A candidate is announced as ONE 128-byte record {header, 7 near granules}: the header carries
//    |a|, the row and the SIGN of the candidate, the near granules the candidate row's entries in the rest of
//    the current 8-column block.  With the sign in the header the owner forms 1/pivot and all its multipliers
//    while the winner's near granules are still in flight.  Everything right of the current block is "far":
//    published (one store per wave, the row's entries transposed across lanes through LDS) and fetched by the
//    waves that own those columns, one barrier behind (with PX_WC = 16 the owner wave's own second block included,
//    which it brings up to date after the barrier while its header shot for the next column is in flight).
//  * Arg-max.  The three-phase DPP arg-max runs its first phase only when the high word of |a| already
//    separates the candidates (ties fall back to the full form, so the choice is unchanged).
//  * Ends.  Outside its column loop (marks: PX_TMARK) a launch issues the tile's loads in front of the
//    placement handshake and the *info test, and a whole aligned panel travels through an LDS image both ways, whole rows
//    per wave instruction (px_load_tile, the scatter behind the loop); the bookkeeping follows the scatter's stores.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "panel_xchg.h"

namespace lsx {

constexpr int PX_WC = 8;      // panel columns per wave: 8 (16 waves, 128 registers per lane) or 16 (8 waves, 256)
constexpr int PX_NT = 64 * (128 / PX_WC);
constexpr int PX_REC = 128;   // bytes of one record: granule 0 = header, granules 1..7 = near values
constexpr int PX_NONE = 0x7fffffff;
// Development builds only (-DLSX_PX_SEG=k, tools/seg_panel.sh): time ONE segment of the owner step -- between
// marks k and k+1 -- with two clock reads, so that the reads' own cost is the same for every segment.
#ifndef LSX_PX_SEG
#define LSX_PX_SEG -1
#endif
#define PX_MARK(k)                                                                  \
    if (LSX_PX_SEG >= 0) {                                                          \
        if (LSX_PX_SEG == (k)) seg_t0 = __builtin_amdgcn_s_memtime();               \
        if (LSX_PX_SEG + 1 == (k)) seg_acc += __builtin_amdgcn_s_memtime() - seg_t0; \
    }

// wave-wide arg-max (largest key, lowest idx on ties); idx == PX_NONE: no candidate (key must be 0 then).
// Returns the winning idx, wave-uniform, or PX_NONE.  All 64 lanes active.
__device__ __forceinline__ int argmax64_fast(unsigned khi, unsigned klo, int idx) {
    const unsigned mhi = rows_max_u32<4>(row16_max_u32(khi), 0);
    const bool top = (khi == mhi) & (idx != PX_NONE);
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(top);
    if (mask == 0ull) return PX_NONE;
    if ((mask & (mask - 1ull)) == 0ull)   // the high word decides
        return __builtin_amdgcn_readlane(idx, __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask)));
    const unsigned mlo = rows_max_u32<4>(row16_max_u32(top ? klo : 0u), 0);
    return rows_min_i32<4>(row16_min_i32((top & (klo == mlo)) ? idx : PX_NONE), 0);
}

template <typename T>
__device__ __forceinline__ unsigned long long value_bits(T v) {
    if (sizeof(T) == 8) return (unsigned long long)__double_as_longlong((double)v);
    return (unsigned long long)__float_as_uint((float)v);
}
template <typename T>
__device__ __forceinline__ T bits_value(unsigned lo, unsigned hi) {
    if (sizeof(T) == 8) return (T)__longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    return (T)__uint_as_float(lo);
}

// ---- The tile's way between memory and registers.  In registers lane l of wave w holds rows 64 r + l, columns
// [WC w, WC w + WC): read or written directly, one instruction touches 64 rows in pieces of 16 bytes, `ldp` apart, and the
// waves fetch every 128-byte line in halves at different times.  A whole panel (jb == PC_COLS, rows 16-byte aligned) goes
// through LDS instead, one 64-row slab at a time: a wave instruction moves whole rows (64 lanes x 16 bytes = one fp64 row,
// two fp32 rows), and the lanes pick their row-per-lane pieces out of the LDS image (or put them in, on the way back).
// Bank conflicts, by the rule (not measured: no counter run of this kernel was taken).  An image row is the data plus
// one 16-byte piece, so the row pitch is 16 bytes more than a multiple of the 256-byte bank row.  A lane-per-row 16-byte
// access (lane l at l * pitch + constant) therefore lands on 16-byte slot (l + constant) mod 16.  A 16-byte LDS read is
// served in four groups of 16 lanes (lanes 0-3, 12-15 and 20-27 form the first) and a 16-byte write in groups of 8
// consecutive lanes; inside every such group the lane numbers differ mod 16, so the slots differ: no conflict.  The
// row-wise accesses (a wave reads or writes one or two whole rows) are contiguous and conflict-free in any layout.
enum { PX_PLAIN = 0, PX_WIDE = 1, PX_STAGED = 2 };
// A copy the compiler cannot see through.  The tile's entries live in registers of their own from the load to the
// scatter; handed to a 16-byte LDS access directly, they are merged into its four-register tuples for the whole kernel,
// and a tile that has to sit on aligned tuples no longer fits the budget beside store16's fixed registers.
__device__ __forceinline__ unsigned px_mov(const unsigned x) {
    unsigned y;
    asm("v_mov_b32 %0, %1" : "=v"(y) : "v"(x));
    return y;
}
__device__ __forceinline__ double px_own_reg(const double v) {
    return __hiloint2double((int)px_mov((unsigned)__double2hiint(v)), (int)px_mov((unsigned)__double2loint(v)));
}
__device__ __forceinline__ float px_own_reg(const float v) { return __uint_as_float(px_mov(__float_as_uint(v))); }
template <typename T>
struct PxImg {
    static constexpr int EPV = 16 / (int)sizeof(T);             // elements of a 16-byte piece
    static constexpr int LPR = PC_COLS / EPV;                    // lanes that cover a row: 64 (fp64), 32 (fp32)
    static constexpr int RPI = 64 / LPR;                         // rows per wave instruction
    static constexpr int NI = 64 / ((PX_NT / 64) * RPI);         // row instructions per wave and slab
    static constexpr int ROWB = PC_COLS * (int)sizeof(T) + 16;   // bytes from row to row
    static constexpr int BYTES = 64 * ROWB;
    typedef T vec __attribute__((ext_vector_type(EPV)));
};
template <typename T>
__device__ __forceinline__ int px_tile_mode(const int jb, const T *P, const int ldp) {
    if (jb != PC_COLS || (size_t)P % 16 != 0 || ldp % 2 != 0) return PX_PLAIN;
    return (ldp * sizeof(T)) % 16 == 0 ? PX_STAGED : PX_WIDE;
}
// Loads the workgroup's slice (rows >= m and columns >= jb read as zero).  The global loads are issued here and, in the
// staged form, consumed here; in the other forms they may still be in flight on return.
template <typename T, int RT>
__device__ __forceinline__ void px_load_tile(T (&a)[RT][PX_WC], const int mode, char *img, const T *__restrict__ P,
                                             const int ldp, const int m, const int jb, const int base) {
    constexpr int WC = PX_WC, NW = PX_NT / 64;
    typedef PxImg<T> I;
    typedef typename I::vec vec;
    typedef T v2t __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c0 = WC * wave;
    if (mode == PX_STAGED) {
        const int sub = lane / I::LPR, piece = lane % I::LPR;
        vec t[I::NI];
        auto issue = [&](const int r) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < I::NI; ++i) {
                const int gi = base + 64 * r + (i * NW + wave) * I::RPI + sub;
                t[i] = *(const vec *)(P + (size_t)(gi < m ? gi : 0) * ldp + I::EPV * piece);
                if (gi >= m) t[i] = vec{};
            }
        };
        issue(0);
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            if (r > 0) __syncthreads();   // the previous slab has left the image
#pragma unroll
            for (int i = 0; i < I::NI; ++i)
                *(vec *)(img + ((i * NW + wave) * I::RPI + sub) * I::ROWB + 16 * piece) = t[i];
            __syncthreads();
            if (r + 1 < RT) issue(r + 1);   // in flight while this slab is read out
#pragma unroll
            for (int k = 0; k < WC / I::EPV; ++k) {
                const vec v = *(const vec *)(img + lane * I::ROWB + (c0 + I::EPV * k) * (int)sizeof(T));
#pragma unroll
                for (int e = 0; e < I::EPV; ++e) a[r][I::EPV * k + e] = v[e];
            }
        }
    } else if (mode == PX_WIDE) {
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int gi = base + 64 * r + lane;
            const T *src = P + (size_t)(gi < m ? gi : 0) * ldp + c0;
#pragma unroll
            for (int c = 0; c < WC; c += 2) {
                const v2t v = *(const v2t *)(src + c);
                a[r][c] = gi < m ? v[0] : T(0);
                a[r][c + 1] = gi < m ? v[1] : T(0);
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int gi = base + 64 * r + lane;
            const T *src = P + (size_t)gi * ldp + c0;
#pragma unroll
            for (int c = 0; c < WC; ++c) a[r][c] = (gi < m && c0 + c < jb) ? src[c] : T(0);
        }
    }
}

// Marks of a launch outside its column loop (stamped builds only: panel_debug, -DLSX_TSTAMP), wave 0 of a workgroup:
// 0 kernel entry, 1 handshake decided, 2 tile in registers, 3 first header shot, 4 end of the column loop,
// 5 scatter issued, 6 scatter acknowledged (the last instruction).  dbg words 8-11, 13, 14: marks 1..6 minus mark 0.
// The numbers name events, not program order: mark 2 is taken in front of mark 1, because the tile is loaded in front of
// the handshake's spin.  PX_TMARK writes the `tm` array of the function it stands in; PX_TM is defined by each of the
// two (kernel and body) from its own DBG.  A stamped build drains the tile's loads in front of mark 2, which the
// production build does not: for the direct (not staged) forms its prologue is not the production schedule.
#define PX_TMARK(k) if (PX_TM) tm[k] = __builtin_amdgcn_s_memrealtime();

// FIRST (the reference's pivot rule, linalg.py:548-552, for the rank-deficient / bar_col < n row reductions of api.hip's
// rref_first): the pivot of a column is not the largest entry but the FIRST row in the current row order whose entry
// exceeds `tol`.  Rows do not move inside this kernel, so every lane carries the current POSITION of its rows (an
// interchange j <-> p sends the row that sat at position j down to p); candidates are ordered by position, the
// position travels in bits 8..21 of the header's epoch word, and a column without a candidate is reported like an
// exactly zero pivot (info = column + 1).  Everything else -- record, exchange, bookkeeping, scatter -- is shared.
template <typename T, int RT, bool DBG, bool XCD, bool FIRST = false>
__device__ __forceinline__ void panel_x_body(const int G, const int g, int m, int jb, T *__restrict__ P, int ldp,
                                             int row0, int col0, int32_t *__restrict__ ipiv,
                                             int *__restrict__ info, char *rec, XGran *far, int *status,
                                             unsigned long long *dbg, int2 *__restrict__ moves, const int spin_limit,
                                             unsigned long long (&tm)[7], T (&a)[RT][PX_WC], const int tmode, char *img,
                                             const double tol = -1.0) {
    constexpr int NT = PX_NT, WC = PX_WC;
    constexpr int NW = NT / 64;   // waves
    constexpr int RB = 64 * RT;   // panel rows per workgroup
    constexpr int NONE = PX_NONE;
#define PX_TM (DBG || LSX_TS_MARKS)
    __shared__ T s_l[2][RB];                                   // multipliers of column j, by slice-local row
    // x: winner row (-1 none), y: bit0 act, bit1 failed, z: candidate of the next column (slice-local, -1 none)
    __shared__ __attribute__((aligned(16))) int4 s_info[2];
    __shared__ int s_cl2;                                      // candidate chosen at a wave boundary
    __shared__ int s_hist[PC_COLS], s_topid[PC_COLS], s_postop[PC_COLS];
    __shared__ int s_mark[PC_COLS];                            // top row d is the pivot of some column (gather list)
    __shared__ int s_order[RB];
    __shared__ __attribute__((aligned(16))) T s_stage[NW][WC];   // per wave: a row's entries on their way across lanes

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = g * RB;
    const int c0 = WC * wave;           // first panel column of this wave
    const bool has_cols = c0 < jb;
    const int nown = (jb + WC - 1) / WC;   // waves that own columns

    unsigned long long seg[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // DBG: 100 MHz ticks per segment (slot 15 of dbg: XCC id)
    unsigned long long seg_t0 = 0, seg_acc = 0;             // LSX_PX_SEG builds: shader clocks of the chosen segment
    unsigned long long tlast = 0;
#define STAMP(i)                                                              \
    if (DBG && LSX_PX_SEG < 0) {                                              \
        const unsigned long long tn_ = __builtin_amdgcn_s_memrealtime();      \
        seg[i] += tn_ - tlast;                                                \
        tlast = tn_;                                                          \
    }

    // one descriptor per exchange region, shared by the builtin loads and the inline-asm loads / stores
    // far granule rows: a ring of four columns.  The waves that consume them run one barrier behind their
    // owner wave, so a workgroup can still be reading column j - 1 while a faster one publishes column j + 1.
    const __amdgpu_buffer_rsrc_t r_rec = __builtin_amdgcn_make_buffer_rsrc(rec, 0, 2 * G * PX_REC, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_far =
        __builtin_amdgcn_make_buffer_rsrc(far, 0, 4 * G * PC_COLS * (int)sizeof(XGran), 0x00020000);
#define d_rec r_rec
#define d_far r_far

    typedef T v2t __attribute__((ext_vector_type(2)));
    for (int t = tid; t < PC_COLS; t += NT) { s_topid[t] = t; s_postop[t] = t; s_mark[t] = 0; }
    for (int t = tid; t < RB; t += NT) s_order[t] = -1;
    unsigned frozen = 0;  // bit r: local row 64 r + lane already used as a pivot (or outside the panel)
#pragma unroll
    for (int r = 0; r < RT; ++r)
        if (base + 64 * r + lane >= m) frozen |= 1u << r;
    int pos[FIRST ? RT : 1];   // FIRST: current position of row r of this lane in the panel's row order
    if (FIRST) {
#pragma unroll
        for (int r = 0; r < RT; ++r) pos[r] = base + 64 * r + lane;
    }
    constexpr unsigned EMASK = FIRST ? 0xffu : 0x7fffffffu;   // epoch bits of a header's fourth word
    // the interchange of column j (winner row `win` sat at position wpos): whatever sat at position j goes to wpos
    auto track_swap = [&](const int j, const int win, const int wpos) __attribute__((always_inline)) {
        if (FIRST) {
#pragma unroll
            for (int r = 0; r < RT; ++r)
                if (pos[r] == j && base + 64 * r + lane != win) pos[r] = wpos;
        }
    };
    bool failed = false;
    u4 hA = u4{0u, 0u, 0u, 0u}, hB = u4{0u, 0u, 0u, 0u};   // the two pre-issued header shots
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the tile is in registers before the column loop
    __syncthreads();

    // replay of interchange jj on the position maps (one lane; LAPACK order bookkeeping)
    auto replay = [&](int jj) __attribute__((always_inline)) {
        const int c = s_hist[jj] & 0x3fffffff;
        const bool zero_piv = (s_hist[jj] >> 30) & 1;
        const int p = (c < jb) ? s_postop[c] : c;
        const int d = s_topid[jj];
        if (p != jj) {
            s_topid[jj] = c;
            if (p < jb) s_topid[p] = d;
            s_postop[d] = p;
            if (c < jb) s_postop[c] = jj;
        }
        if (g == 0) {
            ipiv[jj] = row0 + p;
            if (zero_piv && info && *info == 0) *info = col0 + jj + 1;
        }
    };

    // header shot at column jn, pre-issued (lane q reads the header of workgroup q): the compiler does not
    // know the load is in flight.  Shot A is issued before the step's barrier, shot B right after it and
    // nothing else in between or behind: "at most one outstanding" means A has landed.  B is drained (wait_b)
    // before its registers are read or given up -- a load in flight must never see its registers reassigned.
    auto shot_async = [&](u4 &h, const int jn) __attribute__((always_inline)) {
        const int off = ((jn & 1) * G + (lane < G ? lane : 0)) * PX_REC;
        asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen sc1" : "+v"(h) : "v"(off), "s"(d_rec));
    };
    auto wait_a = [&]() __attribute__((always_inline)) { asm volatile("s_waitcnt vmcnt(1)" : "+v"(hA), "+v"(hB)); };
    auto wait_b = [&]() __attribute__((always_inline)) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(hA), "+v"(hB)); };
    // Exchange stores are inline asm.  (i) Given builtin stores inside the `row == k` ladders below, hipcc turns a
    // ladder into an indexed read of a stack copy of the whole tile (the tile then lives in scratch for the entire
    // kernel).  (ii) Given the 16-byte store operand as one register tuple, it builds that tuple in place around the
    // tile entry -- every fp64 entry then wants a four-register home and the tile no longer fits.  So the asm takes
    // the four dwords separately and assembles the tuple itself in the top four registers of the budget, which the
    // kernel gives up for this
    // (the budget at two waves per SIMD is 256 registers either way).  s_nop: a store wider than 64 bits reads its
    // data registers for two more cycles.
    auto store16 = [&](const unsigned lo, const unsigned hi, const unsigned z, const unsigned w, const int off,
                       const __amdgpu_buffer_rsrc_t &desc) __attribute__((always_inline)) {
#define LSX_ST16(R0, R1, R2, R3, POL)                                                                                   \
    asm volatile("v_mov_b32 v" #R0 ", %0\n\tv_mov_b32 v" #R1 ", %1\n\tv_mov_b32 v" #R2 ", %2\n\tv_mov_b32 v" #R3 ", %3\n\t"    \
                 "buffer_store_dwordx4 v[" #R0 ":" #R3 "], %4, %5, 0 offen" POL "\n\ts_nop 1"                             \
                 : : "v"(lo), "v"(hi), "s"(z), "v"(w), "v"(off), "s"(desc) : "v" #R0, "v" #R1, "v" #R2, "v" #R3)
        if (WC == 8) {   // 16 waves: the budget is 128 registers
            if (XCD) LSX_ST16(124, 125, 126, 127, ""); else LSX_ST16(124, 125, 126, 127, " sc1");
        } else {
            if (XCD) LSX_ST16(252, 253, 254, 255, ""); else LSX_ST16(252, 253, 254, 255, " sc1");
        }
#undef LSX_ST16
    };
    // header of column jn: {|a| of the candidate (fp64 bits), row (-1: none), epoch jn + 1 | sign << 31}
    auto store_header = [&](const int jn, const double val, const int row, const bool neg, const int rpos = 0)
                            __attribute__((always_inline)) {
        store16((unsigned)__double2loint(val), (unsigned)__double2hiint(val),
                (unsigned)__builtin_amdgcn_readfirstlane(row),
                (unsigned)(jn + 1) | (neg ? 0x80000000u : 0u) | (FIRST ? ((unsigned)rpos << 8) : 0u),
                ((jn & 1) * G + g) * PX_REC, d_rec);
    };
    // granule of column jn: {value bits, epoch jn + 1, 0}
    auto store_gran = [&](const __amdgpu_buffer_rsrc_t &desc, const int off, const T v, const int jn) __attribute__((always_inline)) {
        unsigned lo, hi;
        if (sizeof(T) == 8) { lo = (unsigned)__double2loint((double)v); hi = (unsigned)__double2hiint((double)v); }
        else { lo = __float_as_uint((float)v); hi = 0u; }
        store16(lo, hi, (unsigned)(jn + 1), 0u, off, desc);
    };
    // Owner wave, all lanes: candidates on tile column CN, arg-max, record of column jn = header + near granules
    // (the rest of CN's 8-column block).  Returns the slice-local candidate row (-1: none), wave-uniform.
    auto choose_and_announce = [&](auto CNt, const int jn) __attribute__((always_inline)) -> int {
        constexpr int CN = decltype(CNt)::value;
        double nv = -1.0;
        int ni = NONE;
        int np = NONE;   // FIRST: the candidate's position
#pragma unroll
        for (int r = 0; r < RT; ++r) {   // rows of a lane ascend with r: the first maximum is the lowest row
            const double av = fabs((double)a[r][CN]);
            bool better;
            if (FIRST) better = (((frozen >> r) & 1u) == 0u) & (av > tol) & (pos[r] < np);
            else better = (((frozen >> r) & 1u) == 0u) & (av > nv);
            nv = better ? av : nv;
            ni = better ? base + 64 * r + lane : ni;
            if (FIRST) np = better ? pos[r] : np;
        }
        const unsigned long long kb = (ni != NONE) ? (unsigned long long)__double_as_longlong(nv) : 0ull;
        // FIRST: the key is the position, inverted (the arg-max then finds the first row); positions are unique
        const int win = FIRST ? argmax64_fast((ni != NONE) ? (unsigned)(0x7fffffff - np) : 0u, 0u, ni)
                              : argmax64_fast((unsigned)(kb >> 32), (unsigned)kb, ni);
        const bool have = win != NONE;
        const int cl = have ? win - base : -1;
        if (have) {
            if (lane == (cl & 63)) {
                const int ck = cl >> 6;
                const int roff = ((jn & 1) * G + g) * PX_REC;
#pragma unroll
                for (int k = 0; k < RT; ++k)
                    if (ck == k) {
                        store_header(jn, fabs((double)a[k][CN]), win, a[k][CN] < T(0), FIRST ? pos[k] : 0);
#pragma unroll
                        for (int c = (CN & 7) + 1; c < 8; ++c)
                            store_gran(d_rec, roff + 16 * c, a[k][(CN & 8) + c], jn);
                    }
            }
        } else if (lane == 0) {
            store_header(jn, 0.0, -1, false);
        }
        return cl;
    };
    // Far granules of column jn: this wave's entries [CLO, CLO + NC) of slice-local row cl.  The lane that holds
    // the row writes them to the wave's LDS staging line, NC lanes read one each and store it: ONE store
    // instruction per wave instead of NC single-lane ones (LDS runs in order within a wave: no barrier).
    // All of it inline asm -- see store16 for what hipcc does to tile entries inside a `row == k` ladder.
    const unsigned stage_addr = (unsigned)(unsigned long long)(T __attribute__((address_space(3))) *)&s_stage[wave][0];
    auto publish_far = [&](auto CLOt, auto NCt, const int jn, const int cl_) __attribute__((always_inline)) {
        constexpr int CLO = decltype(CLOt)::value, NC = decltype(NCt)::value;
        const int cl = __builtin_amdgcn_readfirstlane(cl_);
        if (cl < 0 || !has_cols) return;
        if (lane == (cl & 63)) {
            const int ck = cl >> 6;
#pragma unroll
            for (int k = 0; k < RT; ++k)
                if (ck == k) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        if (sizeof(T) == 8)
                            asm volatile("ds_write_b64 %0, %1 offset:%2" : : "v"(stage_addr), "v"(a[k][CLO + c]), "n"(8 * c) : "memory");
                        else
                            asm volatile("ds_write_b32 %0, %1 offset:%2" : : "v"(stage_addr), "v"(a[k][CLO + c]), "n"(4 * c) : "memory");
                    }
                }
        }
        const int q = lane & (NC - 1);
        unsigned lo, hi = 0u;
        if (sizeof(T) == 8) {
            double v;
            asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(stage_addr + 8u * q) : "memory");
            lo = (unsigned)__double2loint(v); hi = (unsigned)__double2hiint(v);
        } else {
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(lo) : "v"(stage_addr + 4u * q) : "memory");
        }
        if (lane < NC)
            store16(lo, hi, (unsigned)(jn + 1), 0u, (((jn & 3) * G + g) * PC_COLS + c0 + CLO + q) * (int)sizeof(XGran), d_far);
    };
    // Rank-1 update of this wave's tile columns [CLO, CLO + NC) for column j: multipliers from LDS, the pivot
    // row's entries from the far granules of the winner's workgroup bg.  false: the granules never came.
    auto far_update = [&](auto CLOt, auto NCt, const int j, const int bg) __attribute__((always_inline)) -> bool {
        constexpr int CLO = decltype(CLOt)::value, NC = decltype(NCt)::value;
        const int off = (((j & 3) * G + bg) * PC_COLS + c0 + CLO + (lane & (NC - 1))) * (int)sizeof(XGran);
        u4 v;
        int spins = failed ? spin_limit : 0;
        for (;;) {
            v = __builtin_amdgcn_raw_buffer_load_b128(r_far, off, opaque_zero(), 16);
            if (!__any(v.z != (unsigned)(j + 1))) break;
            if (++spins > spin_limit) return false;
        }
        T l[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) l[r] = s_l[j & 1][64 * r + lane];
        // a -= l * u with u taken straight from the lane that loaded it: a DPP operand (row_newbcast: lane c of the
        // reader's own 16-lane row; every row holds the NC granules) instead of a readlane into scalar registers per
        // entry.  (-u) * l + a is the same fused multiply-add as a - l * u.  s_nop: a DPP read of a register the
        // previous instruction wrote needs two wait states, which the assembler does not insert inside asm.
        const T un = -bits_value<T>(v.x, v.y);
        asm volatile("s_nop 1" : : "v"(un));
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                if (sizeof(T) == 8)
                    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                                 : "+v"(a[r][CLO + c]) : "v"(un), "v"(l[r]), "n"(c));
                else
                    asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                                 : "+v"(a[r][CLO + c]) : "v"(un), "v"(l[r]), "n"(c));
            }
        }
        return true;
    };
    typedef std::integral_constant<int, 0> I0;
    typedef std::integral_constant<int, 8> I8;
    typedef std::integral_constant<int, WC> IWC;
    // the step of a wave that does not own column j (owner wave ow): follow the owner one barrier behind
    auto follow = [&](const int j, const int ow) __attribute__((always_inline)) {
        const int par = j & 1;
        const bool stamp = DBG && wave == ow + 1;
        if (stamp) tlast = __builtin_amdgcn_s_memrealtime();
        __syncthreads();
        if (stamp) STAMP(4)
        const int4 inf = s_info[par];
        const int wrow = inf.x;
        const bool act = (inf.y & 1) != 0;
        failed |= (inf.y & 2) != 0;
        const bool valid = wrow >= 0;
        const int bg = valid ? wrow / RB : 0;
        // bookkeeping on a wave that is not the owner: the last wave while wave 0 owns, wave 0 afterwards
        if (wave == (ow == 0 ? NW - 1 : 0) && lane == 63) {
            s_hist[j] = valid ? (wrow | (act ? 0 : (1 << 30))) : j;
            if (j > 0) replay(j - 1);
            if (valid && bg == g) s_order[wrow - base] = j;
        }
        if (valid && bg == g) {
            const int wl = wrow - base;
            if ((wl & 63) == lane) frozen |= 1u << (wl >> 6);
        }
        if (valid) track_swap(j, wrow, inf.w);
        bool ok = true;
        if (act && wave > ow && has_cols) ok = far_update(I0{}, IWC{}, j, bg);
        if (stamp) STAMP(5)
        if (!ok && !failed) {
            failed = true;
            if (lane == 0) atomicExch(status, 1);
        }
        if (j + 1 < jb) {
            if ((j & 7) < 7) {
                if (wave > ow) publish_far(I0{}, IWC{}, j + 1, inf.z);
            } else {
                // block boundary: the candidate of column j + 1 is chosen behind this step's update -- by the
                // owner wave itself in the middle of its sixteen columns, by wave ow + 1 at their end
                const bool hand_over = (j & (WC - 1)) == WC - 1;
                if (hand_over && wave == ow + 1) {
                    __builtin_amdgcn_s_setprio(3);
                    const int cl = choose_and_announce(I0{}, j + 1);
                    if (lane == 0) s_cl2 = cl;
                    shot_async(hA, j + 1);
                }
                __syncthreads();
                const int nown_ = hand_over ? ow + 1 : ow;
                if (hand_over && wave == ow + 1) {
                    if constexpr (WC == 16) publish_far(I8{}, I8{}, j + 1, s_cl2);
                    shot_async(hB, j + 1);
                }
                else if (wave > nown_) publish_far(I0{}, IWC{}, j + 1, s_cl2);
            }
        }
        if (stamp) STAMP(6)
    };

    // one column in its owner wave; CJ = j & 15 (the tile column) is a compile-time constant
    auto own = [&](auto CJt, const int j) __attribute__((always_inline)) {
        constexpr int CJ = decltype(CJt)::value;
        constexpr int JC = CJ & 7;        // column inside its 8-column block
        constexpr int CB = CJ & 8;        // tile column of the block's first column
        constexpr bool FIRSTB = WC == 16 && CJ < 8;   // the wave's first block: its second block is "far" and follows behind
        constexpr bool NEAR = JC < 7;     // the block has columns right of j
        const int par = j & 1;
        const bool more = j + 1 < jb;
        if (DBG && CJ == 0) tlast = __builtin_amdgcn_s_memrealtime();
        PX_MARK(0)
        // ---------------- O1: all headers of column j, the winner
        bool failed_now = failed;
        bool pend = lane < G;
        unsigned hlo = 0u, hhi = 0u, hneg = 0u;
        int hrow = NONE;
        int hpos = 0;
        auto absorb = [&](const u4 &h) __attribute__((always_inline)) {
            const bool ok = pend & ((h.w & EMASK) == (unsigned)(j + 1));
            hlo = ok ? h.x : hlo;
            hhi = ok ? h.y : hhi;
            hneg = ok ? (h.w >> 31) : hneg;
            if (FIRST) hpos = ok ? (int)((h.w >> 8) & 0x3fffu) : hpos;
            hrow = ok ? ((int)h.z >= 0 ? (int)h.z : NONE) : hrow;
            pend = ok ? false : pend;
        };
        // Shots in flight: in the second block and at a block start A (before the previous barrier) and B (after
        // it); inside the first block only A, and it has landed: the second block's far load behind it was waited for
        constexpr bool TWO = !FIRSTB || JC == 0;
        if (TWO) wait_a(); else wait_b();
        PX_MARK(1)
        absorb(hA);
        if (__any(pend)) {
            if (TWO) { wait_b(); absorb(hB); }
            int spins = failed ? spin_limit : 0;
            while (__any(pend)) {
                if (++spins > spin_limit) { failed_now = true; break; }
                const u4 h = __builtin_amdgcn_raw_buffer_load_b128(
                    r_rec, (par * G + (lane < G ? lane : 0)) * PX_REC, opaque_zero(), 16);
                absorb(h);
            }
        }
        const bool hv = hrow != NONE;
        const int win = FIRST ? argmax64_fast(hv ? (unsigned)(0x7fffffff - hpos) : 0u, 0u, hrow)
                              : argmax64_fast(hv ? hhi : 0u, hv ? hlo : 0u, hrow);
        const bool valid = (win != NONE) & !failed_now;
        const int bg = valid ? win / RB : 0;     // lane bg holds the winner's header
        const int wpos = FIRST ? __builtin_amdgcn_readlane(hpos, bg) : 0;
        const unsigned plo = (unsigned)__builtin_amdgcn_readlane((int)hlo, bg);
        const unsigned phi = (unsigned)__builtin_amdgcn_readlane((int)hhi, bg);
        const bool pneg = __builtin_amdgcn_readlane((int)hneg, bg) != 0;
        const double pabs = __longlong_as_double((long long)(((unsigned long long)phi << 32) | plo));
        PX_MARK(2)
        STAMP(0)
        // ---------------- O2: the winner's near granules -- issued now, consumed after the multipliers, which
        // need only |pivot| and its sign from the header
        const bool act = valid & (pabs != 0.0);
        const bool fetch = NEAR && more && act;
        u4 nq = u4{0u, 0u, 0u, 0u};
        const int noff = (par * G + bg) * PX_REC + 16 * (lane & 7);
        if (fetch) nq = __builtin_amdgcn_raw_buffer_load_b128(r_rec, noff, opaque_zero(), 16);
        PivotRecip<T> rinv = act ? pivot_recip<T>((T)pabs) : PivotRecip<T>{T(1), T(0)};
        if (pneg) rinv.rinv = -rinv.rinv;   // fast_recip is odd: the same bits as pivot_recip(pivot)
        if (valid && bg == g) {
            const int wl = win - base;
            if ((wl & 63) == lane) frozen |= 1u << (wl >> 6);
        }
        if (valid) track_swap(j, win, wpos);
        T l[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const T v = rinv.apply(a[r][CJ]);
            l[r] = ((frozen >> r) & 1u) ? T(0) : v;
            s_l[par][64 * r + lane] = l[r];
            a[r][CJ] = (act & (((frozen >> r) & 1u) == 0u)) ? l[r] : a[r][CJ];
        }
        PX_MARK(3)
        wait_b();   // shot B (unread when A was complete) and the granule load have landed
        bool upd = false;   // the granules are valid: the block takes the update of this column
        if (fetch) {
            int spins = 0;
            for (;;) {
                const int q = lane & 7;
                if (!__any((q > JC) & (nq.z != (unsigned)(j + 1)))) break;
                if (++spins > spin_limit) { failed_now = true; break; }
                nq = __builtin_amdgcn_raw_buffer_load_b128(r_rec, noff, opaque_zero(), 16);
            }
            upd = !failed_now;
        }
        STAMP(1)
        PX_MARK(4)
        if (upd) {   // the same DPP-operand form as far_update: lane c of every 16-lane row holds granule c
            const T un = -bits_value<T>(nq.x, nq.y);
            asm volatile("s_nop 1" : : "v"(un));
#pragma unroll
            for (int c = JC + 1; c < 8; ++c) {
#pragma unroll
                for (int r = 0; r < RT; ++r) {
                    if (sizeof(T) == 8)
                        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                                     : "+v"(a[r][CB + c]) : "v"(un), "v"(l[r]), "n"(c));
                    else
                        asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                                     : "+v"(a[r][CB + c]) : "v"(un), "v"(l[r]), "n"(c));
                }
            }
        }
        PX_MARK(5)
        // ---------------- O3: candidate and record of the next column (at a block end: behind the barrier)
        int cl = -1;
        if (NEAR && more) cl = choose_and_announce(std::integral_constant<int, (CJ < WC - 1 ? CJ + 1 : WC - 1)>{}, j + 1);
        PX_MARK(6)
        const bool act2 = act & !failed_now;
        if (lane == 0) s_info[par] = make_int4(valid ? win : -1, (act2 ? 1 : 0) | (failed_now ? 2 : 0), cl, wpos);
        if (failed_now && !failed) {
            failed = true;
            if (lane == 0) atomicExch(status, 1);
        }
        if (NEAR && more) shot_async(hA, j + 1);
        STAMP(2)
        PX_MARK(7)
        __syncthreads();
        if (!FIRSTB && NEAR && more) shot_async(hB, j + 1);
        PX_MARK(8)
        STAMP(3)
        if constexpr (FIRSTB) { if (more) {
            // the second block follows behind the barrier like any far block; at the end of the first block it is
            // brought up to date BEFORE its first column's candidate is chosen (second barrier: see follow)
            bool ok = true;
            if (act2) ok = far_update(I8{}, I8{}, j, bg);
            if (!ok && !failed) {
                failed = true;
                if (lane == 0) atomicExch(status, 1);
            }
            if (NEAR) {
                publish_far(I8{}, I8{}, j + 1, cl);
            } else {
                const int cl8 = choose_and_announce(I8{}, j + 1);
                if (lane == 0) s_cl2 = cl8;
                shot_async(hA, j + 1);
                __syncthreads();
                shot_async(hB, j + 1);
            }
            STAMP(7)
        } } else if (!NEAR && more) {
            __syncthreads();   // end of the wave's columns: the hand-over barrier (see follow)
        }
    };

    // ---- column 0: wave 0 announces, the others publish their part of its candidate row
    if (wave == 0) {
        __builtin_amdgcn_s_setprio(3);
        const int cl = choose_and_announce(I0{}, 0);
        if (lane == 0) s_cl2 = cl;
        shot_async(hA, 0);
        PX_TMARK(3)
    }
    __syncthreads();
    if (wave == 0) {
        if constexpr (WC == 16) publish_far(I8{}, I8{}, 0, s_cl2);
        shot_async(hB, 0);
    }
    else publish_far(I0{}, IWC{}, 0, s_cl2);

    for (int ow = 0; ow < nown; ++ow) {
        const int j0 = WC * ow;
        if (wave == ow) {
#define COL(k) if constexpr (k < WC) { if (j0 + k < jb) own(std::integral_constant<int, k>{}, j0 + k); }
            COL(0) COL(1) COL(2) COL(3) COL(4) COL(5) COL(6) COL(7)
            COL(8) COL(9) COL(10) COL(11) COL(12) COL(13) COL(14) COL(15)
#undef COL
            __builtin_amdgcn_s_setprio(0);
        } else {
            for (int k = 0; k < WC; ++k)
                if (j0 + k < jb) follow(j0 + k, ow);
        }
    }
    PX_TMARK(4)
    if (DBG && lane == 0)
        for (int i = 0; i < 8; ++i) atomicAdd(&dbg[g * 16 + i], seg[i]);
    if (DBG && LSX_PX_SEG >= 0 && lane == 0) atomicAdd(&dbg[g * 16 + 12], seg_acc);
#undef STAMP
#undef d_rec
#undef d_far
    __syncthreads();
    // ---- behind the loop.  Every row goes straight to its final (LAPACK-order) position; the stores are issued first,
    // the bookkeeping that only touches LDS and small global words follows them.  One barrier publishes the last replay
    // (its s_postop entries are destinations), the pivot marks and, in the staged form, the first slab's image.
    if (tid == NT - 1) replay(jb - 1);   // the keeper recorded s_hist[jb - 1]; only its replay is left
    // a workgroup whose exchange timed out reports it through info (negative = protocol failure):
    // the host entry points turn that into LSX_ERR_INTERNAL instead of returning garbage factors
    if (failed && info && lane == 0) atomicMin(info, -0x40000000);
    const bool list = g == 0 && moves;
    if (list)
        for (int t = tid; t < jb; t += NT) {
            const int c = s_hist[t] & 0x3fffffff;
            if (c < PC_COLS) s_mark[c] = 1;
        }
    auto dest_of = [&](const int lr) __attribute__((always_inline)) -> int {
        const int gi = base + lr, ord = s_order[lr];
        return ord >= 0 ? ord : (gi < jb ? s_postop[gi] : gi);
    };
    if (tmode == PX_STAGED) {
        typedef PxImg<T> I;
        typedef typename I::vec vec;
        const int sub = lane / I::LPR, piece = lane % I::LPR;
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            if (r > 0) __syncthreads();   // the previous slab has left the image
#pragma unroll
            for (int k = 0; k < WC / I::EPV; ++k) {
                vec v;
#pragma unroll
                for (int e = 0; e < I::EPV; ++e) v[e] = px_own_reg(a[r][I::EPV * k + e]);
                *(vec *)(img + lane * I::ROWB + (c0 + I::EPV * k) * (int)sizeof(T)) = v;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < I::NI; ++i) {
                const int sr = (i * NW + wave) * I::RPI + sub;
                if (base + 64 * r + sr < m) {
                    // opaque: most rows stay where they were, and given the chance the compiler keeps the load's
                    // row addresses alive through the column loop (in scratch) to select them here
                    int dest = dest_of(64 * r + sr);
                    asm volatile("" : "+v"(dest));
                    *(vec *)(P + (size_t)dest * ldp + I::EPV * piece) = *(const vec *)(img + sr * I::ROWB + 16 * piece);
                }
            }
        }
    } else {
        __syncthreads();
        if (has_cols) {
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const int lr = 64 * r + lane;
                if (base + lr < m) {
                    T *dst = P + (size_t)dest_of(lr) * ldp + c0;
                    if (tmode == PX_WIDE) {
#pragma unroll
                        for (int c = 0; c < WC; c += 2) {
                            v2t v;
                            v[0] = a[r][c]; v[1] = a[r][c + 1];
                            *(v2t *)(dst + c) = v;
                        }
                    } else {
#pragma unroll
                        for (int c = 0; c < WC; ++c)
                            if (c0 + c < jb) dst[c] = a[r][c];
                    }
                }
            }
        }
    }
    PX_TMARK(5)
    // ---- the same permutation as a gather list for the columns outside the panel:
    // final[row0 + dst] = old[row0 + src]; slot j: pivot j, slot PC_COLS + d: displaced top row d
    if (list) {
        for (int t = tid; t < 2 * PC_COLS; t += NT) {
            int dst = -1, src = -1;
            if (t < jb) {
                dst = t;
                src = s_hist[t] & 0x3fffffff;
            } else if (t >= PC_COLS && t - PC_COLS < jb) {
                const int d = t - PC_COLS;
                if (!s_mark[d]) { dst = s_postop[d]; src = d; }
            }
            if (dst == src) dst = src = -1;
            moves[t] = make_int2(dst, src);
        }
    }
    if (PX_TM) {
        __builtin_amdgcn_s_waitcnt(0x0F70);   // the scatter's stores are acknowledged
        PX_TMARK(6)
        if (tid == 0) {
            if (DBG && dbg) {
                const int slot[7] = {0, 8, 9, 10, 11, 13, 14};
                for (int k = 1; k < 7; ++k) dbg[g * 16 + slot[k]] = tm[k] - tm[0];
            }
            for (int k = 0; k < 7; ++k) LSX_TS_MARK(1, k, tm[k]);
        }
    }
#undef PX_TM
}

// 8 G workgroups, the G with blockIdx.x % 8 == 0 take part.  `xcc` (G words, zero at launch) is the placement
// handshake: participant g stores 1 + its XCC id device-scope, everybody reads all G (bounded spin) and takes the
// XCD-scope protocol only if all ids agree -- the decision is a function of the same G words for every
// participant, so they all take the same branch.
template <typename T, int RT, bool DBG, bool FIRST = false>
__global__ __launch_bounds__(PX_NT, PX_NT / 256) void panel_x_kernel(int m, int jb, T *__restrict__ P, int ldp, int row0, int col0,
                                                        int32_t *__restrict__ ipiv, int *__restrict__ info,
                                                        char *rec, XGran *far, int *status, unsigned long long *dbg,
                                                        int2 *__restrict__ moves, int *xcc, int *xcc_word,
                                                        int spin_limit, double tol) {
    if (blockIdx.x & 7) return;
    LSX_TS(1);
#define PX_TM (DBG || LSX_TS_MARKS)
    unsigned long long tm[7] = {0, 0, 0, 0, 0, 0, 0};
    PX_TMARK(0)
    const int G = gridDim.x >> 3, g = blockIdx.x >> 3;
    if (spin_limit < 0) {   // fault injection (tests): the last participant shows up ~3 ms late, the others give up
        spin_limit = -spin_limit;
        if (g == G - 1 && G > 1)
            for (int i = 0; i < 900; ++i) __builtin_amdgcn_s_sleep(127);
    }
    // Order of the prologue: the XCC id goes out first, then the tile's loads and the load of *info are issued, and only
    // then does anything wait -- the handshake spin, the early return on *info < 0 and the protocol choice consume their
    // results with the tile already on its way (in the staged form: already in registers).
    __shared__ int s_same;
    // Staging image of one 64-row slab: 66,560 bytes in fp64, 33,792 in fp32.  With the bodies' own arrays (both
    // instantiations count) a workgroup asks for 75-83 KB of the CU's 160 KB in fp64 -- more than 64 KB, and more than
    // half a CU.  That costs no occupancy: 16 waves at 128 registers are one workgroup per CU already.  The seven
    // workgroups of every eight that leave at once ask for the same amount while they last.
    __shared__ __attribute__((aligned(16))) char s_img[PxImg<T>::BYTES];
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(id));
    if (threadIdx.x == 0) {
        __hip_atomic_store(&xcc[g], (int)id + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // for the trailing update that runs beside this panel (gemm_sub_queue_kernel stays off this XCD)
        if (g == 0 && xcc_word) __hip_atomic_store(xcc_word, (int)id + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int info_v = info ? *info : 0;
    T a[RT][PX_WC];
    const int tmode = px_tile_mode(jb, P, ldp);
    px_load_tile<T, RT>(a, tmode, s_img, P, ldp, m, jb, g * 64 * RT);
    if (PX_TM) __builtin_amdgcn_s_waitcnt(0x0F70);   // stamped builds: the mark means what it says in every form
    PX_TMARK(2)
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        bool pend = lane < G, same = true;
        int spins = 0;
        while (__any(pend)) {
            const int v = __hip_atomic_load(&xcc[lane < G ? lane : 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (pend && v != 0) { pend = false; same = v == (int)id + 1; }
            if (++spins > spin_limit) { same = false; break; }
        }
        const bool all_same = !__any(!same);
        if (lane == 0) {
            s_same = all_same ? 1 : 0;
            if (DBG && dbg) dbg[g * 16 + 15] = ((unsigned long long)id << 8) | (all_same ? 1u : 0u);
        }
    }
    __syncthreads();
    PX_TMARK(1)
#undef PX_TM
    // an earlier panel of this factorisation already failed (exchange time-out): do not spin again.  The tile's loads
    // were issued in front of this test: none of them is left in flight on the way out.
    __builtin_amdgcn_s_waitcnt(0x0F70);
    if (__builtin_amdgcn_readfirstlane(info_v) < 0) {
        // Leave an EMPTY gather list behind.  The driver's later launches apply this panel's list whatever became of the
        // panel; left as it was, the list is that of an earlier factorisation on this handle, and its rows -- counted
        // from this panel's first row -- can lie past the end of a smaller matrix.
        if (g == 0 && moves)
            for (int t = threadIdx.x; t < 2 * PC_COLS; t += PX_NT) moves[t] = make_int2(-1, -1);
        return;
    }
    if (__builtin_amdgcn_readfirstlane(s_same)) {
        panel_x_body<T, RT, DBG, true, FIRST>(G, g, m, jb, P, ldp, row0, col0, ipiv, info, rec, far, status, dbg, moves, spin_limit, tm, a, tmode, s_img, tol);
    } else {
        // The write-through form loads the tile again.  The compiler lays the two bodies out one behind the other, so
        // a tile handed to both stays alive -- in scratch -- through all of the first body's column loop; this form
        // runs only when the placement failed and gives up the early load instead.
        T a2[RT][PX_WC];   // (the first load's image has been read: the barrier behind the handshake)
        px_load_tile<T, RT>(a2, tmode, s_img, P, ldp, m, jb, g * 64 * RT);
        panel_x_body<T, RT, DBG, false, FIRST>(G, g, m, jb, P, ldp, row0, col0, ipiv, info, rec, far, status, dbg, moves, spin_limit, tm, a2, tmode, s_img, tol);
    }
}

// One exchange area, in the order the kernel and the tools' stamp readers rely on: status word at 0, XCC handshake words
// at +64 | records[2][G] at 256 | far granule rows[4][G][128] | debug stamps at the next 256-byte boundary.  Records and
// granules are multiples of 256 bytes, so taken in this order the Carver's alignment leaves them back to back.
struct XArea {
    int *status, *xcc; char *rec; XGran *far; unsigned long long *dbg = nullptr;
    size_t bytes;   // all of it is zero at every launch
    void lay(Carver &c, int G, bool debug) {
        status = c.take<int>(64), xcc = status + 16;
        rec = c.take<char>((size_t)2 * G * PX_REC);
        far = c.take<XGran>((size_t)4 * G * PC_COLS);
        if (debug) dbg = c.take<unsigned long long>((size_t)G * 16);
        bytes = c.off;
    }
};
// Rows per lane (RT) and workgroups (G, of 64 RT rows; 0 = height not served): as few rows per lane as the panel's height
// allows with at most 32 workgroups -- 1 up to 2048 rows, 2 up to 4096, 4 up to 8192, and in fp32 (which has the registers)
// 8 up to 16384.  The owner wave's per-column work (multipliers, update of its block, choice of the next candidate) is
// proportional to RT and outweighs the dearer all-gather of more workgroups: 4 -> 2 -> 1 took 8192^2 fp64 from 17.1 to 16.6 to
// 16.3 ms and 4096^2 from 6.95 to 6.36 to 6.23 ms, 8 -> 4 took 8192^2 fp32 from 16.9 to 14.5 ms.  Same arithmetic per element, same pivots.
struct XShape { int rt, G; };
static XShape x_shape(lsx_handle_t h, int m, size_t elem) {
    const int rt = m <= 32 * 64 * 1 ? 1 : m <= 32 * 64 * 2 ? 2 : (elem == 4 && m > 32 * 64 * 4) ? 8 : 4;
    const int G = (m + 64 * rt - 1) / (64 * rt);
    return {rt, (G > 32 || G > h->num_cu) ? 0 : G};
}

size_t panel_x_area_bytes(lsx_handle_t h, int mode, int m, size_t elem, bool for_driver) {
    if (mode != 4 || (for_driver && (h->panel_debug || h->nb > PC_COLS))) return 0;
    m = std::min(m, 32 * 64 * (elem == 8 ? 4 : 8));   // taller panels take the device-scope kernel (its own area size)
    const size_t need = max_over_heights(m, for_driver, [&](int mm) {
        const int G = x_shape(h, mm, elem).G;
        return G ? carve_bytes([&](Carver &c) { XArea().lay(c, G, h->panel_debug); }) : (size_t)0;
    });
    return (need + 255) & ~(size_t)255;   // a driver takes several, back to back
}

// Returns 1 when the shape is outside what the kernel serves (caller falls back to the device-scope kernel).
template <typename T, int RT>
static int panel_xcd_rt(lsx_handle_t h, int m, int jb, T *P, int ldp, int row0, int col0, int32_t *d_ipiv, int *d_info,
                        PanelArgs &pa, const double first_tol = -1.0) {
    const int G = x_shape(h, m, sizeof(T)).G;
    if (jb > PC_COLS || G == 0) return 1;
    XArea a;
    LSX_TRY(carve_in(pa.area, pa.area_bytes, "panel_xcd", [&](Carver &c) { a.lay(c, G, h->panel_debug); }));
    if (!pa.cleared) LSX_HIP(hipMemsetAsync(a.status, 0, a.bytes, h->stream));
    if (first_tol >= 0.0) {   // the reference's first-non-zero rule (fp64, up to 8192 rows: callers check)
        if constexpr (sizeof(T) == 8 && RT <= 4)
            hipLaunchKernelGGL((panel_x_kernel<T, RT, false, true>), dim3(8 * G), dim3(PX_NT), 0, h->stream, m, jb, P, ldp, row0,
                               col0, d_ipiv, d_info, a.rec, a.far, a.status, a.dbg, (int2 *)pa.list, a.xcc, pa.xcc_word, h->panel_spin_limit, first_tol);
        else
            return 1;
    } else if (h->panel_debug)
        hipLaunchKernelGGL((panel_x_kernel<T, RT, true>), dim3(8 * G), dim3(PX_NT), 0, h->stream, m, jb, P, ldp, row0,
                           col0, d_ipiv, d_info, a.rec, a.far, a.status, a.dbg, (int2 *)pa.list, a.xcc, pa.xcc_word, h->panel_spin_limit, -1.0);
    else
        hipLaunchKernelGGL((panel_x_kernel<T, RT, false>), dim3(8 * G), dim3(PX_NT), 0, h->stream, m, jb, P, ldp, row0,
                           col0, d_ipiv, d_info, a.rec, a.far, a.status, a.dbg, (int2 *)pa.list, a.xcc, pa.xcc_word, h->panel_spin_limit, -1.0);
    LSX_HIP(hipGetLastError());
    pa.listed = true;
    return LSX_OK;
}

template <typename T>
int panel_xcd(lsx_handle_t h, int m, int jb, T *P, int ldp, int row0, int col0, int32_t *d_ipiv, int *d_info, PanelArgs &pa) {
    const int rt = x_shape(h, m, sizeof(T)).rt;
    if (rt == 1) return panel_xcd_rt<T, 1>(h, m, jb, P, ldp, row0, col0, d_ipiv, d_info, pa);
    if (rt == 2) return panel_xcd_rt<T, 2>(h, m, jb, P, ldp, row0, col0, d_ipiv, d_info, pa);
    if (rt == 8) return panel_xcd_rt<T, sizeof(T) == 4 ? 8 : 4>(h, m, jb, P, ldp, row0, col0, d_ipiv, d_info, pa);
    return panel_xcd_rt<T, 4>(h, m, jb, P, ldp, row0, col0, d_ipiv, d_info, pa);
}

// The same panel under the reference's pivot rule (first row in the current order with |a| > tol); fp64, at most 8192
// rows.  Returns 1 for anything else.
int panel_xcd_first(lsx_handle_t h, int m, int jb, double *P, int ldp, int row0, int col0, int32_t *d_ipiv, int *d_info,
                    double tol, PanelArgs &pa) {
    pa.listed = false;
    if (tol < 0.0 || m > 32 * 64 * 4) return 1;
    if (m <= 32 * 64 * 1) return panel_xcd_rt<double, 1>(h, m, jb, P, ldp, row0, col0, d_ipiv, d_info, pa, tol);
    if (m <= 32 * 64 * 2) return panel_xcd_rt<double, 2>(h, m, jb, P, ldp, row0, col0, d_ipiv, d_info, pa, tol);
    return panel_xcd_rt<double, 4>(h, m, jb, P, ldp, row0, col0, d_ipiv, d_info, pa, tol);
}

template int panel_xcd<double>(lsx_handle_t, int, int, double *, int, int, int, int32_t *, int *, PanelArgs &);
template int panel_xcd<float>(lsx_handle_t, int, int, float *, int, int, int, int32_t *, int *, PanelArgs &);

}  // namespace lsx

LSX_TS_SETTER(panelx)
