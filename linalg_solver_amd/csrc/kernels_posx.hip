// Condition estimate and error bounds for the Cholesky family (lsx_pocon_*, lsx_porfs_*, api.hip): the kernels that
// read a symmetric matrix, or an upper factor, from its upper triangle alone.  DESIGN section 3.8.
//
//   sym_part / sym_final   r = b - A x and w = |b| + |A| |x| for up to 8 columns, A symmetric, upper triangle stored.
//                          One workgroup per 128 x 128 tile (I, J), J >= I, the tile in registers in the layout of
//                          tile_gemv_t (kernels_trsvt.hip): a lane holds 16 bytes of RPT rows.  From the same registers
//                          it forms the row part A_IJ x_J (a sum along the lanes of a row: a fixed halving tree of
//                          shuffles) and, for the elements strictly above the diagonal, the column part A_IJ^T x_I
//                          (a sum down the thread's rows, then over the row groups through LDS, ascending).  Every
//                          stored a_ij, j > i, is loaded once and used twice, a diagonal element once.  The diagonal
//                          tile predicates its LOADS on col >= row.  Block row b receives one partial sum per tile
//                          column: slot s comes from tile (min(s, b), max(s, b)), the diagonal tile adds its two parts
//                          itself, so every slot of the workspace P[t][t * 128][ncols][2] is written exactly once.  The
//                          second kernel adds the slots in ascending order and forms r and w.
//   sym_part<NORM>         the same pass with x = 1: the slots' second halves are the absolute row sums of the tile
//                          parts, which sym_norm_final adds and maximises (lansy: 1-norm = infinity-norm; NaN wins).
//   posx_back_step         U x = y for up to 8 right-hand sides, one launch per 128-row block step from the last block
//                          upwards, no workgroup waits for another.  Workgroup j < k forms b_j -= U[j, k] x_k (row sums
//                          of a tile strictly above the diagonal blocks), and the one that owns block k - 1 then applies
//                          inv(U_jj) from launch_chol_inv's natural-orientation inverse with the same routine.  The
//                          forward half, U^T y = b, is trsvt_step_kernel as it is (launch_trsvt_forward_upper).
// Sums are accumulated in fp64 in the residual pass and the norm (rounded once), in T in the solve; every order is fixed
// and there are no floating-point atomics: two calls give identical bits, a column's bits do not depend on the columns
// that ride along (one column is processed after the other), nor on lda or alignment (the element-wise form of a load
// fills the same registers).  Nothing below the diagonal of A or U is loaded, nothing of either is written.
#include "common.h"

namespace lsx {

constexpr int PB = 128;    // tile edge
constexpr int PNR = 8;     // columns per pass

template <typename T>
struct PosTile {
    static constexpr int CPL = 16 / (int)sizeof(T);   // columns per lane: one 16-byte load
    static constexpr int LPR = PB / CPL;              // lanes per tile row (fp64: 64, fp32: 32)
    static constexpr int G = 256 / LPR;               // row groups of a workgroup (fp64: 4, fp32: 8)
    static constexpr int RPT = PB / G;                // rows per thread (fp64: 32, fp32: 16)
    static_assert(RPT * 2 == LPR, "the halving tree pairs every row of a thread with one lane pair");
};

static __device__ __forceinline__ double posx_nan_max(const double a, const double b) { return (b > a || b != b) ? b : a; }

// v[u] of lane cg: the lane's share of the sum of the thread's row u.  The LPR lanes of a tile row exchange halves:
// at distance d the lane with bit d set keeps the upper half of what it still holds and hands over the lower half.
// Afterwards v[0] of lanes 2u and 2u + 1 holds the whole sum of row u, always added in the same order.
template <typename S, int RPT, int DIST>
struct RowReduce {
    static __device__ __forceinline__ void run(S (&v)[RPT], const int cg) {
        constexpr int cnt = DIST >> 1;
        const bool up = (cg & DIST) != 0;
#pragma unroll
        for (int i = 0; i < cnt; ++i) {
            const S keep = up ? v[i + cnt] : v[i];
            const S send = up ? v[i] : v[i + cnt];
            v[i] = keep + __shfl_xor(send, DIST, 64);
        }
        RowReduce<S, RPT, cnt>::run(v, cg);
    }
};
template <typename S, int RPT>
struct RowReduce<S, RPT, 1> {
    static __device__ __forceinline__ void run(S (&v)[RPT], const int) { v[0] += __shfl_xor(v[0], 1, 64); }
};
template <typename S, int RPT>
__device__ __forceinline__ void row_reduce(S (&v)[RPT], const int cg) {
    RowReduce<S, RPT, RPT>::run(v, cg);
}

// a[u][d] <- M[g + G u][c0 + d] of a 128 x 128 tile at M.  vec: base and ld allow 16-byte loads; rows >= rows_ok and
// columns >= cols_ok are not read, nor, with upper, anything with column < row (they count as zero).  A 16-byte load
// is taken only where all its elements are wanted.
template <typename T>
__device__ __forceinline__ void tile_load(const T *__restrict__ M, const int ld, const bool vec, const int rows_ok,
                                          const int cols_ok, const bool upper, T (&a)[PosTile<T>::RPT][PosTile<T>::CPL]) {
    typedef PosTile<T> S;
    typedef T vt __attribute__((ext_vector_type(S::CPL)));
    const int tid = threadIdx.x, cg = tid % S::LPR, g = tid / S::LPR, c0 = cg * S::CPL;
#pragma unroll
    for (int u = 0; u < S::RPT; ++u) {
        const int r = g + S::G * u;
        const T *p = M + (size_t)r * ld + c0;
        const bool rok = r < rows_ok;
        if (vec && rok && c0 + S::CPL <= cols_ok && (!upper || c0 >= r)) {
            const vt v = *(const vt *)p;
#pragma unroll
            for (int d = 0; d < S::CPL; ++d) a[u][d] = v[d];
        } else {
#pragma unroll
            for (int d = 0; d < S::CPL; ++d) a[u][d] = (rok && c0 + d < cols_ok && (!upper || c0 + d >= r)) ? p[d] : T(0);
        }
    }
}

// ------------------------------------------------------------------ symmetric residual and bound, symmetric norm
// grid (t, t), t = ceil(n / 128): workgroup (J, I) = (blockIdx.x, blockIdx.y) with J >= I owns tile (I, J).
// P[((s * npad + i) * ncols + q) * 2 + {0: A x, 1: |A| |x|}], npad = 128 t: slot s of row i, column q.
template <typename T, bool NORM>
__global__ __launch_bounds__(256) void sym_part_kernel(int n, int ncols, const T *__restrict__ A, int lda,
                                                       const T *__restrict__ X, int ldx, double *__restrict__ P) {
    typedef PosTile<T> S;
    const int I = blockIdx.y, J = blockIdx.x;
    if (J < I) return;
    __shared__ double xJ[PB * PNR], xI[PB * PNR];
    __shared__ double part[S::G][PB][2];
    __shared__ double cs[PB][2];
    __shared__ double dgs[PB];
    const int tid = threadIdx.x, cg = tid % S::LPR, g = tid / S::LPR, c0 = cg * S::CPL;
    const int ri = I * PB, cj = J * PB;
    const bool diag = I == J;
    const size_t npad = (size_t)gridDim.x * PB;
    for (int e = tid; e < PB * ncols; e += 256) {
        const int k = e / ncols, q = e % ncols;
        if (NORM) {
            xJ[k * PNR + q] = cj + k < n ? 1.0 : 0.0;
            xI[k * PNR + q] = ri + k < n ? 1.0 : 0.0;
        } else {
            xJ[k * PNR + q] = cj + k < n ? (double)X[(size_t)(cj + k) * ldx + q] : 0.0;
            xI[k * PNR + q] = ri + k < n ? (double)X[(size_t)(ri + k) * ldx + q] : 0.0;
        }
    }
    T a[S::RPT][S::CPL];
    const bool vec = ((size_t)A % 16 == 0) && (lda % S::CPL == 0);
    tile_load<T>(A + (size_t)ri * lda + cj, lda, vec, n - ri, n - cj, diag, a);
    if (diag) {   // a diagonal element is used once: it leaves the registers (every thread holds at most one)
#pragma unroll
        for (int u = 0; u < S::RPT; ++u)
#pragma unroll
            for (int d = 0; d < S::CPL; ++d)
                if (c0 + d == g + S::G * u) {
                    dgs[c0 + d] = (double)a[u][d];
                    a[u][d] = T(0);
                }
    }
    __syncthreads();
#pragma unroll 1
    for (int q = 0; q < ncols; ++q) {
        // row part into pr / pw; column part (the same elements once more, for the rows that mirror them) into ar / aw
        double ar[S::CPL], aw[S::CPL];
#pragma unroll
        for (int d = 0; d < S::CPL; ++d) ar[d] = aw[d] = 0.0;
        double pr[S::RPT], pw[S::RPT];
#pragma unroll
        for (int u = 0; u < S::RPT; ++u) {
            const int r = g + S::G * u;
            const double xr = xI[r * PNR + q];
            double sr = 0.0, sw = 0.0;
#pragma unroll
            for (int d = 0; d < S::CPL; ++d) {
                const double av = (double)a[u][d];
                const double xc = xJ[(c0 + d) * PNR + q];
                sr = __builtin_fma(av, xc, sr);
                sw = __builtin_fma(fabs(av), fabs(xc), sw);
                ar[d] = __builtin_fma(av, xr, ar[d]);
                aw[d] = __builtin_fma(fabs(av), fabs(xr), aw[d]);
            }
            pr[u] = sr;
            pw[u] = sw;
        }
#pragma unroll
        for (int d = 0; d < S::CPL; ++d) {
            part[g][c0 + d][0] = ar[d];
            part[g][c0 + d][1] = aw[d];
        }
        row_reduce<double, S::RPT>(pr, cg);
        row_reduce<double, S::RPT>(pw, cg);
        __syncthreads();
        if (tid < PB) {
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int gg = 0; gg < S::G; ++gg) {
                s0 += part[gg][tid][0];
                s1 += part[gg][tid][1];
            }
            if (diag) {
                cs[tid][0] = s0;
                cs[tid][1] = s1;
            } else {                                           // slot I of block row J
                double *o = P + (((size_t)I * npad + cj + tid) * ncols + q) * 2;
                o[0] = s0;
                o[1] = s1;
            }
        }
        __syncthreads();
        if ((cg & 1) == 0) {                                   // slot J of block row I
            const int r = g + S::G * (cg >> 1);
            double s0 = pr[0], s1 = pw[0];
            if (diag) {                                        // row part + column part + the diagonal term
                const double dv = dgs[r], xd = xJ[r * PNR + q];
                s0 = __builtin_fma(dv, xd, s0 + cs[r][0]);
                s1 = __builtin_fma(fabs(dv), fabs(xd), s1 + cs[r][1]);
            }
            double *o = P + (((size_t)J * npad + ri + r) * ncols + q) * 2;
            o[0] = s0;
            o[1] = s1;
        }
    }
}

// thread = one row, blockIdx.y = right-hand side: the slots in ascending order, then r and w
template <typename T>
__global__ __launch_bounds__(256) void sym_final_kernel(int n, int t, int ncols, const double *__restrict__ P,
                                                        const T *__restrict__ B, int ldb, T *__restrict__ R,
                                                        T *__restrict__ W, int ldr) {
    const int i = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y;
    if (i >= n) return;
    const size_t npad = (size_t)t * PB;
    double rs = 0, ws = 0;
    for (int s = 0; s < t; ++s) {
        const double *p = P + (((size_t)s * npad + i) * ncols + q) * 2;
        rs += p[0];
        ws += p[1];
    }
    const double b = (double)B[(size_t)i * ldb + q];
    R[(size_t)i * ldr + q] = (T)(b - rs);
    W[(size_t)i * ldr + q] = (T)(fabs(b) + ws);
}

constexpr int SN_T = 1024;
// one workgroup: the absolute row sums from the slots (ascending), then their maximum
__global__ __launch_bounds__(SN_T) void sym_norm_final_kernel(int n, int t, const double *__restrict__ P,
                                                              double *__restrict__ out) {
    __shared__ double s_v[SN_T];
    const size_t npad = (size_t)t * PB;
    double v = 0;
    for (int i = threadIdx.x; i < n; i += SN_T) {
        double ws = 0;
        for (int s = 0; s < t; ++s) ws += P[((size_t)s * npad + i) * 2 + 1];
        v = posx_nan_max(v, ws);
    }
    s_v[threadIdx.x] = v;
    __syncthreads();
    for (int k = SN_T / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) s_v[threadIdx.x] = posx_nan_max(s_v[threadIdx.x], s_v[threadIdx.x + k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = s_v[0];
}

// bytes of the slot workspace of the symmetric pass over ncols columns (lansy: 1): t slots of 128 t rows, two sums each
size_t resid_bound_sym_work_bytes(int n, int ncols) {
    if (n <= 0 || ncols <= 0) return 0;
    const size_t t = (size_t)(n + PB - 1) / PB;
    return sizeof(double) * t * t * PB * (size_t)ncols * 2;
}

template <typename T>
int launch_resid_bound_sym(lsx_handle_t h, int n, int ncols, const T *A, int lda, const T *B, int ldb, const T *X, int ldx,
                           T *R, T *W, int ldr, double *d_work) {
    if (n <= 0 || ncols <= 0) return LSX_OK;
    if (ncols > PNR) {
        set_error("launch_resid_bound_sym: at most 8 right-hand sides per pass");
        return LSX_ERR_INTERNAL;
    }
    const int t = (n + PB - 1) / PB;
    ProfScope ps(h, LSX_PROF_OTHER, 4.0 * n * (double)n * ncols, sizeof(T) * (double)n * (n + 1) / 2);
    hipLaunchKernelGGL((sym_part_kernel<T, false>), dim3(t, t), dim3(256), 0, h->stream, n, ncols, A, lda, X, ldx, d_work);
    hipLaunchKernelGGL(sym_final_kernel<T>, dim3((n + 255) / 256, ncols), dim3(256), 0, h->stream, n, t, ncols,
                       (const double *)d_work, B, ldb, R, W, ldr);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// d_out[0] = the 1-norm (= infinity-norm) of the symmetric matrix; d_work: resid_bound_sym_work_bytes(n, 1) bytes
template <typename T>
int launch_lansy(lsx_handle_t h, int n, const T *A, int lda, double *d_work, double *d_out) {
    if (n <= 0) {
        LSX_HIP(hipMemsetAsync(d_out, 0, sizeof(double), h->stream));
        return LSX_OK;
    }
    const int t = (n + PB - 1) / PB;
    ProfScope ps(h, LSX_PROF_OTHER, (double)n * n, sizeof(T) * (double)n * (n + 1) / 2);
    hipLaunchKernelGGL((sym_part_kernel<T, true>), dim3(t, t), dim3(256), 0, h->stream, n, 1, A, lda, (const T *)nullptr, 0,
                       d_work);
    hipLaunchKernelGGL(sym_norm_final_kernel, dim3(1), dim3(SN_T), 0, h->stream, n, t, (const double *)d_work, d_out);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// ------------------------------------------------------------------ U x = y, few right-hand sides
// s[u] (lanes 2u, 2u + 1 of row group g) <- row g + G u of  M (128 x 128 in registers) * xs[:, q]
template <typename T, int NR>
__device__ __forceinline__ void tile_gemv_rows(const T (&a)[PosTile<T>::RPT][PosTile<T>::CPL], const T *xs, const int q,
                                               T (&s)[PosTile<T>::RPT]) {
    typedef PosTile<T> S;
    const int cg = threadIdx.x % S::LPR, c0 = cg * S::CPL;
    T x[S::CPL];
#pragma unroll
    for (int d = 0; d < S::CPL; ++d) x[d] = xs[(c0 + d) * NR + q];
#pragma unroll
    for (int u = 0; u < S::RPT; ++u) {
        T acc = T(0);
#pragma unroll
        for (int d = 0; d < S::CPL; ++d) acc += a[u][d] * x[d];
        s[u] = acc;
    }
    row_reduce<T, S::RPT>(s, cg);
}

// One block step of the backward sweep on W (n x NR, dense, in place: block kblk already holds x_k).  Workgroup
// j = blockIdx.x < kblk updates block j, and j = kblk - 1 finishes it.  kblk >= the number of blocks: the seed launch,
// one workgroup that only finishes the last block.
template <typename T, int NR>
__global__ __launch_bounds__(256) void posx_back_step_kernel(int n, const T *__restrict__ U, int lda,
                                                             const T *__restrict__ inv128, int kblk, T *__restrict__ W) {
    typedef PosTile<T> S;
    __shared__ __attribute__((aligned(16))) T xs[PB * NR];
    __shared__ __attribute__((aligned(16))) T bs[PB * NR];
    const int tid = threadIdx.x, cg = tid % S::LPR, g = tid / S::LPR;
    const int nblk = (n + PB - 1) / PB;
    const bool seed = kblk >= nblk;
    const int j = seed ? nblk - 1 : (int)blockIdx.x;
    if (j < 0 || j >= nblk || (!seed && j >= kblk)) return;
    const bool finish = seed || j == kblk - 1;
    const int rj = j * PB;
    const int r = g + S::G * (cg >> 1);      // the row whose sum this lane pair ends up with
    const bool writer = (cg & 1) == 0;
    T a[S::RPT][S::CPL];
    T s[S::RPT];
    if (!seed) {
        const int ck = kblk * PB;
        for (int e = tid; e < PB * NR; e += 256) xs[e] = (ck + e / NR < n) ? W[(size_t)ck * NR + e] : T(0);
        const bool vec = ((size_t)U % 16 == 0) && (lda % S::CPL == 0);
        tile_load<T>(U + (size_t)rj * lda + ck, lda, vec, n - rj, n - ck, false, a);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            tile_gemv_rows<T, NR>(a, xs, q, s);
            if (writer) {
                const bool in = rj + r < n;
                const T b = in ? W[(size_t)(rj + r) * NR + q] - s[0] : T(0);
                if (finish) bs[r * NR + q] = b;
                else if (in) W[(size_t)(rj + r) * NR + q] = b;
            }
        }
    } else {
        for (int e = tid; e < PB * NR; e += 256) bs[e] = (rj + e / NR < n) ? W[(size_t)rj * NR + e] : T(0);
    }
    if (!finish) return;
    __syncthreads();
    // x_j = inv(U_jj) b_j: the block inverse is work space, written whole (zero below its diagonal, identity outside)
    tile_load<T>(inv128 + (size_t)j * PB * PB, PB, true, PB, PB, false, a);
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        tile_gemv_rows<T, NR>(a, bs, q, s);
        if (writer && rj + r < n) W[(size_t)(rj + r) * NR + q] = s[0];
    }
}

// B[:, c0 .. c0 + w) <- W (n x NR, dense)
template <typename T>
__global__ __launch_bounds__(256) void posx_unpack_kernel(int n, int NR, int w, const T *__restrict__ W, T *__restrict__ B,
                                                          int ldb, int c0) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n * NR) return;
    const int i = e / NR, q = e % NR;
    if (q < w) B[(size_t)i * ldb + c0 + q] = W[e];
}

template <typename T, int NR>
static int posx_backward_nr(lsx_handle_t h, int n, const T *U, int lda, const T *inv128, T *W) {
    const int nblk = (n + PB - 1) / PB;
    hipLaunchKernelGGL((posx_back_step_kernel<T, NR>), dim3(1), dim3(256), 0, h->stream, n, U, lda, inv128, nblk, W);
    for (int k = nblk - 1; k > 0; --k)
        hipLaunchKernelGGL((posx_back_step_kernel<T, NR>), dim3(k), dim3(256), 0, h->stream, n, U, lda, inv128, k, W);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// W (n x nr, dense, nr in {1, 2, 4, 8}) <- inv(U) W, then columns [c0, c0 + w) of B <- W
template <typename T>
int launch_posx_backward(lsx_handle_t h, int n, int nr, int w, const T *U, int lda, const T *inv128, T *W, T *B, int ldb,
                         int c0) {
    if (n <= 0 || w <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_TRSM, (double)n * n * w, sizeof(T) * (double)n * n / 2);
    switch (nr) {
        case 1: LSX_TRY((posx_backward_nr<T, 1>(h, n, U, lda, inv128, W))); break;
        case 2: LSX_TRY((posx_backward_nr<T, 2>(h, n, U, lda, inv128, W))); break;
        case 4: LSX_TRY((posx_backward_nr<T, 4>(h, n, U, lda, inv128, W))); break;
        case 8: LSX_TRY((posx_backward_nr<T, 8>(h, n, U, lda, inv128, W))); break;
        default: set_error("launch_posx_backward: nr must be 1, 2, 4 or 8"); return LSX_ERR_INTERNAL;
    }
    hipLaunchKernelGGL(posx_unpack_kernel<T>, dim3((n * nr + 255) / 256), dim3(256), 0, h->stream, n, nr, w, (const T *)W, B,
                       ldb, c0);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

#define LSX_INST_POSX(T)                                                                                                 \
    template int launch_resid_bound_sym<T>(lsx_handle_t, int, int, const T *, int, const T *, int, const T *, int, T *, \
                                           T *, int, double *);                                                         \
    template int launch_lansy<T>(lsx_handle_t, int, const T *, int, double *, double *);                                \
    template int launch_posx_backward<T>(lsx_handle_t, int, int, int, const T *, int, const T *, T *, T *, int, int);
LSX_INST_POSX(double)
LSX_INST_POSX(float)
#undef LSX_INST_POSX

}  // namespace lsx
