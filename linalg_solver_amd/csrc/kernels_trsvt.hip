// Transposed solves from the LU factors, the matrix norms and the device side of the condition estimate.
//
//   A^T X = B with P A = L U (row-major):   U^T Y = B   (forward: U^T is lower triangular)
//                                           L^T Z = Y   (backward, unit diagonal)
//                                           X[perm[i], :] = Z[i, :]   (perm: the gather list of launch_ipiv_to_perm)
//
//   trsvt_step   one launch per 128-row block step, no workgroup waits for another.  Block k of the unknown is known;
//                workgroup j owns the 128 entries of block j and forms  b_j -= T[k-rows, j-cols]^T x_k.  In row-major
//                storage that tile is read ROW BY ROW with adjacent columns in adjacent lanes, 16 bytes per lane,
//                straight into registers and every load of a thread in flight before the first use: the tile is
//                streamed once and shared by nobody, so an LDS round trip would be overhead.  Only x_k (128 x NR) and
//                the partial sums of the row groups go through LDS.  The workgroup that owns the NEXT block then
//                applies inv(T_next)^T with the same routine: the 128 x 128 inverses are stored in their natural
//                orientation for this solve (merge128_kernel, natural = 1), so inv^T b is again "row by row".
//                These kernels serve up to getrs_t_blocked_min - 1 right-hand sides in groups of 8 columns; from there on
//                api.hip runs the same sweeps blocked on the TN form of the MFMA tile (lu_solve_transposed_blocked) and only
//                the final row scatter (scatter_rows_kernel) lives here.
//   trsvt_small  n <= 128: one workgroup, the factors in LDS, plain substitution, interchanges included.
//   Summation order is fixed everywhere (rows ascending inside a thread, then the row groups ascending): two calls
//   give identical bits.
#include "common.h"

namespace lsx {

constexpr int WB = 128;   // block edge of the transposed solve

template <typename T>
struct TileShape {
    static constexpr int CPL = 16 / (int)sizeof(T);   // columns per lane: one 16-byte load
    static constexpr int LPR = WB / CPL;              // lanes per tile row
    static constexpr int G = 256 / LPR;               // row groups of a workgroup (fp64: 4, fp32: 8)
    static constexpr int RPT = WB / G;                // rows per thread (fp64: 32, fp32: 16)
};

// part[g][c][q] = sum over the rows r = g, g + G, ... of the tile of  M[r][c] * xs[r][q]   (M: 128 x 128 at ld).
// vec: the whole tile is inside the matrix and 16-byte aligned; otherwise rows >= rows_ok and columns >= cols_ok
// are not read (they count as zero).
template <typename T, int NR>
__device__ __forceinline__ void tile_gemv_t(const T *__restrict__ M, const int ld, const bool vec, const int rows_ok,
                                            const int cols_ok, const T *xs, T *part) {
    typedef TileShape<T> S;
    typedef T vt __attribute__((ext_vector_type(S::CPL)));
    constexpr int U = S::RPT < 16 ? S::RPT : 16;      // loads per batch; two batches are in flight
    constexpr int NBATCH = S::RPT / U;
    static_assert(NBATCH <= 2, "two register sets cover the tile");
    const int tid = threadIdx.x, cg = tid % S::LPR, g = tid / S::LPR;
    const int c0 = cg * S::CPL;
    T acc[S::CPL][NR];
#pragma unroll
    for (int d = 0; d < S::CPL; ++d)
#pragma unroll
        for (int q = 0; q < NR; ++q) acc[d][q] = T(0);
    auto load = [&](vt (&v)[U], const int b) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = g + S::G * (b * U + u);
            const T *p = M + (size_t)r * ld + c0;
            if (vec) {
                v[u] = *(const vt *)p;
            } else {
#pragma unroll
                for (int d = 0; d < S::CPL; ++d) v[u][d] = (r < rows_ok && c0 + d < cols_ok) ? p[d] : T(0);
            }
        }
    };
    auto fma = [&](const vt (&v)[U], const int b) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = g + S::G * (b * U + u);
#pragma unroll
            for (int q = 0; q < NR; ++q) {
                const T x = xs[r * NR + q];
#pragma unroll
                for (int d = 0; d < S::CPL; ++d) acc[d][q] += v[u][d] * x;
            }
        }
    };
    vt va[U], vb[U];
    load(va, 0);
    if (NBATCH > 1) load(vb, 1);
    fma(va, 0);
    if (NBATCH > 1) fma(vb, 1);
#pragma unroll
    for (int d = 0; d < S::CPL; ++d)
#pragma unroll
        for (int q = 0; q < NR; ++q) part[(g * WB + c0 + d) * NR + q] = acc[d][q];
}

// One block step.  Forward sweep with U^T: blocks j > kblk; backward sweep with L^T: blocks j < kblk (the host chooses
// jfirst, the grid and `next`; the tile of block row kblk and block column j lies in the right triangle either way).
// Workgroup blockIdx.x owns block j = jfirst + blockIdx.x of W (n x NR, dense, solved in place: block kblk already
// holds x_k).  kblk < 0: the seed launch, one workgroup that only finishes block `next`.
template <typename T, int NR>
__global__ __launch_bounds__(256) void trsvt_step_kernel(int n, const T *__restrict__ LU, int lda,
                                                         const T *__restrict__ inv128, int kblk, int jfirst, int next,
                                                         T *__restrict__ W) {
    typedef TileShape<T> S;
    __shared__ __attribute__((aligned(16))) T xs[WB * NR];
    __shared__ __attribute__((aligned(16))) T part[S::G * WB * NR];
    const int tid = threadIdx.x;
    const int nblk = (n + WB - 1) / WB;
    const int j = jfirst + (int)blockIdx.x;
    if (j < 0 || j >= nblk || kblk >= nblk) return;
    const bool finish = j == next;
    const int cj = j * WB;
    if (kblk >= 0) {
        const int rk = kblk * WB;
        for (int e = tid; e < WB * NR; e += 256) xs[e] = (rk + e / NR < n) ? W[(size_t)rk * NR + e] : T(0);
        __syncthreads();
        const bool vec = ((size_t)LU % 16 == 0) && (lda % S::CPL == 0) && rk + WB <= n && cj + WB <= n;
        tile_gemv_t<T, NR>(LU + (size_t)rk * lda + cj, lda, vec, n - rk, n - cj, xs, part);
        __syncthreads();
        for (int e = tid; e < WB * NR; e += 256) {
            T s = T(0);
#pragma unroll
            for (int g = 0; g < S::G; ++g) s += part[g * WB * NR + e];
            const bool in = cj + e / NR < n;
            const T b = in ? W[(size_t)cj * NR + e] - s : T(0);
            if (finish) xs[e] = b;
            else if (in) W[(size_t)cj * NR + e] = b;
        }
    } else {
        if (!finish) return;
        for (int e = tid; e < WB * NR; e += 256) xs[e] = (cj + e / NR < n) ? W[(size_t)cj * NR + e] : T(0);
    }
    if (!finish) return;
    __syncthreads();
    // x_j = inv(T_jj)^T b_j: the same row-by-row product on the block inverse (identity outside the matrix)
    tile_gemv_t<T, NR>(inv128 + (size_t)j * WB * WB, WB, true, WB, WB, xs, part);
    __syncthreads();
    for (int e = tid; e < WB * NR; e += 256) {
        T s = T(0);
#pragma unroll
        for (int g = 0; g < S::G; ++g) s += part[g * WB * NR + e];
        if (cj + e / NR < n) W[(size_t)cj * NR + e] = s;
    }
}

// W (n x NR, dense) <- columns [c0, c0 + w) of B, the others zero
template <typename T>
__global__ __launch_bounds__(256) void trsvt_pack_kernel(int n, int NR, int w, const T *__restrict__ B, int ldb, int c0,
                                                         T *__restrict__ W) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n * NR) return;
    const int i = e / NR, q = e % NR;
    W[e] = q < w ? B[(size_t)i * ldb + c0 + q] : T(0);
}

// X[perm[i], c0 + q] = W[i, q]: the inverse of the row gather of the plain solve
template <typename T>
__global__ __launch_bounds__(256) void trsvt_scatter_kernel(int n, int NR, int w, const T *__restrict__ W,
                                                            const int32_t *__restrict__ perm, T *__restrict__ X, int ldx,
                                                            int c0) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n * NR) return;
    const int i = e / NR, q = e % NR;
    const int p = perm[i];
    if (q < w && p >= 0 && p < n) X[(size_t)p * ldx + c0 + q] = W[e];
}

// The same scatter for a whole right-hand-side block (blocked path): one workgroup per row, lanes along the row
template <typename T>
__global__ __launch_bounds__(256) void scatter_rows_kernel(int n, int ncols, const int32_t *__restrict__ perm,
                                                           const T *__restrict__ W, int ldw, T *__restrict__ X, int ldx) {
    const int i = blockIdx.x;
    const int p = perm[i];
    if (p < 0 || p >= n) return;
    for (int q = threadIdx.x; q < ncols; q += 256) X[(size_t)p * ldx + q] = W[(size_t)i * ldw + q];
}

template <typename T>
int launch_scatter_rows(lsx_handle_t h, int n, int ncols, const int32_t *d_perm, const T *W, int ldw, T *X, int ldx) {
    if (n <= 0 || ncols <= 0) return LSX_OK;
    hipLaunchKernelGGL(scatter_rows_kernel<T>, dim3(n), dim3(256), 0, h->stream, n, ncols, d_perm, W, ldw, X, ldx);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}
template int launch_scatter_rows<double>(lsx_handle_t, int, int, const int32_t *, const double *, int, double *, int);
template int launch_scatter_rows<float>(lsx_handle_t, int, int, const int32_t *, const float *, int, float *, int);

// n <= 128, columns [c0, c0 + w) of B with w <= NR: the factors in LDS (dynamic, n x 128 elements), thread (c, hf)
// keeps entry c of every second column in registers.  Step i hands y_i to the others through a two-slot LDS buffer:
// one barrier per step.
template <typename T, int NR>
__global__ __launch_bounds__(256) void trsvt_small_kernel(int n, int w, const T *__restrict__ LU, int lda,
                                                          const int32_t *__restrict__ ipiv, T *__restrict__ B, int ldb,
                                                          int c0) {
    extern __shared__ __attribute__((aligned(16))) char smem_small[];
    T *Fs = (T *)smem_small;                  // Fs[i * WB + c] = LU[i][c]
    __shared__ T ys[2][NR];
    __shared__ int prm[WB];
    constexpr int NQ = NR > 1 ? NR / 2 : 1;
    const int tid = threadIdx.x, c = tid & (WB - 1), hf = tid >> 7;
    for (int e = tid; e < n * WB; e += 256) {
        const int i = e / WB, cc = e % WB;
        Fs[e] = cc < n ? LU[(size_t)i * lda + cc] : T(0);
    }
    if (tid < WB) prm[tid] = tid;
    __syncthreads();
    if (tid == 0) {   // the interchanges in order: afterwards (P b)[i] = b[prm[i]]
        for (int k = 0; k < n; ++k) {
            const int p = ipiv[k];
            if (p > k && p < n) { const int t = prm[k]; prm[k] = prm[p]; prm[p] = t; }
        }
    }
    const bool active = c < n && (NR > 1 || hf == 0);
    T b[NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        const int q = hf + 2 * t;
        b[t] = (active && q < w) ? B[(size_t)c * ldb + c0 + q] : T(0);
    }
    __syncthreads();
    for (int i = 0; i < n; ++i) {             // U^T y = b
        if (c == i && active) {
            const T d = Fs[i * WB + i];
#pragma unroll
            for (int t = 0; t < NQ; ++t) { b[t] = b[t] / d; ys[i & 1][hf + 2 * t] = b[t]; }
        }
        __syncthreads();
        if (c > i && active) {
            const T u = Fs[i * WB + c];
#pragma unroll
            for (int t = 0; t < NQ; ++t) b[t] -= u * ys[i & 1][hf + 2 * t];
        }
    }
    __syncthreads();
    for (int i = n - 1; i >= 0; --i) {        // L^T z = y, unit diagonal
        if (c == i && active) {
#pragma unroll
            for (int t = 0; t < NQ; ++t) ys[i & 1][hf + 2 * t] = b[t];
        }
        __syncthreads();
        if (c < i && active) {
            const T l = Fs[i * WB + c];
#pragma unroll
            for (int t = 0; t < NQ; ++t) b[t] -= l * ys[i & 1][hf + 2 * t];
        }
    }
    if (active) {
        const int p = prm[c];
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            const int q = hf + 2 * t;
            if (q < w) B[(size_t)p * ldb + c0 + q] = b[t];
        }
    }
}

template <typename T, int NR>
static int trsvt_sweeps(lsx_handle_t h, int n, const T *LU, int lda, const T *inv128L, const T *inv128U, T *W) {
    const int nblk = (n + WB - 1) / WB;
    // forward, U^T: the seed launch finishes block 0, step k updates blocks k + 1 .. and finishes block k + 1
    hipLaunchKernelGGL((trsvt_step_kernel<T, NR>), dim3(1), dim3(256), 0, h->stream, n, LU, lda, inv128U, -1, 0, 0, W);
    for (int k = 0; k + 1 < nblk; ++k)
        hipLaunchKernelGGL((trsvt_step_kernel<T, NR>), dim3(nblk - 1 - k), dim3(256), 0, h->stream, n, LU, lda, inv128U,
                           k, k + 1, k + 1, W);
    // backward, L^T: from the last block upwards
    hipLaunchKernelGGL((trsvt_step_kernel<T, NR>), dim3(1), dim3(256), 0, h->stream, n, LU, lda, inv128L, -1, nblk - 1,
                       nblk - 1, W);
    for (int k = nblk - 1; k > 0; --k)
        hipLaunchKernelGGL((trsvt_step_kernel<T, NR>), dim3(k), dim3(256), 0, h->stream, n, LU, lda, inv128L, k, 0, k - 1,
                           W);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// The U half alone, for the few-column Cholesky solve (kernels_posx.hip): W (n x nr, dense, nr in {1, 2, 4, 8}) <-
// columns [c0, c0 + w) of B, then U^T Y = W in place with the same launches as the forward half of trsvt_sweeps.
// Only tiles strictly above the diagonal blocks of U are read; inv128U is launch_chol_inv's natural-orientation inverse.
template <typename T>
int launch_trsvt_forward_upper(lsx_handle_t h, int n, int nr, int w, const T *U, int lda, const T *inv128U, const T *B,
                               int ldb, int c0, T *W) {
    if (n <= 0 || w <= 0) return LSX_OK;
    const int nblk = (n + WB - 1) / WB;
    ProfScope ps(h, LSX_PROF_TRSM, (double)n * n * w, sizeof(T) * (double)n * n / 2);
    hipLaunchKernelGGL(trsvt_pack_kernel<T>, dim3((n * nr + 255) / 256), dim3(256), 0, h->stream, n, nr, w, B, ldb, c0, W);
#define TF_LAUNCH(NRV)                                                                                                      \
    hipLaunchKernelGGL((trsvt_step_kernel<T, NRV>), dim3(1), dim3(256), 0, h->stream, n, U, lda, inv128U, -1, 0, 0, W);      \
    for (int k = 0; k + 1 < nblk; ++k)                                                                                      \
        hipLaunchKernelGGL((trsvt_step_kernel<T, NRV>), dim3(nblk - 1 - k), dim3(256), 0, h->stream, n, U, lda, inv128U, k, \
                           k + 1, k + 1, W)
    switch (nr) {
        case 1: TF_LAUNCH(1); break;
        case 2: TF_LAUNCH(2); break;
        case 4: TF_LAUNCH(4); break;
        case 8: TF_LAUNCH(8); break;
        default: set_error("launch_trsvt_forward_upper: nr must be 1, 2, 4 or 8"); return LSX_ERR_INTERNAL;
    }
#undef TF_LAUNCH
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}
template int launch_trsvt_forward_upper<double>(lsx_handle_t, int, int, int, const double *, int, const double *,
                                                const double *, int, int, double *);
template int launch_trsvt_forward_upper<float>(lsx_handle_t, int, int, int, const float *, int, const float *, const float *,
                                               int, int, float *);

// B (n x nrhs) <- the solution of A^T X = B, any nrhs, in groups of up to 8 columns.  n > 128: inv64* / inv128* are
// work space for the block inverses (as in the plain solve), perm the gather list, W an n x 8 work vector.
template <typename T>
int lu_solve_transposed(lsx_handle_t h, int n, int nrhs, const T *LU, int lda, const int32_t *d_ipiv, const int32_t *perm,
                        T *B, int ldb, T *inv64L, T *inv64U, T *inv128L, T *inv128U, T *W) {
    if (n <= WB) {
        const size_t shm = (size_t)n * WB * sizeof(T);
        for (int c0 = 0; c0 < nrhs; c0 += 8) {
            const int w = nrhs - c0 < 8 ? nrhs - c0 : 8;
            const int nr = w <= 1 ? 1 : w <= 2 ? 2 : w <= 4 ? 4 : 8;
            ProfScope ps(h, LSX_PROF_TRSM, 2.0 * n * (double)n * w, sizeof(T) * n * (double)n);
#define TS_LAUNCH(NRV)                                                                                                       \
    LSX_HIP(hipFuncSetAttribute((const void *)trsvt_small_kernel<T, NRV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm)); \
    hipLaunchKernelGGL((trsvt_small_kernel<T, NRV>), dim3(1), dim3(256), shm, h->stream, n, w, LU, lda, d_ipiv, B, ldb, c0)
            switch (nr) {
                case 1: TS_LAUNCH(1); break;
                case 2: TS_LAUNCH(2); break;
                case 4: TS_LAUNCH(4); break;
                default: TS_LAUNCH(8); break;
            }
#undef TS_LAUNCH
        }
        LSX_HIP(hipGetLastError());
        return LSX_OK;
    }
    LSX_TRY(launch_inv128_natural<T>(h, n, LU, lda, inv64L, inv64U, inv128L, inv128U));
    for (int c0 = 0; c0 < nrhs; c0 += 8) {
        const int w = nrhs - c0 < 8 ? nrhs - c0 : 8;
        const int nr = w <= 1 ? 1 : w <= 2 ? 2 : w <= 4 ? 4 : 8;
        ProfScope ps(h, LSX_PROF_TRSM, 2.0 * n * (double)n * w, sizeof(T) * n * (double)n);
        const int grid = (n * nr + 255) / 256;
        hipLaunchKernelGGL(trsvt_pack_kernel<T>, dim3(grid), dim3(256), 0, h->stream, n, nr, w, (const T *)B, ldb, c0, W);
        switch (nr) {
            case 1: LSX_TRY((trsvt_sweeps<T, 1>(h, n, LU, lda, inv128L, inv128U, W))); break;
            case 2: LSX_TRY((trsvt_sweeps<T, 2>(h, n, LU, lda, inv128L, inv128U, W))); break;
            case 4: LSX_TRY((trsvt_sweeps<T, 4>(h, n, LU, lda, inv128L, inv128U, W))); break;
            default: LSX_TRY((trsvt_sweeps<T, 8>(h, n, LU, lda, inv128L, inv128U, W))); break;
        }
        hipLaunchKernelGGL(trsvt_scatter_kernel<T>, dim3(grid), dim3(256), 0, h->stream, n, nr, w, (const T *)W, perm, B,
                           ldb, c0);
    }
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}
template int lu_solve_transposed<double>(lsx_handle_t, int, int, const double *, int, const int32_t *, const int32_t *,
                                         double *, int, double *, double *, double *, double *, double *);
template int lu_solve_transposed<float>(lsx_handle_t, int, int, const float *, int, const int32_t *, const int32_t *, float *,
                                        int, float *, float *, float *, float *, float *);

// ------------------------------------------------------------------ matrix norms
// Two passes, no floating-point atomics: partial sums P[r][c] in a fixed partition, then one workgroup adds the
// partials of every c in ascending r and takes the maximum (a NaN sum wins, as in LAPACK's lange).
constexpr int LN_T = 1024;
constexpr int LN_ROWS = 256;   // rows per partial sum of the 1-norm

// 1-norm, first pass: thread = one column, workgroup row = one chunk of rows
template <typename T>
__global__ __launch_bounds__(256) void lange_colpart_kernel(int m, int n, const T *__restrict__ A, int lda, int rows_per,
                                                            double *__restrict__ P) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const int r0 = blockIdx.y * rows_per, r1 = min(m, r0 + rows_per);
    double s = 0;
    for (int r = r0; r < r1; ++r) s += fabs((double)A[(size_t)r * lda + c]);
    P[(size_t)blockIdx.y * n + c] = s;
}

// infinity-norm, first pass: one wave per row, lanes across the columns, fixed tree over the lanes
template <typename T>
__global__ __launch_bounds__(256) void lange_rowsum_kernel(int m, int n, const T *__restrict__ A, int lda,
                                                           double *__restrict__ P) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= m) return;
    double s = 0;
    for (int c = lane; c < n; c += 64) s += fabs((double)A[(size_t)r * lda + c]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if (lane == 0) P[r] = s;
}

__device__ __forceinline__ double nan_max(const double a, const double b) { return (b > a || b != b) ? b : a; }

__global__ __launch_bounds__(LN_T) void lange_final_kernel(int R, int len, const double *__restrict__ P,
                                                           double *__restrict__ out) {
    __shared__ double s_v[LN_T];
    double v = 0;
    for (int c = threadIdx.x; c < len; c += LN_T) {
        double s = 0;
        for (int r = 0; r < R; ++r) s += P[(size_t)r * len + c];
        v = nan_max(v, s);
    }
    s_v[threadIdx.x] = v;
    __syncthreads();
    for (int k = LN_T / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) s_v[threadIdx.x] = nan_max(s_v[threadIdx.x], s_v[threadIdx.x + k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = s_v[0];
}

size_t lange_work_bytes(int norm, int m, int n) {
    if (m <= 0 || n <= 0) return 0;
    if (norm == LSX_NORM_INF) return sizeof(double) * (size_t)m;
    return sizeof(double) * (size_t)((m + LN_ROWS - 1) / LN_ROWS) * n;
}

// d_out[0] = the norm; d_work: lange_work_bytes(norm, m, n) bytes
template <typename T>
int launch_lange(lsx_handle_t h, int norm, int m, int n, const T *A, int lda, double *d_work, double *d_out) {
    if (m <= 0 || n <= 0) {
        LSX_HIP(hipMemsetAsync(d_out, 0, sizeof(double), h->stream));
        return LSX_OK;
    }
    ProfScope ps(h, LSX_PROF_OTHER, (double)m * n, sizeof(T) * (double)m * n);
    if (norm == LSX_NORM_INF) {
        hipLaunchKernelGGL(lange_rowsum_kernel<T>, dim3((m + 3) / 4), dim3(256), 0, h->stream, m, n, A, lda, d_work);
        hipLaunchKernelGGL(lange_final_kernel, dim3(1), dim3(LN_T), 0, h->stream, 1, m, (const double *)d_work, d_out);
    } else {
        const int R = (m + LN_ROWS - 1) / LN_ROWS;
        hipLaunchKernelGGL(lange_colpart_kernel<T>, dim3((n + 255) / 256, R), dim3(256), 0, h->stream, m, n, A, lda,
                           LN_ROWS, d_work);
        hipLaunchKernelGGL(lange_final_kernel, dim3(1), dim3(LN_T), 0, h->stream, R, n, (const double *)d_work, d_out);
    }
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}
template int launch_lange<double>(lsx_handle_t, int, int, int, const double *, int, double *, double *);
template int launch_lange<float>(lsx_handle_t, int, int, int, const float *, int, double *, double *);

// ------------------------------------------------------------------ condition estimate: the device side
// The vector operations of LAPACK's lacn2 between two solves, one workgroup each; the host reads rec after each.
//   rec[0] = ||x||_1     rec[1] = j (first index of max |x_i|)     rec[2] = |x_j|     rec[3] = x_jlast (signed: lacn2
//   compares it with |x_j| as it is)     rec[4] = 1 if sign(x) equals the stored sign vector
constexpr int EST_T = 1024;

// mode 0: x_i = 1 / n;  mode 1: the alternating vector x_i = (-1)^i (1 + i / (n - 1));  also ident[i] = i when given
template <typename T>
__global__ __launch_bounds__(256) void est_fill_kernel(int n, int mode, T *__restrict__ x, int32_t *__restrict__ ident) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (mode == 0) x[i] = (T)(1.0 / (double)n);
    else x[i] = (T)(((i & 1) ? -1.0 : 1.0) * (1.0 + (double)i / (double)(n - 1)));
    if (ident) ident[i] = i;
}

// rec[0] = sum |x_i| (accumulated in fp64), rec[4] = sign vector unchanged; then x <- sign(x) and the stored sign
// vector with it (sign(0) = +1).  The overwrite is what the next step of the iteration needs; a caller that stops
// here does not read x again.
template <typename T>
__global__ __launch_bounds__(EST_T) void est_asum_sign_kernel(int n, T *__restrict__ x, signed char *__restrict__ isgn,
                                                              double *__restrict__ rec) {
    __shared__ double s_sum[EST_T];
    __shared__ int s_diff[EST_T];
    double s = 0;
    int diff = 0;
    for (int i = threadIdx.x; i < n; i += EST_T) {
        const T v = x[i];
        s += fabs((double)v);
        const signed char sg = v >= T(0) ? 1 : -1;
        diff |= sg != isgn[i];
        isgn[i] = sg;
        x[i] = (T)sg;
    }
    s_sum[threadIdx.x] = s;
    s_diff[threadIdx.x] = diff;
    __syncthreads();
    for (int k = EST_T / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            s_sum[threadIdx.x] += s_sum[threadIdx.x + k];
            s_diff[threadIdx.x] |= s_diff[threadIdx.x + k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { rec[0] = s_sum[0]; rec[4] = s_diff[0] ? 0.0 : 1.0; }
}

// rec[1] = j, rec[2] = |x_j|, rec[3] = x[jlast] (0 without a jlast); then x <- e_j
template <typename T>
__global__ __launch_bounds__(EST_T) void est_amax_unit_kernel(int n, T *__restrict__ x, int jlast, double *__restrict__ rec) {
    __shared__ double s_v[EST_T];
    __shared__ int s_i[EST_T];
    double best = -1.0;
    int bi = 0;
    for (int i = threadIdx.x; i < n; i += EST_T) {
        const double a = fabs((double)x[i]);
        if (a > best) { best = a; bi = i; }      // ascending i: the first of equals stays
    }
    s_v[threadIdx.x] = best;
    s_i[threadIdx.x] = bi;
    const double xl = (threadIdx.x == 0 && jlast >= 0 && jlast < n) ? (double)x[jlast] : 0.0;
    __syncthreads();
    for (int k = EST_T / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            const double o = s_v[threadIdx.x + k];
            const int oi = s_i[threadIdx.x + k];
            if (o > s_v[threadIdx.x] || (o == s_v[threadIdx.x] && oi < s_i[threadIdx.x])) {
                s_v[threadIdx.x] = o;
                s_i[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    const int j = s_i[0];
    if (threadIdx.x == 0) { rec[1] = (double)j; rec[2] = s_v[0] < 0 ? 0.0 : s_v[0]; rec[3] = xl; }
    for (int i = threadIdx.x; i < n; i += EST_T) x[i] = i == j ? T(1) : T(0);
}

template <typename T>
int launch_est_fill(lsx_handle_t h, int n, int mode, T *x, int32_t *ident) {
    hipLaunchKernelGGL(est_fill_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, mode, x, ident);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}
template <typename T>
int launch_est_asum_sign(lsx_handle_t h, int n, T *x, signed char *isgn, double *rec) {
    hipLaunchKernelGGL(est_asum_sign_kernel<T>, dim3(1), dim3(EST_T), 0, h->stream, n, x, isgn, rec);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}
template <typename T>
int launch_est_amax_unit(lsx_handle_t h, int n, T *x, int jlast, double *rec) {
    hipLaunchKernelGGL(est_amax_unit_kernel<T>, dim3(1), dim3(EST_T), 0, h->stream, n, x, jlast, rec);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}
#define LSX_INST_EST(T)                                                         \
    template int launch_est_fill<T>(lsx_handle_t, int, int, T *, int32_t *);   \
    template int launch_est_asum_sign<T>(lsx_handle_t, int, T *, signed char *, double *); \
    template int launch_est_amax_unit<T>(lsx_handle_t, int, T *, int, double *);
LSX_INST_EST(double)
LSX_INST_EST(float)
#undef LSX_INST_EST

}  // namespace lsx
