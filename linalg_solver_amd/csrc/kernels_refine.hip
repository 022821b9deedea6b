// Refined solves with error bounds (lsx_gerfs_*, gerfs_dev in api.hip): the residual r = b - op(A) x together with
// the componentwise bound w = |b| + |op(A)| |x| in one pass over A, LAPACK's backward error from the two, and the
// small vector steps of the refinement loop and of the forward-error estimate.  DESIGN section 3.5.
//
// Every sum has a fixed order and there are no floating-point atomics: two calls give identical bits, and a column
// gets the same bits whether it is processed alone or in a group of up to 8 (the order of its own sum does not
// depend on how many columns ride along).  Sums are accumulated in fp64 for both element types and rounded once.
#include "common.h"

namespace lsx {

static __device__ __forceinline__ double nan_max(const double a, const double b) { return (b > a || b != b) ? b : a; }

template <typename T> struct Vec16;
template <> struct Vec16<double> { typedef double2 type; };
template <> struct Vec16<float> { typedef float4 type; };

// ------------------------------------------------------------------ r = b - A x, w = |b| + |A| |x|
// One wave per RB_ROWS rows, lanes across the columns: lane l of a chunk takes the V = 16 / sizeof(T) adjacent
// columns (it * 64 + l) * V ..., one 16-byte load per row, straight to registers (no other wave wants this tile
// of A: nothing goes through LDS but x).  x is staged in LDS as fp64, RB_KC rows of it at a time, for all NR
// columns, laid out [column j][row k]: adjacent lanes then read adjacent 16-byte (fp64) / 32-byte (fp32) pieces of
// one column's chunk, which is free of bank conflicts ([k][j] would put the 16 lanes of a read group 128 or 256
// bytes apart, on one or two slots of the 256-byte bank row).  |x| is the operand modifier of the second product.
// The sums of a lane run over its columns in ascending order, chunk after chunk; the 64 lanes are then added in a
// fixed shuffle tree.
// VEC = false is the element-wise form for a base that is not 16-byte aligned or an lda / n that is no multiple of
// V: the same lane owns the same columns in the same order, so on data both forms can read the bits are the same.
constexpr int RB_T = 256;     // 4 waves
constexpr int RB_ROWS = 2;    // rows per wave
constexpr int RB_KC = 512;    // columns (rows of x) per staged chunk

template <typename T, int NR, bool VEC>
__global__ __launch_bounds__(RB_T) void resid_bound_kernel(int n, int ncols, const T *__restrict__ A, int lda,
                                                           const T *__restrict__ B, int ldb, const T *__restrict__ X,
                                                           int ldx, T *__restrict__ R, T *__restrict__ W, int ldr) {
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int ITERS = RB_KC / (64 * V);
    typedef typename Vec16<T>::type vec_t;
    __shared__ double s_x[RB_KC * NR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (blockIdx.x * (RB_T / 64) + wave) * RB_ROWS;
    double r[RB_ROWS][NR], w[RB_ROWS][NR];
#pragma unroll
    for (int q = 0; q < RB_ROWS; ++q)
#pragma unroll
        for (int j = 0; j < NR; ++j) r[q][j] = w[q][j] = 0.0;

    for (int k0 = 0; k0 < n; k0 += RB_KC) {
        const int kc = min(RB_KC, n - k0);
        __syncthreads();                                   // the previous chunk of x has been consumed
#pragma unroll
        for (int j = 0; j < NR; ++j)
            for (int k = threadIdx.x; k < RB_KC; k += RB_T)
                s_x[j * RB_KC + k] = (k < kc && j < ncols) ? (double)X[(size_t)(k0 + k) * ldx + j] : 0.0;
        __syncthreads();
        // all loads of the chunk first, then the arithmetic: RB_ROWS * ITERS loads in flight per lane
        T a[ITERS][RB_ROWS][V];
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int kk = (it * 64 + lane) * V;
#pragma unroll
            for (int q = 0; q < RB_ROWS; ++q) {
                const int row = row0 + q;
                const T *p = A + (size_t)row * lda + k0 + kk;
                if (VEC) {
                    if (row < n && kk < kc) {              // n % V == 0: all V columns are inside
                        const vec_t v = *reinterpret_cast<const vec_t *>(p);
                        const T *e = reinterpret_cast<const T *>(&v);
#pragma unroll
                        for (int c = 0; c < V; ++c) a[it][q][c] = e[c];
                    } else {
#pragma unroll
                        for (int c = 0; c < V; ++c) a[it][q][c] = T(0);
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < V; ++c) a[it][q][c] = (row < n && kk + c < kc) ? p[c] : T(0);
                }
            }
        }
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int kk = (it * 64 + lane) * V;
#pragma unroll
            for (int c = 0; c < V; ++c) {
                if (kk + c < kc) {                         // a column past the end adds nothing, not even a zero
#pragma unroll
                    for (int j = 0; j < NR; ++j) {
                        const double xv = s_x[j * RB_KC + kk + c];
#pragma unroll
                        for (int q = 0; q < RB_ROWS; ++q) {
                            const double av = (double)a[it][q][c];
                            r[q][j] = __builtin_fma(av, xv, r[q][j]);
                            w[q][j] = __builtin_fma(fabs(av), fabs(xv), w[q][j]);
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < RB_ROWS; ++q) {
        const int row = row0 + q;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            double rs = r[q][j], ws = w[q][j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                rs += __shfl_down(rs, off, 64);
                ws += __shfl_down(ws, off, 64);
            }
            if (lane == 0 && row < n && j < ncols) {
                const double b = (double)B[(size_t)row * ldb + j];
                R[(size_t)row * ldr + j] = (T)(b - rs);
                W[(size_t)row * ldr + j] = (T)(fabs(b) + ws);
            }
        }
    }
}

// ------------------------------------------------------------------ r = b - A^T x, w = |b| + |A^T| |x|
// Column sums of a row-major matrix, in the shape of the 1-norm (lange_colpart_kernel): thread = one column (a wave
// reads 64 adjacent elements of a row), workgroup row = one chunk of RT_ROWS rows, the chunk's x staged in LDS
// (every lane reads the same word: a broadcast).  P[chunk][r | w][j][column] receives the partial sums; the second
// kernel adds them in ascending chunk order.  Element-wise loads only, so alignment never matters here.
constexpr int RT_ROWS = 256;

template <typename T, int NR>
__global__ __launch_bounds__(256) void resid_bound_t_part_kernel(int n, int ncols, const T *__restrict__ A, int lda,
                                                                 const T *__restrict__ X, int ldx,
                                                                 double *__restrict__ P) {
    __shared__ double s_x[RT_ROWS * NR];
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int r0 = blockIdx.y * RT_ROWS, rows = min(n - r0, RT_ROWS);
    for (int t = threadIdx.x; t < rows * NR; t += 256) {
        const int i = t / NR, j = t % NR;
        s_x[t] = j < ncols ? (double)X[(size_t)(r0 + i) * ldx + j] : 0.0;
    }
    __syncthreads();
    if (c >= n) return;
    double r[NR], w[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) r[j] = w[j] = 0.0;
    const T *a = A + (size_t)r0 * lda + c;
#pragma unroll 4
    for (int i = 0; i < rows; ++i) {
        const double av = (double)a[(size_t)i * lda];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const double xv = s_x[i * NR + j];
            r[j] = __builtin_fma(av, xv, r[j]);
            w[j] = __builtin_fma(fabs(av), fabs(xv), w[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        P[((size_t)(blockIdx.y * 2 + 0) * NR + j) * n + c] = r[j];
        P[((size_t)(blockIdx.y * 2 + 1) * NR + j) * n + c] = w[j];
    }
}

// thread = one column of A (one entry of r), blockIdx.y = right-hand side
template <typename T>
__global__ __launch_bounds__(256) void resid_bound_t_final_kernel(int n, int nr, int chunks, const double *__restrict__ P,
                                                                  const T *__restrict__ B, int ldb, T *__restrict__ R,
                                                                  T *__restrict__ W, int ldr) {
    const int c = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (c >= n) return;
    double rs = 0, ws = 0;
    for (int ch = 0; ch < chunks; ++ch) {
        rs += P[((size_t)(ch * 2 + 0) * nr + j) * n + c];
        ws += P[((size_t)(ch * 2 + 1) * nr + j) * n + c];
    }
    const double b = (double)B[(size_t)c * ldb + j];
    R[(size_t)c * ldr + j] = (T)(b - rs);
    W[(size_t)c * ldr + j] = (T)(fabs(b) + ws);
}

// ------------------------------------------------------------------ backward error and max |x| of every column
// One workgroup per right-hand side: rec[j] = max_i |r_i| / w_i (LAPACK's guarded form below safe2; a NaN wins),
// rec[8 + j] = max_i |x_ij|.
constexpr int BE_T = 1024;

template <typename T>
__global__ __launch_bounds__(BE_T) void berr_kernel(int n, const T *__restrict__ R, const T *__restrict__ W, int ldr,
                                                    const T *__restrict__ X, int ldx, double safe1, double safe2,
                                                    double *__restrict__ rec) {
    __shared__ double s_b[BE_T], s_x[BE_T];
    const int j = blockIdx.x;
    double vb = 0, vx = 0;
    for (int i = threadIdx.x; i < n; i += BE_T) {
        const double r = fabs((double)R[(size_t)i * ldr + j]), w = (double)W[(size_t)i * ldr + j];
        const double q = w > safe2 ? r / w : (r + safe1) / (w + safe1);
        vb = nan_max(vb, q);
        vx = nan_max(vx, fabs((double)X[(size_t)i * ldx + j]));
    }
    s_b[threadIdx.x] = vb;
    s_x[threadIdx.x] = vx;
    __syncthreads();
    for (int k = BE_T / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            s_b[threadIdx.x] = nan_max(s_b[threadIdx.x], s_b[threadIdx.x + k]);
            s_x[threadIdx.x] = nan_max(s_x[threadIdx.x], s_x[threadIdx.x + k]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { rec[j] = s_b[0]; rec[8 + j] = s_x[0]; }
}

// ------------------------------------------------------------------ vector steps
// d <- column j of R (the right-hand side of one correction solve)
template <typename T>
__global__ __launch_bounds__(256) void refine_take_kernel(int n, const T *__restrict__ R, int ldr, T *__restrict__ d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) d[i] = R[(size_t)i * ldr];
}
// x <- x + d on one column of X
template <typename T>
__global__ __launch_bounds__(256) void refine_add_kernel(int n, const T *__restrict__ d, T *__restrict__ X, int ldx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) X[(size_t)i * ldx] += d[i];
}
// the weights of the forward bound: W_i = |r_i| + nu * w_i, plus safe1 where w_i <= safe2 (nu = (n + 1) u)
template <typename T>
__global__ __launch_bounds__(256) void ferr_weight_kernel(int n, const T *__restrict__ R, const T *__restrict__ W, int ldr,
                                                          double nu, double safe1, double safe2, T *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double r = fabs((double)R[(size_t)i * ldr]), w = (double)W[(size_t)i * ldr];
    double v = __builtin_fma(nu, w, r);
    if (!(w > safe2)) v += safe1;
    out[i] = (T)v;
}
// v <- wt o v
template <typename T>
__global__ __launch_bounds__(256) void vec_mul_kernel(int n, const T *__restrict__ wt, T *__restrict__ v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] *= wt[i];
}

// ------------------------------------------------------------------ launchers
size_t resid_bound_work_bytes(int trans, int n) {
    if (!trans || n <= 0) return 0;
    return sizeof(double) * (size_t)((n + RT_ROWS - 1) / RT_ROWS) * 2 * 8 * (size_t)n;
}

template <typename T, int NR>
static int resid_bound_nr(lsx_handle_t h, int trans, int n, int ncols, const T *A, int lda, const T *B, int ldb, const T *X,
                          int ldx, T *R, T *W, int ldr, double *d_work) {
    if (trans) {
        const int chunks = (n + RT_ROWS - 1) / RT_ROWS;
        hipLaunchKernelGGL((resid_bound_t_part_kernel<T, NR>), dim3((n + 255) / 256, chunks), dim3(256), 0, h->stream, n,
                           ncols, A, lda, X, ldx, d_work);
        hipLaunchKernelGGL(resid_bound_t_final_kernel<T>, dim3((n + 255) / 256, ncols), dim3(256), 0, h->stream, n, NR,
                           chunks, (const double *)d_work, B, ldb, R, W, ldr);
    } else {
        constexpr int V = 16 / (int)sizeof(T);
        const bool vec = ((uintptr_t)A % 16 == 0) && lda % V == 0 && n % V == 0;
        const dim3 grid((n + (RB_T / 64) * RB_ROWS - 1) / ((RB_T / 64) * RB_ROWS));
        if (vec)
            hipLaunchKernelGGL((resid_bound_kernel<T, NR, true>), grid, dim3(RB_T), 0, h->stream, n, ncols, A, lda, B, ldb,
                               X, ldx, R, W, ldr);
        else
            hipLaunchKernelGGL((resid_bound_kernel<T, NR, false>), grid, dim3(RB_T), 0, h->stream, n, ncols, A, lda, B, ldb,
                               X, ldx, R, W, ldr);
    }
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// R, W (n x ncols, leading dimension ldr) <- residual and bound of ncols <= 8 right-hand sides; d_work:
// resid_bound_work_bytes(trans, n) bytes
template <typename T>
int launch_resid_bound(lsx_handle_t h, int trans, int n, int ncols, const T *A, int lda, const T *B, int ldb, const T *X,
                       int ldx, T *R, T *W, int ldr, double *d_work) {
    if (n <= 0 || ncols <= 0) return LSX_OK;
    if (ncols > 8) {
        set_error("launch_resid_bound: at most 8 right-hand sides per pass");
        return LSX_ERR_INTERNAL;
    }
    ProfScope ps(h, LSX_PROF_OTHER, 4.0 * n * (double)n * ncols, sizeof(T) * (double)n * n);
    if (ncols <= 1) return resid_bound_nr<T, 1>(h, trans, n, ncols, A, lda, B, ldb, X, ldx, R, W, ldr, d_work);
    if (ncols <= 2) return resid_bound_nr<T, 2>(h, trans, n, ncols, A, lda, B, ldb, X, ldx, R, W, ldr, d_work);
    if (ncols <= 4) return resid_bound_nr<T, 4>(h, trans, n, ncols, A, lda, B, ldb, X, ldx, R, W, ldr, d_work);
    return resid_bound_nr<T, 8>(h, trans, n, ncols, A, lda, B, ldb, X, ldx, R, W, ldr, d_work);
}

template <typename T>
int launch_berr(lsx_handle_t h, int n, int ncols, const T *R, const T *W, int ldr, const T *X, int ldx, double safe1,
                double safe2, double *rec) {
    hipLaunchKernelGGL(berr_kernel<T>, dim3(ncols), dim3(BE_T), 0, h->stream, n, R, W, ldr, X, ldx, safe1, safe2, rec);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}
template <typename T>
int launch_refine_take(lsx_handle_t h, int n, const T *Rj, int ldr, T *d) {
    hipLaunchKernelGGL(refine_take_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, Rj, ldr, d);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}
template <typename T>
int launch_refine_add(lsx_handle_t h, int n, const T *d, T *Xj, int ldx) {
    hipLaunchKernelGGL(refine_add_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, d, Xj, ldx);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}
template <typename T>
int launch_ferr_weight(lsx_handle_t h, int n, const T *Rj, const T *Wj, int ldr, double nu, double safe1, double safe2,
                       T *out) {
    hipLaunchKernelGGL(ferr_weight_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, Rj, Wj, ldr, nu, safe1,
                       safe2, out);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}
template <typename T>
int launch_vec_mul(lsx_handle_t h, int n, const T *wt, T *v) {
    hipLaunchKernelGGL(vec_mul_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, wt, v);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

#define LSX_INST_REFINE(T)                                                                                              \
    template int launch_resid_bound<T>(lsx_handle_t, int, int, int, const T *, int, const T *, int, const T *, int, T *, \
                                       T *, int, double *);                                                             \
    template int launch_berr<T>(lsx_handle_t, int, int, const T *, const T *, int, const T *, int, double, double,      \
                                double *);                                                                              \
    template int launch_refine_take<T>(lsx_handle_t, int, const T *, int, T *);                                         \
    template int launch_refine_add<T>(lsx_handle_t, int, const T *, T *, int);                                          \
    template int launch_ferr_weight<T>(lsx_handle_t, int, const T *, const T *, int, double, double, double, T *);      \
    template int launch_vec_mul<T>(lsx_handle_t, int, const T *, T *);
LSX_INST_REFINE(double)
LSX_INST_REFINE(float)
#undef LSX_INST_REFINE

}  // namespace lsx
