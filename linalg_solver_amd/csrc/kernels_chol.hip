// Cholesky factorisation A = U^T U (row-major, upper): the diagonal-block kernel and the block inverses of a factor.
//
// One workgroup owns a 128 x 128 block in REGISTERS, in 4 x 8 pieces of 32 values (no LDS copy of the block: fp64
// 128 x 128 is 128 KiB, which would fit the 160 KiB of a CU but leave nothing for a second operand).  Two logical
// matrices are eliminated side by side: the upper triangle of the block, and W = inv(U)^T, which starts as the identity
// and stays lower triangular -- the elimination is the forward substitution with U^T applied to [A | I], and
// inv(U^T) [A | I] = [U | inv(U)^T].  Of the 512 pieces of each, 272 touch its triangle; a thread owns ONE piece of ONE
// matrix (threads 0 .. 271 the pieces of A row by row, 272 .. 543 those of W: 9 waves, the last half empty), so the
// update is the same statement for every thread, m_ic -= u_ji x_c, with no case distinction per element; the elements
// of a diagonal piece that lie outside its triangle are carried along and never stored.  Nothing below the diagonal of
// the caller's matrix is loaded or stored.
//
// Step j = 0 .. jb - 1, rows in dpotf2's order, one barrier per step:
//   the owners of row j publish it UNSCALED in LDS (two buffers per matrix in turn): a_jc, and w_jc with w_jj = 1;
//   the thread that holds the pivot d = a_jj publishes u_jj = sqrt(d) (IEEE) and rinv = 1 / u_jj (reciprocal + Newton,
//   <= 1 ulp, the panel kernels' fast_recip) with it -- dpotf2 scales the row by the reciprocal too; every thread
//   reads d, and d <= 0 or NaN ends the factorisation (info = j + 1: the rows before j are final, the prefix property);
//   rows i > j:  a_ic -= (a_ji rinv) (a_jc rinv),   w_ic -= (a_ji rinv) (w_jc rinv)  (columns c <= j only: w_jc = 0 beyond),
//   every multiply-add an explicit fused operation.  A wave whose rows are all final skips the step.
// At the end u_ic = a_ic rinv_i, u_ii = sqrt(d_i), and inv(U)[c][i] = w_ic rinv_i.
// The inverse needs pivots whose reciprocal is a finite number, like the block inverses of the LU solves.
#include "common.h"

namespace lsx {

constexpr int CB = 128;   // block edge
constexpr int CR = 4, CC = 8;   // rows x columns of a thread's piece
constexpr int CPIECES = 272;    // pieces of 4 x 8 that touch a triangle of the block: sum over ti of 16 - ti / 2
constexpr int CT = 576;         // 9 waves: 2 x 272 pieces, 32 threads spare

__device__ __forceinline__ double chol_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float chol_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double chol_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float chol_sqrt(float x) { return sqrtf(x); }

// which piece a thread owns: cls 0 = the matrix (pieces with some c >= i: tj >= ti / 2), 1 = W (pieces with some
// c <= i: tj <= ti / 2), 2 = spare thread
struct CholPiece {
    int cls, r0, c0;
    __device__ __forceinline__ bool both() const { return c0 + CC - 1 >= r0 && c0 <= r0 + CR - 1; }   // a diagonal piece
};
__device__ __forceinline__ CholPiece chol_piece(int tid) {
    CholPiece p;
    p.cls = tid < CPIECES ? 0 : (tid < 2 * CPIECES ? 1 : 2);
    int rem = tid - (p.cls == 1 ? CPIECES : 0), ti = 0;
    if (p.cls == 2) rem = 0;
    for (;; ++ti) {
        const int cnt = p.cls == 1 ? (ti >> 1) + 1 : 16 - (ti >> 1);
        if (rem < cnt) break;
        rem -= cnt;
    }
    p.r0 = CR * ti;
    p.c0 = CC * (p.cls == 1 ? rem : (ti >> 1) + rem);
    return p;
}

// FACTORED = false: factor the block and carry W along; returns jb, or the row whose pivot failed.
// FACTORED = true: the upper half already holds U; only W is formed (no pivot test: u_jj > 0 is the caller's contract).
// ujj_s / rinv_s (LDS, CB entries, preset to 1) receive u_jj and 1 / u_jj of every row reached.
template <typename T, bool FACTORED>
__device__ __forceinline__ int chol_sweep(int jb, const CholPiece &pc, T (&M)[CR][CC], T (*rowA)[CB], T (*rowW)[CB], T *ujj_s,
                                          T *rinv_s) {
    const int r0 = pc.r0, c0 = pc.c0;
    const bool isW = pc.cls == 1;
    for (int j = 0; j < jb; ++j) {
        const T *rbA = rowA[j & 1];
        T *mine = isW ? rowW[j & 1] : rowA[j & 1];
        if (pc.cls < 2 && (j >> 2) == (r0 >> 2)) {
#pragma unroll
            for (int r = 0; r < CR; ++r)
                if (r == (j & 3)) {
#pragma unroll
                    for (int q = 0; q < CC; ++q) mine[c0 + q] = M[r][q];
                    // the thread that holds a_jj (final since the last step) forms u_jj and its reciprocal for everybody
                    if (!isW && (j >> 3) == (c0 >> 3)) {
                        T d = T(0);
#pragma unroll
                        for (int q = 0; q < CC; ++q)
                            if (q == (j & 7)) d = M[r][q];
                        const T ujj = FACTORED ? d : chol_sqrt(d);
                        const T rinv = fast_recip<T>(ujj);
                        ujj_s[j] = ujj;
                        rinv_s[j] = rinv;
                    }
                }
        }
        __syncthreads();
        if (!FACTORED && !(rbA[j] > T(0))) return j;   // uniform: every thread reads the same word
        const T rinv = rinv_s[j];
        // nothing to do: rows final; W right of column j (w_jc = 0 there); the matrix when it is given; spare threads
        if (r0 + CR - 1 <= j || (isW ? c0 > j : FACTORED) || pc.cls == 2) continue;
        T x[CC];
#pragma unroll
        for (int q = 0; q < CC; ++q) x[q] = mine[c0 + q] * rinv;
#pragma unroll
        for (int r = 0; r < CR; ++r) {
            const int i = r0 + r;
            const T ui = FACTORED ? rbA[i] : rbA[i] * rinv;
            if (i > j) {
#pragma unroll
                for (int q = 0; q < CC; ++q) M[r][q] = chol_fma(-ui, x[q], M[r][q]);
            }
        }
    }
    return jb;
}

// the pieces at the start: the upper part of the block at A (zero below the diagonal and outside jb), the identity for W
template <typename T>
__device__ __forceinline__ void chol_load(int jb, const CholPiece &pc, const T *__restrict__ A, int lda, T (&M)[CR][CC]) {
#pragma unroll
    for (int r = 0; r < CR; ++r)
#pragma unroll
        for (int q = 0; q < CC; ++q) {
            const int i = pc.r0 + r, c = pc.c0 + q;
            if (pc.cls == 0) M[r][q] = (c >= i && c < jb) ? A[(size_t)i * lda + c] : T(0);
            else M[r][q] = (c == i) ? T(1) : T(0);
        }
}

// element (c, i) of inv(U), c and i inside this thread's piece: from W (w_ic rinv_i, zero above W's diagonal) or, for
// the pieces of the matrix that W does not cover, zero; the identity when ident.  false: not this thread's to write.
template <typename T>
__device__ __forceinline__ bool chol_inv_elem(bool ident, const CholPiece &pc, int r, int q, const T (&M)[CR][CC],
                                              const T *rinv_s, T &v) {
    if (pc.cls == 2 || (pc.cls == 0 && pc.both())) return false;
    const int i = pc.r0 + r, c = pc.c0 + q;
    if (pc.cls == 0) v = T(0);
    else v = ident ? ((c == i) ? T(1) : T(0)) : M[r][q] * rinv_s[i];
    return true;
}

template <typename T>
__device__ __forceinline__ void chol_store_inv(bool ident, const CholPiece &pc, const T (&M)[CR][CC], const T *rinv_s,
                                               T *__restrict__ V) {
#pragma unroll
    for (int r = 0; r < CR; ++r)
#pragma unroll
        for (int q = 0; q < CC; ++q) {
            T v;
            if (chol_inv_elem<T>(ident, pc, r, q, M, rinv_s, v)) V[(size_t)(pc.c0 + q) * CB + pc.r0 + r] = v;
        }
}

template <typename T>
__global__ __launch_bounds__(CT) void chol_diag_kernel(int jb, T *__restrict__ A, int lda, int col0, T *__restrict__ Vinv,
                                                       int *__restrict__ info) {
    __shared__ __attribute__((aligned(16))) T rowA[2][CB], rowW[2][CB];
    __shared__ T ujj_s[CB], rinv_s[CB];
    const int tid = threadIdx.x;
    const CholPiece pc = chol_piece(tid);
    T M[CR][CC];
    if (*info != 0) {   // an earlier block failed: leave the matrix alone, hand the strip product an identity
        chol_store_inv<T>(true, pc, M, rinv_s, Vinv);
        return;
    }
    if (tid < CB) {
        ujj_s[tid] = T(1);
        rinv_s[tid] = T(1);
        rowA[0][tid] = rowA[1][tid] = T(0);
    }
    chol_load<T>(jb, pc, A, lda, M);
    __syncthreads();
    const int done = chol_sweep<T, false>(jb, pc, M, rowA, rowW, ujj_s, rinv_s);
    __syncthreads();
    if (done < jb && tid == 0) *info = col0 + done + 1;
    if (pc.cls == 0) {
#pragma unroll
        for (int r = 0; r < CR; ++r)
#pragma unroll
            for (int q = 0; q < CC; ++q) {
                const int i = pc.r0 + r, c = pc.c0 + q;
                if (i < done && c >= i && c < jb) A[(size_t)i * lda + c] = (c == i) ? ujj_s[i] : M[r][q] * rinv_s[i];
            }
    }
    chol_store_inv<T>(done < jb, pc, M, rinv_s, Vinv);
}

// one workgroup per 128-row diagonal block of the factor U
template <typename T>
__global__ __launch_bounds__(CT) void chol_inv_kernel(int n, const T *__restrict__ U, int lda, T *__restrict__ inv64,
                                                      T *__restrict__ inv128) {
    __shared__ __attribute__((aligned(16))) T rowA[2][CB], rowW[2][CB];
    __shared__ T ujj_s[CB], rinv_s[CB];
    const int tid = threadIdx.x;
    const CholPiece pc = chol_piece(tid);
    const int kb = (int)blockIdx.x * CB;
    const int jb = min(n - kb, CB);
    T M[CR][CC];
    if (tid < CB) {
        ujj_s[tid] = T(1);
        rinv_s[tid] = T(1);
        rowA[0][tid] = rowA[1][tid] = T(0);
    }
    chol_load<T>(jb, pc, U + (size_t)kb * lda + kb, lda, M);
    __syncthreads();
    chol_sweep<T, true>(jb, pc, M, rowA, rowW, ujj_s, rinv_s);
    __syncthreads();
    chol_store_inv<T>(false, pc, M, rinv_s, inv128 + (size_t)blockIdx.x * CB * CB);
    // the 64 x 64 diagonal blocks of inv(U_kk) are the inverses of U_kk's 64 x 64 diagonal blocks
#pragma unroll
    for (int r = 0; r < CR; ++r)
#pragma unroll
        for (int q = 0; q < CC; ++q) {
            const int i = pc.r0 + r, c = pc.c0 + q;   // element (c, i) of the inverse
            const int hb = i >> 6;
            T v;
            if ((c >> 6) != hb || kb + 64 * hb >= n || !chol_inv_elem<T>(false, pc, r, q, M, rinv_s, v)) continue;
            inv64[((size_t)(kb >> 6) + hb) * 4096 + (size_t)(c & 63) * 64 + (i & 63)] = v;
        }
}

template <typename T>
int launch_chol_diag(lsx_handle_t h, int jb, T *A, int lda, int col0, T *Vinv, int *info) {
    if (jb <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_PANEL, (double)jb * jb * jb / 3.0 * 2.0);
    hipLaunchKernelGGL(chol_diag_kernel<T>, dim3(1), dim3(CT), 0, h->stream, jb, A, lda, col0, Vinv, info);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

template <typename T>
int launch_chol_inv(lsx_handle_t h, int n, const T *U, int lda, T *inv64, T *inv128) {
    if (n <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_TRSM);
    hipLaunchKernelGGL(chol_inv_kernel<T>, dim3((n + CB - 1) / CB), dim3(CT), 0, h->stream, n, U, lda, inv64, inv128);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// ---------------------------------------------------------------- pieces of the SPD inverse (api.hip, potri_dev)
// The identity on and below the diagonal 128-blocks of X: row i gets columns [0, 128 (i / 128 + 1)), cut at n.  The
// blocks strictly above the diagonal blocks are not written.
template <typename T>
__global__ __launch_bounds__(256) void lower_identity_kernel(int n, T *__restrict__ X, int ldx) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= n || j >= CB * (i / CB + 1)) return;
    X[(size_t)i * ldx + j] = (i == j) ? T(1) : T(0);
}
template <typename T>
int launch_lower_identity(lsx_handle_t h, int n, T *X, int ldx) {
    if (n <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER);
    hipLaunchKernelGGL(lower_identity_kernel<T>, dim3((n + 255) / 256, n), dim3(256), 0, h->stream, n, X, ldx);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// dtrtri's singularity test on the diagonal of the factor: *info = 0, or i + 1 for the first u_ii that is exactly zero
// or NaN.  One workgroup.
template <typename T>
__global__ __launch_bounds__(256) void diag_zero_info_kernel(int n, const T *__restrict__ U, int lda, int *__restrict__ info) {
    __shared__ int s_first;
    if (threadIdx.x == 0) s_first = n;
    __syncthreads();
    int first = n;
    for (int i = threadIdx.x; i < n; i += 256) {
        const T d = U[(size_t)i * lda + i];
        if (d == T(0) || d != d) { first = i; break; }   // ascending per thread: its first hit is its smallest
    }
    if (first < n) atomicMin(&s_first, first);
    __syncthreads();
    if (threadIdx.x == 0) *info = s_first < n ? s_first + 1 : 0;
}
template <typename T>
int launch_diag_zero_info(lsx_handle_t h, int n, const T *U, int lda, int *info) {
    if (n <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER);
    hipLaunchKernelGGL(diag_zero_info_kernel<T>, dim3(1), dim3(256), 0, h->stream, n, U, lda, info);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// a_ji = a_ij for j > i: a transpose-copy of 32 x 32 tiles through LDS (padded rows: the transposed reads are
// conflict-free).  Workgroup (bx, by), bx >= by, reads the tile at rows 32 by, columns 32 bx of the upper triangle and
// writes its transpose at rows 32 bx, columns 32 by.  VEC: a complete tile off the diagonal of a 16-byte aligned matrix
// moves in 16-byte pieces on both sides; diagonal tiles (predicate j > i on both sides), edge tiles and unaligned
// matrices go element by element.  Copies only, so both forms give the same bits.  The diagonal and the upper triangle
// are not written.
constexpr int ST = 32;
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void symmetrize_upper_kernel(int n, T *__restrict__ A, int lda) {
    typedef T vec_t __attribute__((ext_vector_type(16 / sizeof(T))));
    constexpr int W = 16 / (int)sizeof(T);       // elements per 16 bytes
    constexpr int RP = 256 / (ST / W);           // tile rows per pass of the vector form
    __shared__ T s[ST][ST + 1];
    const int bx = blockIdx.x, by = blockIdx.y;
    if (bx < by) return;
    const int i0 = by * ST, j0 = bx * ST;
    const int tid = threadIdx.x;
    if (VEC && bx > by && j0 + ST <= n) {   // (i0 + ST <= j0: the tile is complete and strictly above the diagonal)
        const int q = (tid % (ST / W)) * W, r = tid / (ST / W);
#pragma unroll
        for (int rr = r; rr < ST; rr += RP) {
            const vec_t v = *(const vec_t *)(A + (size_t)(i0 + rr) * lda + j0 + q);
#pragma unroll
            for (int e = 0; e < W; ++e) s[rr][q + e] = v[e];
        }
        __syncthreads();
#pragma unroll
        for (int rr = r; rr < ST; rr += RP) {
            vec_t v;
#pragma unroll
            for (int e = 0; e < W; ++e) v[e] = s[q + e][rr];
            *(vec_t *)(A + (size_t)(j0 + rr) * lda + i0 + q) = v;
        }
        return;
    }
    const int c = tid & (ST - 1), r = tid >> 5;
    for (int rr = r; rr < ST; rr += 256 / ST) {
        const int i = i0 + rr, j = j0 + c;
        if (i < n && j < n && j > i) s[rr][c] = A[(size_t)i * lda + j];
    }
    __syncthreads();
    for (int rr = r; rr < ST; rr += 256 / ST) {
        const int j = j0 + rr, i = i0 + c;   // writes a_ji, row j, column i
        if (i < n && j < n && j > i) A[(size_t)j * lda + i] = s[c][rr];
    }
}
template <typename T>
int launch_symmetrize_upper(lsx_handle_t h, int n, T *A, int lda) {
    if (n <= 1) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER, 0, sizeof(T) * (double)n * n);
    const int t = (n + ST - 1) / ST;
    const bool aligned = ((size_t)A % 16 == 0) && (lda % (16 / (int)sizeof(T)) == 0);
    if (aligned) hipLaunchKernelGGL((symmetrize_upper_kernel<T, true>), dim3(t, t), dim3(256), 0, h->stream, n, A, lda);
    else hipLaunchKernelGGL((symmetrize_upper_kernel<T, false>), dim3(t, t), dim3(256), 0, h->stream, n, A, lda);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

#define LSX_POTRI_PIECES(T)                                                  \
    template int launch_lower_identity<T>(lsx_handle_t, int, T *, int);      \
    template int launch_diag_zero_info<T>(lsx_handle_t, int, const T *, int, int *); \
    template int launch_symmetrize_upper<T>(lsx_handle_t, int, T *, int);
LSX_POTRI_PIECES(double)
LSX_POTRI_PIECES(float)
#undef LSX_POTRI_PIECES

template int launch_chol_diag<double>(lsx_handle_t, int, double *, int, int, double *, int *);
template int launch_chol_diag<float>(lsx_handle_t, int, float *, int, int, float *, int *);
template int launch_chol_inv<double>(lsx_handle_t, int, const double *, int, double *, double *);
template int launch_chol_inv<float>(lsx_handle_t, int, const float *, int, float *, float *);

}  // namespace lsx
