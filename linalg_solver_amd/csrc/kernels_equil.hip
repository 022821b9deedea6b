// Equilibration (lsx_geequ_*, lsx_laqge_*, the scaling steps of lsx_gesvx_*): LAPACK's geequ row and column scale
// factors, laqge's scaling of the matrix, and the max-abs reductions behind the reciprocal pivot growth.  DESIGN
// section 3.6.
//
// Every kernel streams the matrix once and sizes its grid from the matrix; there are no atomics and no workgroup
// waits for another: a reduction is two launches (partial results in a fixed partition, then one workgroup).  The
// only arithmetic is |a|, maxima, products and one IEEE division per scale factor, in the working precision T, step
// for step as dgeequ.f / dlaqge.f: r, c, rowcnd, colcnd, amax and the scaled matrix have LAPACK's bits.  A maximum
// does not depend on the order of its operands, so the 16-byte form (base 16-byte aligned, leading dimension and
// column count multiples of 16 / sizeof(T)) and the element-wise form of a kernel give the same result.
#include "common.h"

namespace lsx {

namespace {

__device__ __forceinline__ double eq_nan_max(const double a, const double b) { return (b > a || b != b) ? b : a; }

template <typename T> struct EqVec;
template <> struct EqVec<double> { typedef double2 type; };
template <> struct EqVec<float> { typedef float4 type; };

// smlnum = lamch('S'), bignum = 1 / smlnum
template <typename T> struct EqLim;
template <> struct EqLim<double> { static constexpr double sml = 0x1p-1022, big = 0x1p+1022; };
template <> struct EqLim<float> { static constexpr float sml = 0x1p-126f, big = 0x1p+126f; };

// 1 / min(max(v, smlnum), bignum): the one division per scale factor (a NaN maximum takes smlnum)
template <typename T>
__device__ __forceinline__ T eq_scale_of(const T v) {
    T t = v > EqLim<T>::sml ? v : EqLim<T>::sml;
    t = t < EqLim<T>::big ? t : EqLim<T>::big;
    return T(1) / t;
}

constexpr int EQ_FT = 1024;    // threads of the one-workgroup final steps
constexpr int EQ_ROWS = 256;   // rows per partial column maximum
constexpr int LQ_ROWS = 16;    // rows per workgroup of the scaling kernel

// ------------------------------------------------------------------ row maxima
// One wave per row, lanes across the columns [0, k) -- upper != 0: [row, k), the upper triangle with the diagonal --
// and a fixed tree over the lanes: P[row] = max |a| as a double (exact for both element types; a NaN wins).
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void equil_rowmax_kernel(int m, int k, const T *__restrict__ A, int lda, int upper,
                                                           double *__restrict__ P) {
    constexpr int V = 16 / (int)sizeof(T);
    typedef typename EqVec<T>::type vec_t;
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;
    const int j0 = upper ? min(row, k) : 0;
    const T *a = A + (size_t)row * lda;
    double v = 0;
    if (VEC) {
        // whole 16-byte pieces from the one that holds column j0: k % V == 0, so a piece never crosses column k
        for (int c = (j0 / V + lane) * V; c < k; c += 64 * V) {
            const vec_t q = *reinterpret_cast<const vec_t *>(a + c);
            const T *e = reinterpret_cast<const T *>(&q);
#pragma unroll
            for (int t = 0; t < V; ++t)
                if (c + t >= j0) v = eq_nan_max(v, fabs((double)e[t]));
        }
    } else {
        for (int c = j0 + lane; c < k; c += 64) v = eq_nan_max(v, fabs((double)a[c]));
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = eq_nan_max(v, __shfl_down(v, d, 64));
    if (lane == 0) P[row] = v;
}

// one workgroup: out[0] = max of P[0 .. len) (a NaN wins; 0 for len == 0)
__global__ __launch_bounds__(EQ_FT) void equil_max_final_kernel(int len, const double *__restrict__ P,
                                                                double *__restrict__ out) {
    __shared__ double s_v[EQ_FT];
    double v = 0;
    for (int i = threadIdx.x; i < len; i += EQ_FT) v = eq_nan_max(v, P[i]);
    s_v[threadIdx.x] = v;
    __syncthreads();
    for (int s = EQ_FT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_v[threadIdx.x] = eq_nan_max(s_v[threadIdx.x], s_v[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = s_v[0];
}

// Smallest and largest of the len maxima a thread block was handed, and the first index whose maximum is exactly 0
// (len if none): the RCMIN / RCMAX loop of geequ.  Every thread returns the block's result.
template <typename T>
__device__ __forceinline__ void eq_block_minmax(T &mn, T &mx, int &zi) {
    __shared__ double s_mn[EQ_FT], s_mx[EQ_FT];
    __shared__ int s_zi[EQ_FT];
    s_mn[threadIdx.x] = (double)mn;
    s_mx[threadIdx.x] = (double)mx;
    s_zi[threadIdx.x] = zi;
    __syncthreads();
    for (int s = EQ_FT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double o = s_mn[threadIdx.x + s];
            if (o < s_mn[threadIdx.x]) s_mn[threadIdx.x] = o;
            s_mx[threadIdx.x] = eq_nan_max(s_mx[threadIdx.x], s_mx[threadIdx.x + s]);
            s_zi[threadIdx.x] = min(s_zi[threadIdx.x], s_zi[threadIdx.x + s]);
        }
        __syncthreads();
    }
    mn = (T)s_mn[0];
    mx = (T)s_mx[0];
    zi = s_zi[0];
}

// One workgroup after the row pass: r_i, and stats = {rowcnd, colcnd (1 until the column pass), amax, info}.
// A zero row: info = its 1-based index, rowcnd = colcnd = 0 (LAPACK leaves them unset), r unspecified.
template <typename T>
__global__ __launch_bounds__(EQ_FT) void equil_row_final_kernel(int m, const double *__restrict__ P, T *__restrict__ r,
                                                                double *__restrict__ stats) {
    T mn = EqLim<T>::big, mx = 0;
    int zi = m;
    for (int i = threadIdx.x; i < m; i += EQ_FT) {
        const T v = (T)P[i];
        mx = (T)eq_nan_max((double)mx, (double)v);
        if (v < mn) mn = v;
        if (v == T(0)) zi = min(zi, i);
        r[i] = eq_scale_of<T>(v);
    }
    eq_block_minmax<T>(mn, mx, zi);
    if (threadIdx.x != 0) return;
    stats[2] = (double)mx;                                   // amax
    if (mn == T(0)) {
        stats[0] = 0.0;
        stats[1] = 0.0;
        stats[3] = (double)(zi + 1);
    } else {
        const T lo = mn > EqLim<T>::sml ? mn : EqLim<T>::sml, hi = mx < EqLim<T>::big ? mx : EqLim<T>::big;
        stats[0] = (double)(lo / hi);
        stats[1] = 1.0;
        stats[3] = 0.0;
    }
}

// ------------------------------------------------------------------ column maxima of the row-scaled matrix
// Thread = V adjacent columns (a wave reads 64 adjacent 16-byte pieces of a row; element-wise form: V = 1), workgroup
// row = one chunk of EQ_ROWS rows: Pc[chunk][column] = max_i |a_ij| * r_i over the chunk, products in T.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void equil_colpart_kernel(int m, int n, const T *__restrict__ A, int lda,
                                                            const T *__restrict__ r, T *__restrict__ Pc) {
    constexpr int V = VEC ? 16 / (int)sizeof(T) : 1;
    typedef typename EqVec<T>::type vec_t;
    __shared__ T s_r[EQ_ROWS];
    const int r0 = blockIdx.y * EQ_ROWS, rows = min(m - r0, EQ_ROWS);
    for (int i = threadIdx.x; i < rows; i += 256) s_r[i] = r[r0 + i];
    __syncthreads();
    const int c = (blockIdx.x * 256 + threadIdx.x) * V;
    if (c >= n) return;
    double v[V];
#pragma unroll
    for (int t = 0; t < V; ++t) v[t] = 0;
    const T *a = A + (size_t)r0 * lda + c;
#pragma unroll 4
    for (int i = 0; i < rows; ++i) {
        const T ri = s_r[i];
        if (VEC) {
            const vec_t q = *reinterpret_cast<const vec_t *>(a + (size_t)i * lda);
            const T *e = reinterpret_cast<const T *>(&q);
#pragma unroll
            for (int t = 0; t < V; ++t) v[t] = eq_nan_max(v[t], (double)(T)(fabs(e[t]) * ri));
        } else {
            v[0] = eq_nan_max(v[0], (double)(T)(fabs(a[(size_t)i * lda]) * ri));
        }
    }
#pragma unroll
    for (int t = 0; t < V; ++t) Pc[(size_t)blockIdx.y * n + c + t] = (T)v[t];
}

// One workgroup after the column pass: c_j, colcnd, and info = m + j (1-based j) for the first zero column of the
// row-scaled matrix.  Nothing is done when the row pass already set info.
template <typename T>
__global__ __launch_bounds__(EQ_FT) void equil_col_final_kernel(int m, int n, int chunks, const T *__restrict__ Pc,
                                                                T *__restrict__ c, double *__restrict__ stats) {
    if (stats[3] != 0.0) return;
    T mn = EqLim<T>::big, mx = 0;
    int zi = n;
    for (int j = threadIdx.x; j < n; j += EQ_FT) {
        double w = 0;
        for (int ch = 0; ch < chunks; ++ch) w = eq_nan_max(w, (double)Pc[(size_t)ch * n + j]);
        const T v = (T)w;
        mx = (T)eq_nan_max((double)mx, w);
        if (v < mn) mn = v;
        if (v == T(0)) zi = min(zi, j);
        c[j] = eq_scale_of<T>(v);
    }
    eq_block_minmax<T>(mn, mx, zi);
    if (threadIdx.x != 0) return;
    if (mn == T(0)) {
        stats[1] = 0.0;
        stats[3] = (double)m + (double)(zi + 1);
    } else {
        const T lo = mn > EqLim<T>::sml ? mn : EqLim<T>::sml, hi = mx < EqLim<T>::big ? mx : EqLim<T>::big;
        stats[1] = (double)(lo / hi);
    }
}

// m == 0 or n == 0
__global__ void equil_empty_stats_kernel(double *__restrict__ stats) {
    if (threadIdx.x == 0) { stats[0] = 1.0; stats[1] = 1.0; stats[2] = 0.0; stats[3] = 0.0; }
}

// ------------------------------------------------------------------ laqge: A <- diag(r) A diag(c)
// r null: columns only; c null: rows only; both: a_ij = (c_j * r_i) * a_ij, dlaqge's association.  D2 non-null: the
// scaled matrix is also written there in the same pass (the copy the driver factors).  Thread = V adjacent columns
// of LQ_ROWS rows, its c_j kept in registers; grid = (row groups, column blocks).
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void laqge_kernel(int m, int n, T *A, int lda, const T *__restrict__ r,
                                                    const T *__restrict__ c, T *D2, int ld2) {
    constexpr int V = VEC ? 16 / (int)sizeof(T) : 1;
    typedef typename EqVec<T>::type vec_t;
    const int col = (blockIdx.y * 256 + threadIdx.x) * V;
    if (col >= n) return;
    const int r0 = blockIdx.x * LQ_ROWS, r1 = min(m, r0 + LQ_ROWS);
    T cj[V];
#pragma unroll
    for (int t = 0; t < V; ++t) cj[t] = c ? c[col + t] : T(1);
#pragma unroll 4
    for (int i = r0; i < r1; ++i) {
        T *p = A + (size_t)i * lda + col;
        T e[V];
        if (VEC) {
            const vec_t q = *reinterpret_cast<const vec_t *>(p);
            const T *s = reinterpret_cast<const T *>(&q);
#pragma unroll
            for (int t = 0; t < V; ++t) e[t] = s[t];
        } else {
            e[0] = p[0];
        }
        if (r) {
            const T ri = r[i];
#pragma unroll
            for (int t = 0; t < V; ++t) e[t] = (c ? cj[t] * ri : ri) * e[t];
        } else {
#pragma unroll
            for (int t = 0; t < V; ++t) e[t] = cj[t] * e[t];
        }
        if (VEC) {
            vec_t q;
            T *s = reinterpret_cast<T *>(&q);
#pragma unroll
            for (int t = 0; t < V; ++t) s[t] = e[t];
            *reinterpret_cast<vec_t *>(p) = q;
            if (D2) *reinterpret_cast<vec_t *>(D2 + (size_t)i * ld2 + col) = q;
        } else {
            p[0] = e[0];
            if (D2) D2[(size_t)i * ld2 + col] = e[0];
        }
    }
}

template <typename T>
bool eq_vec_ok(const T *p, int ld, int cols) {
    constexpr int V = 16 / (int)sizeof(T);
    return ((uintptr_t)p % 16 == 0) && ld % V == 0 && cols % V == 0;
}

}  // namespace

// ------------------------------------------------------------------ launchers
size_t geequ_work_bytes(int m, int n, size_t elem) {
    if (m <= 0 || n <= 0) return 0;
    const size_t rows = (sizeof(double) * (size_t)m + 255) & ~(size_t)255;
    return rows + elem * (size_t)((m + EQ_ROWS - 1) / EQ_ROWS) * (size_t)n;
}

// r[m], c[n], stats[4] = {rowcnd, colcnd, amax, info}; d_work: geequ_work_bytes(m, n, sizeof(T)) bytes.
// passes: 1 = the row pass and its final step, 2 = the column pass and its (r and stats from a row pass), 3 = geequ
template <typename T>
int launch_geequ(lsx_handle_t h, int m, int n, const T *A, int lda, T *r, T *c, double *stats, void *d_work, int passes) {
    if (m <= 0 || n <= 0) {
        hipLaunchKernelGGL(equil_empty_stats_kernel, dim3(1), dim3(64), 0, h->stream, stats);
        LSX_HIP(hipGetLastError());
        return LSX_OK;
    }
    ProfScope ps(h, LSX_PROF_OTHER, 3.0 * m * (double)n, 2.0 * sizeof(T) * (double)m * n);
    constexpr int V = 16 / (int)sizeof(T);
    double *P = (double *)d_work;
    T *Pc = (T *)((char *)d_work + ((sizeof(double) * (size_t)m + 255) & ~(size_t)255));
    const int chunks = (m + EQ_ROWS - 1) / EQ_ROWS;
    const bool vec = eq_vec_ok(A, lda, n);
    if (passes & 1) {
        if (vec)
            hipLaunchKernelGGL((equil_rowmax_kernel<T, true>), dim3((m + 3) / 4), dim3(256), 0, h->stream, m, n, A, lda, 0, P);
        else
            hipLaunchKernelGGL((equil_rowmax_kernel<T, false>), dim3((m + 3) / 4), dim3(256), 0, h->stream, m, n, A, lda, 0, P);
        hipLaunchKernelGGL(equil_row_final_kernel<T>, dim3(1), dim3(EQ_FT), 0, h->stream, m, (const double *)P, r, stats);
    }
    if (passes & 2) {
        if (vec)
            hipLaunchKernelGGL((equil_colpart_kernel<T, true>), dim3((n / V + 255) / 256, chunks), dim3(256), 0, h->stream,
                               m, n, A, lda, (const T *)r, Pc);
        else
            hipLaunchKernelGGL((equil_colpart_kernel<T, false>), dim3((n + 255) / 256, chunks), dim3(256), 0, h->stream, m,
                               n, A, lda, (const T *)r, Pc);
        hipLaunchKernelGGL(equil_col_final_kernel<T>, dim3(1), dim3(EQ_FT), 0, h->stream, m, n, chunks, (const T *)Pc, c,
                           stats);
    }
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// A (m x n) <- diag(r) A diag(c), r or c null = that side unscaled; D2 (may be null): a second copy of the result
template <typename T>
int launch_laqge(lsx_handle_t h, int m, int n, T *A, int lda, const T *r, const T *c, T *D2, int ld2) {
    if (m <= 0 || n <= 0 || (!r && !c)) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER, 2.0 * m * (double)n, (D2 ? 3.0 : 2.0) * sizeof(T) * (double)m * n);
    constexpr int V = 16 / (int)sizeof(T);
    const int gy = (m + LQ_ROWS - 1) / LQ_ROWS;
    if (eq_vec_ok(A, lda, n) && (!D2 || eq_vec_ok(D2, ld2, n)))
        hipLaunchKernelGGL((laqge_kernel<T, true>), dim3(gy, (n / V + 255) / 256), dim3(256), 0, h->stream, m, n, A, lda, r,
                           c, D2, ld2);
    else
        hipLaunchKernelGGL((laqge_kernel<T, false>), dim3(gy, (n + 255) / 256), dim3(256), 0, h->stream, m, n, A, lda, r, c,
                           D2, ld2);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

size_t maxabs_work_bytes(int m) { return m > 0 ? sizeof(double) * (size_t)m : 0; }

// d_out[0] = max |a_ij| over the first k columns of the m x (>= k) matrix at A: all rows, or (upper) the entries on
// and above the diagonal.  0 for an empty range, NaN if it holds one; d_work: maxabs_work_bytes(m) bytes
template <typename T>
int launch_maxabs(lsx_handle_t h, int m, int k, const T *A, int lda, int upper, double *d_work, double *d_out) {
    if (upper && m > k) m = k;                               // the rows below the triangle hold nothing of it
    if (m <= 0 || k <= 0) {
        LSX_HIP(hipMemsetAsync(d_out, 0, sizeof(double), h->stream));
        return LSX_OK;
    }
    ProfScope ps(h, LSX_PROF_OTHER, (double)m * k, sizeof(T) * (double)m * k * (upper ? 0.5 : 1.0));
    if (eq_vec_ok(A, lda, k))
        hipLaunchKernelGGL((equil_rowmax_kernel<T, true>), dim3((m + 3) / 4), dim3(256), 0, h->stream, m, k, A, lda, upper,
                           d_work);
    else
        hipLaunchKernelGGL((equil_rowmax_kernel<T, false>), dim3((m + 3) / 4), dim3(256), 0, h->stream, m, k, A, lda, upper,
                           d_work);
    hipLaunchKernelGGL(equil_max_final_kernel, dim3(1), dim3(EQ_FT), 0, h->stream, m, (const double *)d_work, d_out);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

#define LSX_INST_EQUIL(T)                                                                                          \
    template int launch_geequ<T>(lsx_handle_t, int, int, const T *, int, T *, T *, double *, void *, int);         \
    template int launch_laqge<T>(lsx_handle_t, int, int, T *, int, const T *, const T *, T *, int);                \
    template int launch_maxabs<T>(lsx_handle_t, int, int, const T *, int, int, double *, double *);
LSX_INST_EQUIL(double)
LSX_INST_EQUIL(float)
#undef LSX_INST_EQUIL

}  // namespace lsx
