// Two-sided Jacobi for the symmetric eigenproblem A = V diag(w) V^T (row-major, UPPER): the decision and rotation
// kernels of a round, and the small kernels around them.  Nothing here is cooperative: no kernel waits on another
// workgroup, every launch is ordered by the stream alone; the only atomic is the integer rotation counter.
//
// The work matrix W (n x n, BOTH triangles) and the accumulated rotations Z (n x n) live in the handle's eig_work, laid
// out like the SVD's work arrays (svd_ld): 16-byte aligned, a leading dimension that is a multiple of 16 bytes, zeros in
// the columns beyond n.  The caller's arrays are only copied from (upper triangle) and gathered into.
//
// Round r of a sweep (round-robin over P = n + (n & 1) players, api.hip: syevj_dev), two launches:
//   eig_decide_kernel   thread t takes the pair (i, j) at positions t and P - 1 - t, reads a = w_ii, b = w_jj, c = w_ij
//                       (the upper element) of W as it stands before the round, and leaves (i, j), (cs, sn) and the
//                       flag |c| > thr for the rotation launch.
//   eig_round_kernel    workgroup t owns ROWS i, j of its pair, thread u of it the COLUMNS (i_u, j_u) of pair u: the four
//                       elements w[i][i_u], w[i][j_u], w[j][i_u], w[j][j_u].  It applies the row rotation of pair t
//                       (rounded to T), then the column rotation of pair u (rounded again), and stores the four back.
//                       The pairs of a round partition the indices, so every element of W is read and written by exactly
//                       one thread of one workgroup and the update is done IN PLACE: no second buffer, and a quadruple
//                       whose row pair and column pair both stay is neither loaded nor stored.  Then rows i, j of Z.
// The two triangles of W are computed in different orders and may differ at rounding level; decisions read the upper
// element only, the eigenvalues are the diagonal.
#include "common.h"
#include "jacobi.h"

namespace lsx {

constexpr int EIG_NT = 256;     // threads of a pair's workgroup

// W (n x ldw, every column up to ldw written) from the upper triangle of A: w_ij = a_min(i,j),max(i,j), zeros beyond n
template <typename T>
__global__ __launch_bounds__(256) void eig_init_kernel(int n, const T *__restrict__ A, int lda, T *__restrict__ W, int ldw) {
    const int j = (int)blockIdx.y * 256 + (int)threadIdx.x, i = blockIdx.x;
    if (j >= ldw) return;
    T v = T(0);
    if (j < n) v = j >= i ? A[(size_t)i * lda + j] : A[(size_t)j * lda + i];
    W[(size_t)i * ldw + j] = v;
}
template <typename T>
int launch_eig_init(lsx_handle_t h, int n, const T *A, int lda, T *W, int ldw) {
    if (n <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER, 0, 2.0 * sizeof(T) * (double)n * ldw);
    hipLaunchKernelGGL(eig_init_kernel<T>, dim3(n, (ldw + 255) / 256), dim3(256), 0, h->stream, n, A, lda, W, ldw);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// the sum of v over the workgroup (EIG_NT threads) in thread 0: lanes by the butterfly, the four waves in order 0 .. 3
__device__ __forceinline__ double eig_block_sum(double v, double *red_s) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red_s[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
}

// rowsq[i] = w_ii^2 + 2 sum_{j > i} w_ij^2 in fp64: thread t adds columns i + t, i + t + 256, .. ascending
template <typename T>
__global__ __launch_bounds__(EIG_NT) void eig_rowsq_kernel(int n, const T *__restrict__ W, int ldw, double *__restrict__ rowsq) {
    __shared__ double red_s[EIG_NT / 64];
    const int i = blockIdx.x;
    const T *w = W + (size_t)i * ldw;
    double a = 0.0;
    for (int j = i + (int)threadIdx.x; j < n; j += EIG_NT) {
        const double x = (double)w[j];
        a = fma(j == i ? x : 2.0 * x, x, a);
    }
    a = eig_block_sum(a, red_s);
    if (threadIdx.x == 0) rowsq[i] = a;
}
// *nrm = sqrt(sum_i rowsq[i]): one workgroup, thread t adds rows t, t + 256, .. ascending
__global__ __launch_bounds__(EIG_NT) void eig_norm_kernel(int n, const double *__restrict__ rowsq, double *__restrict__ nrm) {
    __shared__ double red_s[EIG_NT / 64];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += EIG_NT) a += rowsq[i];
    a = eig_block_sum(a, red_s);
    if (threadIdx.x == 0) *nrm = sqrt(a);
}
template <typename T>
int launch_eig_norm(lsx_handle_t h, int n, const T *W, int ldw, double *rowsq, double *nrm) {
    if (n <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER, (double)n * n, 0.5 * sizeof(T) * (double)n * n);
    hipLaunchKernelGGL(eig_rowsq_kernel<T>, dim3(n), dim3(EIG_NT), 0, h->stream, n, W, ldw, rowsq);
    hipLaunchKernelGGL(eig_norm_kernel, dim3(1), dim3(EIG_NT), 0, h->stream, n, rowsq, nrm);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// The decisions of round r, all from W as it stands: one thread per position t < P / 2.
template <typename T>
__global__ __launch_bounds__(EIG_NT) void eig_decide_kernel(int n, int P, int r, const T *__restrict__ W, int ldw, double thr,
                                                            int2 *__restrict__ pair, double2 *__restrict__ rot,
                                                            int *__restrict__ flag, int *__restrict__ count) {
    const int t = (int)blockIdx.x * EIG_NT + (int)threadIdx.x;
    bool rotate = false;
    if (t < P / 2) {
        int i, j;
        round_robin_pair(P, r, t, &i, &j);
        double cs = 1.0, sn = 0.0;
        if (j < n) {   // else: the phantom player of an odd n
            const double a = (double)W[(size_t)i * ldw + i], b = (double)W[(size_t)j * ldw + j], c = (double)W[(size_t)i * ldw + j];
            rotate = fabs(c) > thr;   // a NaN fails the comparison
            if (rotate) jacobi_cs_sn(a, b, c, &cs, &sn);
        }
        pair[t] = make_int2(i, j);
        rot[t] = make_double2(cs, sn);
        flag[t] = rotate ? 1 : 0;
    }
    const unsigned long long votes = __ballot(rotate);
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(count, __popcll(votes));
}
template <typename T>
int launch_eig_decide(lsx_handle_t h, int n, int r, const T *W, int ldw, double thr, EigRound er, int *count) {
    if (n < 2) return LSX_OK;
    const int P = n + (n & 1);
    ProfScope ps(h, LSX_PROF_OTHER, 10.0 * (P / 2), 3.0 * sizeof(T) * (P / 2));
    hipLaunchKernelGGL(eig_decide_kernel<T>, dim3((P / 2 + EIG_NT - 1) / EIG_NT), dim3(EIG_NT), 0, h->stream, n, P, r, W, ldw, thr,
                       er.pair, er.rot, er.flag, count);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// x <- cs x - sn y, y <- sn x + cs y in fp64, each rounded to T once
template <typename T>
__device__ __forceinline__ void rotate1(T &x, T &y, double cs, double sn) {
    const double xi = (double)x, yj = (double)y;
    x = (T)(cs * xi - sn * yj);
    y = (T)(sn * xi + cs * yj);
}

// np = P / 2 pairs, one workgroup each; gz: 16-byte groups of a row of Z.  Rows i and j of W and Z belong to this
// workgroup alone, and inside it every element to one thread.
template <typename T>
__global__ __launch_bounds__(EIG_NT) void eig_round_kernel(int n, int np, int gz, T *__restrict__ W, int ldw, T *__restrict__ Z,
                                                           int ldz, const int2 *__restrict__ pair, const double2 *__restrict__ rot,
                                                           const int *__restrict__ flag) {
    constexpr int VE = vec_elems<T>();
    const int tid = threadIdx.x, t = blockIdx.x;
    const int2 rp = pair[t];
    const int i = rp.x, j = rp.y;
    const bool has_j = j < n;              // false: row i meets the phantom player and takes column rotations only
    const bool rrot = flag[t] != 0;        // implies has_j
    const double2 rr = rot[t];
    T *wi = W + (size_t)i * ldw, *wj = W + (size_t)(has_j ? j : i) * ldw;
    for (int u = tid; u < np; u += EIG_NT) {
        const bool crot = flag[u] != 0;    // implies j_u < n
        if (!rrot && !crot) continue;      // the four elements keep their bits
        const int2 cp = pair[u];
        const int iu = cp.x, ju = cp.y;
        const bool has_ju = ju < n;
        T xii = wi[iu], xij = has_ju ? wi[ju] : T(0);
        T xji = has_j ? wj[iu] : T(0), xjj = (has_j && has_ju) ? wj[ju] : T(0);
        if (rrot) {
            rotate1<T>(xii, xji, rr.x, rr.y);
            rotate1<T>(xij, xjj, rr.x, rr.y);
        }
        if (crot) {
            const double2 cr = rot[u];
            rotate1<T>(xii, xij, cr.x, cr.y);
            rotate1<T>(xji, xjj, cr.x, cr.y);
        }
        if (rrot && u == t) { xij = T(0); xji = T(0); }   // w_ij = w_ji = 0 exactly
        wi[iu] = xii;
        if (has_ju) wi[ju] = xij;
        if (has_j) {
            wj[iu] = xji;
            if (has_ju) wj[ju] = xjj;
        }
    }
    if (Z && rrot) {
        T *zi = Z + (size_t)i * ldz, *zj = Z + (size_t)j * ldz;
        T yi[VE], yj[VE];
        for (int g = tid; g < gz; g += EIG_NT) {
            load16<T>(zi + (size_t)g * VE, yi);
            load16<T>(zj + (size_t)g * VE, yj);
            rotate16<T>(yi, yj, rr.x, rr.y);
            store16<T>(zi + (size_t)g * VE, yi);
            store16<T>(zj + (size_t)g * VE, yj);
        }
    }
}
// W: n rows of ldw >= n elements; Z (or null): n rows of ldz elements, 16-byte aligned with ldz a multiple of 16 bytes
template <typename T>
int launch_eig_round(lsx_handle_t h, int n, T *W, int ldw, T *Z, int ldz, EigRound er) {
    if (n < 2) return LSX_OK;
    constexpr int VE = vec_elems<T>();
    if (ldw < n || (Z && (((size_t)Z % 16) || (ldz % VE) || ldz < n))) {
        set_error("eig round: the work arrays are not laid out in 16-byte groups");
        return LSX_ERR_INTERNAL;
    }
    const int P = n + (n & 1);
    ProfScope ps(h, LSX_PROF_PANEL, 12.0 * (double)n * n + (Z ? 6.0 * (double)n * n : 0.0),
                 2.0 * sizeof(T) * (double)n * n * (Z ? 2.0 : 1.0));
    hipLaunchKernelGGL(eig_round_kernel<T>, dim3(P / 2), dim3(EIG_NT), 0, h->stream, n, P / 2, ldz / VE, W, ldw, Z, ldz, er.pair,
                       er.rot, er.flag);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// d[i] = (double) w_ii
template <typename T>
__global__ __launch_bounds__(256) void eig_diag_kernel(int n, const T *__restrict__ W, int ldw, double *__restrict__ d) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i < n) d[i] = (double)W[(size_t)i * ldw + i];
}
template <typename T>
int launch_eig_diag(lsx_handle_t h, int n, const T *W, int ldw, double *d) {
    if (n <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER, 0, (sizeof(T) + 8.0) * n);
    hipLaunchKernelGGL(eig_diag_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, W, ldw, d);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

#define LSX_EIG_PIECES(T)                                                                              \
    template int launch_eig_init<T>(lsx_handle_t, int, const T *, int, T *, int);                      \
    template int launch_eig_norm<T>(lsx_handle_t, int, const T *, int, double *, double *);            \
    template int launch_eig_decide<T>(lsx_handle_t, int, int, const T *, int, double, EigRound, int *); \
    template int launch_eig_round<T>(lsx_handle_t, int, T *, int, T *, int, EigRound);                 \
    template int launch_eig_diag<T>(lsx_handle_t, int, const T *, int, double *);
LSX_EIG_PIECES(double)
LSX_EIG_PIECES(float)
#undef LSX_EIG_PIECES

}  // namespace lsx
