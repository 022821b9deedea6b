// One-sided Jacobi SVD (row-major): the round kernel that rotates pairs of rows, and the small kernels around it.
// Nothing here is cooperative: no kernel waits on another workgroup, every launch is ordered by the stream alone.
//
// The work matrix W (p x q) and the accumulated rotations Z (p x p) live in the handle's svd_work with leading
// dimensions that are multiples of 16 bytes and zero columns up to them (svd_ld), so every access of the round kernel
// is a 16-byte one and a row has no tail: the padding is summed and rotated like data, zeros stay zeros.  A caller's
// matrix, of whatever alignment and leading dimension, is only touched by the copy into W and by the gather out of it,
// both element-wise -- the bits of a result cannot depend on how the caller's array lies.
//
// Round r of a sweep (round-robin over P = p + (p & 1) players, api.hip: gesvdj_run): workgroup t owns the pair at
// positions t and P - 1 - t.  It forms a = w_i.w_i, b = w_j.w_j, c = w_i.w_j in fp64, decides, and rotates the two rows
// of W and of Z.  Order of a sum: thread t adds its 16-byte groups g = t, t + 256, .. ascending, elements ascending
// inside a group, with fused multiply-adds; the 64 lanes of a wave are added by a butterfly (xor 32, 16, .. 1), the four
// waves in order 0 .. 3.  Rows of at most SVD_KEEP groups per thread stay in registers between the sums and the rotation
// (W is read once per round); longer rows are read again, from L2.  Both forms add in the same order.
#include "common.h"
#include "jacobi.h"

namespace lsx {

constexpr int SVD_NT = 256;     // threads of a pair's workgroup
constexpr int SVD_KEEP = 8;     // 16-byte groups per thread and row that stay in registers: rows up to 4096 fp64 / 8192 fp32

int svd_ld(int cols, size_t elem) {
    const int ve = 16 / (int)elem;
    return cols <= 0 ? ve : (cols + ve - 1) / ve * ve;
}
int svd_keep_cols(size_t elem) { return SVD_NT * SVD_KEEP * (16 / (int)elem); }

// cs, sn of the rotation that makes the rows orthogonal; false: the pair is left alone (a NaN fails the comparison)
__device__ __forceinline__ bool jacobi_rotation(double a, double b, double c, double tol, double *cs, double *sn) {
    if (!(fabs(c) > tol * sqrt(a) * sqrt(b))) return false;
    jacobi_cs_sn(a, b, c, cs, sn);
    return true;
}

// gq, gz: 16-byte groups of a row of W and of Z (ld / elements per group).  KEEP: gq <= SVD_NT * SVD_KEEP.
template <typename T, bool KEEP>
__global__ __launch_bounds__(SVD_NT) void svd_round_kernel(int p, int P, int r, int gq, int gz, T *__restrict__ W, int ldw,
                                                           T *__restrict__ Z, int ldz, double tol, int *__restrict__ count) {
    constexpr int VE = vec_elems<T>();
    __shared__ double red_s[3][SVD_NT / 64];
    const int tid = threadIdx.x;
    // positions t and P - 1 - t of round r
    int i, j;
    round_robin_pair(P, r, (int)blockIdx.x, &i, &j);
    if (j >= p) return;   // the phantom player of an odd p
    T *wi = W + (size_t)i * ldw, *wj = W + (size_t)j * ldw;
    T xi[KEEP ? SVD_KEEP : 1][VE], xj[KEEP ? SVD_KEEP : 1][VE];
    double a = 0.0, b = 0.0, c = 0.0;
    if (KEEP) {
#pragma unroll
        for (int u = 0; u < SVD_KEEP; ++u) {
            const int g = tid + u * SVD_NT;
            if (g < gq) {
                load16<T>(wi + (size_t)g * VE, xi[u]);
                load16<T>(wj + (size_t)g * VE, xj[u]);
            } else {
#pragma unroll
                for (int k = 0; k < VE; ++k) { xi[u][k] = T(0); xj[u][k] = T(0); }
            }
        }
#pragma unroll
        for (int u = 0; u < SVD_KEEP; ++u) {
            if (tid + u * SVD_NT < gq) {
#pragma unroll
                for (int k = 0; k < VE; ++k) {
                    const double x = (double)xi[u][k], y = (double)xj[u][k];
                    a = fma(x, x, a); b = fma(y, y, b); c = fma(x, y, c);
                }
            }
        }
    } else {
        for (int g = tid; g < gq; g += SVD_NT) {
            load16<T>(wi + (size_t)g * VE, xi[0]);
            load16<T>(wj + (size_t)g * VE, xj[0]);
#pragma unroll
            for (int k = 0; k < VE; ++k) {
                const double x = (double)xi[0][k], y = (double)xj[0][k];
                a = fma(x, x, a); b = fma(y, y, b); c = fma(x, y, c);
            }
        }
    }
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    if ((tid & 63) == 0) { red_s[0][tid >> 6] = a; red_s[1][tid >> 6] = b; red_s[2][tid >> 6] = c; }
    __syncthreads();
    a = ((red_s[0][0] + red_s[0][1]) + red_s[0][2]) + red_s[0][3];
    b = ((red_s[1][0] + red_s[1][1]) + red_s[1][2]) + red_s[1][3];
    c = ((red_s[2][0] + red_s[2][1]) + red_s[2][2]) + red_s[2][3];
    double cs = 1.0, sn = 0.0;
    if (!jacobi_rotation(a, b, c, tol, &cs, &sn)) return;   // uniform over the workgroup
    if (tid == 0) atomicAdd(count, 1);
    if (KEEP) {
#pragma unroll
        for (int u = 0; u < SVD_KEEP; ++u) {
            const int g = tid + u * SVD_NT;
            if (g < gq) {
                rotate16<T>(xi[u], xj[u], cs, sn);
                store16<T>(wi + (size_t)g * VE, xi[u]);
                store16<T>(wj + (size_t)g * VE, xj[u]);
            }
        }
    } else {
        for (int g = tid; g < gq; g += SVD_NT) {
            load16<T>(wi + (size_t)g * VE, xi[0]);
            load16<T>(wj + (size_t)g * VE, xj[0]);
            rotate16<T>(xi[0], xj[0], cs, sn);
            store16<T>(wi + (size_t)g * VE, xi[0]);
            store16<T>(wj + (size_t)g * VE, xj[0]);
        }
    }
    if (Z) {
        T *zi = Z + (size_t)i * ldz, *zj = Z + (size_t)j * ldz;
        T yi[VE], yj[VE];
        for (int g = tid; g < gz; g += SVD_NT) {
            load16<T>(zi + (size_t)g * VE, yi);
            load16<T>(zj + (size_t)g * VE, yj);
            rotate16<T>(yi, yj, cs, sn);
            store16<T>(zi + (size_t)g * VE, yi);
            store16<T>(zj + (size_t)g * VE, yj);
        }
    }
}

// W: p rows of ldw elements, Z (or null): p rows of ldz; both 16-byte aligned with ld a multiple of 16 bytes and zeros
// in the columns beyond q and p.  count: the sweep's rotation counter.
template <typename T>
int launch_svd_round(lsx_handle_t h, int p, int q, int r, T *W, int ldw, T *Z, int ldz, double tol, int *count) {
    if (p < 2) return LSX_OK;
    constexpr int VE = vec_elems<T>();
    if (((size_t)W % 16) || (ldw % VE) || ldw < q || (Z && (((size_t)Z % 16) || (ldz % VE) || ldz < p))) {
        set_error("svd round: the work arrays are not laid out in 16-byte groups");
        return LSX_ERR_INTERNAL;
    }
    const int P = p + (p & 1), gq = ldw / VE, gz = ldz / VE;
    ProfScope ps(h, LSX_PROF_PANEL, 3.0 * (double)(p / 2) * (3.0 * q + 3.0 * p), 2.0 * sizeof(T) * (double)p * ((double)q + p));
    if (gq <= SVD_NT * SVD_KEEP)
        hipLaunchKernelGGL((svd_round_kernel<T, true>), dim3(P / 2), dim3(SVD_NT), 0, h->stream, p, P, r, gq, gz, W, ldw, Z, ldz,
                           tol, count);
    else
        hipLaunchKernelGGL((svd_round_kernel<T, false>), dim3(P / 2), dim3(SVD_NT), 0, h->stream, p, P, r, gq, gz, W, ldw, Z,
                           ldz, tol, count);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// D (rows x ldd, every column up to ldd written) = S (rows x cols) with zeros beyond cols and, with upper set, below the
// diagonal: the work matrix from A, or from the R of a factored array.  S null: the identity (Z).
template <typename T>
__global__ __launch_bounds__(256) void svd_init_kernel(int cols, const T *__restrict__ S, int lds, int upper, T *__restrict__ D,
                                                       int ldd) {
    const int j = (int)blockIdx.y * 256 + (int)threadIdx.x, i = blockIdx.x;
    if (j >= ldd) return;
    T v = T(0);
    if (j < cols) {
        if (!S) v = (i == j) ? T(1) : T(0);
        else if (!upper || j >= i) v = S[(size_t)i * lds + j];
    }
    D[(size_t)i * ldd + j] = v;
}
template <typename T>
int launch_svd_init(lsx_handle_t h, int rows, int cols, const T *S, int lds, int upper, T *D, int ldd) {
    if (rows <= 0 || ldd <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER, 0, 2.0 * sizeof(T) * (double)rows * ldd);
    hipLaunchKernelGGL(svd_init_kernel<T>, dim3(rows, (ldd + 255) / 256), dim3(256), 0, h->stream, cols, S, lds, upper, D, ldd);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// sigma[i] = sqrt(sum_k w_ik^2), one workgroup per row, the sum in the round kernel's order
template <typename T>
__global__ __launch_bounds__(SVD_NT) void svd_rownorm_kernel(int gq, const T *__restrict__ W, int ldw, double *__restrict__ sigma) {
    constexpr int VE = vec_elems<T>();
    __shared__ double red_s[SVD_NT / 64];
    const int tid = threadIdx.x;
    const T *w = W + (size_t)blockIdx.x * ldw;
    double a = 0.0;
    T x[VE];
    for (int g = tid; g < gq; g += SVD_NT) {
        load16<T>(w + (size_t)g * VE, x);
#pragma unroll
        for (int k = 0; k < VE; ++k) a = fma((double)x[k], (double)x[k], a);
    }
    a = wave_sum(a);
    if ((tid & 63) == 0) red_s[tid >> 6] = a;
    __syncthreads();
    if (tid == 0) sigma[blockIdx.x] = sqrt(((red_s[0] + red_s[1]) + red_s[2]) + red_s[3]);
}
template <typename T>
int launch_svd_rownorm(lsx_handle_t h, int p, int q, const T *W, int ldw, double *sigma) {
    if (p <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER, 2.0 * (double)p * q, sizeof(T) * (double)p * q);
    hipLaunchKernelGGL(svd_rownorm_kernel<T>, dim3(p), dim3(SVD_NT), 0, h->stream, ldw / vec_elems<T>(), W, ldw, sigma);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// The results in the order perm (sorted index i takes row perm[i]).  Workgroups [0, k): s[i] = sigma[perm[i]] and, if Vt
// is given, row i of Vt = w / sigma in fp64, rounded once (a row of zeros for sigma == 0).  Workgroups from k on, if U is
// given: the 32 x 32 tiles of U (urows x k), U[r][i] = Z[perm[i]][r] for r < k through LDS, zeros in the rows below k.
template <typename T>
__global__ __launch_bounds__(256) void svd_gather_kernel(int k, int q, int urows, const T *__restrict__ W, int ldw,
                                                         const T *__restrict__ Z, int ldz, const double *__restrict__ sigma,
                                                         const int *__restrict__ perm, double *__restrict__ s,
                                                         T *__restrict__ Vt, int ldvt, T *__restrict__ U, int ldu) {
    __shared__ T tile_s[32][33];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < k) {
        const int i = blockIdx.x, src = perm[i];
        const double sg = sigma[src];
        if (tid == 0) s[i] = sg;
        if (!Vt) return;
        const T *w = W + (size_t)src * ldw;
        for (int c = tid; c < q; c += 256) Vt[(size_t)i * ldvt + c] = sg == 0.0 ? T(0) : (T)((double)w[c] / sg);
        return;
    }
    const int tiles_c = (k + 31) / 32;
    const int tb = (int)blockIdx.x - k, r0 = tb / tiles_c * 32, i0 = tb % tiles_c * 32;
    const int lx = tid & 31, ly = tid >> 5;
    for (int y = ly; y < 32; y += 8) {     // tile_s[ii][rr] = Z[perm[i0 + ii]][r0 + rr]
        const int ii = i0 + y, rr = r0 + lx;
        tile_s[y][lx] = (ii < k && rr < k) ? Z[(size_t)perm[ii] * ldz + rr] : T(0);
    }
    __syncthreads();
    for (int y = ly; y < 32; y += 8) {
        const int rr = r0 + y, ii = i0 + lx;
        if (rr < urows && ii < k) U[(size_t)rr * ldu + ii] = tile_s[lx][y];
    }
}
template <typename T>
int launch_svd_gather(lsx_handle_t h, int k, int q, int urows, const T *W, int ldw, const T *Z, int ldz, const double *sigma,
                      const int *perm, double *s, T *Vt, int ldvt, T *U, int ldu) {
    if (k <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER, (double)k * q, sizeof(T) * (2.0 * k * q + 2.0 * (double)urows * k));
    const int tiles = U ? ((urows + 31) / 32) * ((k + 31) / 32) : 0;
    hipLaunchKernelGGL(svd_gather_kernel<T>, dim3(k + tiles), dim3(256), 0, h->stream, k, q, urows, W, ldw, Z, ldz, sigma, perm, s,
                       Vt, ldvt, U, ldu);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// gelss: row i of Y (k x nc) times 1 / sigma_i (fp64, rounded once) for i < rank, exact zeros below
template <typename T>
__global__ __launch_bounds__(256) void svd_scale_rows_kernel(int nc, int rank, const double *__restrict__ s, T *__restrict__ Y, int ldy) {
    const int c = (int)blockIdx.y * 256 + (int)threadIdx.x, i = blockIdx.x;
    if (c >= nc) return;
    T *y = Y + (size_t)i * ldy + c;
    *y = i < rank ? (T)((double)*y * (1.0 / s[i])) : T(0);
}
template <typename T>
int launch_svd_scale_rows(lsx_handle_t h, int k, int nc, int rank, const double *s, T *Y, int ldy) {
    if (k <= 0 || nc <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER, (double)k * nc, 2.0 * sizeof(T) * (double)k * nc);
    hipLaunchKernelGGL(svd_scale_rows_kernel<T>, dim3(k, (nc + 255) / 256), dim3(256), 0, h->stream, nc, rank, s, Y, ldy);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// D (rows x cols) = value everywhere: the NaN outcome of s and X, the zero X of a zero matrix
template <typename T>
__global__ __launch_bounds__(256) void svd_fill_kernel(int cols, T value, T *__restrict__ D, int ldd) {
    const int c = (int)blockIdx.y * 256 + (int)threadIdx.x;
    if (c < cols) D[(size_t)blockIdx.x * ldd + c] = value;
}
template <typename T>
int launch_svd_fill(lsx_handle_t h, int rows, int cols, T value, T *D, int ldd) {
    if (rows <= 0 || cols <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER, 0, sizeof(T) * (double)rows * cols);
    hipLaunchKernelGGL(svd_fill_kernel<T>, dim3(rows, (cols + 255) / 256), dim3(256), 0, h->stream, cols, value, D, ldd);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

#define LSX_SVD_PIECES(T)                                                                                        \
    template int launch_svd_round<T>(lsx_handle_t, int, int, int, T *, int, T *, int, double, int *);            \
    template int launch_svd_init<T>(lsx_handle_t, int, int, const T *, int, int, T *, int);                      \
    template int launch_svd_rownorm<T>(lsx_handle_t, int, int, const T *, int, double *);                        \
    template int launch_svd_gather<T>(lsx_handle_t, int, int, int, const T *, int, const T *, int, const double *, \
                                      const int *, double *, T *, int, T *, int);                                \
    template int launch_svd_scale_rows<T>(lsx_handle_t, int, int, int, const double *, T *, int);                \
    template int launch_svd_fill<T>(lsx_handle_t, int, int, T, T *, int);
LSX_SVD_PIECES(double)
LSX_SVD_PIECES(float)
#undef LSX_SVD_PIECES

}  // namespace lsx
