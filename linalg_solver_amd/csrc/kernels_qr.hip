// Householder QR (row-major): the panel steps, the T factor of a block reflector, and the small kernels around them.
// Nothing here is cooperative: no kernel waits on another workgroup, every launch is ordered by the stream alone.
//
// Panel (mp rows, jb <= 128 columns, row-major: a panel row is one contiguous segment).  jb + 1 launches over row slabs.
// Launch j does, in one pass over its slab,
//   (a) reflector j - 1 applied to the slab's rows i >= j - 1, and
//   (b) on the data just updated, the slab's partial sums g_c = sum_{i > j} a_ij a_ic, c = j .. jb - 1, written to the
//       slab's own slot (fp64); the slab that holds row j also copies that row to a small buffer.
// Every workgroup of launch j + 1 then adds the slots in a fixed order and forms the scalars of reflector j from them
// and the copied row by itself -- redundant across workgroups, cheap, and no grid-wide reduction is needed.  The copied
// row (two buffers in turn) is what lets the owner of row j write its final values while the others still read it.
//   alpha = a_jj, g_j = xnorm^2.   g_j == 0: tau_j = 0 and nothing changes (dlarfg).   Otherwise
//   beta = -copysign(sqrt(alpha^2 + g_j), alpha),  tau = (beta - alpha) / beta,  s = 1 / (alpha - beta),
//   v_i = s a_ij,  w_c = a_jc + s g_c,  a_jc -= tau w_c,  a_ic -= tau v_i w_c,  a_jj = beta.
// Sums, their reduction and the scalars are fp64 for both precisions; v_i is rounded to the matrix's type (it is what
// the array stores and what every later product reads) and each updated element is rounded once.  dlarfg's rescaling
// loop is not reproduced: alpha^2 + g_j must be a finite normal number.  A NaN takes the general branch and propagates.
#include "common.h"

namespace lsx {

constexpr int QB = 128;    // panel width and the edge of V^T V and T
constexpr int QCH = 64;    // rows of a slab that are in registers at once: 2 halves of the workgroup x QRT rows
constexpr int QRT = 32;
constexpr int QSLABS = 256;   // most slabs of a panel: the slots every workgroup adds stay below 256 KiB

int qr_slab_rows(int mp) {
    const int per = (mp + QSLABS - 1) / QSLABS;
    const int rows = (per + QCH - 1) / QCH * QCH;
    return rows < QCH ? QCH : rows;
}
size_t qr_slot_elems() { return (size_t)2 * QSLABS * QB; }

template <typename T>
__global__ __launch_bounds__(256) void qr_panel_step_kernel(int mp, int jb, int j, int slab_rows, int nslab, T *__restrict__ P,
                                                            int ldp, T *__restrict__ tau, const double *__restrict__ slots_prev,
                                                            double *__restrict__ slots_cur, const T *__restrict__ prow_prev,
                                                            T *__restrict__ prow_cur) {
    __shared__ double g_s[QB], w_s[QB], part_s[2][QB];
    __shared__ T colv_s[QCH], colj_s[QCH];
    const int tid = threadIdx.x, c = tid & (QB - 1), half = tid >> 7;
    const int jp = j - 1;
    double tauv = 0.0, s = 0.0, beta = 0.0;
    bool act = false;   // uniform over the grid: every workgroup forms it from the same words in the same order
    if (j > 0) {
        double p = 0.0;
        if (c >= jp && c < jb)
            for (int sl = half; sl < nslab; sl += 2) p += slots_prev[(size_t)sl * QB + c];
        part_s[half][c] = p;
        __syncthreads();
        if (half == 0) g_s[c] = part_s[0][c] + part_s[1][c];
        __syncthreads();
        const double g = g_s[jp];
        const double alpha = (double)prow_prev[jp];
        if (g != 0.0) {
            act = true;
            beta = -copysign(sqrt(alpha * alpha + g), alpha);
            tauv = (beta - alpha) / beta;
            s = 1.0 / (alpha - beta);
        }
        if (half == 0 && c > jp && c < jb) w_s[c] = (double)prow_prev[c] + s * g_s[c];
        __syncthreads();
        if (blockIdx.x == 0 && tid == 0) tau[jp] = (T)tauv;
    }
    const double wc = (j > 0 && c > jp && c < jb) ? w_s[c] : 0.0;
    const int lo_row = jp > 0 ? jp : 0;                         // rows above it are final
    const bool live = c < jb && c >= lo_row;                    // columns this launch updates or sums
    const int r_lo = (int)blockIdx.x * slab_rows;
    const int r_hi = min(mp, r_lo + slab_rows);
    double acc = 0.0;
    for (int r0 = r_lo; r0 < r_hi; r0 += QCH) {
        if (r0 + QCH <= lo_row) continue;
        const int ib = r0 + half * QRT;
        T vals[QRT];
#pragma unroll
        for (int r = 0; r < QRT; ++r) {
            const int i = ib + r;
            vals[r] = (live && i < r_hi && i >= lo_row) ? P[(size_t)i * ldp + c] : T(0);
        }
        if (act) {
            if (c == jp) {
#pragma unroll
                for (int r = 0; r < QRT; ++r) colv_s[half * QRT + r] = vals[r];
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < QRT; ++r) {
                const int i = ib + r;
                if (!live || i >= r_hi || i < jp) continue;
                if (i > jp) {
                    const T v = (T)(s * (double)colv_s[half * QRT + r]);
                    vals[r] = (c == jp) ? v : (T)((double)vals[r] - (tauv * (double)v) * wc);
                } else {
                    vals[r] = (c == jp) ? (T)beta : (T)((double)vals[r] - tauv * wc);
                }
                P[(size_t)i * ldp + c] = vals[r];
            }
        }
        if (j < jb) {
            if (c == j) {
#pragma unroll
                for (int r = 0; r < QRT; ++r) colj_s[half * QRT + r] = vals[r];
            }
#pragma unroll
            for (int r = 0; r < QRT; ++r)
                if (ib + r == j && live && j < r_hi) prow_cur[c] = vals[r];
            __syncthreads();
#pragma unroll
            for (int r = 0; r < QRT; ++r) {
                const int i = ib + r;
                if (i > j && i < r_hi && c >= j && c < jb) acc += (double)colj_s[half * QRT + r] * (double)vals[r];
            }
        }
        __syncthreads();   // the next chunk overwrites the two columns
    }
    if (j < jb) {
        part_s[half][c] = acc;
        __syncthreads();
        if (half == 0) slots_cur[(size_t)blockIdx.x * QB + c] = part_s[0][c] + part_s[1][c];
    }
}

// slots: qr_slot_elems() doubles; prow: 2 * QB elements
template <typename T>
int launch_qr_panel(lsx_handle_t h, int mp, int jb, T *P, int ldp, T *tau, double *slots, T *prow) {
    if (mp <= 0 || jb <= 0) return LSX_OK;
    if (jb > QB || jb > mp) {
        set_error("qr panel: %d columns on %d rows not served", jb, mp);
        return LSX_ERR_INTERNAL;
    }
    const int slab_rows = qr_slab_rows(mp), nslab = (mp + slab_rows - 1) / slab_rows;
    for (int j = 0; j <= jb; ++j) {
        ProfScope ps(h, LSX_PROF_PANEL, 4.0 * (double)(mp - j) * (jb - j > 0 ? jb - j : 1), 2.0 * sizeof(T) * (double)mp * jb);
        double *cur = slots + (size_t)(j & 1) * QSLABS * QB, *prev = slots + (size_t)((j + 1) & 1) * QSLABS * QB;
        hipLaunchKernelGGL(qr_panel_step_kernel<T>, dim3(nslab), dim3(256), 0, h->stream, mp, jb, j, slab_rows, nslab, P, ldp,
                           tau, (const double *)prev, cur, (const T *)(prow + ((j + 1) & 1) * QB), prow + (j & 1) * QB);
    }
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// V (mp x 128, dense): the panel's unit lower trapezoid with explicit ones and zeros; columns >= jb are zero
template <typename T>
__global__ __launch_bounds__(256) void qr_extract_v_kernel(int mp, int jb, const T *__restrict__ P, int ldp, T *__restrict__ V) {
    const int c = threadIdx.x & (QB - 1);
    for (int r = threadIdx.x >> 7; r < QCH; r += 2) {
        const int i = (int)blockIdx.x * QCH + r;
        if (i >= mp) return;
        V[(size_t)i * QB + c] = (c < jb && i >= c) ? (i == c ? T(1) : P[(size_t)i * ldp + c]) : T(0);
    }
}
template <typename T>
int launch_qr_extract_v(lsx_handle_t h, int mp, int jb, const T *P, int ldp, T *V) {
    if (mp <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_TRSM, 0, sizeof(T) * (double)mp * (jb + QB));
    hipLaunchKernelGGL(qr_extract_v_kernel<T>, dim3((mp + QCH - 1) / QCH), dim3(256), 0, h->stream, mp, jb, P, ldp, V);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// dlarft, forward, columnwise, from G = V^T V (128 x 128, dense; only above its diagonal is used): one workgroup holds
// the jb x jb block in LDS and runs  T_ii = tau_i,  T(0:i, i) = -tau_i T(0:i, 0:i) G(0:i, i)  in place, column i of T
// taking the place of column i of G.  Row r is the work of two threads (the terms q = r, r + 2, .. and q = r + 1, ..),
// sums in fp64, one rounding per element.  tau_i = 0 gives a zero column.  Tm receives T and Tt its transpose, both
// 128 x 128 with zeros outside the triangle.
template <typename T>
__global__ __launch_bounds__(256) void qr_larft_kernel(int jb, const T *__restrict__ G, const T *__restrict__ tau,
                                                       T *__restrict__ Tm, T *__restrict__ Tt) {
    extern __shared__ __attribute__((aligned(16))) char qr_smem[];
    constexpr int LD = QB + 1;
    T *S = (T *)qr_smem;
    __shared__ double red_s[2][QB];
    const int tid = threadIdx.x, r = tid & (QB - 1), half = tid >> 7;
    for (int e = tid; e < jb * jb; e += 256) {
        const int i = e / jb, c = e % jb;
        S[i * LD + c] = G[(size_t)i * QB + c];
    }
    __syncthreads();
    for (int i = 0; i < jb; ++i) {
        const double ti = (double)tau[i];
        double p = 0.0;
        if (r < i)
            for (int q = r + half; q < i; q += 2) p += (double)S[r * LD + q] * (double)S[q * LD + i];
        red_s[half][r] = p;
        __syncthreads();
        if (half == 0) {
            if (r < i) S[r * LD + i] = ti == 0.0 ? T(0) : (T)(-ti * (red_s[0][r] + red_s[1][r]));
            else if (r == i) S[i * LD + i] = (T)ti;
        }
        __syncthreads();
    }
    for (int e = tid; e < QB * QB; e += 256) {
        const int i = e / QB, c = e % QB;
        const T v = (i < jb && c < jb && c >= i) ? S[i * LD + c] : T(0);
        Tm[(size_t)i * QB + c] = v;
        Tt[(size_t)c * QB + i] = v;
    }
}
template <typename T>
int launch_qr_larft(lsx_handle_t h, int jb, const T *G, const T *tau, T *Tm, T *Tt) {
    if (jb <= 0 || jb > QB) return LSX_OK;
    ProfScope ps(h, LSX_PROF_TRSM, (double)jb * jb * jb / 3.0);
    const size_t shm = (size_t)QB * (QB + 1) * sizeof(T);
    LSX_HIP(hipFuncSetAttribute((const void *)qr_larft_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    hipLaunchKernelGGL(qr_larft_kernel<T>, dim3(1), dim3(256), shm, h->stream, jb, G, tau, Tm, Tt);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// Q (m x n) <- the leading columns of the identity
template <typename T>
__global__ __launch_bounds__(256) void qr_identity_kernel(int n, T *__restrict__ Q, int ldq) {
    const int j = (int)blockIdx.y * 256 + (int)threadIdx.x;
    const int i = blockIdx.x;
    if (j < n) Q[(size_t)i * ldq + j] = (i == j) ? T(1) : T(0);
}
template <typename T>
int launch_qr_identity(lsx_handle_t h, int m, int n, T *Q, int ldq) {
    if (m <= 0 || n <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER, 0, sizeof(T) * (double)m * n);
    hipLaunchKernelGGL(qr_identity_kernel<T>, dim3(m, (n + 255) / 256), dim3(256), 0, h->stream, n, Q, ldq);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// out[c] = sqrt(sum_i a_ic^2): a workgroup takes 32 columns, eight threads a column (rows i = l, l + 8, .. ascending
// each), the eight sums added in order l = 0 .. 7; fp64 throughout, no atomics, no scaling of the squares.
template <typename T>
__global__ __launch_bounds__(256) void colnrm2_kernel(int m, int n, const T *__restrict__ A, int lda, double *__restrict__ out) {
    __shared__ double p_s[8][32];
    const int cl = threadIdx.x & 31, l = threadIdx.x >> 5, c = (int)blockIdx.x * 32 + cl;
    double p = 0.0;
    if (c < n)
        for (int i = l; i < m; i += 8) {
            const double a = (double)A[(size_t)i * lda + c];
            p += a * a;
        }
    p_s[l][cl] = p;
    __syncthreads();
    if (l == 0 && c < n) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) s += p_s[q][cl];
        out[c] = sqrt(s);
    }
}
template <typename T>
int launch_colnrm2(lsx_handle_t h, int m, int n, const T *A, int lda, double *out) {
    if (n <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER, 2.0 * (double)m * n, sizeof(T) * (double)m * n);
    hipLaunchKernelGGL(colnrm2_kernel<T>, dim3((n + 31) / 32), dim3(256), 0, h->stream, m, n, A, lda, out);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

// out (rows x nc) = part 0 + part 1 + .. of a product whose depth was cut into `parts` pieces (api.hip, qr_vt_times):
// part p lies `stride` elements behind part p - 1 with leading dimension ldp; added in that order in fp64, one rounding
template <typename T>
__global__ __launch_bounds__(256) void qr_sum_parts_kernel(int rows, int nc, int parts, const T *__restrict__ P, int ldp,
                                                           size_t stride, T *__restrict__ out, int ldo) {
    const int c = (int)blockIdx.x * 256 + (int)threadIdx.x, i = blockIdx.y;
    if (c >= nc || i >= rows) return;
    double s = 0.0;
    for (int p = 0; p < parts; ++p) s += (double)P[(size_t)p * stride + (size_t)i * ldp + c];
    out[(size_t)i * ldo + c] = (T)s;
}
template <typename T>
int launch_qr_sum_parts(lsx_handle_t h, int rows, int nc, int parts, const T *P, int ldp, size_t stride, T *out, int ldo) {
    if (rows <= 0 || nc <= 0 || parts <= 0) return LSX_OK;
    ProfScope ps(h, LSX_PROF_OTHER, (double)parts * rows * nc, sizeof(T) * (double)(parts + 1) * rows * nc);
    hipLaunchKernelGGL(qr_sum_parts_kernel<T>, dim3((nc + 255) / 256, rows), dim3(256), 0, h->stream, rows, nc, parts, P, ldp,
                       stride, out, ldo);
    LSX_HIP(hipGetLastError());
    return LSX_OK;
}

#define LSX_QR_PIECES(T)                                                                         \
    template int launch_qr_panel<T>(lsx_handle_t, int, int, T *, int, T *, double *, T *);       \
    template int launch_qr_extract_v<T>(lsx_handle_t, int, int, const T *, int, T *);            \
    template int launch_qr_larft<T>(lsx_handle_t, int, const T *, const T *, T *, T *);          \
    template int launch_qr_identity<T>(lsx_handle_t, int, int, T *, int);                        \
    template int launch_qr_sum_parts<T>(lsx_handle_t, int, int, int, const T *, int, size_t, T *, int); \
    template int launch_colnrm2<T>(lsx_handle_t, int, int, const T *, int, double *);
LSX_QR_PIECES(double)
LSX_QR_PIECES(float)
#undef LSX_QR_PIECES

}  // namespace lsx
