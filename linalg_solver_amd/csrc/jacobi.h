// Device helpers shared by the two Jacobi iterations: the one-sided SVD (kernels_svd.hip) and the two-sided symmetric
// eigensolver (kernels_eig.hip).  16-byte accesses of the padded work arrays, the butterfly sum of a wave, the rotation
// and its application to a pair of 16-byte groups.
#pragma once
#include "common.h"

namespace lsx {

template <typename T>
struct Vec16;
template <>
struct Vec16<double> { typedef double2 type; };
template <>
struct Vec16<float> { typedef float4 type; };
template <typename T>
constexpr int vec_elems() { return 16 / (int)sizeof(T); }

template <typename T>
__device__ __forceinline__ void load16(const T *p, T (&v)[vec_elems<T>()]) {
    const typename Vec16<T>::type x = *reinterpret_cast<const typename Vec16<T>::type *>(p);
    const T *e = reinterpret_cast<const T *>(&x);
#pragma unroll
    for (int k = 0; k < vec_elems<T>(); ++k) v[k] = e[k];
}
template <typename T>
__device__ __forceinline__ void store16(T *p, const T (&v)[vec_elems<T>()]) {
    typename Vec16<T>::type x;
    T *e = reinterpret_cast<T *>(&x);
#pragma unroll
    for (int k = 0; k < vec_elems<T>(); ++k) e[k] = v[k];
    *reinterpret_cast<typename Vec16<T>::type *>(p) = x;
}

// the sum of v over the wave, in every lane: a butterfly (xor 32, 16, .. 1)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// cs, sn of the rotation that annihilates c between the diagonal entries (or squared norms) a and b; c != 0
__device__ __forceinline__ void jacobi_cs_sn(double a, double b, double c, double *cs, double *sn) {
    const double zeta = (b - a) / (2.0 * c);
    const double az = fabs(zeta);
    double t;
    if (az > 0x1p500) t = 1.0 / (2.0 * zeta);   // zeta^2 would overflow
    else {
        t = 1.0 / (az + sqrt(1.0 + zeta * zeta));
        if (zeta < 0.0) t = -t;
    }
    *cs = 1.0 / sqrt(1.0 + t * t);
    *sn = *cs * t;
}

template <typename T>
__device__ __forceinline__ void rotate16(T (&x)[vec_elems<T>()], T (&y)[vec_elems<T>()], double cs, double sn) {
#pragma unroll
    for (int k = 0; k < vec_elems<T>(); ++k) {
        const double xi = (double)x[k], yj = (double)y[k];
        x[k] = (T)(cs * xi - sn * yj);
        y[k] = (T)(sn * xi + cs * yj);
    }
}

// players of positions t and P - 1 - t in round r of the round-robin order over P (even) players, the smaller first:
// position 0 holds player 0, position s >= 1 player ((s - 1 - r) mod (P - 1)) + 1
__device__ __forceinline__ void round_robin_pair(int P, int r, int t, int *i, int *j) {
    const int s1 = P - 1 - t, m1 = P - 1;
    const int pa = t == 0 ? 0 : ((t - 1 - r) % m1 + m1) % m1 + 1;
    const int pb = ((s1 - 1 - r) % m1 + m1) % m1 + 1;
    *i = pa < pb ? pa : pb;
    *j = pa < pb ? pb : pa;
}

}  // namespace lsx
