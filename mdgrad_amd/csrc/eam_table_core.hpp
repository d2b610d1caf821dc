// The table side of the tabulated embedded-atom term, shared by the list kernel (csrc/eam_table.hip, K27) and the list-free
// frame-energy kernels (csrc/eam_frames.hip, K36): the layout of the flat node image (pair, density, embed), the bracketing
// cell and cubic-Hermite weights of an argument, the fixed-order dot product with the four node entries, and the power-of-two
// scale of the fixed-point node scatter.  No fused multiply-adds are formed by the compiler in a file that includes this one
// (the pragma below reaches the rest of the translation unit): the float and the Dual instantiation round the value parts
// alike, and K36 rounds a lookup as K27 does.  Every function is internal to the translation unit that includes this file.
#pragma once
#pragma clang fp contract(off)
#include "dual.hpp"

namespace {

constexpr int ET_BOUNDS = 8;                  // int64 words in front of the fixed-point words; their first uint32 hold the bounds

// ---- the flat image: pair [S (S + 1) / 2, n_r, 2] | density [S, n_r, 2] | embed [S, n_rho, 2], offsets in floats (= words)
__host__ __device__ __forceinline__ int et_npair(int S) { return S * (S + 1) / 2; }
__device__ __forceinline__ int et_pair(int a, int b) { const int lo = min(a, b), hi = max(a, b); return hi * (hi + 1) / 2 + lo; }
__host__ __device__ __forceinline__ size_t et_pair_off(int p, int nr) { return 2 * (size_t)p * nr; }
__host__ __device__ __forceinline__ size_t et_dens_off(int S, int b, int nr) { return 2 * (size_t)(et_npair(S) + b) * nr; }
__host__ __device__ __forceinline__ size_t et_embed_off(int S, int a, int nr, int nrho) {
    return 2 * ((size_t)(et_npair(S) + S) * nr + (size_t)a * nrho);
}

// the bracketing cell of x on the grid x0 + g / inv_h, g = 0 .. n - 1, and the weights of its four node entries
// (v_g, d_g, v_{g+1}, d_{g+1}) in the value (b) and in the derivative with respect to t = (x - x_g) inv_h (d)
template <class T> struct EtBasis { int g; T b[4]; T d[4]; };

template <class T>
__device__ __forceinline__ void et_basis(T x, float x0, float inv_h, int n, EtBasis<T>& B) {
    const T one = mk<T>(1.f, 0.f), zero = mk<T>(0.f, 0.f);
    const T u = inv_h * (x - x0);
    const float uv = val(u);
    if (uv < 0.f) {                                          // below the grid: v_0 + t d_0
        B.g = 0;
        B.b[0] = one; B.b[1] = u; B.b[2] = zero; B.b[3] = zero;
        B.d[0] = zero; B.d[1] = one; B.d[2] = zero; B.d[3] = zero;
        return;
    }
    B.g = (int)fminf(uv, (float)(n - 2));                    // (a NaN lands in the last cell: no index leaves the table)
    const T t = u - (float)B.g;
    if (val(t) > 1.f) {                                      // above the grid: v_{n-1} + (t - 1) d_{n-1}
        B.b[0] = zero; B.b[1] = zero; B.b[2] = one; B.b[3] = t - 1.f;
        B.d[0] = zero; B.d[1] = zero; B.d[2] = zero; B.d[3] = one;
        return;
    }
    const T s = 1.f - t, ss = s * s, tt = t * t, ts = t * s;
    B.b[0] = (2.f * t + 1.f) * ss;
    B.b[1] = t * ss;
    B.b[2] = tt * (3.f - 2.f * t);
    B.b[3] = zero - tt * s;
    B.d[0] = -6.f * ts;
    B.d[1] = s * (1.f - 3.f * t);
    B.d[2] = 6.f * ts;
    B.d[3] = t * (3.f * t - 2.f);
}

// sum_k c_k node_k over the four entries at `nd`, in a fixed order
template <class T>
__device__ __forceinline__ T et_dot(const T (&c)[4], const float* __restrict__ nd) {
    return ((nd[0] * c[0] + nd[1] * c[1]) + nd[2] * c[2]) + nd[3] * c[3];
}

// the largest value of a wave, on every lane (the bounds of the fixed-point scales)
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// the power of two that takes a contribution of at most `bound` to at most lim / 2 (1 when there is nothing to scale)
__device__ __forceinline__ float et_pow2(float bound, float lim) {
    if (!(bound > 0.f) || !(bound <= 3.0e38f)) return 1.f;
    const int k = ilogbf(lim) - ilogbf(bound) - 2;
    return ldexpf(1.f, min(max(k, -120), 120));
}

}  // namespace
