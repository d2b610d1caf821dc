// The Sutton-Chen shape functions, shared by the list kernel (csrc/eam.hip, K24) and the list-free frame-energy kernel
// (csrc/eam_frames.hip, K37): the per-thread constants, the integer power, one pair seen from its centre and S_k, S_k'.  No
// fused multiply-adds are formed by the compiler in a file that includes this one (the pragma below reaches the rest of the
// translation unit): the float and the Dual instantiation round the value parts alike, and K37 rounds a pair as K24 does.
// Every function is internal to the translation unit that includes this file.
#pragma once
#pragma clang fp contract(off)
#include "dual.hpp"

namespace {

struct EamK {                                  // per-thread constants
    float eps, a, c, rc, fn, fm;
    float qn, qm;                              // (a/rc)^k of the shifted form, 0 as published
    float ln, lm;                              // k (a/rc)^k / rc, 0 as published
    int n, m;
};

template <class T> __device__ __forceinline__ T eam_pow(T x, int n) {
    T r = mk<T>(1.f, 0.f);
    while (n > 0) { if (n & 1) r = r * x; x = x * x; n >>= 1; }
    return r;
}

// (eps, a, c) = the live parameters; rc, n, m, shifted: the fixed constants of MdgEAMConsts
__device__ __forceinline__ EamK eam_constants(float eps, float a, float c, float rc, int n, int m, int shifted) {
    EamK K;
    K.eps = eps; K.a = a; K.c = c;
    K.rc = rc; K.n = n; K.m = m; K.fn = (float)n; K.fm = (float)m;
    K.qn = K.qm = K.ln = K.lm = 0.f;
    if (shifted) {
        const float s = K.a / K.rc;
        K.qn = eam_pow<float>(s, K.n); K.qm = eam_pow<float>(s, K.m);
        K.ln = K.fn * K.qn / K.rc; K.lm = K.fm * K.qm / K.rc;
    }
    return K;
}

// one list entry seen from its centre: unit vector centre -> end, r, 1/r
template <class T> struct EamEdge { T ex, ey, ez, r, ir; };

// (dx, dy, dz) = end - centre with the stored image applied, (ax, ay, az) = w_end - w_centre.  False outside the support.
template <class T>
__device__ __forceinline__ bool eam_edge(const EamK& K, float dx, float dy, float dz, float ax, float ay, float az, EamEdge<T>& e) {
    const T x = mk<T>(dx, ax), y = mk<T>(dy, ay), z = mk<T>(dz, az);
    const T d2 = x * x + y * y + z * z;
    const float rv = sqrtf(val(d2));
    if (!(rv > 0.f && rv < K.rc)) return false;              // the support test, on the r that r - rc is formed from
    e.r = fsqrt_(d2);
    e.ir = mk<T>(1.f, 0.f) / e.r;
    e.ex = x * e.ir; e.ey = y * e.ir; e.ez = z * e.ir;
    return true;
}

// S_k(r) and S_k'(r) from s = a / r:  S = s^k - q + l (r - rc),  S' = l - k s^k / r   (q = l = 0 as published)
template <class T>
__device__ __forceinline__ void eam_shape(const EamEdge<T>& e, T s, int k, float fk, float q, float l, float rc, T& S, T& dS) {
    const T sk = eam_pow(s, k);
    S = (sk - q) + l * (e.r - rc);
    dS = l - fk * (sk * e.ir);
}

}  // namespace
