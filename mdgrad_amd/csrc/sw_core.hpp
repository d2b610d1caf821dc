// The per-edge formulas of the one-species Stillinger-Weber term, shared by the list kernel (csrc/sw.hip, K23) and the
// list-free frame-energy kernel (csrc/sw_frames.hip, K34): the per-thread constants, the integer power and one entry of an
// atom's row seen from its centre.  No fused multiply-adds are formed by the compiler in a file that includes this one (the
// pragma below reaches the rest of the translation unit): the float and the Dual instantiation round the value parts alike,
// and K34 rounds an edge as K23 does.  Every function is internal to the translation unit that includes this file.
#pragma once
#pragma clang fp contract(off)
#include "dual.hpp"

namespace {

struct SwK {                                   // per-thread constants
    float eps, sigma, lam, le, rc, gs, gamma, cos0, A, B, fp, fq; int p, q;
};

// (eps, sigma, lam) = the live parameters; the rest are the fixed constants of MdgSWConsts
__device__ __forceinline__ SwK sw_constants(float eps, float sigma, float lam, float a, float gamma, float cos0, float A, float B,
                                            int p, int q) {
    SwK K;
    K.eps = eps; K.sigma = sigma; K.lam = lam;
    K.le = K.lam * K.eps; K.rc = a * K.sigma; K.gs = gamma * K.sigma; K.gamma = gamma; K.cos0 = cos0;
    K.A = A; K.B = B; K.p = p; K.q = q; K.fp = (float)p; K.fq = (float)q;
    return K;
}

template <class T> __device__ __forceinline__ T sw_pow(T x, int n) {
    T r = mk<T>(1.f, 0.f);
    while (n > 0) { if (n & 1) r = r * x; x = x * x; n >>= 1; }
    return r;
}

// one list entry seen from its centre: unit vector centre -> end, r, 1/r, 1/(r - rc), g
template <class T> struct SwEdge { T ex, ey, ez, r, ir, inv, g; };

// (dx, dy, dz) = end - centre with the stored image applied, (ax, ay, az) = w_end - w_centre.  False outside the support.
template <class T>
__device__ __forceinline__ bool sw_edge(const SwK& K, float dx, float dy, float dz, float ax, float ay, float az, SwEdge<T>& e) {
    const T x = mk<T>(dx, ax), y = mk<T>(dy, ay), z = mk<T>(dz, az);
    const T one = mk<T>(1.f, 0.f);
    const T d2 = x * x + y * y + z * z;
    const float rv = sqrtf(val(d2));
    if (!(rv > 0.f && rv < K.rc)) return false;              // the support test, on the r that r - rc is formed from
    e.r = fsqrt_(d2);
    e.ir = one / e.r;
    e.ex = x * e.ir; e.ey = y * e.ir; e.ez = z * e.ir;
    e.inv = one / (e.r - K.rc);
    e.g = fexp_(K.gs * e.inv);
    return true;
}

// the pair part of one edge: e2 = A [B s^p - s^q] E with E = exp(sigma / (r - rc)) (phi2 = eps e2), and bs, ps, E for the
// derivatives (bs = B s^p - s^q, ps = p B s^p - q s^q)
template <class T> struct SwPair { T e2, bs, ps, E; };

template <class T>
__device__ __forceinline__ SwPair<T> sw_pair(const SwK& K, const SwEdge<T>& ej) {
    SwPair<T> o;
    const T sr = K.sigma * ej.ir;
    const T sp = sw_pow(sr, K.p), sq = sw_pow(sr, K.q);
    o.E = fexp_(K.sigma * ej.inv);
    o.bs = K.B * sp - sq;
    o.ps = (K.fp * K.B) * sp - K.fq * sq;
    o.e2 = K.A * (o.bs * o.E);
    return o;
}

// d e2 / d sigma = A ps E / sigma + e2 r / (r - rc)^2
template <class T>
__device__ __forceinline__ T sw_pair_dsigma(const SwK& K, const SwEdge<T>& ej, const SwPair<T>& o) {
    return (K.A / K.sigma) * (o.ps * o.E) + o.e2 * (ej.r * (ej.inv * ej.inv));
}

}  // namespace
