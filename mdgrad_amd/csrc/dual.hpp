// Dual numbers (value + one directional derivative) for forward-mode differentiation inside a kernel: the bonded terms
// (csrc/bonded.hip) and the torsion term (csrc/dihedral.hip) get their Hessian-vector products from them.  Every function is
// internal to the translation unit that includes this file.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct Dual {
    float v, d;
};
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return {a.v * b.v, fmaf(a.d, b.v, a.v * b.d)}; }
__device__ __forceinline__ Dual operator*(float a, Dual b) { return {a * b.v, a * b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, float b) { return {a.v - b, a.d}; }
__device__ __forceinline__ Dual operator-(float a, Dual b) { return {a - b.v, -b.d}; }
__device__ __forceinline__ Dual operator/(Dual a, Dual b) {
    const float q = a.v / b.v;
    return {q, (a.d - q * b.d) / b.v};
}
__device__ __forceinline__ Dual dsqrt(Dual a) {
    const float s = sqrtf(a.v);
    return {s, 0.5f * a.d / s};
}
__device__ __forceinline__ Dual dacos(Dual a) { return {acosf(a.v), -a.d / sqrtf(1.f - a.v * a.v)}; }
__device__ __forceinline__ Dual dexp(Dual a) {
    const float e = expf(a.v);
    return {e, e * a.d};
}

__device__ __forceinline__ float fsqrt_(float a) { return sqrtf(a); }
__device__ __forceinline__ Dual fsqrt_(Dual a) { return dsqrt(a); }
__device__ __forceinline__ float facos_(float a) { return acosf(a); }
__device__ __forceinline__ Dual facos_(Dual a) { return dacos(a); }
__device__ __forceinline__ float fexp_(float a) { return expf(a); }
__device__ __forceinline__ Dual fexp_(Dual a) { return dexp(a); }
__device__ __forceinline__ float val(float a) { return a; }
__device__ __forceinline__ float val(Dual a) { return a.v; }
// building and reading a number of either kind: mk<T>(v, d) = v (+ t d), dual_part(x) = d (0 for a float)
template <class T> __device__ __forceinline__ T mk(float v, float d);
template <> __device__ __forceinline__ float mk<float>(float v, float) { return v; }
template <> __device__ __forceinline__ Dual mk<Dual>(float v, float d) { return {v, d}; }
__device__ __forceinline__ float dual_part(float) { return 0.f; }
__device__ __forceinline__ float dual_part(Dual a) { return a.d; }

// ---- what the bond-order term (csrc/tersoff.hip) adds: a constant added to a Dual, log, sin, cos, and x^p for x > 0 and a
// real exponent p as exp(p log x), the same expression in float and in Dual so that the value parts round alike
__device__ __forceinline__ Dual operator+(Dual a, float b) { return {a.v + b, a.d}; }
__device__ __forceinline__ Dual dlog(Dual a) { return {logf(a.v), a.d / a.v}; }
__device__ __forceinline__ Dual dsin(Dual a) { return {sinf(a.v), cosf(a.v) * a.d}; }
__device__ __forceinline__ Dual dcos(Dual a) { return {cosf(a.v), -(sinf(a.v) * a.d)}; }
__device__ __forceinline__ float flog_(float a) { return logf(a); }
__device__ __forceinline__ Dual flog_(Dual a) { return dlog(a); }
__device__ __forceinline__ float fsin_(float a) { return sinf(a); }
__device__ __forceinline__ Dual fsin_(Dual a) { return dsin(a); }
__device__ __forceinline__ float fcos_(float a) { return cosf(a); }
__device__ __forceinline__ Dual fcos_(Dual a) { return dcos(a); }
__device__ __forceinline__ float fpow_(float x, float p) { return fexp_(p * flog_(x)); }
__device__ __forceinline__ Dual fpow_(Dual x, float p) { return fexp_(p * flog_(x)); }

// ---- what the angle term (csrc/bonded.hip) adds: atan2, and the dot / cross product of three-vectors of either kind (the torsion
// term, csrc/dihedral.hip, uses the same two).  d atan2(y, x) = (x dy - y dx) / (x^2 + y^2)
__device__ __forceinline__ Dual datan2(Dual y, Dual x) {
    return {atan2f(y.v, x.v), (x.v * y.d - y.v * x.d) / (x.v * x.v + y.v * y.v)};
}
__device__ __forceinline__ float fatan2_(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ Dual fatan2_(Dual y, Dual x) { return datan2(y, x); }
template <typename T>
__device__ __forceinline__ T dot3(const T (&a)[3], const T (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
template <typename T>
__device__ __forceinline__ void cross3(const T (&a)[3], const T (&b)[3], T (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

}  // namespace
