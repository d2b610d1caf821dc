// The phase arithmetic of the wave-vector observables, shared by K16 (csrc/sk.hip, S(k)) and K18 (csrc/isf.hip, F(k,t)):
// positions to turns, the phase of an integer wave vector, sine / cosine of a phase in turns, the rho sweep over staged
// atoms, the gradient sweep over a staged chunk of vectors, and the look-ups in the vector table.  The derivation of the
// accuracy is in the header of csrc/sk.hip.
#pragma once
#include "common.hpp"

namespace {

struct SkArgs {
    const float* pos;        // [F, N, 3]
    const float* w;          // [N] or null (unit weights)
    const int32_t* kvec;     // [M, 3] integer wave vectors, sorted by bin
    const int32_t* seg;      // [B + 1] segment offsets of the bins in kvec
    const float* gS;         // backward: [F, B]
    float* S;                // forward:  [F, B]
    float* g_pos;            // backward: [F, N, 3]
    float* ws;               // tiled: rho partials [F, nb, M] float2, then coefficients [F, M] float2
    int F, N, M, B;
    float inv_norm;          // 1 / sum_i w_i^2
    float L[3];
};

// ---------------------------------------------------------------------------------- phases
// u = x / L - rint(x / L) in turns, as uh (multiple of 2^-12) + ul; ul takes the remainder of the division too, so uh + ul
// holds u to ~2^-37 and n_d u_d keeps its digits for |n_d| in the hundreds
__device__ __forceinline__ void turns(float x, float L, float& uh, float& ul) {
    const float q = rintf(x / L);
    const float r = fmaf(-q, L, x);
    const float u = r / L;
    uh = rintf(u * 4096.f) * (1.f / 4096.f);
    ul = (u - uh) + fmaf(-u, L, r) / L;
}

// atom = (uh.xyz, w), (ul.xyz, -)
__device__ __forceinline__ void load_atom(const SkArgs& A, const float* p, int i, float4& a, float4& b) {
    turns(p[3 * (size_t)i], A.L[0], a.x, b.x);
    turns(p[3 * (size_t)i + 1], A.L[1], a.y, b.y);
    turns(p[3 * (size_t)i + 2], A.L[2], a.z, b.z);
    a.w = A.w ? A.w[i] : 1.f;
    b.w = 0.f;
}

// n.u mod 1 in [-1/2, 1/2] (+ |n.ul|)
__device__ __forceinline__ float phase(float nx, float ny, float nz, const float4& a, const float4& b) {
    float t = fmaf(nz, a.z, fmaf(ny, a.y, nx * a.x));          // exact: multiples of 2^-12 below 2^11
    t -= rintf(t);
    return fmaf(nz, b.z, fmaf(ny, b.y, fmaf(nx, b.x, t)));
}

// sin and cos of 2 pi t, |t| <= 1/2 + 2^-6
__device__ __forceinline__ void sincos_turns(float t, float& s, float& c) {
    const float q = rintf(4.f * t);
    const float x = fmaf(q, -0.25f, t) * 6.283185307179586f;   // |x| <= pi / 4
    const float x2 = x * x;
    const float sp = fmaf(x * x2, fmaf(x2, fmaf(x2, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f), x);
    const float cp = fmaf(x2 * x2, fmaf(x2, fmaf(x2, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f),
                          fmaf(x2, -0.5f, 1.f));
    const int qi = (int)q;                                      // quarter turns: 0 (c, s)  1 (-s, c)  2 (-c, -s)  3 (s, -c)
    const bool swap = qi & 1;
    const unsigned ss = (unsigned)(qi & 2) << 30, cs = (unsigned)((qi + 1) & 2) << 30;
    s = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, swap ? cp : sp) ^ ss);
    c = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, swap ? sp : cp) ^ cs);
}

// rho(n) over the staged atoms [0, na): re += w cos, im += w sin, in index order
__device__ __forceinline__ void rho_sweep(const float4* sa, const float4* sb, int na, float nx, float ny, float nz, float& re,
                                          float& im) {
    re = 0.f; im = 0.f;
    for (int i = 0; i < na; ++i) {
        const float4 a = sa[i], b = sb[i];
        float s, c;
        sincos_turns(phase(nx, ny, nz, a, b), s, c);
        re = fmaf(a.w, c, re);
        im = fmaf(a.w, s, im);
    }
}

// bin of vector m: the last b with seg[b] <= m (empty bins repeat an offset and are skipped)
__device__ __forceinline__ int bin_of(const int32_t* seg, int B, int m) {
    int lo = 0, hi = B;                                          // seg[lo] <= m < seg[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid] <= m) lo = mid; else hi = mid;
    }
    return lo;
}

// the staged chunk of kc vectors (snv = n, sab = (coef Im rho, coef Re rho)) summed into atom (a, b): g += n (A cos - B sin)
__device__ __forceinline__ void grad_chunk(const float4* snv, const float2* sab, int kc, const float4& a, const float4& b,
                                           float (&g)[3]) {
    float lx = 0.f, ly = 0.f, lz = 0.f;
    for (int k = 0; k < kc; ++k) {
        const float4 n = snv[k];
        const float2 ab = sab[k];
        float s, c;
        sincos_turns(phase(n.x, n.y, n.z, a, b), s, c);
        const float v = fmaf(ab.x, c, -(ab.y * s));
        lx = fmaf(n.x, v, lx); ly = fmaf(n.y, v, ly); lz = fmaf(n.z, v, lz);
    }
    g[0] += lx; g[1] += ly; g[2] += lz;
}

__device__ __forceinline__ float4 load_n(const int32_t* kvec, int m) {
    return make_float4((float)kvec[3 * (size_t)m], (float)kvec[3 * (size_t)m + 1], (float)kvec[3 * (size_t)m + 2], 0.f);
}

}  // namespace
