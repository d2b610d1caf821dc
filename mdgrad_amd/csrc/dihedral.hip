// Dihedral (torsion) terms over a static table of quadruples (i, j, k, l): the four-body level above csrc/bonded.hip.
//
//   vectors   b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k, each re-imaged with topology.get_offsets on the diagonal cell
//             (o = -[b >= L/2] + [b < -L/2] per component, NON-strict on the upper side; piecewise constant, no derivative)
//   normals   n1 = b1 x b2, n2 = b2 x b3
//   cos phi   n1.n2 / sqrt(|n1|^2 |n2|^2)          (torchmd/observable.py:181-197, compute_dihe, for the row (i, j, k, l))
//   phi       atan2(|b2| b1.n2, n1.n2) in (-pi, pi]  (IUPAC sign; the d_i of demo/fold.py:70 is -phi where it does not clamp)
//   energy    U = sum_{m = 0..4} A[type, m] cos^m phi   (the "multiharmonic" form of nff/nn/modules.py:253-257): polynomial in
//             cos phi, so there is no acos and no singularity at phi = 0 or pi
//
// Degenerate terms: a term with |n1|^2 <= eps^2 |b1|^2 |b2|^2 or |n2|^2 <= eps^2 |b2|^2 |b3|^2, eps = 2^-20 (three of its atoms
// collinear to below the f32 rounding of the normals; the threshold of csrc/adf.hip) is SKIPPED everywhere: no energy, force,
// H w, parameter gradient, histogram weight or gradient; its phi and cos phi come out 0 with zero gradient.
//
// (a) dihedral_kernel: energy per atom, dU/dx, H w and the per-term cos phi with its directional derivative in ONE launch.
//     Atom-centric like bonded_kernel: thread n walks the incidence list of atom n (entries 4 term + role, ascending: a fixed
//     summation order) and re-derives each term it takes part in -- no atomics.  dU/dx = U'(c) dc/dx with the closed form
//       p1 = n2 / nrm - c n1 / |n1|^2,  p2 = n1 / nrm - c n2 / |n2|^2,  nrm = sqrt(|n1|^2 |n2|^2)
//       dc/db1 = b2 x p1,  dc/db2 = p1 x b1 + b3 x p2,  dc/db3 = p2 x b2
//     and H w from the same expressions in dual numbers (csrc/dual.hpp) seeded along (w_j - w_i, w_k - w_j, w_l - w_k); the
//     dual part of c is then w.grad c of the term, from which the parameter gradients follow (dihedral_coeff_kernel):
//       dU/dA[s, m] = sum_{t of type s} c_t^m        d(w.dU/dx)/dA[s, m] = sum_t m c_t^(m-1) (w.grad c)_t
// (b) per-term phi and cos phi of many frames, and their gradient (atom-centric over the same incidence list, no atomics):
//     d phi/dx in the Blondel-Karplus closed form (J. Comput. Chem. 17, 1132 (1996)), which has no 1 / sin phi:
//       d phi/dx_i = -|b2| n1 / |n1|^2                       d phi/dx_l = |b2| n2 / |n2|^2
//       d phi/dx_j = -d phi/dx_i + s1 n1 + s2 n2             d phi/dx_k = -d phi/dx_l - s1 n1 - s2 n2
//       s1 = b1.b2 / (|n1|^2 |b2|),  s2 = b2.b3 / (|n2|^2 |b2|)
// (c) periodic soft histogram raw[b] = sum exp(-1/2 (wrap(phi - mu_b) / width)^2), mu_b = -pi + (b + 1/2) 2 pi / nbins, nearest
//     image only (width <= 0.5: the second image is below 3e-9 of a peak term), centres farther than 5.3 / s from phi dropped,
//     s = sqrt(log2 e / 2) / width (<= 2^-28 of a peak term each, the reach of csrc/adf.hip).  Forward: fixed-point integers
//     (fx64, common.hpp) into a per-workgroup LDS histogram, then one int64 word per bin -- integer sums do not depend on the
//     order, so two launches are bitwise equal.  Backward: elementwise d(sum_b g_b raw_b)/d phi.
#include <math.h>
#include "common.hpp"
#include "dual.hpp"

namespace {

constexpr int DH_BLOCK = 256;
constexpr int DH_MAX_BLOCKS = 2048;      // persistent histogram grid: one LDS histogram flush per workgroup
constexpr int DH_MAX_BINS = 4096;
constexpr float DH_EPS2 = 9.094947017729282e-13f;     // (2^-20)^2
constexpr float DH_REACH = 5.3f;
constexpr float DH_SKIPPED = MDG_DIHEDRAL_SKIPPED;      // c_term of a skipped term (no cosine is 2)
constexpr float DH_PI = 3.14159265358979323846f;

__device__ __forceinline__ float dh_image(float b, float L) { return b + ((b < -0.5f * L ? 1.f : 0.f) - (b >= 0.5f * L ? 1.f : 0.f)) * L; }

// (the two mixed operators the Horner form of U'(c) needs beyond csrc/dual.hpp)
__device__ __forceinline__ Dual operator+(float a, Dual b) { return {a + b.v, b.d}; }
__device__ __forceinline__ Dual operator*(Dual a, float b) { return {a.v * b, a.d * b}; }

// (dot3 / cross3 of three-vectors of either kind: csrc/dual.hpp)

// the three imaged bond vectors of term t of a frame at `pos`
__device__ __forceinline__ void bonds_of(const float* __restrict__ pos, const int32_t* __restrict__ q, const float* L, float (&b1)[3],
                                         float (&b2)[3], float (&b3)[3]) {
    const int i = q[0], j = q[1], k = q[2], l = q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float xj = pos[3 * j + a], xk = pos[3 * k + a];
        b1[a] = dh_image(xj - pos[3 * i + a], L[a]);
        b2[a] = dh_image(xk - xj, L[a]);
        b3[a] = dh_image(pos[3 * l + a] - xk, L[a]);
    }
}

__device__ __forceinline__ bool regular(float N1, float N2, float B1, float B2, float B3) {
    return N1 > DH_EPS2 * B1 * B2 && N2 > DH_EPS2 * B2 * B3;
}

// c = cos phi and dc/db1, dc/db2, dc/db3;  T = float (value) or Dual (value + directional derivative)
template <typename T>
__device__ __forceinline__ T cos_grad(const T (&b1)[3], const T (&b2)[3], const T (&b3)[3], T (&g1)[3], T (&g2)[3], T (&g3)[3]) {
    T n1[3], n2[3], p1[3], p2[3], t1[3], t2[3];
    cross3(b1, b2, n1);
    cross3(b2, b3, n2);
    const T N1 = dot3(n1, n1), N2 = dot3(n2, n2);
    const T nrm = fsqrt_(N1 * N2);
    const T c = dot3(n1, n2) / nrm;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p1[a] = n2[a] / nrm - c * (n1[a] / N1);
        p2[a] = n1[a] / nrm - c * (n2[a] / N2);
    }
    cross3(b2, p1, g1);
    cross3(p1, b1, t1);
    cross3(b3, p2, t2);
    cross3(p2, b2, g3);
#pragma unroll
    for (int a = 0; a < 3; ++a) g2[a] = t1[a] + t2[a];
    return c;
}

struct DihedralArgs {
    const float* pos;
    const float* w;
    const int32_t* top;
    const float* coeff;
    const int32_t* type;
    const int32_t* inc_ptr;
    const int32_t* inc;
    float* e_atom;
    float* grad;
    float* hw;
    float* c_term;
    float* cd_term;
    int n_atoms;
    float L[3], scale;
    int accumulate;
};

// role r of a term: dU/dx_r = s1 g1 + s2 g2 + s3 g3 with (x_i: -g1, x_j: g1 - g2, x_k: g2 - g3, x_l: g3)
template <bool HVP>
__global__ __launch_bounds__(DH_BLOCK) void dihedral_kernel(const DihedralArgs A) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= A.n_atoms) return;
    float gx = 0.f, gy = 0.f, gz = 0.f, hx = 0.f, hy = 0.f, hz = 0.f, e = 0.f;
    const int lo = A.inc_ptr[n], hi = A.inc_ptr[n + 1];
    for (int u = lo; u < hi; ++u) {
        const int code = A.inc[u], t = code >> 2, role = code & 3;
        const int32_t* q = A.top + 4 * t;
        float b1[3], b2[3], b3[3];
        bonds_of(A.pos, q, A.L, b1, b2, b3);
        float n1[3], n2[3];
        cross3(b1, b2, n1);
        cross3(b2, b3, n2);
        if (!regular(dot3(n1, n1), dot3(n2, n2), dot3(b1, b1), dot3(b2, b2), dot3(b3, b3))) {
            if (role == 0) {
                if (A.c_term) A.c_term[t] = DH_SKIPPED;
                if (A.cd_term) A.cd_term[t] = 0.f;
            }
            continue;
        }
        const float* a = A.coeff + 5 * (A.type ? A.type[t] : 0);
        const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4];
        const float s1 = role == 0 ? -1.f : (role == 1 ? 1.f : 0.f);
        const float s2 = role == 1 ? -1.f : (role == 2 ? 1.f : 0.f);
        const float s3 = role == 2 ? -1.f : (role == 3 ? 1.f : 0.f);
        float c;
        if (HVP) {
            const int i = q[0], j = q[1], k = q[2], l = q[3];
            Dual d1[3], d2[3], d3[3], g1[3], g2[3], g3[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const float wj = A.w[3 * j + x], wk = A.w[3 * k + x];
                d1[x] = {b1[x], wj - A.w[3 * i + x]};
                d2[x] = {b2[x], wk - wj};
                d3[x] = {b3[x], A.w[3 * l + x] - wk};
            }
            const Dual cd = cos_grad<Dual>(d1, d2, d3, g1, g2, g3);
            const Dual dU = a1 + cd * (2.f * a2 + cd * (3.f * a3 + cd * (4.f * a4)));      // U'(c)
            const Dual r0 = dU * (s1 * g1[0] + s2 * g2[0] + s3 * g3[0]);
            const Dual r1 = dU * (s1 * g1[1] + s2 * g2[1] + s3 * g3[1]);
            const Dual r2 = dU * (s1 * g1[2] + s2 * g2[2] + s3 * g3[2]);
            gx += r0.v; gy += r1.v; gz += r2.v;
            hx += r0.d; hy += r1.d; hz += r2.d;
            c = cd.v;
            if (role == 0 && A.cd_term) A.cd_term[t] = cd.d;
        } else {
            float g1[3], g2[3], g3[3];
            c = cos_grad<float>(b1, b2, b3, g1, g2, g3);
            const float dU = a1 + c * (2.f * a2 + c * (3.f * a3 + c * (4.f * a4)));
            gx += dU * (s1 * g1[0] + s2 * g2[0] + s3 * g3[0]);
            gy += dU * (s1 * g1[1] + s2 * g2[1] + s3 * g3[1]);
            gz += dU * (s1 * g1[2] + s2 * g2[2] + s3 * g3[2]);
            if (role == 0 && A.cd_term) A.cd_term[t] = 0.f;
        }
        if (role == 0) {
            e += a0 + c * (a1 + c * (a2 + c * (a3 + c * a4)));
            if (A.c_term) A.c_term[t] = c;
        }
    }
    if (A.e_atom) A.e_atom[n] = e;
    if (A.grad) {
        float* o = A.grad + 3 * n;
        const float s = A.scale;
        if (A.accumulate) { o[0] = fmaf(s, gx, o[0]); o[1] = fmaf(s, gy, o[1]); o[2] = fmaf(s, gz, o[2]); }
        else { o[0] = s * gx; o[1] = s * gy; o[2] = s * gz; }
    }
    if (HVP && A.hw) {
        float* o = A.hw + 3 * n;
        const float s = A.scale;
        if (A.accumulate) { o[0] = fmaf(s, hx, o[0]); o[1] = fmaf(s, hy, o[1]); o[2] = fmaf(s, hz, o[2]); }
        else { o[0] = s * hx; o[1] = s * hy; o[2] = s * hz; }
    }
}

// one workgroup per type: g_u[s, m] = sum_t c_t^m and g_w[s, m] = sum_t m c_t^(m-1) cd_t over the terms of type s, each thread
// over its strided share in ascending order, then the fixed tree of block_sum_n
__global__ __launch_bounds__(DH_BLOCK) void dihedral_coeff_kernel(const float* __restrict__ c_term, const float* __restrict__ cd_term,
                                                                  const int32_t* __restrict__ type, int n_terms,
                                                                  float* __restrict__ g_u, float* __restrict__ g_w) {
    __shared__ float red[(DH_BLOCK / 64) * 10];
    const int s = blockIdx.x;
    float v[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int t = threadIdx.x; t < n_terms; t += DH_BLOCK) {
        if ((type ? type[t] : 0) != s) continue;
        const float c = c_term[t];
        if (c == DH_SKIPPED) continue;
        const float c2 = c * c, c3 = c2 * c;
        v[0] += 1.f; v[1] += c; v[2] += c2; v[3] += c3; v[4] += c2 * c2;
        if (cd_term) {
            const float d = cd_term[t];
            v[6] += d; v[7] += 2.f * c * d; v[8] += 3.f * c2 * d; v[9] += 4.f * c3 * d;
        }
    }
    block_sum_n<10>(v, red);
    if (threadIdx.x < 5) {
        if (g_u) g_u[5 * s + threadIdx.x] = v[threadIdx.x];
        if (g_w) g_w[5 * s + threadIdx.x] = v[5 + threadIdx.x];
    }
}

// ------------------------------------------------------------------------------------------------ (b) phi of every frame
__global__ __launch_bounds__(DH_BLOCK) void dihedral_phi_fwd_kernel(const float* __restrict__ pos, long long n_frames, int n_atoms,
                                                                    const int32_t* __restrict__ top, int n_terms, float Lx, float Ly,
                                                                    float Lz, float* __restrict__ phi, float* __restrict__ cosphi) {
    const long long idx = (long long)blockIdx.x * DH_BLOCK + threadIdx.x;
    if (idx >= n_frames * n_terms) return;
    const long long f = idx / n_terms;
    const int t = (int)(idx - f * n_terms);
    const float L[3] = {Lx, Ly, Lz};
    float b1[3], b2[3], b3[3], n1[3], n2[3];
    bonds_of(pos + 3 * f * n_atoms, top + 4 * t, L, b1, b2, b3);
    cross3(b1, b2, n1);
    cross3(b2, b3, n2);
    const float N1 = dot3(n1, n1), N2 = dot3(n2, n2), B2 = dot3(b2, b2);
    float ph = 0.f, c = 0.f;
    if (regular(N1, N2, dot3(b1, b1), B2, dot3(b3, b3))) {
        const float d = dot3(n1, n2);
        ph = atan2f(sqrtf(B2) * dot3(b1, n2), d);
        c = d / sqrtf(N1 * N2);
    }
    if (phi) phi[idx] = ph;
    if (cosphi) cosphi[idx] = c;
}

__global__ __launch_bounds__(DH_BLOCK) void dihedral_phi_bwd_kernel(const float* __restrict__ pos, long long n_frames, int n_atoms,
                                                                    const int32_t* __restrict__ top, int n_terms,
                                                                    const int32_t* __restrict__ inc_ptr, const int32_t* __restrict__ inc,
                                                                    float Lx, float Ly, float Lz, const float* __restrict__ g_phi,
                                                                    const float* __restrict__ g_cos, float* __restrict__ g_xyz) {
    const long long idx = (long long)blockIdx.x * DH_BLOCK + threadIdx.x;
    if (idx >= n_frames * n_atoms) return;
    const long long f = idx / n_atoms;
    const int n = (int)(idx - f * n_atoms);
    const float* x = pos + 3 * f * n_atoms;
    const float L[3] = {Lx, Ly, Lz};
    float gx = 0.f, gy = 0.f, gz = 0.f;
    const int lo = inc_ptr[n], hi = inc_ptr[n + 1];
    for (int u = lo; u < hi; ++u) {
        const int code = inc[u], t = code >> 2, role = code & 3;
        const float Gp = g_phi ? g_phi[f * n_terms + t] : 0.f, Gc = g_cos ? g_cos[f * n_terms + t] : 0.f;
        if (Gp == 0.f && Gc == 0.f) continue;
        float b1[3], b2[3], b3[3], n1[3], n2[3];
        bonds_of(x, top + 4 * t, L, b1, b2, b3);
        cross3(b1, b2, n1);
        cross3(b2, b3, n2);
        const float N1 = dot3(n1, n1), N2 = dot3(n2, n2), B2 = dot3(b2, b2);
        if (!regular(N1, N2, dot3(b1, b1), B2, dot3(b3, b3))) continue;
        if (Gp != 0.f) {
            const float lb = sqrtf(B2);
            const float e1 = lb / N1, e2 = lb / N2;                        // d phi/dx_i = -e1 n1 ;  d phi/dx_l = e2 n2
            const float s1 = dot3(b1, b2) / (N1 * lb), s2 = dot3(b2, b3) / (N2 * lb);
            // coefficients of n1 and n2 in d phi/dx_role
            const float k1 = role == 0 ? -e1 : (role == 1 ? e1 + s1 : (role == 2 ? -s1 : 0.f));
            const float k2 = role == 3 ? e2 : (role == 2 ? -e2 - s2 : (role == 1 ? s2 : 0.f));
            gx += Gp * (k1 * n1[0] + k2 * n2[0]);
            gy += Gp * (k1 * n1[1] + k2 * n2[1]);
            gz += Gp * (k1 * n1[2] + k2 * n2[2]);
        }
        if (Gc != 0.f) {
            float g1[3], g2[3], g3[3];
            cos_grad<float>(b1, b2, b3, g1, g2, g3);
            const float s1 = role == 0 ? -1.f : (role == 1 ? 1.f : 0.f);
            const float s2 = role == 1 ? -1.f : (role == 2 ? 1.f : 0.f);
            const float s3 = role == 2 ? -1.f : (role == 3 ? 1.f : 0.f);
            gx += Gc * (s1 * g1[0] + s2 * g2[0] + s3 * g3[0]);
            gy += Gc * (s1 * g1[1] + s2 * g2[1] + s3 * g3[1]);
            gz += Gc * (s1 * g1[2] + s2 * g2[2] + s3 * g3[2]);
        }
    }
    g_xyz[3 * idx] = gx;
    g_xyz[3 * idx + 1] = gy;
    g_xyz[3 * idx + 2] = gz;
}

// ------------------------------------------------------------------------------------------------ (c) histogram
struct HistArgs {
    const float* phi;
    const float* cosphi;     // nullable: with it, phi == 0 and cosphi == 0 marks a skipped term
    long long n;
    int nbins;
    float s2;                // exp(-1/2 (d / width)^2) = exp2(-s2 d^2)
    float h, inv_h, reach_b; // spacing 2 pi / nbins, its inverse, the reach in bins
};

// the centres within the reach of ph: unwrapped indices lo .. hi (b = index mod nbins) and t, the position of ph on the
// centre grid (d = (t - index) h is the nearest-image distance: the reach is below pi); false: none or skipped
__device__ __forceinline__ bool hist_window(const HistArgs& A, long long i, float ph, float& t, int& lo, int& hi) {
    if (A.cosphi && ph == 0.f && A.cosphi[i] == 0.f) return false;
    t = (ph + DH_PI) * A.inv_h - 0.5f;
    lo = (int)ceilf(t - A.reach_b);
    hi = (int)floorf(t + A.reach_b);
    if (hi - lo + 1 > A.nbins) hi = lo + A.nbins - 1;            // (rounding of the reach at its limit: never twice round)
    return hi >= lo;
}

__device__ __forceinline__ int wrap_bin(int idx, int nbins) {
    idx %= nbins;
    return idx < 0 ? idx + nbins : idx;
}

__global__ __launch_bounds__(DH_BLOCK) void dihedral_hist_fwd_kernel(HistArgs A, float scale, unsigned long long* __restrict__ words) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long hist[];      // nbins words, then the flag word
    for (int b = threadIdx.x; b <= A.nbins; b += DH_BLOCK) hist[b] = 0ull;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * DH_BLOCK + threadIdx.x; i < A.n; i += (long long)gridDim.x * DH_BLOCK) {
        const float ph = A.phi[i];
        if (!(fabsf(ph) <= 4.f)) { hist[A.nbins] = 1ull; continue; }          // non-finite (or not an angle): flagged
        float t;
        int lo, hi;
        if (!hist_window(A, i, ph, t, lo, hi)) continue;
        for (int idx = lo; idx <= hi; ++idx) {
            const float d = (t - (float)idx) * A.h;
            atomicAdd(&hist[wrap_bin(idx, A.nbins)], fx64(scale * exp2f(-A.s2 * d * d)));
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b <= A.nbins; b += DH_BLOCK)
        if (hist[b]) atomicAdd(&words[b], hist[b]);
}

__global__ void dihedral_hist_finish_kernel(const unsigned long long* __restrict__ words, int nbins, double inv_scale,
                                            float* __restrict__ raw) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbins) return;
    raw[b] = words[nbins] ? __int_as_float(0x7fc00000) : (float)((double)(long long)words[b] * inv_scale);
}

// g_phi[i] = sum_b g_raw[b] d raw_b / d phi_i ,  d exp2(-s2 d^2) / d phi = -2 ln2 s2 d exp2(-s2 d^2)
__global__ __launch_bounds__(DH_BLOCK) void dihedral_hist_bwd_kernel(HistArgs A, const float* __restrict__ g_raw, float* __restrict__ g_phi) {
    extern __shared__ __attribute__((aligned(16))) float g_s[];
    for (int b = threadIdx.x; b < A.nbins; b += DH_BLOCK) g_s[b] = g_raw[b];
    __syncthreads();
    const long long i = (long long)blockIdx.x * DH_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    const float ph = A.phi[i];
    float acc = 0.f, t;
    int lo, hi;
    if (fabsf(ph) <= 4.f && hist_window(A, i, ph, t, lo, hi)) {
        for (int idx = lo; idx <= hi; ++idx) {
            const float d = (t - (float)idx) * A.h;
            acc = fmaf(g_s[wrap_bin(idx, A.nbins)] * d, exp2f(-A.s2 * d * d), acc);
        }
    }
    g_phi[i] = -2.f * 0.69314718055994531f * A.s2 * acc;
}

int hist_args(HistArgs& A, const float* phi, const float* cosphi, int64_t n, int nbins, float width) {
    MDG_CHECK_ARG(phi, "dihedral_hist: phi is null");
    MDG_CHECK_ARG(n >= 0, "dihedral_hist: n must not be negative, got %lld", (long long)n);
    MDG_CHECK_ARG(nbins >= 1 && nbins <= DH_MAX_BINS, "dihedral_hist: nbins must be in [1, %d], got %d", DH_MAX_BINS, nbins);
    MDG_CHECK_ARG(width > 0.f && width <= 0.5f, "dihedral_hist: width must be in (0, 0.5], got %g", (double)width);
    A.phi = phi; A.cosphi = cosphi; A.n = n; A.nbins = nbins;
    A.s2 = 0.5f * 1.4426950408889634f / (width * width);
    A.h = 2.f * DH_PI / (float)nbins;
    A.inv_h = (float)nbins / (2.f * DH_PI);
    A.reach_b = DH_REACH / sqrtf(A.s2) * A.inv_h;
    return MDG_OK;
}

int check_table(const char* who, const float* pos, int n_atoms, const float* cell_len, const int32_t* top, int n_terms) {
    MDG_CHECK_ARG(pos, "%s: pos is null", who);
    MDG_CHECK_ARG(cell_len, "%s: cell_len is null", who);
    MDG_CHECK_ARG(n_atoms > 0, "%s: n_atoms must be positive, got %d", who, n_atoms);
    MDG_CHECK_ARG(n_terms >= 0, "%s: n_terms must not be negative, got %d", who, n_terms);
    MDG_CHECK_ARG(n_terms == 0 || top, "%s: top is null", who);
    return MDG_OK;
}

}  // namespace

extern "C" int mdg_dihedral_eval(const float* pos, int n_atoms, const float* cell_len, const int32_t* top, int n_terms,
                                 const float* coeff, const int32_t* type, int n_types, const int32_t* inc_ptr, const int32_t* inc,
                                 const float* w, float* e_atom, float* grad, float* hw, float* c_term, float* cd_term,
                                 float out_scale, int accumulate, void* stream) {
    const int rc = check_table("dihedral_eval", pos, n_atoms, cell_len, top, n_terms);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(coeff, "dihedral_eval: coeff is null");
    MDG_CHECK_ARG(n_types >= 1, "dihedral_eval: n_types must be at least 1, got %d", n_types);
    MDG_CHECK_ARG(inc_ptr && (n_terms == 0 || inc), "dihedral_eval: the incidence list (inc_ptr, inc) is missing");
    MDG_CHECK_ARG(!hw || w, "dihedral_eval: the Hessian-vector product (hw) needs w");
    MDG_CHECK_ARG(e_atom || grad || hw || c_term || cd_term, "dihedral_eval: no output requested");
    DihedralArgs a{pos, w, top, coeff, type, inc_ptr, inc, e_atom, grad, hw, c_term, cd_term, n_atoms,
                   {cell_len[0], cell_len[1], cell_len[2]}, out_scale, accumulate};
    const dim3 grid((n_atoms + DH_BLOCK - 1) / DH_BLOCK), block(DH_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    if (w) hipLaunchKernelGGL((dihedral_kernel<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((dihedral_kernel<false>), grid, block, 0, st, a);
    MDG_CHECK_LAUNCH("dihedral_kernel");
    return MDG_OK;
}

extern "C" int mdg_dihedral_coeff_grad(const float* c_term, const float* cd_term, const int32_t* type, int n_terms, int n_types,
                                       float* g_u, float* g_w, void* stream) {
    MDG_CHECK_ARG(n_terms >= 0, "dihedral_coeff_grad: n_terms must not be negative, got %d", n_terms);
    MDG_CHECK_ARG(n_types >= 1, "dihedral_coeff_grad: n_types must be at least 1, got %d", n_types);
    MDG_CHECK_ARG(n_terms == 0 || c_term, "dihedral_coeff_grad: c_term is null");
    MDG_CHECK_ARG(g_u || g_w, "dihedral_coeff_grad: no output requested (g_u, g_w)");
    MDG_CHECK_ARG(!g_w || n_terms == 0 || cd_term, "dihedral_coeff_grad: g_w needs cd_term");
    hipLaunchKernelGGL(dihedral_coeff_kernel, dim3(n_types), dim3(DH_BLOCK), 0, (hipStream_t)stream, c_term, g_w ? cd_term : nullptr,
                       type, n_terms, g_u, g_w);
    MDG_CHECK_LAUNCH("dihedral_coeff_kernel");
    return MDG_OK;
}

extern "C" int mdg_dihedral_phi_fwd(const float* pos, int n_frames, int n_atoms, const float* cell_len, const int32_t* top,
                                    int n_terms, float* phi, float* cosphi, void* stream) {
    const int rc = check_table("dihedral_phi_fwd", pos, n_atoms, cell_len, top, n_terms);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(n_frames > 0, "dihedral_phi_fwd: n_frames must be positive, got %d", n_frames);
    MDG_CHECK_ARG(phi || cosphi, "dihedral_phi_fwd: no output requested (phi, cosphi)");
    const long long total = (long long)n_frames * n_terms;
    if (total == 0) return MDG_OK;
    MDG_CHECK_ARG((total + DH_BLOCK - 1) / DH_BLOCK < (1ll << 31), "dihedral_phi_fwd: too many terms in one call (chunk the frames)");
    hipLaunchKernelGGL(dihedral_phi_fwd_kernel, dim3((unsigned)((total + DH_BLOCK - 1) / DH_BLOCK)), dim3(DH_BLOCK), 0,
                       (hipStream_t)stream, pos, (long long)n_frames, n_atoms, top, n_terms, cell_len[0], cell_len[1], cell_len[2],
                       phi, cosphi);
    MDG_CHECK_LAUNCH("dihedral_phi_fwd_kernel");
    return MDG_OK;
}

extern "C" int mdg_dihedral_phi_bwd(const float* pos, int n_frames, int n_atoms, const float* cell_len, const int32_t* top,
                                    int n_terms, const int32_t* inc_ptr, const int32_t* inc, const float* g_phi, const float* g_cos,
                                    float* g_xyz, void* stream) {
    const int rc = check_table("dihedral_phi_bwd", pos, n_atoms, cell_len, top, n_terms);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(n_frames > 0, "dihedral_phi_bwd: n_frames must be positive, got %d", n_frames);
    MDG_CHECK_ARG(inc_ptr && (n_terms == 0 || inc), "dihedral_phi_bwd: the incidence list (inc_ptr, inc) is missing");
    MDG_CHECK_ARG(g_phi || g_cos, "dihedral_phi_bwd: no cotangent given (g_phi, g_cos)");
    MDG_CHECK_ARG(g_xyz, "dihedral_phi_bwd: g_xyz is null");
    const long long total = (long long)n_frames * n_atoms;
    MDG_CHECK_ARG((total + DH_BLOCK - 1) / DH_BLOCK < (1ll << 31), "dihedral_phi_bwd: too many atoms in one call (chunk the frames)");
    hipLaunchKernelGGL(dihedral_phi_bwd_kernel, dim3((unsigned)((total + DH_BLOCK - 1) / DH_BLOCK)), dim3(DH_BLOCK), 0,
                       (hipStream_t)stream, pos, (long long)n_frames, n_atoms, top, n_terms, inc_ptr, inc, cell_len[0], cell_len[1],
                       cell_len[2], g_phi, g_cos, g_xyz);
    MDG_CHECK_LAUNCH("dihedral_phi_bwd_kernel");
    return MDG_OK;
}

extern "C" int64_t mdg_dihedral_hist_scratch(int64_t n, int nbins) {
    (void)n;
    return (int64_t)nbins + 2;          // one int64 word per bin, then the flag word (and one spare: a 16-byte multiple)
}

extern "C" int mdg_dihedral_hist_fwd(const float* phi, const float* cosphi, int64_t n, int nbins, float width, float* raw,
                                     int64_t* scratch, void* stream) {
    HistArgs A;
    const int rc = hist_args(A, phi, cosphi, n, nbins, width);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(raw, "dihedral_hist_fwd: raw is null");
    MDG_CHECK_ARG(scratch, "dihedral_hist_fwd: scratch is null");
    hipStream_t st = (hipStream_t)stream;
    const float scale = fx64_limit((double)n);                    // every contribution is <= 1
    MDG_HIP(hipMemsetAsync(scratch, 0, sizeof(int64_t) * mdg_dihedral_hist_scratch(n, nbins), st));
    if (n > 0) {
        const long long blocks = (n + DH_BLOCK - 1) / DH_BLOCK;
        hipLaunchKernelGGL(dihedral_hist_fwd_kernel, dim3((unsigned)(blocks < DH_MAX_BLOCKS ? blocks : DH_MAX_BLOCKS)), dim3(DH_BLOCK),
                           (size_t)(nbins + 2) * sizeof(unsigned long long), st, A, scale, reinterpret_cast<unsigned long long*>(scratch));
        MDG_CHECK_LAUNCH("dihedral_hist_fwd_kernel");
    }
    hipLaunchKernelGGL(dihedral_hist_finish_kernel, dim3((nbins + 255) / 256), dim3(256), 0, st,
                       reinterpret_cast<const unsigned long long*>(scratch), nbins, 1.0 / (double)scale, raw);
    MDG_CHECK_LAUNCH("dihedral_hist_finish_kernel");
    return MDG_OK;
}

extern "C" int mdg_dihedral_hist_bwd(const float* phi, const float* cosphi, int64_t n, int nbins, float width, const float* g_raw,
                                     float* g_phi, void* stream) {
    HistArgs A;
    const int rc = hist_args(A, phi, cosphi, n, nbins, width);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(g_raw, "dihedral_hist_bwd: g_raw is null");
    MDG_CHECK_ARG(n == 0 || g_phi, "dihedral_hist_bwd: g_phi is null");
    if (n == 0) return MDG_OK;
    const long long blocks = (n + DH_BLOCK - 1) / DH_BLOCK;
    MDG_CHECK_ARG(blocks < (1ll << 31), "dihedral_hist_bwd: too many angles in one call");
    hipLaunchKernelGGL(dihedral_hist_bwd_kernel, dim3((unsigned)blocks), dim3(DH_BLOCK), (size_t)nbins * sizeof(float),
                       (hipStream_t)stream, A, g_raw, g_phi);
    MDG_CHECK_LAUNCH("dihedral_hist_bwd_kernel");
    return MDG_OK;
}
