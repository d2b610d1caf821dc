// K22: the erf correction of the Ewald sum for excluded and scaled pairs (mdgrad_amd/interface.py EwaldExclusions; the
// reference has no Ewald sum, the definition is this project's).  The reciprocal sum (K21) runs over all charges and cannot
// leave a pair out; for every pair p = (i, j) of a static list with a scale s_p in [0, 1] this term adds
//
//   E1 = erf(alpha r), G = g0 exp(-alpha^2 r^2), g0 = 2 alpha / sqrt(pi):
//   chi(r) = (s - E1)/r,   chi'(r) = -(s - E1)/r^2 - G/r,   chi''(r) = 2 (s - E1)/r^3 + 2 G/r^2 + 2 alpha^2 G
//   U = conversion * sum_{p, every replica} q_i q_j chi_{s_p}(r_ij)
//
// r_ij = |d|, d = x_lo - x_hi (lo = min(i, j)) re-imaged like a bond vector: topology.get_offsets on the diagonal cell, non-strict
// on the +L/2 side, piecewise constant (no derivative).  s = 0 removes the pair's erf(alpha r)/r from the reciprocal sum (the
// real-space mask has removed erfc/r already); s = 1 gives back psi of K20 with shift "none".
//
// The kernel works with three radial coefficients per pair, C0 = chi, C1 = chi'/r and C2 = chi'' (closed form, like K20):
//   dU/dx_i += qq C1 d,   (H w)_i += qq [ C2 (rhat.a) rhat + C1 (a - (rhat.a) rhat) ],   a = w_i - w_j,  rhat = d / r
//   pot_i += q_j C0,   potw_i += q_j C1 (d.a)
// each the sum of an s part (s/r, -s/r^3, 2s/r^3; dropped at r == 0 like the pair kernels' d2 != 0 test) and an erf part:
//   u = (alpha r)^2 < 1   the power series erf(x)/x = (2/sqrt(pi)) sum_n (-1)^n u^n / (n! (2n+1)), n <= 13 (truncation 4e-10 of
//                         the slowest of the three sums at u = 1), and its derivatives term by term:
//                           erf part of C0 = -alpha F0(u),  of C1 = -alpha^3 F1(u),  of C2 = -alpha^3 F2(u)
//                           F0 = sum a_n u^n,  F1 = sum 2n a_n u^(n-1),  F2 = sum 2n(2n-1) a_n u^(n-1)
//                         all smooth in d: the closed forms (G r - E1)/r^2 ... cancel catastrophically in float32 below
//                         alpha r ~ 0.3 (3e-4 relative at 0.02).  A coincident pair takes this branch with rhat = 0 and gets
//                         the limits: energy -qq g0, zero gradient, (H w)_i = qq (4 alpha^3 / (3 sqrt(pi))) a, pot -q_j g0,
//                         potw 0.
//   u >= 1                erfcf / expf (the library functions, as in K20) with s - E1 = (s - 1) + erfc(alpha r): for s = 1 the
//                         difference 1 - erf would lose what erfc keeps.
//
// Atom-centric like bonded_kernel / dihedral_kernel: thread (replica, atom) walks the atom's row of a CSR incidence list
// (partner index and scale, ascending partner: a fixed summation order), built once on the host for one replica and shared
// by all replicas.  Every output word has one writer, the energy goes through per-block partial sums in double and a
// one-block finish: no atomics, two launches give the same bits.  An atom with an empty row leaves accumulated (`into`)
// buffers untouched.
#include "common.hpp"

namespace {

constexpr int XC_BLOCK = 256;
constexpr int XC_TERMS = 14;             // n = 0 .. 13 of the series

// topology.get_offsets (topology.py:75-80) on one component
__device__ __forceinline__ float xc_image(float b, float L) { return fmaf((b < -0.5f * L ? 1.f : 0.f) - (b >= 0.5f * L ? 1.f : 0.f), L, b); }

struct ExclArgs {
    const float* pos; const float* q; const float* w;
    const int32_t* row_ptr; const int32_t* col; const float* scl;
    float* grad; float* hw; float* pot; float* potw; double* partial;
    long long n_total; int n;
    float L[3];
    float alpha, alpha2, g0, conv;
    float f0[XC_TERMS], f1[XC_TERMS], f2[XC_TERMS];      // -alpha a_n; -alpha^3 2n a_n and -alpha^3 2n(2n-1) a_n, both at n - 1
    float oscale; int oacc;
};

// LEVEL 0: pot (energy)        1: + grad        2: + hw, potw
template <int LEVEL>
__global__ __launch_bounds__(XC_BLOCK) void ewald_excl_kernel(const ExclArgs A) {
    __shared__ double red[XC_BLOCK / 64];
    const long long t = (long long)blockIdx.x * XC_BLOCK + threadIdx.x;
    double e = 0.0;
    if (t < A.n_total) {
        const int ia = (int)(t % A.n);
        const size_t base = (size_t)(t - ia), i = (size_t)t;
        const int lo = A.row_ptr[ia], hi = A.row_ptr[ia + 1];
        const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
        const float qi = A.q[i], qc = A.conv * qi;
        float wxi = 0.f, wyi = 0.f, wzi = 0.f;
        if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
        float gx = 0.f, gy = 0.f, gz = 0.f, hx = 0.f, hy = 0.f, hz = 0.f, pt = 0.f, pw = 0.f;
        for (int k = lo; k < hi; ++k) {
            const int ja = A.col[k];
            const float s = A.scl[k];
            const size_t j = base + ja;
            // d = x_lo - x_hi re-imaged, then turned to x_i - x_j: both atoms of a pair see the same image
            const float sg = ja > ia ? 1.f : -1.f;
            const float dx = sg * xc_image(sg * (xi - A.pos[3 * j]), A.L[0]);
            const float dy = sg * xc_image(sg * (yi - A.pos[3 * j + 1]), A.L[1]);
            const float dz = sg * xc_image(sg * (zi - A.pos[3 * j + 2]), A.L[2]);
            const float d2 = dx * dx + dy * dy + dz * dz;
            const float u = A.alpha2 * d2;
            const float ir = d2 != 0.f ? __builtin_amdgcn_rsqf(d2) : 0.f;       // (r == 0: the s part is dropped)
            const float ir2 = ir * ir;
            float C0, C1 = 0.f, C2 = 0.f;
            if (u < 1.f) {
                float p0 = A.f0[XC_TERMS - 1];
#pragma unroll
                for (int n = XC_TERMS - 2; n >= 0; --n) p0 = fmaf(p0, u, A.f0[n]);
                const float sr = s * ir;
                C0 = sr + p0;
                if (LEVEL >= 1) {
                    float p1 = A.f1[XC_TERMS - 1];
#pragma unroll
                    for (int n = XC_TERMS - 2; n >= 1; --n) p1 = fmaf(p1, u, A.f1[n]);
                    const float sr3 = sr * ir2;
                    C1 = p1 - sr3;
                    if (LEVEL >= 2) {
                        float p2 = A.f2[XC_TERMS - 1];
#pragma unroll
                        for (int n = XC_TERMS - 2; n >= 1; --n) p2 = fmaf(p2, u, A.f2[n]);
                        C2 = fmaf(2.f, sr3, p2);
                    }
                }
            } else {
                const float sm = (s - 1.f) + erfcf(A.alpha * (d2 * ir));
                C0 = sm * ir;
                if (LEVEL >= 1) {
                    const float G = A.g0 * expf(-u);
                    const float tt = (C0 + G) * ir;                            // (s - E1)/r^2 + G/r = -chi'
                    C1 = -(tt * ir);
                    if (LEVEL >= 2) C2 = 2.f * fmaf(tt, ir, A.alpha2 * G);
                }
            }
            const float qj = A.q[j];
            pt = fmaf(qj, C0, pt);
            if (LEVEL >= 1) {
                const float c1 = qj * C1;
                gx = fmaf(c1, dx, gx); gy = fmaf(c1, dy, gy); gz = fmaf(c1, dz, gz);
                if (LEVEL >= 2) {
                    const float ax = wxi - A.w[3 * j], ay = wyi - A.w[3 * j + 1], az = wzi - A.w[3 * j + 2];
                    const float rx = dx * ir, ry = dy * ir, rz = dz * ir;           // (r == 0: rhat = 0, H w = C1 a)
                    const float ap = rx * ax + ry * ay + rz * az;
                    const float c2 = qj * C2 * ap;
                    hx += c2 * rx + c1 * (ax - ap * rx);
                    hy += c2 * ry + c1 * (ay - ap * ry);
                    hz += c2 * rz + c1 * (az - ap * rz);
                    pw = fmaf(c1, dx * ax + dy * ay + dz * az, pw);
                }
            }
        }
        e = 0.5 * (double)qc * (double)pt;
        const float os = A.oscale;
        const bool touch = !(A.oacc && lo == hi);        // an empty row adds nothing: the buffer keeps its bits
        if (LEVEL >= 1 && A.grad && touch) store3(A.grad + 3 * i, 0, os, A.oacc, qc * gx, qc * gy, qc * gz);
        if (A.pot) A.pot[i] = pt;
        if (LEVEL >= 2) {
            if (A.hw && touch) store3(A.hw + 3 * i, 0, os, A.oacc, qc * hx, qc * hy, qc * hz);
            if (A.potw) A.potw[i] = pw;
        }
    }
    if (A.partial) {                         // (block-uniform: a force-only evaluation has no scalar to reduce)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int k = 0; k < XC_BLOCK / 64; ++k) s += red[k];
            A.partial[blockIdx.x] = s;
        }
    }
}

// one workgroup: thread t sums the partials t, t + XC_BLOCK, ... in double, then a fixed tree
__global__ __launch_bounds__(XC_BLOCK) void ewald_excl_finish(const double* __restrict__ partial, long long nblocks, float* energy) {
    __shared__ double red[XC_BLOCK];
    const int t = threadIdx.x;
    double s = 0.0;
    for (long long b = t; b < nblocks; b += XC_BLOCK) s += partial[b];
    tree_sum<XC_BLOCK>(s, red);
    if (t == 0) energy[0] = (float)red[0];
}

}  // namespace

extern "C" int64_t mdg_ewald_excl_partial_size(int n_rep, int n_atoms) {
    if (n_rep <= 0 || n_atoms <= 0) return 0;
    return ((int64_t)n_rep * n_atoms + XC_BLOCK - 1) / XC_BLOCK;
}

extern "C" int mdg_ewald_excl_eval(const float* pos, int n_rep, int n_atoms, const float* cell_len, const int32_t* row_ptr,
                                   const int32_t* col, const float* scale, const float* q, double alpha, double conversion,
                                   const float* w, float* energy, float* grad, float* hw, float* pot, float* potw,
                                   double* partial, float out_scale, int accumulate, void* stream) {
    MDG_CHECK_ARG(pos && cell_len && q, "ewald_excl_eval: null argument (pos, cell_len or q)");
    MDG_CHECK_ARG(row_ptr && col && scale, "ewald_excl_eval: the incidence list is missing (row_ptr, col or scale)");
    MDG_CHECK_ARG(n_rep > 0 && n_atoms > 0, "ewald_excl_eval: n_rep and n_atoms must be positive");
    MDG_CHECK_ARG((long long)n_rep * n_atoms < (1LL << 31) / 4, "ewald_excl_eval: n_rep * n_atoms too large for one call");
    MDG_CHECK_ARG(cell_len[0] > 0.f && cell_len[1] > 0.f && cell_len[2] > 0.f, "ewald_excl_eval: the cell lengths must be positive");
    MDG_CHECK_ARG(alpha > 0.0, "ewald_excl_eval: the splitting parameter alpha must be positive");
    MDG_CHECK_ARG(w || !(hw || potw), "ewald_excl_eval: hw / potw need w");
    MDG_CHECK_ARG(!w || hw || potw, "ewald_excl_eval: w given without hw or potw output");
    MDG_CHECK_ARG(energy || grad || hw || pot || potw, "ewald_excl_eval: no output requested");
    MDG_CHECK_ARG(!energy || partial, "ewald_excl_eval: energy needs the partial buffer (mdg_ewald_excl_partial_size() doubles)");
    ExclArgs a{};
    a.pos = pos; a.q = q; a.w = w; a.row_ptr = row_ptr; a.col = col; a.scl = scale;
    a.grad = grad; a.hw = hw; a.pot = pot; a.potw = potw; a.partial = energy ? partial : nullptr;
    a.n_total = (long long)n_rep * n_atoms; a.n = n_atoms;
    for (int d = 0; d < 3; ++d) a.L[d] = cell_len[d];
    const double g0 = 2.0 * alpha / 1.7724538509055160273;
    a.alpha = (float)alpha; a.alpha2 = (float)(alpha * alpha); a.g0 = (float)g0; a.conv = (float)conversion;
    const double a3 = alpha * alpha * alpha;
    double fact = 1.0;
    for (int n = 0; n < XC_TERMS; ++n) {
        if (n > 0) fact *= n;
        const double an = (n % 2 ? -1.0 : 1.0) * (2.0 / 1.7724538509055160273) / (fact * (2 * n + 1));   // a_n of the series
        a.f0[n] = (float)(-alpha * an);
        a.f1[n] = (float)(-a3 * 2.0 * n * an);
        a.f2[n] = (float)(-a3 * 2.0 * n * (2 * n - 1) * an);
    }
    a.oscale = out_scale; a.oacc = accumulate & 1;
    const long long nblocks = (a.n_total + XC_BLOCK - 1) / XC_BLOCK;
    const dim3 grid((unsigned)nblocks), block(XC_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    const int level = w ? 2 : (grad ? 1 : 0);
    with_level(level, [&](auto L) { hipLaunchKernelGGL((ewald_excl_kernel<decltype(L)::value>), grid, block, 0, st, a); });
    MDG_CHECK_LAUNCH("ewald_excl_kernel");
    if (energy) {
        hipLaunchKernelGGL(ewald_excl_finish, dim3(1), block, 0, st, partial, nblocks, energy);
        MDG_CHECK_LAUNCH("ewald_excl_finish");
    }
    return MDG_OK;
}
