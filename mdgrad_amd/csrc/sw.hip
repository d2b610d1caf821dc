// K23: Stillinger-Weber two- plus three-body potential for one species over the per-atom (ELL) list
// (mdgrad_amd/interface.py StillingerWeber; Stillinger and Weber 1985, Molinero and Moore 2009 for mW water).
//
//   rc = a sigma,  g(r) = exp(gamma sigma / (r - rc)) for r < rc, else exactly 0
//   phi2(r)       = A eps [B (sigma/r)^p - (sigma/r)^q] exp(sigma / (r - rc))
//   phi3(j, i, k) = lam eps (cos theta_jik - cos0)^2 g(r_ij) g(r_ik)                 (i = the centre)
//   U = sum_{i<j} phi2 + sum_i sum_{j<k in row(i)} phi3
//
// Laid out like coulomb_ell_kernel (csrc/coulomb.hip): LPA lanes walk one atom's row, wave shuffles combine the per-atom sums,
// the energy goes through a fixed-order block partial and a finish kernel.  No float atomics => bitwise reproducible.
//
// Atom-centric gather.  The lane that holds slot s of row(i) (neighbour j) adds
//   - the pair (i, j),
//   - the triplets centred on i with the ends j and k = every later slot of row(i)   (centre part of dU/dx_i),
//   - the triplets centred on j with the ends i and k = every entry of row(j) but i  (end part of dU/dx_i; x_k - x_j is taken
//     with j's own stored image).
// Rows are read from global memory where they are needed (they are short and stay in L1/L2): nothing is staged, so there is no
// row cap.  r - rc is formed from r = sqrtf(d2), the exponentials are expf; every pair with r >= rc is skipped, so a list
// searched with a larger radius (a skin, or a cutoff kept while sigma shrank) is exact.
//
// LEVEL 2 runs the same code on Dual numbers seeded with w: x + t w gives dU/dx + t H w in one pass, and the per-atom
// parameter terms d u_i / d(eps, sigma, lam) of u_i = 1/2 sum_j phi2 + the triplets centred on i carry
// d(w . grad)(d u_i / d theta) in their dual parts.
// No fused multiply-adds are formed by the compiler in this file: the float and the Dual instantiation then round the value
// parts identically, so dU/dx of a LEVEL 1 launch equals that of a LEVEL 2 launch bit for bit.
#pragma clang fp contract(off)
#include "sw_core.hpp"          // SwK, sw_pow, SwEdge, sw_edge: shared with csrc/sw_frames.hip (K34)
#include "manybody.hpp"

namespace {

constexpr int SW_LPA = 16;                    // lanes per atom (rows hold 4 - 20 neighbours)
constexpr int SW_BLOCK = 256;

struct SwArgs {
    const float* pos; int N; MdgCell cell;
    const int32_t* col; const int32_t* shift; const int32_t* cnt; int max_nbr;
    const float* theta;                        // device (eps, sigma, lam), or null: the three host values below
    const float* w;
    float eps, sigma, lam;
    float a, gamma, cos0, A, B; int p, q;
    float* grad; float* hw; float* pth; float* pthw; float* partial;
    float oscale; int oacc;
};

template <class T, int LEVEL>
__device__ __forceinline__ void sw_atom(const SwArgs& A, const SwK& K, int i, int sub, float (&out)[14]) {
    const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
    float wxi = 0.f, wyi = 0.f, wzi = 0.f;
    if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
    const T zero = mk<T>(0.f, 0.f);
    T gx = zero, gy = zero, gz = zero;                       // dU/dx_i
    T S2 = zero, S2s = zero, S3 = zero, S3s = zero;          // sum e2, sum d e2 / d sigma, sum t3, sum d t3 / d sigma
    const int n = min(A.cnt[i], A.max_nbr);
    const size_t row = (size_t)i * A.max_nbr;
    for (int s = sub; s < n; s += SW_LPA) {
        const int j = A.col[row + s];
        if ((unsigned)j >= (unsigned)A.N) continue;
        float dx = xi - A.pos[3 * j], dy = yi - A.pos[3 * j + 1], dz = zi - A.pos[3 * j + 2];
        apply_shift(A.cell, A.shift[row + s], dx, dy, dz);                  // x_i - x_j - o.h
        float wxj = 0.f, wyj = 0.f, wzj = 0.f;
        if (LEVEL >= 2) { wxj = A.w[3 * j]; wyj = A.w[3 * j + 1]; wzj = A.w[3 * j + 2]; }
        SwEdge<T> ej;                                                       // centre i -> end j
        if (!sw_edge<T>(K, -dx, -dy, -dz, wxj - wxi, wyj - wyi, wzj - wzi, ej)) continue;
        // ---- the pair (i, j): e2 = A [B s^p - s^q] E, E = exp(sigma / (r - rc)); phi2 = eps e2
        {
            const T sr = K.sigma * ej.ir;
            const T sp = sw_pow(sr, K.p), sq = sw_pow(sr, K.q);
            const T E = fexp_(K.sigma * ej.inv);
            const T bs = K.B * sp - sq;
            const T ps = (K.fp * K.B) * sp - K.fq * sq;
            const T e2 = K.A * (bs * E);
            const T inv2 = ej.inv * ej.inv;
            S2 = S2 + e2;
            if (LEVEL >= 1) {
                // d e2 / d sigma = A ps E / sigma + e2 r / (r - rc)^2;  phi2' = -eps A E [ps / r + bs sigma / (r - rc)^2]
                S2s = S2s + ((K.A / K.sigma) * (ps * E) + e2 * (ej.r * inv2));
                const T du = (K.eps * K.A) * (E * (ps * ej.ir + K.sigma * (bs * inv2)));      // = -phi2'
                gx = gx + du * ej.ex; gy = gy + du * ej.ey; gz = gz + du * ej.ez;             // d r / d x_i = -e
            }
        }
        // ---- triplets centred on i: the ends j and k = later slots of row(i)
        for (int t = s + 1; t < n; ++t) {
            const int k = A.col[row + t];
            if ((unsigned)k >= (unsigned)A.N) continue;
            float bx = xi - A.pos[3 * k], by = yi - A.pos[3 * k + 1], bz = zi - A.pos[3 * k + 2];
            apply_shift(A.cell, A.shift[row + t], bx, by, bz);
            float ax = 0.f, ay = 0.f, az = 0.f;
            if (LEVEL >= 2) { ax = A.w[3 * k] - wxi; ay = A.w[3 * k + 1] - wyi; az = A.w[3 * k + 2] - wzi; }
            SwEdge<T> ek;
            if (!sw_edge<T>(K, -bx, -by, -bz, ax, ay, az, ek)) continue;
            const T c = ej.ex * ek.ex + ej.ey * ek.ey + ej.ez * ek.ez;
            const T dc = c - K.cos0;
            const T gg = ej.g * ek.g;
            const T t3 = dc * dc * gg;
            S3 = S3 + t3;
            if (LEVEL >= 1) {
                const T q1 = ej.inv * ej.inv, q2 = ek.inv * ek.inv;
                S3s = S3s + K.gamma * (t3 * (ej.r * q1 + ek.r * q2));
                // G1 = d phi3 / d x_j = pre [t1 e_k + (s1 - t1 c) e_j],  t1 = 2 / r_ij,  s1 = -gamma sigma dc / (r_ij - rc)^2
                const T pre = K.le * (gg * dc);
                const T t1 = 2.f * ej.ir, t2 = 2.f * ek.ir;
                const T m1 = t1 * c + K.gs * (dc * q1), m2 = t2 * c + K.gs * (dc * q2);      // -(s - t c)
                // d phi3 / d x_i = -(G1 + G2)
                const T cj = pre * (m1 - t2), ck = pre * (m2 - t1);
                gx = gx + (cj * ej.ex + ck * ek.ex); gy = gy + (cj * ej.ey + ck * ek.ey); gz = gz + (cj * ej.ez + ck * ek.ez);
            }
        }
        if (LEVEL >= 1) {
            // ---- triplets centred on j: the ends i and k = every entry of row(j) but i
            const int nj = min(A.cnt[j], A.max_nbr);
            const size_t rowj = (size_t)j * A.max_nbr;
            const float xj = A.pos[3 * j], yj = A.pos[3 * j + 1], zj = A.pos[3 * j + 2];
            const T q1 = ej.inv * ej.inv;
            const T t1 = 2.f * ej.ir;
            for (int t = 0; t < nj; ++t) {
                const int k = A.col[rowj + t];
                if (k == i || (unsigned)k >= (unsigned)A.N) continue;
                float bx = xj - A.pos[3 * k], by = yj - A.pos[3 * k + 1], bz = zj - A.pos[3 * k + 2];
                apply_shift(A.cell, A.shift[rowj + t], bx, by, bz);          // x_j - x_k - o.h
                float ax = 0.f, ay = 0.f, az = 0.f;
                if (LEVEL >= 2) { ax = A.w[3 * k] - wxj; ay = A.w[3 * k + 1] - wyj; az = A.w[3 * k + 2] - wzj; }
                SwEdge<T> ek;                                                // centre j -> end k
                if (!sw_edge<T>(K, -bx, -by, -bz, ax, ay, az, ek)) continue;
                // the unit vector j -> i is -ej.e
                const T c = zero - (ej.ex * ek.ex + ej.ey * ek.ey + ej.ez * ek.ez);
                const T dc = c - K.cos0;
                const T pre = K.le * ((ej.g * ek.g) * dc);
                const T m1 = t1 * c + K.gs * (dc * q1);
                // G1 = pre [t1 e_jk - m1 e_ji] = pre [t1 e_jk + m1 ej.e]
                const T ca = pre * t1, cb = pre * m1;
                gx = gx + (ca * ek.ex + cb * ej.ex); gy = gy + (ca * ek.ey + cb * ej.ey); gz = gz + (ca * ek.ez + cb * ej.ez);
            }
        }
    }
    // u_i = eps (S2 / 2 + lam S3) and its parameter derivatives
    const T pe = 0.5f * S2 + K.lam * S3;
    out[0] = K.eps * val(pe);
    if (LEVEL >= 1) {
        const T psg = K.eps * (0.5f * S2s + K.lam * S3s);
        const T pl = K.eps * S3;
        out[1] = val(gx); out[2] = val(gy); out[3] = val(gz);
        out[4] = val(pe); out[5] = val(psg); out[6] = val(pl);
        if (LEVEL >= 2) {
            out[7] = dual_part(gx); out[8] = dual_part(gy); out[9] = dual_part(gz);
            out[10] = dual_part(pe); out[11] = dual_part(psg); out[12] = dual_part(pl);
        }
    }
}

// LEVEL 0: U        1: + grad, pth        2: + hw, pthw
template <int LEVEL>
__global__ void __launch_bounds__(SW_BLOCK) sw_ell_kernel(const SwArgs A) {
    __shared__ float red[17];
    constexpr int apb = SW_BLOCK / SW_LPA;
    const int i = blockIdx.x * apb + threadIdx.x / SW_LPA, sub = threadIdx.x % SW_LPA;
    float e = 0.f;
    if (i < A.N) {
        SwK K;
        K.eps = A.theta ? A.theta[0] : A.eps;
        K.sigma = A.theta ? A.theta[1] : A.sigma;
        K.lam = A.theta ? A.theta[2] : A.lam;
        K.le = K.lam * K.eps; K.rc = A.a * K.sigma; K.gs = A.gamma * K.sigma; K.gamma = A.gamma; K.cos0 = A.cos0;
        K.A = A.A; K.B = A.B; K.p = A.p; K.q = A.q; K.fp = (float)A.p; K.fq = (float)A.q;
        float o[14];
#pragma unroll
        for (int k = 0; k < 14; ++k) o[k] = 0.f;
        if (LEVEL >= 2) sw_atom<Dual, LEVEL>(A, K, i, sub, o);
        else sw_atom<float, LEVEL>(A, K, i, sub, o);
        constexpr int NV = LEVEL >= 2 ? 13 : (LEVEL >= 1 ? 7 : 1);
#pragma unroll
        for (int k = 0; k < NV; ++k) o[k] = group_sum<SW_LPA>(o[k]);
        if (sub == 0) {
            e = o[0];
            if (LEVEL >= 1) {
                if (A.grad) store3(A.grad, i, A.oscale, A.oacc, o[1], o[2], o[3]);
                if (A.pth) { A.pth[3 * i] = o[4]; A.pth[3 * i + 1] = o[5]; A.pth[3 * i + 2] = o[6]; }
            }
            if (LEVEL >= 2) {
                if (A.hw) store3(A.hw, i, A.oscale, A.oacc, o[7], o[8], o[9]);
                if (A.pthw) { A.pthw[3 * i] = o[10]; A.pthw[3 * i + 1] = o[11]; A.pthw[3 * i + 2] = o[12]; }
            }
        }
    }
    if (A.partial) {                         // (block-uniform: a force-only evaluation has no scalar to reduce)
        e = block_sum(e, red);
        if (threadIdx.x == 0) A.partial[blockIdx.x] = e;
    }
}

}  // namespace

extern "C" int64_t mdg_sw_partial_size(int n_atoms) { return atom_blocks(n_atoms, SW_LPA, SW_BLOCK); }

extern "C" int mdg_sw_eval(const float* pos, int n_atoms, const MdgCell* cell, const int32_t* col, const int32_t* shift,
                           const int32_t* cnt, int max_nbr, const MdgSWConsts* k, const float* theta, const float* w,
                           float* energy, float* grad, float* hw, float* pth, float* pthw, float* partial, float out_scale,
                           int accumulate, void* stream) {
    MDG_CHECK_ARG(pos && cell && col && shift && cnt, "sw_eval: null buffer (pos, cell or list)");
    MDG_CHECK_ARG(k, "sw_eval: consts is null");
    MDG_CHECK_ARG(n_atoms > 0 && max_nbr > 0, "sw_eval: bad sizes (n_atoms, max_nbr must be positive)");
    MDG_CHECK_ARG(theta || (k->epsilon > 0.0 && k->sigma > 0.0 && k->lam >= 0.0),
                  "sw_eval: consts need epsilon > 0, sigma > 0 and lam >= 0 (or a device theta)");
    MDG_CHECK_ARG(k->a > 0.0 && k->gamma >= 0.0, "sw_eval: consts need a > 0 and gamma >= 0");
    MDG_CHECK_ARG(k->q >= 0 && k->q < k->p && k->p <= 12, "sw_eval: exponents need 0 <= q < p <= 12");
    MDG_CHECK_ARG(w || !(hw || pthw), "sw_eval: hw / pthw need w");
    MDG_CHECK_ARG(!w || hw || pthw, "sw_eval: w given without hw or pthw output");
    MDG_CHECK_ARG(energy || grad || hw || pth || pthw, "sw_eval: no output requested");
    MDG_CHECK_ARG(!energy || partial, "sw_eval: energy needs the partial buffer");
    const int level = w ? 2 : ((grad || pth) ? 1 : 0);
    // (accumulate bit 2, "the list was searched with a skin", needs nothing here: the support test r < a sigma is always applied)
    SwArgs a{pos, n_atoms, *cell, col, shift, cnt, max_nbr, theta, w,
             (float)k->epsilon, (float)k->sigma, (float)k->lam, (float)k->a, (float)k->gamma, (float)k->cos0, (float)k->A,
             (float)k->B, (int)k->p, (int)k->q, grad, hw, pth, pthw, energy ? partial : nullptr, out_scale, accumulate & 1};
    const int nblocks = (int)mdg_sw_partial_size(n_atoms);
    dim3 grid(nblocks);
    hipStream_t st = (hipStream_t)stream;
    with_level(level, [&](auto L) { hipLaunchKernelGGL((sw_ell_kernel<decltype(L)::value>), grid, dim3(SW_BLOCK), 0, st, a); });
    if (energy) hipLaunchKernelGGL(energy_finish, dim3(1), dim3(64), 0, st, partial, nblocks, energy);
    MDG_CHECK_LAUNCH("sw_ell_kernel");
    return MDG_OK;
}
