// K24: Sutton-Chen (Finnis-Sinclair) embedded-atom potential for one species over the per-atom (ELL) list
// (mdgrad_amd/interface.py SuttonChen; Sutton and Chen 1990).
//
//   U      = sum_i [ 1/2 sum_{j in row(i)} phi(r_ij) - eps c sqrt(rho_i) ],   rho_i = sum_{j in row(i)} f(r_ij)
//   phi(r) = eps S_n(r),  f(r) = S_m(r)
//   S_k(r) = (a/r)^k - (a/rc)^k + k (r - rc) (a/rc)^k / rc   for r < rc, else exactly 0        (shifted)
//   S_k(r) = (a/r)^k                                         for r < rc, else exactly 0        (as published)
//
// The force on atom i needs the embedding derivative F'(rho_j) = -eps c / (2 sqrt(rho_j)) of every neighbour j, and rho_j is a
// sum over row(j): two passes.
//   1. density pass:  rho_i (and, at LEVEL 2, d rho_i = sum_j f'(r_ij) e_ij . (w_j - w_i)) -> atom_work[i] =
//                     (rho_i, d rho_i, F'(rho_i), F''(rho_i) d rho_i).  rho_i <= 0 (an empty row): F' = F'' = 0 by definition.
//   2. force pass:    dU/dx_i = -sum_j [phi'(r_ij) + (F'_i + F'_j) f'(r_ij)] e_ij   (e_ij = the unit vector i -> j), an
//                     atom-centric gather with one writer per output word; u_i and its parameter terms; the energy through a
//                     fixed-order block partial and a finish kernel.
// Both are laid out like sw_kernel (csrc/sw_core.hpp): LPA lanes walk one atom's row, wave shuffles combine the per-atom sums.  No
// float atomics => bitwise reproducible.  Rows are read from global memory, nothing is staged, so there is no row cap.  The
// support test is applied on r = sqrtf(d2) against rc; a list searched with a larger radius (a skin) is exact.
//
// S_k is homogeneous of degree k in (a, r, rc) jointly, and r, rc do not depend on a: a dS_k/da = k S_k with or without the
// shift, so d u_i/da = (n/2 sum_j phi + m rho_i F'(rho_i)) / a needs no further sum.
//
// LEVEL 2 runs the same code on Dual numbers seeded with w: x + t w gives dU/dx + t H w, and the per-atom parameter terms carry
// d(w . grad)(d u_i / d theta) in their dual parts.  No fused multiply-adds are formed by the compiler in this file: the float
// and the Dual instantiation round the value parts identically, so dU/dx of a LEVEL 1 launch equals that of a LEVEL 2 launch bit
// for bit.  The per-thread constants, the integer power, the edge and S_k / S_k' live in csrc/eam_core.hpp, shared with the
// list-free frame energy (csrc/eam_frames.hip, K37).
#include "eam_core.hpp"
#include "manybody.hpp"

namespace {

constexpr int EAM_LPA = 16;                   // lanes per atom: one DPP row (metal rows hold 54 - 134 neighbours: 4 - 9 trips)
constexpr int EAM_BLOCK = 256;

struct EamArgs {
    const float* pos; int N; MdgCell cell;
    const int32_t* col; const int32_t* shift; const int32_t* cnt; int max_nbr;
    const float* theta;                        // device (eps, a, c), or null: the three host values below
    const float* w;
    float eps, a, c;
    float rc; int n, m, shifted;
    float* work;                               // atom_work [N, 4]
    float* grad; float* hw; float* pth; float* pthw; float* partial;
    float oscale; int oacc;
};

// the per-thread constants (csrc/eam_core.hpp) from the device theta, or from the host values when there is none
__device__ __forceinline__ EamK eam_constants(const EamArgs& A) {
    return eam_constants(A.theta ? A.theta[0] : A.eps, A.theta ? A.theta[1] : A.a, A.theta ? A.theta[2] : A.c, A.rc, A.n, A.m,
                         A.shifted);
}

// the entry in slot s of row(i) as an edge i -> j; returns j, or -1 when there is nothing to add
template <class T, int LEVEL>
__device__ __forceinline__ int eam_entry(const EamArgs& A, const EamK& K, size_t row, int s, float xi, float yi, float zi,
                                         float wxi, float wyi, float wzi, EamEdge<T>& e) {
    const int j = A.col[row + s];
    if ((unsigned)j >= (unsigned)A.N) return -1;
    float dx = xi - A.pos[3 * j], dy = yi - A.pos[3 * j + 1], dz = zi - A.pos[3 * j + 2];
    apply_shift(A.cell, A.shift[row + s], dx, dy, dz);                      // x_i - x_j - o.h
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (LEVEL >= 2) { ax = A.w[3 * j] - wxi; ay = A.w[3 * j + 1] - wyi; az = A.w[3 * j + 2] - wzi; }
    return eam_edge<T>(K, -dx, -dy, -dz, ax, ay, az, e) ? j : -1;
}

// ---- pass 1: rho_i, F'(rho_i) and their dual parts.  LEVEL 2: with w
template <class T, int LEVEL>
__device__ __forceinline__ T eam_density(const EamArgs& A, const EamK& K, int i, int sub) {
    const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
    float wxi = 0.f, wyi = 0.f, wzi = 0.f;
    if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
    T rho = mk<T>(0.f, 0.f);
    const int n = min(A.cnt[i], A.max_nbr);
    const size_t row = (size_t)i * A.max_nbr;
    for (int s = sub; s < n; s += EAM_LPA) {
        EamEdge<T> e;
        if (eam_entry<T, LEVEL>(A, K, row, s, xi, yi, zi, wxi, wyi, wzi, e) < 0) continue;
        T S, dS;
        eam_shape<T>(e, K.a * e.ir, K.m, K.fm, K.qm, K.lm, K.rc, S, dS);
        rho = rho + S;
    }
    return rho;
}

template <int LEVEL>
__global__ void __launch_bounds__(EAM_BLOCK) eam_density_kernel(const EamArgs A) {
    using T = typename std::conditional<LEVEL >= 2, Dual, float>::type;
    constexpr int apb = EAM_BLOCK / EAM_LPA;
    const int i = blockIdx.x * apb + threadIdx.x / EAM_LPA, sub = threadIdx.x % EAM_LPA;
    if (i >= A.N) return;
    const EamK K = eam_constants(A);
    const T part = eam_density<T, LEVEL>(A, K, i, sub);
    const float rho = group_sum<EAM_LPA>(val(part));
    float drho = 0.f;
    if (LEVEL >= 2) drho = group_sum<EAM_LPA>(dual_part(part));
    if (sub != 0) return;
    T Fp = mk<T>(0.f, 0.f);
    if (rho > 0.f) Fp = mk<T>(-0.5f * (K.eps * K.c), 0.f) / fsqrt_(mk<T>(rho, drho));   // dual part: F''(rho) d rho
    float* o = A.work + 4 * (size_t)i;
    o[0] = rho > 0.f ? rho : 0.f; o[1] = rho > 0.f ? drho : 0.f; o[2] = val(Fp); o[3] = dual_part(Fp);
}

// ---- pass 2
template <class T, int LEVEL>
__device__ __forceinline__ void eam_atom(const EamArgs& A, const EamK& K, int i, int sub, T FpI, T& SP, T& gx, T& gy, T& gz) {
    const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
    float wxi = 0.f, wyi = 0.f, wzi = 0.f;
    if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
    const int n = min(A.cnt[i], A.max_nbr);
    const size_t row = (size_t)i * A.max_nbr;
    for (int s = sub; s < n; s += EAM_LPA) {
        EamEdge<T> e;
        const int j = eam_entry<T, LEVEL>(A, K, row, s, xi, yi, zi, wxi, wyi, wzi, e);
        if (j < 0) continue;
        const T sr = K.a * e.ir;
        T Sn, dSn;
        eam_shape<T>(e, sr, K.n, K.fn, K.qn, K.ln, K.rc, Sn, dSn);
        SP = SP + Sn;
        if (LEVEL >= 1) {
            T Sm, dSm;
            eam_shape<T>(e, sr, K.m, K.fm, K.qm, K.lm, K.rc, Sm, dSm);
            const float* wj = A.work + 4 * (size_t)j;
            const T FpJ = mk<T>(wj[2], wj[3]);
            const T du = K.eps * dSn + (FpI + FpJ) * dSm;                   // dU/dr_ij;  d r / d x_i = -e
            gx = gx - du * e.ex; gy = gy - du * e.ey; gz = gz - du * e.ez;
        }
    }
}

// LEVEL 0: U        1: + grad, pth        2: + hw, pthw
template <int LEVEL>
__global__ void __launch_bounds__(EAM_BLOCK) eam_force_kernel(const EamArgs A) {
    using T = typename std::conditional<LEVEL >= 2, Dual, float>::type;
    __shared__ float red[17];
    constexpr int apb = EAM_BLOCK / EAM_LPA;
    const int i = blockIdx.x * apb + threadIdx.x / EAM_LPA, sub = threadIdx.x % EAM_LPA;
    float en = 0.f;
    if (i < A.N) {
        const EamK K = eam_constants(A);
        const float* wi = A.work + 4 * (size_t)i;
        const T zero = mk<T>(0.f, 0.f);
        const T R = mk<T>(wi[0], wi[1]), FpI = mk<T>(wi[2], wi[3]);
        T SP = zero, gx = zero, gy = zero, gz = zero;
        eam_atom<T, LEVEL>(A, K, i, sub, FpI, SP, gx, gy, gz);
        float o[8];
        o[0] = val(SP); o[1] = val(gx); o[2] = val(gy); o[3] = val(gz);
        o[4] = dual_part(SP); o[5] = dual_part(gx); o[6] = dual_part(gy); o[7] = dual_part(gz);
        o[0] = group_sum<EAM_LPA>(o[0]);
        if (LEVEL >= 1) {
#pragma unroll
            for (int k = 1; k < 4; ++k) o[k] = group_sum<EAM_LPA>(o[k]);
        }
        if (LEVEL >= 2) {
#pragma unroll
            for (int k = 4; k < 8; ++k) o[k] = group_sum<EAM_LPA>(o[k]);
        }
        if (sub == 0) {
            // u_i = eps (1/2 sum_j S_n - c sqrt(rho_i)) and its parameter derivatives
            const T S = mk<T>(o[0], o[4]);
            const T sq = val(R) > 0.f ? fsqrt_(R) : zero;
            const T pe = 0.5f * S - K.c * sq;
            en = K.eps * val(pe);
            if (LEVEL >= 1) {
                const T pa = (1.f / K.a) * ((0.5f * K.fn * K.eps) * S + K.fm * (R * FpI));
                const T pc = (-K.eps) * sq;
                if (A.grad) store3(A.grad, i, A.oscale, A.oacc, o[1], o[2], o[3]);
                if (A.pth) { A.pth[3 * i] = val(pe); A.pth[3 * i + 1] = val(pa); A.pth[3 * i + 2] = val(pc); }
                if (LEVEL >= 2) {
                    if (A.hw) store3(A.hw, i, A.oscale, A.oacc, o[5], o[6], o[7]);
                    if (A.pthw) { A.pthw[3 * i] = dual_part(pe); A.pthw[3 * i + 1] = dual_part(pa); A.pthw[3 * i + 2] = dual_part(pc); }
                }
            }
        }
    }
    if (A.partial) {                         // (block-uniform: a force-only evaluation has no scalar to reduce)
        en = block_sum(en, red);
        if (threadIdx.x == 0) A.partial[blockIdx.x] = en;
    }
}

}  // namespace

extern "C" int64_t mdg_eam_partial_size(int n_atoms) { return atom_blocks(n_atoms, EAM_LPA, EAM_BLOCK); }

extern "C" int mdg_eam_eval(const float* pos, int n_atoms, const MdgCell* cell, const int32_t* col, const int32_t* shift,
                            const int32_t* cnt, int max_nbr, const MdgEAMConsts* k, const float* theta, const float* w,
                            float* energy, float* grad, float* hw, float* pth, float* pthw, float* partial, float* atom_work,
                            float out_scale, int accumulate, void* stream) {
    MDG_CHECK_ARG(pos && cell && col && shift && cnt, "eam_eval: null buffer (pos, cell or list)");
    MDG_CHECK_ARG(k, "eam_eval: consts is null");
    MDG_CHECK_ARG(n_atoms > 0 && max_nbr > 0, "eam_eval: bad sizes (n_atoms, max_nbr must be positive)");
    MDG_CHECK_ARG(theta || (k->epsilon > 0.0 && k->a > 0.0 && k->c >= 0.0),
                  "eam_eval: consts need epsilon > 0, a > 0 and c >= 0 (or a device theta)");
    MDG_CHECK_ARG(k->rc > 0.0, "eam_eval: consts need rc > 0");
    MDG_CHECK_ARG(k->m >= 1 && k->m < k->n && k->n <= 16, "eam_eval: exponents need 1 <= m < n <= 16");
    MDG_CHECK_ARG(k->shift == 0 || k->shift == 1, "eam_eval: shift must be 0 (as published) or 1 (shifted force)");
    MDG_CHECK_ARG(w || !(hw || pthw), "eam_eval: hw / pthw need w");
    MDG_CHECK_ARG(!w || hw || pthw, "eam_eval: w given without hw or pthw output");
    MDG_CHECK_ARG(energy || grad || hw || pth || pthw, "eam_eval: no output requested");
    MDG_CHECK_ARG(!energy || partial, "eam_eval: energy needs the partial buffer");
    MDG_CHECK_ARG(atom_work, "eam_eval: atom_work is null (the scratch of the density pass, 4 floats per atom)");
    const int level = w ? 2 : ((grad || pth) ? 1 : 0);
    // (accumulate bit 2, "the list was searched with a skin", needs nothing here: the support test r < rc is always applied)
    EamArgs a{pos, n_atoms, *cell, col, shift, cnt, max_nbr, theta, w,
              (float)k->epsilon, (float)k->a, (float)k->c, (float)k->rc, (int)k->n, (int)k->m, (int)k->shift, atom_work,
              grad, hw, pth, pthw, energy ? partial : nullptr, out_scale, accumulate & 1};
    const int nblocks = (int)mdg_eam_partial_size(n_atoms);
    dim3 grid(nblocks);
    hipStream_t st = (hipStream_t)stream;
    with_level(level, [&](auto L) {
        constexpr int LV = decltype(L)::value;
        hipLaunchKernelGGL((eam_density_kernel<(LV >= 2 ? 2 : 1)>), grid, dim3(EAM_BLOCK), 0, st, a);    // (0 and 1: the float pass)
        hipLaunchKernelGGL((eam_force_kernel<LV>), grid, dim3(EAM_BLOCK), 0, st, a);
    });
    if (energy) hipLaunchKernelGGL(energy_finish, dim3(1), dim3(64), 0, st, partial, nblocks, energy);
    MDG_CHECK_LAUNCH("eam_force_kernel");
    return MDG_OK;
}
