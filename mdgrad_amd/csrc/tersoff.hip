// K25: Tersoff bond-order potential for one species over the per-atom (ELL) list
// (mdgrad_amd/interface.py Tersoff; Tersoff 1988 for silicon, 1989 for carbon; the LAMMPS convention).
//
// The formulas, the two passes and both kernel templates are those of csrc/tersoff_core.hpp; read its header first.  What is
// particular to this file is where the constants come from: there is one pair entry and one centre entry, derived per thread
// from the kernel arguments and held in registers (uniform, so in scalar registers), with (A, B, h) read from the `theta`
// device buffer when it is given.  No `types` array, no table in LDS and no barrier beyond the block reduction of the energy.
// This view has the exponential exp[(lam3 (r_ij - r_ik))^m] of zeta (HAS_LAM3); a row of pth / pthw is (A, B, h).
#pragma clang fp contract(off)
#include "tersoff_core.hpp"

namespace {

struct TersArgs {
    const float* theta;                        // device (A, B, h), or null: the three host values below
    float A, B, h;
    float lam1, lam2, beta, n, c, d, R, D, rc, rin, lam3, gamma; int m;            // rc = R + D, rin = R - D, rounded on the host
};

struct TersOneView {
    using Args = TersArgs;
    static constexpr bool HAS_LAM3 = true;
    static constexpr int SMAX = 1;
    static constexpr int S = 1;
    TersEntry pp, cc;
    float lam3; int m;

    __device__ __forceinline__ explicit TersOneView(const TersArgs& a) {
        const float A = a.theta ? a.theta[0] : a.A, B = a.theta ? a.theta[1] : a.B, h = a.theta ? a.theta[2] : a.h;
        const float cd = a.c / a.d, d2 = a.d * a.d, gcd = a.gamma * (cd * cd);
        pp.v[PA_A] = A; pp.v[PA_B] = B; pp.v[PA_L1] = a.lam1; pp.v[PA_L2] = a.lam2;
        pp.v[PA_R] = a.R; pp.v[PA_RIN] = a.rin; pp.v[PA_RC] = a.rc; pp.v[PA_PD] = 1.57079632679489662f / a.D;
        cc.v[CE_H] = h; cc.v[CE_BETA] = a.beta; cc.v[CE_N] = a.n; cc.v[CE_MH] = -0.5f / a.n;
        cc.v[CE_D2] = d2; cc.v[CE_GAMMA] = a.gamma; cc.v[CE_GCD] = gcd; cc.v[CE_GU2] = 2.f * (gcd * d2);
        lam3 = a.lam3; m = a.m;
    }
    __device__ __forceinline__ int species(int) const { return 0; }
    __device__ __forceinline__ const TersEntry& pair(int, int) const { return pp; }
    __device__ __forceinline__ const TersEntry& centre(int) const { return cc; }
    __device__ __forceinline__ void store_theta(float* dst, int i, int, const float (&va)[1], const float (&vb)[1], float vh) const {
        dst[3 * i] = va[0]; dst[3 * i + 1] = vb[0]; dst[3 * i + 2] = vh;
    }
};

}  // namespace

extern "C" int64_t mdg_tersoff_partial_size(int n_atoms) { return atom_blocks(n_atoms, TERS_LPA, TERS_BLOCK); }

extern "C" int64_t mdg_tersoff_work_size(int n_atoms, int max_nbr) { return tersoff_work_floats(n_atoms, max_nbr); }

extern "C" int mdg_tersoff_eval(const float* pos, int n_atoms, const MdgCell* cell, const int32_t* col, const int32_t* shift,
                                const int32_t* cnt, int max_nbr, const MdgTersoffConsts* k, const float* theta, const float* w,
                                float* energy, float* grad, float* hw, float* pth, float* pthw, float* partial, float* bond_work,
                                float out_scale, int accumulate, void* stream) {
    MDG_CHECK_ARG(pos && cell && col && shift && cnt, "tersoff_eval: null buffer (pos, cell or list)");
    MDG_CHECK_ARG(k, "tersoff_eval: consts is null");
    MDG_CHECK_ARG(n_atoms > 0 && max_nbr > 0, "tersoff_eval: bad sizes (n_atoms, max_nbr must be positive)");
    MDG_CHECK_ARG(theta || (k->A > 0.0 && k->B > 0.0), "tersoff_eval: consts need A > 0 and B > 0 (or a device theta)");
    MDG_CHECK_ARG(k->lam1 > 0.0 && k->lam2 > 0.0, "tersoff_eval: consts need lam1 > 0 and lam2 > 0");
    MDG_CHECK_ARG(k->D > 0.0 && k->R > k->D, "tersoff_eval: consts need D > 0 and R > D");
    MDG_CHECK_ARG(k->m == 1 || k->m == 3, "tersoff_eval: m must be 1 or 3");
    MDG_CHECK_ARG(k->n > 0.0 && k->beta >= 0.0, "tersoff_eval: consts need n > 0 and beta >= 0");
    MDG_CHECK_ARG(k->d != 0.0, "tersoff_eval: d must not be 0");
    MDG_CHECK_ARG(w || !(hw || pthw), "tersoff_eval: hw / pthw need w");
    MDG_CHECK_ARG(!w || hw || pthw, "tersoff_eval: w given without hw or pthw output");
    MDG_CHECK_ARG(energy || grad || hw || pth || pthw, "tersoff_eval: no output requested");
    MDG_CHECK_ARG(!energy || partial, "tersoff_eval: energy needs the partial buffer");
    MDG_CHECK_ARG(bond_work || !(grad || hw),
                  "tersoff_eval: grad / hw need bond_work (the scratch of the bond pass, mdg_tersoff_work_size() floats)");
    const int level = w ? 2 : ((grad || pth) ? 1 : 0);
    // (accumulate bit 2, "the list was searched with a skin", needs nothing here: the support test r < R + D is always applied)
    const TersIO a{pos, n_atoms, *cell, col, shift, cnt, max_nbr, w, bond_work, grad, hw, pth, pthw,
                   energy ? partial : nullptr, out_scale, accumulate & 1};
    const TersArgs v{theta, (float)k->A, (float)k->B, (float)k->h, (float)k->lam1, (float)k->lam2, (float)k->beta, (float)k->n,
                     (float)k->c, (float)k->d, (float)k->R, (float)k->D, (float)(k->R + k->D), (float)(k->R - k->D),
                     (float)k->lam3, (float)k->gamma, (int)k->m};
    tersoff_launch<TersOneView>(a, v, level, grad || hw, energy, partial, (hipStream_t)stream);
    MDG_CHECK_LAUNCH("tersoff_kernel");
    return MDG_OK;
}
