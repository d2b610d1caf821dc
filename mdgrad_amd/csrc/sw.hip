// K23: Stillinger-Weber two- plus three-body potential for one species over the per-atom (ELL) list
// (mdgrad_amd/interface.py StillingerWeber; Stillinger and Weber 1985, Molinero and Moore 2009 for mW water).
//
//   rc = a sigma,  g(r) = exp(gamma sigma / (r - rc)) for r < rc, else exactly 0
//   phi2(r)       = A eps [B (sigma/r)^p - (sigma/r)^q] exp(sigma / (r - rc))
//   phi3(j, i, k) = lam eps (cos theta_jik - cos0)^2 g(r_ij) g(r_ik)                 (i = the centre)
//   U = sum_{i<j} phi2 + sum_i sum_{j<k in row(i)} phi3
//
// The formulas, the gather and the kernel template are those of csrc/sw_core.hpp; read its header first.  What is particular to
// this file is where the constants come from: there is one pair entry and one triplet entry, derived per thread from the
// kernel arguments and held in registers, with (eps, sigma, lam) read from the `theta` device buffer when it is given; the
// derived values rc = a sigma, gamma sigma, A eps and K = lam eps are float32 products.  The exponents stay integers.  No
// `types` array, no table in LDS and no barrier beyond the block reduction of the energy.
// A row of pth / pthw is d u_i / d(eps, sigma, lam) with u_i = eps (1/2 sum_j e2 + lam sum t3): eps scales the pair and the
// three-body term alike, so the row is formed from the core's sums as (1/2 S2 + lam S3, eps 1/2 S2s + S3s, eps S3).
#pragma clang fp contract(off)
#include "sw_core.hpp"

namespace {

struct SwArgs {
    const float* theta;                        // device (eps, sigma, lam), or null: the three host values below
    float eps, sigma, lam;
    float a, gamma, cos0, A, B; int p, q;
};

struct SwOneView {
    using Args = SwArgs;
    static constexpr int SMAX = 1;
    static constexpr int S = 1;
    SwPairE pp; SwTripE tt;
    float lam; int ip, iq;

    __device__ __forceinline__ explicit SwOneView(const SwArgs& k) {
        const float eps = k.theta ? k.theta[0] : k.eps, sigma = k.theta ? k.theta[1] : k.sigma;
        lam = k.theta ? k.theta[2] : k.lam;
        ip = k.p; iq = k.q;
        pp = SwPairE{eps, sigma, k.a * sigma, k.gamma * sigma, k.gamma, k.A, k.B, (float)k.p, (float)k.q, k.a, eps * k.A, 0.f};
        tt = SwTripE{lam * eps, k.cos0, 0.f, 0.f};
    }
    __device__ __forceinline__ int species(int) const { return 0; }
    __device__ __forceinline__ const SwPairE& pair(int, int) const { return pp; }
    __device__ __forceinline__ const SwTripE& trip(int, int, int) const { return tt; }
    __device__ __forceinline__ int p(const SwPairE&) const { return ip; }
    __device__ __forceinline__ int q(const SwPairE&) const { return iq; }
    // (d/d eps, d/d sigma, d/d lam) of u_i = eps (1/2 sum e2 + lam sum t3) from v = (1/2 sum e2, eps 1/2 sum d e2 / d sigma +
    // the triplets' sigma terms, sum t3): eps scales the pair and the three-body term alike
    __device__ __forceinline__ void store_theta(float* dst, int i, int, int sub, const float* v) const {
        if (sub != 0) return;
        dst[3 * i] = v[0] + lam * v[2]; dst[3 * i + 1] = v[1]; dst[3 * i + 2] = pp.eps * v[2];
    }
};

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
    const SwIO a{pos, n_atoms, *cell, col, shift, cnt, max_nbr, w, grad, hw, pth, pthw, energy ? partial : nullptr, out_scale,
                 accumulate & 1};
    const SwArgs v{theta, (float)k->epsilon, (float)k->sigma, (float)k->lam, (float)k->a, (float)k->gamma, (float)k->cos0,
                   (float)k->A, (float)k->B, (int)k->p, (int)k->q};
    sw_launch<SwOneView>(a, v, level, energy, partial, (hipStream_t)stream);
    MDG_CHECK_LAUNCH("sw_ell_kernel");
    return MDG_OK;
}
