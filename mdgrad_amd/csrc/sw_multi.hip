// K28: Stillinger-Weber two- plus three-body potential for up to four species over the per-atom (ELL) list
// (mdgrad_amd/interface.py StillingerWeberMulti; the LAMMPS `pair_style sw` convention).
//
// The formulas, the gather and the kernel template are those of csrc/sw_core.hpp; read its header first.  What is particular
// to this file is where the constants come from:
//  - every constant comes from one flat device table (mdg_sw_multi_table_size floats), staged into LDS once per block (one
//    barrier):
//      pair entry    tab[12 (a S + b) ...]                 = eps, sigma, a sigma, gamma sigma, gamma, A, B, p, q, a, A eps, 0
//      triplet entry tab[12 S S + 4 ((a S + b) S + c) ...] = K_a{bc}, cos0_abc, w_abc, 0
//    row = the species of the centre.  w_abc = eps3_abc / 2 (eps3_abb for b = c) is the weight with which lam[a, b, c] enters
//    K_a{bc}.  A lane indexes the table with the species of its own atoms; a species read from `types` is clamped into it.
//  - the pair tables need not be symmetric: the force of the pair (i, j) is the derivative of (phi2_ab + phi2_ba) / 2 and both
//    directions are evaluated (once when a = b).
//  - the per-lane sums are kept per end species (4) and per unordered pair of end species (10); a row of pth / pthw is
//    [2 S S + S S S] = d u_i / d(eps [S, S], sigma [S, S], lam [S, S, S]), zero but for eps[a, :], sigma[a, :], lam[a, :, :],
//    where lam[a, b, c] and lam[a, c, b] hold w_abc T and w_acb T of their class's sum T: the column sums over the atoms are
//    dU/d(eps, sigma, lam).
#pragma clang fp contract(off)
#include "sw_core.hpp"

namespace {

constexpr int SWM_SMAX = 4;                   // species
constexpr int SWM_TABLE_MAX = SW_PAIR * SWM_SMAX * SWM_SMAX + SW_TRIP * SWM_SMAX * SWM_SMAX * SWM_SMAX;

struct SwmArgs {
    const int32_t* types; int S;
    const float* tables;                       // device, mdg_sw_multi_table_size(S) floats
};

struct SwTableView {
    using Args = SwmArgs;
    static constexpr int SMAX = SWM_SMAX;
    const int32_t* types; int S;
    const float* tab;                          // the block's copy of the table in LDS

    // every thread of the block constructs the view (one barrier)
    __device__ __forceinline__ explicit SwTableView(const SwmArgs& a) : types(a.types), S(a.S) {
        __shared__ float lds[SWM_TABLE_MAX];
        const int nt = SW_PAIR * S * S + SW_TRIP * S * S * S;
        for (int k = threadIdx.x; k < nt; k += SW_BLOCK) lds[k] = a.tables[k];
        __syncthreads();
        tab = lds;
    }
    // a species read from `types`, kept inside the table whatever the buffer holds
    __device__ __forceinline__ int species(int i) const { return min(max(types[i], 0), S - 1); }
    __device__ __forceinline__ const SwPairE& pair(int a, int b) const {
        return reinterpret_cast<const SwPairE*>(tab)[a * S + b];
    }
    __device__ __forceinline__ const SwTripE& trip(int a, int b, int c) const {
        return reinterpret_cast<const SwTripE*>(tab + SW_PAIR * S * S)[(a * S + b) * S + c];
    }
    __device__ __forceinline__ int p(const SwPairE& P) const { return (int)P.fp; }
    __device__ __forceinline__ int q(const SwPairE& P) const { return (int)P.fq; }

    // row i of a per-atom parameter table [N, 2 S S + S S S] from the group's sums v = (pe[4], ps[4], class sums[10]): the lanes
    // of the group zero the entries of the other species' blocks, lane 0 writes eps[a, :], sigma[a, :], lam[a, :, :]
    __device__ __forceinline__ void store_theta(float* dst, int i, int a, int sub, const float* v) const {
        const int S2 = S * S, P = 2 * S2 + S2 * S;
        float* r = dst + (size_t)i * P;
        for (int k = sub; k < P; k += SW_LPA) {
            const int owner = k < 2 * S2 ? (k < S2 ? k : k - S2) / S : (k - 2 * S2) / S2;
            if (owner != a) r[k] = 0.f;
        }
        if (sub != 0) return;
#pragma unroll
        for (int q = 0; q < SMAX; ++q) {
            if (q < S) { r[a * S + q] = v[q]; r[S2 + a * S + q] = v[SMAX + q]; }
        }
        float* l = r + 2 * S2 + a * S2;
#pragma unroll
        for (int bb = 0; bb < SMAX; ++bb) {
#pragma unroll
            for (int cc = bb; cc < SMAX; ++cc) {
                if (cc < S) {
                    const float t = v[2 * SMAX + sw_cls<SMAX>(bb, cc)];
                    l[bb * S + cc] = trip(a, bb, cc).w * t;
                    if (cc != bb) l[cc * S + bb] = trip(a, cc, bb).w * t;
                }
            }
        }
    }
};

}  // namespace

extern "C" int64_t mdg_sw_multi_partial_size(int n_atoms) { return atom_blocks(n_atoms, SW_LPA, SW_BLOCK); }

extern "C" int64_t mdg_sw_multi_table_size(int n_species) {
    if (n_species < 1 || n_species > SWM_SMAX) return 0;
    const int64_t S = n_species;
    return SW_PAIR * S * S + SW_TRIP * S * S * S;
}

extern "C" int mdg_sw_multi_eval(const float* pos, int n_atoms, const MdgCell* cell, const int32_t* col, const int32_t* shift,
                                 const int32_t* cnt, int max_nbr, const int32_t* types, int n_species, const float* tables,
                                 const float* w, float* energy, float* grad, float* hw, float* pth, float* pthw, float* partial,
                                 float out_scale, int accumulate, void* stream) {
    MDG_CHECK_ARG(pos && cell && col && shift && cnt, "sw_multi_eval: null buffer (pos, cell or list)");
    MDG_CHECK_ARG(n_atoms > 0 && max_nbr > 0, "sw_multi_eval: bad sizes (n_atoms, max_nbr must be positive)");
    MDG_CHECK_ARG(n_species >= 1 && n_species <= SWM_SMAX, "sw_multi_eval: n_species must lie in [1, %d] (got %d)", SWM_SMAX,
                  n_species);
    MDG_CHECK_ARG(types, "sw_multi_eval: types is null (device int32 [n_atoms])");
    MDG_CHECK_ARG(tables, "sw_multi_eval: tables is null (device float [mdg_sw_multi_table_size(n_species)])");
    MDG_CHECK_ARG(w || !(hw || pthw), "sw_multi_eval: hw / pthw need w");
    MDG_CHECK_ARG(!w || hw || pthw, "sw_multi_eval: w given without hw or pthw output");
    MDG_CHECK_ARG(energy || grad || hw || pth || pthw, "sw_multi_eval: no output requested");
    MDG_CHECK_ARG(!energy || partial, "sw_multi_eval: energy needs the partial buffer");
    const int level = w ? 2 : ((grad || pth) ? 1 : 0);
    // (accumulate bit 2, "the list was searched with a skin", needs nothing here: every entry's own support test is always applied)
    const SwIO a{pos, n_atoms, *cell, col, shift, cnt, max_nbr, w, grad, hw, pth, pthw, energy ? partial : nullptr, out_scale,
                 accumulate & 1};
    const SwmArgs v{types, n_species, tables};
    sw_launch<SwTableView>(a, v, level, energy, partial, (hipStream_t)stream);
    MDG_CHECK_LAUNCH("sw_multi_kernel");
    return MDG_OK;
}
