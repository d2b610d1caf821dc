// K26: Tersoff bond-order potential for up to four species over the per-atom (ELL) list
// (mdgrad_amd/interface.py TersoffMulti; Tersoff 1989, "Modeling solid-state chemistry: interatomic potentials for
// multicomponent systems"; the LAMMPS convention with lam3 = 0).
//
// The formulas, the two passes, both kernel templates and the list of which entry is read where are those of
// csrc/tersoff_core.hpp; read its header first.  What is particular to this file is that every constant is looked up by
// species, from one flat device table of derived constants (mdg_tersoff_multi_table_size floats):
//   pair entry   tab[8 (a S + b) ...]   = A, B, lam1, lam2, R, R - D, R + D, pi / (2 D)          row = centre, column = end
//   centre entry tab[8 S S + 8 a ...]   = h, beta, n, -1/(2n), d^2, gamma, gamma (c/d)^2, 2 gamma (c/d)^2 d^2
// The table is staged into LDS once per block (at most 160 floats, one barrier); a lane indexes it with the species of its
// own atoms, which differ from lane to lane.  A species read from `types` is clamped into the table.  This view has no
// exponential in zeta (HAS_LAM3 is false: no lam3 code is compiled); a row of pth / pthw is [2 S S + S], zero but for
// A[a, :], B[a, :], h[a], so the column sums over the atoms are dU/d(A, B, h).
#pragma clang fp contract(off)
#include "tersoff_core.hpp"

namespace {

constexpr int TERSM_SMAX = 4;                 // species

struct TersMArgs {
    const int32_t* types; int S;
    const float* tables;                       // device, 8 S (S + 1) floats
};

struct TersTableView {
    using Args = TersMArgs;
    static constexpr bool HAS_LAM3 = false;
    static constexpr int SMAX = TERSM_SMAX;
    const int32_t* types; int S;
    const TersEntry* tab;                      // the block's copy of the table in LDS

    // every thread of the block constructs the view (one barrier)
    __device__ __forceinline__ explicit TersTableView(const TersMArgs& a) : types(a.types), S(a.S) {
        __shared__ TersEntry lds[TERSM_SMAX * (TERSM_SMAX + 1)];
        float* flat = lds[0].v;              // (entries of eight floats, back to back: the layout of `tables`)
        const int n = 8 * S * (S + 1);
        for (int k = threadIdx.x; k < n; k += TERS_BLOCK) flat[k] = a.tables[k];
        __syncthreads();
        tab = lds;
    }
    // a species read from `types`, kept inside the table whatever the buffer holds
    __device__ __forceinline__ int species(int i) const { return min(max(types[i], 0), S - 1); }
    __device__ __forceinline__ const TersEntry& pair(int a, int b) const { return tab[a * S + b]; }
    __device__ __forceinline__ const TersEntry& centre(int a) const { return tab[S * S + a]; }
    // row i of a per-atom parameter table [N, 2 S S + S]: zero but for A[a, :], B[a, :], h[a]
    __device__ __forceinline__ void store_theta(float* dst, int i, int a, const float (&va)[TERSM_SMAX],
                                                const float (&vb)[TERSM_SMAX], float vh) const {
        const int S2 = S * S, P = 2 * S2 + S;
        float* r = dst + (size_t)i * P;
        for (int k = 0; k < P; ++k) r[k] = 0.f;
#pragma unroll
        for (int q = 0; q < TERSM_SMAX; ++q) {
            if (q < S) { r[a * S + q] = va[q]; r[S2 + a * S + q] = vb[q]; }
        }
        r[2 * S2 + a] = vh;
    }
};

}  // namespace

extern "C" int64_t mdg_tersoff_multi_partial_size(int n_atoms) { return atom_blocks(n_atoms, TERS_LPA, TERS_BLOCK); }

extern "C" int64_t mdg_tersoff_multi_work_size(int n_atoms, int max_nbr) { return tersoff_work_floats(n_atoms, max_nbr); }

extern "C" int64_t mdg_tersoff_multi_table_size(int n_species) {
    if (n_species < 1 || n_species > TERSM_SMAX) return 0;
    return 8 * (int64_t)n_species * (n_species + 1);
}

extern "C" int mdg_tersoff_multi_eval(const float* pos, int n_atoms, const MdgCell* cell, const int32_t* col, const int32_t* shift,
                                      const int32_t* cnt, int max_nbr, const int32_t* types, int n_species, const float* tables,
                                      const float* w, float* energy, float* grad, float* hw, float* pth, float* pthw,
                                      float* partial, float* bond_work, float out_scale, int accumulate, void* stream) {
    MDG_CHECK_ARG(pos && cell && col && shift && cnt, "tersoff_multi_eval: null buffer (pos, cell or list)");
    MDG_CHECK_ARG(n_atoms > 0 && max_nbr > 0, "tersoff_multi_eval: bad sizes (n_atoms, max_nbr must be positive)");
    MDG_CHECK_ARG(n_species >= 1 && n_species <= TERSM_SMAX, "tersoff_multi_eval: n_species must lie in [1, %d] (got %d)",
                  TERSM_SMAX, n_species);
    MDG_CHECK_ARG(types, "tersoff_multi_eval: types is null (device int32 [n_atoms])");
    MDG_CHECK_ARG(tables, "tersoff_multi_eval: tables is null (device float [mdg_tersoff_multi_table_size(n_species)])");
    MDG_CHECK_ARG(w || !(hw || pthw), "tersoff_multi_eval: hw / pthw need w");
    MDG_CHECK_ARG(!w || hw || pthw, "tersoff_multi_eval: w given without hw or pthw output");
    MDG_CHECK_ARG(energy || grad || hw || pth || pthw, "tersoff_multi_eval: no output requested");
    MDG_CHECK_ARG(!energy || partial, "tersoff_multi_eval: energy needs the partial buffer");
    MDG_CHECK_ARG(bond_work || !(grad || hw),
                  "tersoff_multi_eval: grad / hw need bond_work (the scratch of the bond pass, mdg_tersoff_multi_work_size() floats)");
    const int level = w ? 2 : ((grad || pth) ? 1 : 0);
    // (accumulate bit 2, "the list was searched with a skin", needs nothing here: the support test is always applied)
    const TersIO a{pos, n_atoms, *cell, col, shift, cnt, max_nbr, w, bond_work, grad, hw, pth, pthw,
                   energy ? partial : nullptr, out_scale, accumulate & 1};
    const TersMArgs v{types, n_species, tables};
    tersoff_launch<TersTableView>(a, v, level, grad || hw, energy, partial, (hipStream_t)stream);
    MDG_CHECK_LAUNCH("tersoff_multi_kernel");
    return MDG_OK;
}
