// What the terms over the per-atom (ELL) list share around their formulas: the Stillinger-Weber, Sutton-Chen and Tersoff
// kernels (csrc/sw.hip, eam.hip, tersoff.hip, tersoff_multi.hip) and the Coulomb term (csrc/coulomb.hip) take the block count and
// the finish kernel from here (the accumulating store `store3` and the level dispatch `with_level`, which the Ewald terms on
// their static tables use as well, are in common.hpp).  Every function is internal to the translation unit that includes this file.
#pragma once
#include "common.hpp"

namespace {

// blocks of `block` threads for n_atoms atoms at `lpa` lanes per atom: the grid, and the length of the energy partial
inline int64_t atom_blocks(int n_atoms, int lpa, int block) {
    if (n_atoms <= 0) return 0;
    const int apb = block / lpa;
    return (int64_t)((n_atoms + apb - 1) / apb);
}

// the energy from the block partials: one wave, fixed summation order
__global__ void energy_finish(const float* __restrict__ partial, int nblocks, float* energy) {
    const int lane = threadIdx.x;
    float s = 0.f;
    for (int b = lane; b < nblocks; b += 64) s += partial[b];
    s = wave_sum(s);
    if (lane == 0) energy[0] = s;
}

}  // namespace
