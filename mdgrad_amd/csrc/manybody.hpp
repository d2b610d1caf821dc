// What the terms over the per-atom (ELL) list share around their formulas: the Stillinger-Weber, Sutton-Chen and Tersoff
// kernels (csrc/sw.hip, eam.hip, tersoff.hip, tersoff_multi.hip) take all of it, the Coulomb term (csrc/coulomb.hip) the block
// count and the finish kernel.  Every function is internal to the translation unit that includes this file.
#pragma once
#include <type_traits>
#include "common.hpp"

namespace {

// blocks of `block` threads for n_atoms atoms at `lpa` lanes per atom: the grid, and the length of the energy partial
inline int64_t atom_blocks(int n_atoms, int lpa, int block) {
    if (n_atoms <= 0) return 0;
    const int apb = block / lpa;
    return (int64_t)((n_atoms + apb - 1) / apb);
}

// dst[3 i ...] = os * (x, y, z), added onto what is there when oacc (the force sums of a Stack)
__device__ __forceinline__ void store3(float* dst, int i, float os, int oacc, float x, float y, float z) {
    if (oacc) { dst[3 * i] = fmaf(os, x, dst[3 * i]); dst[3 * i + 1] = fmaf(os, y, dst[3 * i + 1]); dst[3 * i + 2] = fmaf(os, z, dst[3 * i + 2]); }
    else { dst[3 * i] = os * x; dst[3 * i + 1] = os * y; dst[3 * i + 2] = os * z; }
}

// the energy from the block partials: one wave, fixed summation order
__global__ void energy_finish(const float* __restrict__ partial, int nblocks, float* energy) {
    const int lane = threadIdx.x;
    float s = 0.f;
    for (int b = lane; b < nblocks; b += 64) s += partial[b];
    s = wave_sum(s);
    if (lane == 0) energy[0] = s;
}

// f(std::integral_constant<int, LEVEL>()) for the run-time level 0, 1 or 2: the caller launches kernel<decltype(L)::value>
template <class F>
inline void with_level(int level, F&& f) {
    if (level == 2) f(std::integral_constant<int, 2>());
    else if (level == 1) f(std::integral_constant<int, 1>());
    else f(std::integral_constant<int, 0>());
}

}  // namespace
