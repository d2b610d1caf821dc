// The scaffold of the per-frame many-body energies: what csrc/sw_frames.hip (K34), csrc/eam_frames.hip (K36, K37) and
// csrc/tersoff_frames.hip (K38) share and what knows nothing of a potential.  Their kernels keep the formulas.
//
// Shape: the frame's positions are staged in LDS (a wave per frame up to FP_WAVE_ATOMS atoms, four frames per workgroup; a
// workgroup per frame up to FP_GROUP_ATOMS); every thread owns the atoms t, t + TPF, ... and walks the WHOLE frame for each of
// them in index order: D = x_j - x_i re-imaged with the strict minimum image on the diagonal cell (pair_in of
// csrc/frame_pairs.hpp), r = sqrtf(d2) with the un-contracted d2.  Nothing is searched and no list exists.
//   open_frame    the staged-frame context of a thread: stages the frame into the kernel's own `sp` and waits for it
//   walk_all      atom i against every other atom of its frame, j = 0 .. N - 1 (walk_row's rotated order sums differently)
//   build_row     the atoms inside a support, written into the thread's OWN compact row in LDS (uint16, slot-major:
//                 lane-consecutive, no bank conflict); the row belongs to one thread from here to the pass that reads it
//                 (row_at), so no barrier separates them.  A row is never truncated silently: the caller counts the
//                 overflowing rows and stores nan_if() for the frame, alone
//   frame_sums    the per-frame sums over the wave or the workgroup (the shuffle / LDS trees of common.hpp, a fixed order)
//   launch_frames the grid and TPF of a launch from the atoms per frame, as compile-time constants (cf. with_form)
// The __shared__ arrays stay declared in the kernels: the LDS layout of a kernel reads in one place.
#pragma once
#include "frame_pairs.hpp"

namespace frame_pairs {

// one thread's view of its frame: thread t of the TPF that share frame f (slot g of the workgroup), staged at sx | sy | sz
template <int TPF>
struct FrameCtx {
    static_assert(TPF == MDG_WAVE || TPF == FP_BLOCK, "a wave or the whole workgroup per frame");
    static constexpr int CAP = TPF == MDG_WAVE ? FP_WAVE_ATOMS : FP_GROUP_ATOMS, FPB = FP_BLOCK / TPF;
    int t, g, N;
    long long f;
    bool live;                       // false for the frame slots past the last frame (the last workgroup of the wave shape)
    const float *sf, *sx, *sy, *sz;
};

// sp: the kernel's __shared__ float [FPB * 3 * CAP].  Every thread of the workgroup calls it (one barrier).
template <int TPF>
__device__ __forceinline__ FrameCtx<TPF> open_frame(float* sp, const float* pos, int F, int N) {
    using C = FrameCtx<TPF>;
    C c;
    c.t = threadIdx.x % TPF; c.g = threadIdx.x / TPF; c.N = N;
    c.f = (long long)blockIdx.x * C::FPB + c.g;
    c.live = c.f < F;
    float* sf = sp + c.g * 3 * C::CAP;
    if (c.live) stage_frame<TPF, C::CAP>(sf, pos + (size_t)c.f * N * 3, N, c.t);
    __syncthreads();
    c.sf = sf; c.sx = sf; c.sy = sf + C::CAP; c.sz = sf + 2 * C::CAP;
    return c;
}

// atom i of a staged frame against every other atom in index order: fn(j, dx, dy, dz, d2) with D = x_j - x_i re-imaged,
// for every j != i with d2 != 0 (the support is the caller's: r = sqrtf(d2), 0 < r < its cutoff)
template <int CAP, class Fn>
__device__ __forceinline__ void walk_all(const MdgCell& cell, const float* sf, int N, int i, Fn&& fn) {
    const float *sx = sf, *sy = sf + CAP, *sz = sf + 2 * CAP;
    const float xi = sx[i], yi = sy[i], zi = sz[i];
    const float inf = __int_as_float(0x7f800000);
    for (int j = 0; j < N; ++j) {
        float dx = sx[j] - xi, dy = sy[j] - yi, dz = sz[j] - zi, d2;
        if (j != i && pair_in(cell, inf, dx, dy, dz, d2)) fn(j, dx, dy, dz, d2);
    }
}

// slot s of a thread's row (row = the kernel's __shared__ uint16_t [ROW_CAP * FP_BLOCK] + threadIdx.x)
__device__ __forceinline__ uint16_t& row_at(uint16_t* row, int s) { return row[s * FP_BLOCK]; }

// the row of atom i: the atoms j with 0 < r and support(j, r), in index order; returns the entries written (at most
// ROW_CAP), over = whether more were found
template <int ROW_CAP, int CAP, class Support>
__device__ __forceinline__ int build_row(uint16_t* row, const MdgCell& cell, const float* sf, int N, int i, int& over,
                                         Support&& support) {
    int n = 0;
    over = 0;
    walk_all<CAP>(cell, sf, N, i, [&](int j, float, float, float, float d2) {
        const float rv = sqrtf(d2);
        if (rv > 0.f && support(j, rv)) {
            if (n < ROW_CAP) row_at(row, n++) = (uint16_t)j;
            else over = 1;
        }
    });
    return n;
}

// v[k] <- its sum over the threads of the frame (red: the kernel's __shared__ float [(FP_BLOCK / MDG_WAVE) * NV], read by the
// workgroup shape); true on the one thread that stores the frame's results
template <int TPF, int NV>
__device__ __forceinline__ bool frame_sums(const FrameCtx<TPF>& c, float (&v)[NV], float* red) {
    if constexpr (TPF == MDG_WAVE) {
        for (float& x : v) x = wave_sum(x);
    } else {
        block_sum_n<NV>(v, red);
    }
    return c.live && c.t == 0;
}

// what a frame with an overflowing row stores in place of v
__device__ __forceinline__ float nan_if(bool bad, float v) { return bad ? __int_as_float(0x7fc00000) : v; }

// ---------------------------------------------------------------------------------- host side
// fn(TPF as std::integral_constant, grid): a wave per frame up to FP_WAVE_ATOMS atoms, a workgroup per frame beyond
template <class Fn>
inline void launch_frames(int n_frames, int n_atoms, Fn&& fn) {
    if (n_atoms <= FP_WAVE_ATOMS) {
        constexpr int FPB = FP_BLOCK / MDG_WAVE;
        fn(std::integral_constant<int, MDG_WAVE>{}, dim3((n_frames + FPB - 1) / FPB));
    } else {
        fn(std::integral_constant<int, FP_BLOCK>{}, dim3(n_frames));
    }
}

// the same with a kernel's boolean template argument: fn(TPF, flag as std::bool_constant, grid)
template <class Fn>
inline void launch_frames(int n_frames, int n_atoms, bool flag, Fn&& fn) {
    launch_frames(n_frames, n_atoms, [&](auto tpf, dim3 grid) {
        if (flag) fn(tpf, std::true_type{}, grid);
        else fn(tpf, std::false_type{}, grid);
    });
}

}  // namespace frame_pairs
