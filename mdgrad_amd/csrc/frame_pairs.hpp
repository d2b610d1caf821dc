// List-free all-pairs sweeps over every frame of a trajectory, parameterised by what a visit accumulates: the scaffolding of
// the per-frame pair observables.  Who takes what:
//   csrc/virial.hip (K15), csrc/energy.hip (K31)   a visit policy on the kernels of this file
//   csrc/rdf_frames.hip (K32)                      kernels of its own (its visit scatters into an integer histogram) on the
//                                                  pair walk (stage_frame, once_partners, walk_row) and the frame checks
//   csrc/energy_table.hip (K33)                    the pair test, the tile staging, the second-stage sums and the frame
//                                                  checks; it writes its sweeps out
//   csrc/frame_atoms.hpp                           stage_frame and pair_in, for the many-body frame energies (K34, K36 - K38:
//                                                  csrc/sw_frames.hip, eam_frames.hip, tersoff_frames.hip), whose atoms walk
//                                                  the whole frame in index order; those take the frame checks from here
//
// Pair set of a term = the one PairPotentials sums the energy over (torchmd/topology.py:30-73, interface.py:298-300):
// pairs i < j, D = x_j - x_i re-imaged with the reference's strict +-1/2 minimum image on the diagonal cell,
// 0 < d^2 < cutoff^2 with the un-contracted d^2 of the list builders (csrc/nbr.hip), the term's [N, N] selection mask,
// every term its own cutoff.  The test is odd in D bit for bit, so a pair is in or out whichever end visits it.
//
// A visit policy V names what is summed:
//   V::FWD_LEVEL, V::BWD_LEVEL          pair_eval levels of the value and of its gradient
//   V::SIGN                             out[f] = SIGN * sum_pairs V::value
//   V::value(o, r, acc)                 acc + the summand of a pair (the policy states the arithmetic: a sum or an fma)
//   V::radial(o, r, ir)                 c of  d(sum)/dx_i = sum_j c D          (D = x_j - x_i)
//   V::dtheta(o, r, k, acc)             acc + d(summand)/dtheta_k
// Three shapes by frame size, positions staged in LDS in all of them:
//   N <= 128     a wave per frame, four frames per workgroup
//   N <= 1024    a workgroup per frame
//   larger       (i-block, j-block) tiles of 256 x 256 atoms
// and three sweeps (MODE):
//   FP_VALUE     every unordered pair once: row i takes the partners (i + k) mod N, k = 1 .. (N - 1) / 2 (for even N also
//                k = N / 2 on the first half of the rows) -- the same work for every lane; across the blocks of a tiled frame
//                the same rotation over blocks
//   FP_THETA     the same once-per-pair sweep at BWD_LEVEL, accumulating g[f] d(summand)/dtheta only: no position is written
//   FP_ROWS      full rows -- atom i sums over every j, so each pair is evaluated from both ends and nothing is accumulated
//                across lanes; the parameter gradient takes half of each visit
// Every sum runs in a fixed order: per lane, then the shuffle / LDS trees of common.hpp, then per-frame (per-tile) partials
// added by a second tiny kernel in index order.  No floating-point atomics: two launches give the same bits.
// The functional form is dispatched once per term around the whole sweep (evaluation and accumulation), so PairOut's
// parameter slots stay in registers (see pair_ell_kernel).
#pragma once
#include <type_traits>
#include "common.hpp"

namespace frame_pairs {

constexpr int FP_BLOCK = 256;
constexpr int FP_WAVE_ATOMS = 128;      // up to here a wave per frame
constexpr int FP_GROUP_ATOMS = 1024;    // up to here a workgroup per frame
constexpr int FP_TILE = 256;            // beyond: tiles of FP_TILE x FP_TILE atoms
constexpr int FP_MAX_ATOMS = 32768;
constexpr int FP_VALUE = 0, FP_THETA = 1, FP_ROWS = 2;

struct FpArgs {
    const float* pos;        // [F, N, 3]
    const float* theta;
    const float* g;          // FP_THETA, FP_ROWS: upstream gradient [F]
    float* out;              // FP_VALUE: [F]
    float* g_pos;            // FP_ROWS: [F, N, 3]
    float* partial;          // tiled FP_VALUE: [F, tiles];  FP_THETA / FP_ROWS: [rows, K]
    int F, N, K;
    MdgCell cell;
    MdgTerms terms;
};

struct FpAcc {
    float w;                         // FP_VALUE: sum of the summands
    float gx, gy, gz;                // FP_ROWS:  sum c D of one atom
    float th[MDG_MAX_THETA];         // FP_THETA, FP_ROWS: sum d(summand)/dtheta over the visits of this lane
};

constexpr int form_ntheta(int KIND) { return kind_ntheta(KIND == KIND_LJ126 ? MDG_PAIR_LJ : KIND); }

// calls fn with the term's functional form as a compile-time constant
template <class Fn>
__device__ __forceinline__ void with_form(const TermConst& tc, Fn&& fn) {
    switch (tc.kind) {
    case MDG_PAIR_LJ:
        if (tc.p == 12 && tc.q == 6) fn(std::integral_constant<int, KIND_LJ126>{});
        else fn(std::integral_constant<int, MDG_PAIR_LJ>{});
        break;
    case MDG_PAIR_MORSE: fn(std::integral_constant<int, MDG_PAIR_MORSE>{}); break;
    case MDG_PAIR_BUCK: fn(std::integral_constant<int, MDG_PAIR_BUCK>{}); break;
    default: fn(std::integral_constant<int, MDG_PAIR_YUKAWA>{}); break;
    }
}

// D = x_j - x_i -> its minimum image; true when the pair counts for a term of squared cutoff rc2
__device__ __forceinline__ bool pair_in(const MdgCell& c, float rc2, float& dx, float& dy, float& dz, float& d2) {
    min_image<true>(c, dx, dy, dz);
    d2 = norm2_ref(dx, dy, dz);
    return (d2 < rc2) && (d2 != 0.f);
}

template <class V, int KIND, int MODE>
__device__ __forceinline__ void visit(const TermConst& tc, float dx, float dy, float dz, float d2, FpAcc& a) {
    PairOut o{};
    float r, ir;
    pair_eval<MODE == FP_VALUE ? V::FWD_LEVEL : V::BWD_LEVEL, KIND>(tc, d2, r, ir, o);
    if (MODE == FP_VALUE) {
        a.w = V::value(o, r, a.w);
    } else {
        if (MODE == FP_ROWS) {
            const float c = V::radial(o, r, ir);
            a.gx = fmaf(c, dx, a.gx); a.gy = fmaf(c, dy, a.gy); a.gz = fmaf(c, dz, a.gz);
        }
#pragma unroll
        for (int t = 0; t < form_ntheta(KIND); ++t) a.th[t] = V::dtheta(o, r, t, a.th[t]);
    }
}

// dL/dx of one atom for one term: the first term of a frame writes, the others add (one thread owns the atom throughout)
__device__ __forceinline__ void put_grad(float* g, const FpAcc& a, float gw, bool first) {
    if (first) { g[0] = gw * a.gx; g[1] = gw * a.gy; g[2] = gw * a.gz; }
    else { g[0] = fmaf(gw, a.gx, g[0]); g[1] = fmaf(gw, a.gy, g[1]); g[2] = fmaf(gw, a.gz, g[2]); }
}

// ---------------------------------------------------------------------------------- the pair walk
// What the sweeps of every user share and what knows nothing of the sums: a visit is the callable fn(dx, dy, dz, d2), called
// for the pairs of the set above with D = x_j - x_i already re-imaged.
//
// the frame p [N, 3] into sf = x [CAP] | y [CAP] | z [CAP], by the TPF threads that share it (t = 0 .. TPF - 1)
template <int TPF, int CAP>
__device__ __forceinline__ void stage_frame(float* sf, const float* p, int N, int t) {
    for (int e = t; e < 3 * N; e += TPF) sf[(e % 3) * CAP + e / 3] = p[e];
}

// partners of row i in the once-per-pair sweep: k = 1 .. (N - 1) / 2, for even N also k = N / 2 on the first half of the rows
__device__ __forceinline__ int once_partners(int N, int i) { return ((N - 1) >> 1) + ((!(N & 1) && i < (N >> 1)) ? 1 : 0); }

// atom i of a staged frame against its partners (i + k) mod N, k = 1 .. kmax (once_partners, or N - 1 for the full row)
template <int CAP, class Fn>
__device__ __forceinline__ void walk_row(const MdgCell& cell, float rc2, const uint8_t* mask, const float* sf, int N, int i,
                                         int kmax, Fn&& fn) {
    const float *sx = sf, *sy = sf + CAP, *sz = sf + 2 * CAP;
    const float xi = sx[i], yi = sy[i], zi = sz[i];
    for (int k = 1; k <= kmax; ++k) {
        int j = i + k;
        if (j >= N) j -= N;
        if (mask && !mask[(size_t)i * N + j]) continue;
        float dx = sx[j] - xi, dy = sy[j] - yi, dz = sz[j] - zi, d2;
        if (!pair_in(cell, rc2, dx, dy, dz, d2)) continue;
        fn(dx, dy, dz, d2);
    }
}

// thread-owned atom i (mrow = its mask row) against the staged atoms [jlo, nj) of the tile that starts at atom j0
template <class Fn>
__device__ __forceinline__ void walk_tile(const MdgCell& cell, float rc2, const uint8_t* mrow, const float* sj, int j0, int jlo,
                                          int nj, float xi, float yi, float zi, Fn&& fn) {
    for (int jj = jlo; jj < nj; ++jj) {
        if (mrow && !mrow[j0 + jj]) continue;
        float dx = sj[jj] - xi, dy = sj[FP_TILE + jj] - yi, dz = sj[2 * FP_TILE + jj] - zi, d2;
        if (!pair_in(cell, rc2, dx, dy, dz, d2)) continue;
        fn(dx, dy, dz, d2);
    }
}

__device__ __forceinline__ void stage_tile(float* sj, const float* p, int j0, int nj) {
    for (int e = threadIdx.x; e < 3 * nj; e += FP_BLOCK) sj[(e % 3) * FP_TILE + e / 3] = p[3 * (size_t)j0 + e];
}

// ---------------------------------------------------------------------------------- whole frame in LDS (N <= 1024)
// TPF threads share a frame: lane t of them owns the atoms t, t + TPF, ...
template <class V, int TPF, int MODE>
__global__ __launch_bounds__(FP_BLOCK) void fp_frame_kernel(const FpArgs A) {
    constexpr int CAP = TPF == MDG_WAVE ? FP_WAVE_ATOMS : FP_GROUP_ATOMS, FPB = FP_BLOCK / TPF;
    static_assert(TPF == MDG_WAVE || TPF == FP_BLOCK, "a wave or the whole workgroup per frame");
    __shared__ float sp[FPB * 3 * CAP];
    __shared__ float red[4 * MDG_MAX_THETA];
    const int t = threadIdx.x % TPF, g = threadIdx.x / TPF, N = A.N;
    const long long f = (long long)blockIdx.x * FPB + g;
    const bool live = f < A.F;
    float* sf = sp + g * 3 * CAP;
    if (live) stage_frame<TPF, CAP>(sf, A.pos + (size_t)f * N * 3, N, t);
    __syncthreads();
    const float gw = (MODE != FP_VALUE && live) ? A.g[f] : 0.f;
    float w = 0.f;
    for (int m = 0; m < A.terms.n_terms; ++m) {
        const MdgPairTerm& term = A.terms.t[m];
        const TermConst tc = term_prepare(term, A.theta);
        const uint8_t* mask = term.mask;
        with_form(tc, [&](auto form) {
            constexpr int KIND = decltype(form)::value;
            FpAcc a{};
            if (live) {
                for (int i = t; i < N; i += TPF) {
                    if (MODE == FP_ROWS) a.gx = a.gy = a.gz = 0.f;
                    walk_row<CAP>(A.cell, tc.rc2, mask, sf, N, i, MODE == FP_ROWS ? N - 1 : once_partners(N, i),
                                  [&](float dx, float dy, float dz, float d2) { visit<V, KIND, MODE>(tc, dx, dy, dz, d2, a); });
                    if (MODE == FP_ROWS) put_grad(A.g_pos + ((size_t)f * N + i) * 3, a, gw, m == 0);
                }
            }
            w += a.w;
            if constexpr (MODE != FP_VALUE && form_ntheta(KIND) > 0) {
                if constexpr (TPF == MDG_WAVE) {
#pragma unroll
                    for (int k = 0; k < form_ntheta(KIND); ++k) a.th[k] = wave_sum(a.th[k]);
                } else {
                    block_sum_n<MDG_MAX_THETA>(a.th, red);
                }
                if (live && t == 0) {
                    // (full rows visit each pair from both ends: half of each visit)
                    const float s = (MODE == FP_ROWS ? 0.5f : 1.f) * V::SIGN * gw;
#pragma unroll
                    for (int k = 0; k < form_ntheta(KIND); ++k) A.partial[(size_t)f * A.K + term.theta_off + k] = s * a.th[k];
                }
            }
        });
    }
    if (MODE == FP_VALUE) {
        w = TPF == MDG_WAVE ? wave_sum(w) : block_sum(w, red);
        if (live && t == 0) A.out[f] = V::SIGN * w;
    }
}

// ---------------------------------------------------------------------------------- tiles (N > 1024)
// grid (F, nb * (nb / 2 + 1)): tile id = ib + nb * k pairs the i-block ib with the j-block (ib + k) mod nb; k = 0 is the
// diagonal tile (j > i), and for even nb the shell k = nb / 2 belongs to the first half of the i-blocks (the other tiles of
// that shell write zeros).  MODE = FP_VALUE or FP_THETA.
template <class V, int MODE>
__global__ __launch_bounds__(FP_BLOCK) void fp_tile_once_kernel(const FpArgs A, int nb) {
    __shared__ float sj[3 * FP_TILE];
    __shared__ float red[4 * MDG_MAX_THETA];
    const int f = blockIdx.x, id = blockIdx.y, ib = id % nb, k = id / nb, t = threadIdx.x, N = A.N;
    const bool tile_on = (nb & 1) || k != (nb >> 1) || ib < (nb >> 1);
    int jb = ib + k;
    if (jb >= nb) jb -= nb;
    const float* p = A.pos + (size_t)f * N * 3;
    const int i = ib * FP_TILE + t, j0 = jb * FP_TILE, nj = min(FP_TILE, N - j0);
    const bool live = tile_on && i < N;
    if (tile_on) stage_tile(sj, p, j0, nj);
    __syncthreads();
    const float xi = live ? p[3 * i] : 0.f, yi = live ? p[3 * i + 1] : 0.f, zi = live ? p[3 * i + 2] : 0.f;
    const float gw = MODE == FP_THETA ? A.g[f] : 0.f;
    float w = 0.f;
    for (int m = 0; m < A.terms.n_terms; ++m) {
        const MdgPairTerm& term = A.terms.t[m];
        const TermConst tc = term_prepare(term, A.theta);
        const uint8_t* mrow = (term.mask && live) ? term.mask + (size_t)i * N : nullptr;
        with_form(tc, [&](auto form) {
            constexpr int KIND = decltype(form)::value;
            FpAcc a{};
            if (live)
                walk_tile(A.cell, tc.rc2, mrow, sj, j0, k == 0 ? t + 1 : 0, nj, xi, yi, zi,
                          [&](float dx, float dy, float dz, float d2) { visit<V, KIND, MODE>(tc, dx, dy, dz, d2, a); });
            w += a.w;
            if constexpr (MODE == FP_THETA && form_ntheta(KIND) > 0) {
                block_sum_n<MDG_MAX_THETA>(a.th, red);
                if (t == 0) {
#pragma unroll
                    for (int c = 0; c < form_ntheta(KIND); ++c)
                        A.partial[((size_t)f * gridDim.y + id) * A.K + term.theta_off + c] = V::SIGN * gw * a.th[c];
                }
            }
        });
    }
    if (MODE == FP_VALUE) {
        w = block_sum(w, red);
        if (t == 0) A.partial[(size_t)f * gridDim.y + id] = w;
    }
}

// grid (F, nb): the i-block against every j-block (FP_ROWS)
template <class V>
__global__ __launch_bounds__(FP_BLOCK) void fp_tile_rows_kernel(const FpArgs A, int nb) {
    __shared__ float sj[3 * FP_TILE];
    __shared__ float red[4 * MDG_MAX_THETA];
    const int f = blockIdx.x, ib = blockIdx.y, t = threadIdx.x, N = A.N;
    const float* p = A.pos + (size_t)f * N * 3;
    const int i = ib * FP_TILE + t;
    const bool live = i < N;
    const float xi = live ? p[3 * i] : 0.f, yi = live ? p[3 * i + 1] : 0.f, zi = live ? p[3 * i + 2] : 0.f;
    const float gw = A.g[f];
    for (int m = 0; m < A.terms.n_terms; ++m) {
        const MdgPairTerm& term = A.terms.t[m];
        const TermConst tc = term_prepare(term, A.theta);
        const uint8_t* mrow = (term.mask && live) ? term.mask + (size_t)i * N : nullptr;
        with_form(tc, [&](auto form) {
            constexpr int KIND = decltype(form)::value;
            FpAcc a{};
            for (int jb = 0; jb < nb; ++jb) {
                const int j0 = jb * FP_TILE, nj = min(FP_TILE, N - j0);
                __syncthreads();                       // the previous tile has been read
                stage_tile(sj, p, j0, nj);
                __syncthreads();
                if (live)
                    walk_tile(A.cell, tc.rc2, mrow, sj, j0, 0, nj, xi, yi, zi,
                              [&](float dx, float dy, float dz, float d2) { visit<V, KIND, FP_ROWS>(tc, dx, dy, dz, d2, a); });
            }
            if (live) put_grad(A.g_pos + ((size_t)f * N + i) * 3, a, gw, m == 0);
            if constexpr (form_ntheta(KIND) > 0) {
                block_sum_n<MDG_MAX_THETA>(a.th, red);
                if (t == 0) {
#pragma unroll
                    for (int c = 0; c < form_ntheta(KIND); ++c)
                        A.partial[((size_t)f * nb + ib) * A.K + term.theta_off + c] = 0.5f * V::SIGN * gw * a.th[c];
                }
            }
        });
    }
}

// ---------------------------------------------------------------------------------- second stage: partials in index order
// out[r] = sign * sum_c in[r, c]: a wave per row
static __global__ __launch_bounds__(FP_BLOCK) void fp_row_sum_kernel(const float* __restrict__ in, int nrow, int ncol, float sign,
                                                                      float* __restrict__ out) {
    const int r = blockIdx.x * (FP_BLOCK / MDG_WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= nrow) return;
    float s = 0.f;
    for (int c = lane; c < ncol; c += MDG_WAVE) s += in[(size_t)r * ncol + c];
    s = wave_sum(s);
    if (lane == 0) out[r] = sign * s;
}

// out[k] = sum_r in[r, k]: a workgroup per column
static __global__ __launch_bounds__(FP_BLOCK) void fp_col_sum_kernel(const float* __restrict__ in, long long nrow, int K,
                                                                      float* __restrict__ out) {
    __shared__ float red[16];
    const int k = blockIdx.x;
    float s = 0.f;
    for (long long r = threadIdx.x; r < nrow; r += FP_BLOCK) s += in[r * K + k];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[k] = s;
}

// ---------------------------------------------------------------------------------- host side
inline int tile_blocks(int n_atoms) { return (n_atoms + FP_TILE - 1) / FP_TILE; }
inline int tile_count(int n_atoms) { const int nb = tile_blocks(n_atoms); return nb * (nb / 2 + 1); }
// rows of the [rows, K] parameter partials of a sweep
inline long long theta_rows(int n_frames, int n_atoms, int mode) {
    if (n_atoms <= FP_GROUP_ATOMS) return n_frames;
    return (long long)n_frames * (mode == FP_ROWS ? tile_blocks(n_atoms) : tile_count(n_atoms));
}

// floats of the workspace: the forward's tile partials or the parameter partials of the widest backward sweep the caller has
// (bwd_mode = FP_THETA when it has the parameters-only route, FP_ROWS otherwise)
inline int64_t workspace(int n_frames, int n_atoms, int n_theta_total, int bwd_mode) {
    if (n_frames <= 0 || n_atoms <= 0) return 1;
    const long long fwd = n_atoms > FP_GROUP_ATOMS ? (long long)n_frames * tile_count(n_atoms) : 0;
    const long long bwd = theta_rows(n_frames, n_atoms, bwd_mode) * (n_theta_total > 0 ? n_theta_total : 0);
    const long long n = fwd > bwd ? fwd : bwd;
    return n > 0 ? n : 1;
}

// the checks on the frames that every entry point of a per-frame family states (`who` names it in the messages; `model` = the
// family's own input beside the positions and the cell: terms, table or centres)
inline int check_frames(const char* who, const float* pos, const MdgCell* cell, const void* model, int n_frames, int n_atoms,
                        int max_atoms) {
    MDG_CHECK_ARG(pos && cell && model, "%s: null argument", who);
    MDG_CHECK_ARG(n_frames > 0 && n_atoms > 0, "%s: empty trajectory", who);
    MDG_CHECK_ARG(n_atoms <= max_atoms, "%s: at most %d atoms per frame, got %d", who, max_atoms, n_atoms);
    MDG_CHECK_ARG(cell->diag, "%s: the cell must be diagonal (triclinic cells are not supported)", who);
    return MDG_OK;
}

// the limit on the frames of one call of K15, K31 and K33
inline int check_frame_count(const char* who, int n_frames) {
    MDG_CHECK_ARG(n_frames < (1 << 24), "%s: fewer than 2^24 frames in one call (chunk the frames)", who);
    return MDG_OK;
}

// the checks of the built-in pair terms, and the argument block
inline int make_args(const char* who, FpArgs& A, const float* pos, int n_frames, int n_atoms, const MdgCell* cell,
                     const MdgTerms* terms, const float* theta) {
    int rc = check_frames(who, pos, cell, terms, n_frames, n_atoms, FP_MAX_ATOMS);
    if (rc == MDG_OK) rc = check_frame_count(who, n_frames);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(terms->n_terms >= 1 && terms->n_terms <= MDG_MAX_TERMS, "%s: 1..%d pair terms, got %d", who, MDG_MAX_TERMS,
                  terms->n_terms);
    int off = 0;
    for (int m = 0; m < terms->n_terms; ++m) {
        const MdgPairTerm& t = terms->t[m];
        MDG_CHECK_ARG(t.kind >= MDG_PAIR_LJ && t.kind <= MDG_PAIR_YUKAWA,
                      "%s: term %d is not a built-in pair form (LJ family, Morse, Buckingham, Yukawa)", who, m);
        MDG_CHECK_ARG(t.n_theta == kind_ntheta(t.kind) && t.theta_off == off,
                      "%s: term %d must hold its form's %d parameters at offset %d of theta", who, m, kind_ntheta(t.kind), off);
        MDG_CHECK_ARG(t.cutoff > 0.f, "%s: term %d has no positive cutoff", who, m);
        MDG_CHECK_ARG(t.kind != MDG_PAIR_LJ || (t.p >= 0 && t.q >= 0), "%s: term %d has negative LJ powers", who, m);
        off += t.n_theta;
    }
    MDG_CHECK_ARG(off == terms->n_theta_total, "%s: n_theta_total = %d, the terms hold %d parameters", who, terms->n_theta_total, off);
    MDG_CHECK_ARG(off == 0 || theta, "%s: theta is null", who);
    A.pos = pos; A.theta = theta; A.g = nullptr; A.out = nullptr; A.g_pos = nullptr; A.partial = nullptr;
    A.F = n_frames; A.N = n_atoms; A.K = off;
    A.cell = *cell; A.terms = *terms;
    return MDG_OK;
}

// out[F] = SIGN * sum over the pairs of every frame (A.out and A.partial set)
template <class V>
inline int launch_value(const char* who, const FpArgs& A, hipStream_t st) {
    if (A.N <= FP_WAVE_ATOMS) {
        constexpr int FPB = FP_BLOCK / MDG_WAVE;
        hipLaunchKernelGGL((fp_frame_kernel<V, MDG_WAVE, FP_VALUE>), dim3((A.F + FPB - 1) / FPB), dim3(FP_BLOCK), 0, st, A);
    } else if (A.N <= FP_GROUP_ATOMS) {
        hipLaunchKernelGGL((fp_frame_kernel<V, FP_BLOCK, FP_VALUE>), dim3(A.F), dim3(FP_BLOCK), 0, st, A);
    } else {
        const int nt = tile_count(A.N);
        hipLaunchKernelGGL((fp_tile_once_kernel<V, FP_VALUE>), dim3(A.F, nt), dim3(FP_BLOCK), 0, st, A, tile_blocks(A.N));
        MDG_CHECK_LAUNCH(who);
        constexpr int RPB = FP_BLOCK / MDG_WAVE;
        hipLaunchKernelGGL(fp_row_sum_kernel, dim3((A.F + RPB - 1) / RPB), dim3(FP_BLOCK), 0, st, A.partial, A.F, nt, V::SIGN, A.out);
    }
    MDG_CHECK_LAUNCH(who);
    return MDG_OK;
}

// the gradient of sum_f g[f] out[f] by the sweep MODE: FP_ROWS (A.g_pos set) or the once-per-pair parameter sweep FP_THETA
// (A.g and A.partial set; g_theta [K], null when K == 0 or not wanted)
template <class V, int MODE>
inline int launch_grad(const char* who, const FpArgs& A, float* g_theta, hipStream_t st) {
    static_assert(MODE == FP_ROWS || MODE == FP_THETA, "a gradient sweep");
    if (MODE == FP_THETA && (A.K == 0 || !g_theta)) return MDG_OK;          // nothing to compute
    if (A.N <= FP_WAVE_ATOMS) {
        constexpr int FPB = FP_BLOCK / MDG_WAVE;
        hipLaunchKernelGGL((fp_frame_kernel<V, MDG_WAVE, MODE>), dim3((A.F + FPB - 1) / FPB), dim3(FP_BLOCK), 0, st, A);
    } else if (A.N <= FP_GROUP_ATOMS) {
        hipLaunchKernelGGL((fp_frame_kernel<V, FP_BLOCK, MODE>), dim3(A.F), dim3(FP_BLOCK), 0, st, A);
    } else {
        const int nb = tile_blocks(A.N);
        if constexpr (MODE == FP_ROWS) hipLaunchKernelGGL((fp_tile_rows_kernel<V>), dim3(A.F, nb), dim3(FP_BLOCK), 0, st, A, nb);
        else hipLaunchKernelGGL((fp_tile_once_kernel<V, FP_THETA>), dim3(A.F, tile_count(A.N)), dim3(FP_BLOCK), 0, st, A, nb);
    }
    MDG_CHECK_LAUNCH(who);
    if (A.K > 0 && g_theta) {
        hipLaunchKernelGGL(fp_col_sum_kernel, dim3(A.K), dim3(FP_BLOCK), 0, st, A.partial, theta_rows(A.F, A.N, MODE), A.K, g_theta);
        MDG_CHECK_LAUNCH(who);
    }
    return MDG_OK;
}

}  // namespace frame_pairs
