// K15: pair virial of every frame of a trajectory, and its gradient -- the configurational part of the pressure observable
// (mdgrad_amd/thermo.py Pressure; the reference's torchmd/thermo.py:17-54 does not run).
//
//   W[f] = - sum_terms sum_pairs r phi'(r)            P = (sum_i m_i |v_i|^2 + W) / (dim V)
//
// Pair set of a term = the one PairPotentials sums the energy over (torchmd/topology.py:30-73, interface.py:298-300):
// pairs i < j, D = x_j - x_i re-imaged with the reference's strict +-1/2 minimum image on the diagonal cell,
// 0 < d^2 < cutoff^2 with the un-contracted d^2 of the list builders (csrc/nbr.hip), the term's [N, N] selection mask,
// every term its own cutoff.  The test is odd in D bit for bit, so a pair is in or out whichever end visits it.
//
// List-free: the headline shape is 10^5-10^6 frames of ~100 atoms, where a neighbour list over 10^8 atoms costs more than
// the all-pairs sweep, and at a few thousand atoms the sweep with its early distance test is still a few milliseconds for
// hundreds of frames.  Three shapes by frame size, positions staged in LDS in all of them:
//   N <= 128     a wave per frame, four frames per workgroup
//   N <= 1024    a workgroup per frame
//   larger       (i-block, j-block) tiles of 256 x 256 atoms
// Forward: every pair once.  Within a frame (or across the blocks of a tiled frame) row i takes the partners
// (i + k) mod N, k = 1 .. (N - 1) / 2 (for even N also k = N / 2 on the first half of the rows): every unordered pair once and
// the same work for every lane.
// Backward: full rows -- atom i sums over every j, so each pair is evaluated from both ends and nothing is accumulated
// across lanes; the parameter gradient takes half of each visit.
//   dW/dx_i = sum_j (phi' + r phi'') D / r          dW/dtheta = - sum_pairs r dphi'/dtheta
// Every sum runs in a fixed order: per lane, then the shuffle / LDS trees of common.hpp, then per-frame (per-tile) partials
// added by a second tiny kernel in index order.  No floating-point atomics: two launches give the same bits.
// The functional form is dispatched once per term around the whole sweep (evaluation and accumulation), so PairOut's
// parameter slots stay in registers (see pair_ell_kernel).
#include <type_traits>
#include "common.hpp"

namespace {

constexpr int VIR_BLOCK = 256;
constexpr int VIR_WAVE_ATOMS = 128;      // up to here a wave per frame
constexpr int VIR_GROUP_ATOMS = 1024;    // up to here a workgroup per frame
constexpr int VIR_TILE = 256;            // beyond: tiles of VIR_TILE x VIR_TILE atoms
constexpr int VIR_MAX_ATOMS = 32768;

struct VirArgs {
    const float* pos;        // [F, N, 3]
    const float* theta;
    const float* gW;         // backward: [F]
    float* W;                // forward:  [F]
    float* g_pos;            // backward: [F, N, 3]
    float* partial;          // tiled forward: [F, tiles];  backward: [rows, K] (rows = F, tiled F * blocks)
    int F, N, K;
    MdgCell cell;
    MdgTerms terms;
};

struct Acc {
    float w;                         // forward:  sum r phi'
    float gx, gy, gz;                // backward: sum (phi' + r phi'') D / r of one atom
    float th[MDG_MAX_THETA];         //           sum r dphi'/dtheta over the visits of this lane
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

template <int KIND, bool BWD>
__device__ __forceinline__ void visit(const TermConst& tc, float dx, float dy, float dz, float d2, Acc& a) {
    PairOut o{};
    float r, ir;
    pair_eval<BWD ? 2 : 1, KIND>(tc, d2, r, ir, o);
    if (!BWD) {
        a.w = fmaf(r, o.du, a.w);
    } else {
        const float c = fmaf(r, o.d2u, o.du) * ir;
        a.gx = fmaf(c, dx, a.gx); a.gy = fmaf(c, dy, a.gy); a.gz = fmaf(c, dz, a.gz);
#pragma unroll
        for (int t = 0; t < form_ntheta(KIND); ++t) a.th[t] = fmaf(r, o.ddu_dth[t], a.th[t]);
    }
}

// dL/dx of one atom for one term: the first term of a frame writes, the others add (one thread owns the atom throughout)
__device__ __forceinline__ void put_grad(float* g, const Acc& a, float gw, bool first) {
    if (first) { g[0] = gw * a.gx; g[1] = gw * a.gy; g[2] = gw * a.gz; }
    else { g[0] = fmaf(gw, a.gx, g[0]); g[1] = fmaf(gw, a.gy, g[1]); g[2] = fmaf(gw, a.gz, g[2]); }
}

// ---------------------------------------------------------------------------------- whole frame in LDS (N <= 1024)
// TPF threads share a frame: lane t of them owns the atoms t, t + TPF, ...; sx / sy / sz = the frame, one array per component
template <int KIND, int TPF>
__device__ __forceinline__ void frame_fwd(const VirArgs& A, const TermConst& tc, const uint8_t* mask, const float* sx,
                                          const float* sy, const float* sz, int t, Acc& a) {
    const int N = A.N, half = (N - 1) >> 1;
    for (int i = t; i < N; i += TPF) {
        const float xi = sx[i], yi = sy[i], zi = sz[i];
        const int kmax = half + ((!(N & 1) && i < (N >> 1)) ? 1 : 0);
        for (int k = 1; k <= kmax; ++k) {
            int j = i + k;
            if (j >= N) j -= N;
            if (mask && !mask[(size_t)i * N + j]) continue;
            float dx = sx[j] - xi, dy = sy[j] - yi, dz = sz[j] - zi, d2;
            if (!pair_in(A.cell, tc.rc2, dx, dy, dz, d2)) continue;
            visit<KIND, false>(tc, dx, dy, dz, d2, a);
        }
    }
}

template <int KIND, int TPF>
__device__ __forceinline__ void frame_bwd(const VirArgs& A, const TermConst& tc, const uint8_t* mask, const float* sx,
                                          const float* sy, const float* sz, int t, long long f, float gw, bool first, Acc& a) {
    const int N = A.N;
    for (int i = t; i < N; i += TPF) {
        const float xi = sx[i], yi = sy[i], zi = sz[i];
        a.gx = a.gy = a.gz = 0.f;
        for (int k = 1; k < N; ++k) {
            int j = i + k;
            if (j >= N) j -= N;
            if (mask && !mask[(size_t)i * N + j]) continue;
            float dx = sx[j] - xi, dy = sy[j] - yi, dz = sz[j] - zi, d2;
            if (!pair_in(A.cell, tc.rc2, dx, dy, dz, d2)) continue;
            visit<KIND, true>(tc, dx, dy, dz, d2, a);
        }
        put_grad(A.g_pos + ((size_t)f * N + i) * 3, a, gw, first);
    }
}

template <int TPF, bool BWD>
__global__ __launch_bounds__(VIR_BLOCK) void virial_frame_kernel(const VirArgs A) {
    constexpr int CAP = TPF == MDG_WAVE ? VIR_WAVE_ATOMS : VIR_GROUP_ATOMS, FPB = VIR_BLOCK / TPF;
    static_assert(TPF == MDG_WAVE || TPF == VIR_BLOCK, "a wave or the whole workgroup per frame");
    __shared__ float sp[FPB * 3 * CAP];
    __shared__ float red[16];
    const int t = threadIdx.x % TPF, g = threadIdx.x / TPF, N = A.N;
    const long long f = (long long)blockIdx.x * FPB + g;
    const bool live = f < A.F;
    float* sx = sp + g * 3 * CAP;
    float* sy = sx + CAP;
    float* sz = sy + CAP;
    if (live) {
        const float* p = A.pos + (size_t)f * N * 3;
        for (int e = t; e < 3 * N; e += TPF) sp[g * 3 * CAP + (e % 3) * CAP + e / 3] = p[e];
    }
    __syncthreads();
    const float gw = (BWD && live) ? A.gW[f] : 0.f;
    float w = 0.f;
    for (int m = 0; m < A.terms.n_terms; ++m) {
        const MdgPairTerm& term = A.terms.t[m];
        const TermConst tc = term_prepare(term, A.theta);
        with_form(tc, [&](auto form) {
            constexpr int KIND = decltype(form)::value;
            Acc a{};
            if (live) {
                if (BWD) frame_bwd<KIND, TPF>(A, tc, term.mask, sx, sy, sz, t, f, gw, m == 0, a);
                else frame_fwd<KIND, TPF>(A, tc, term.mask, sx, sy, sz, t, a);
            }
            w += a.w;
            if constexpr (BWD && form_ntheta(KIND) > 0) {
                // (each pair was visited from both ends: half of each visit)
                if constexpr (TPF == MDG_WAVE) {
#pragma unroll
                    for (int k = 0; k < form_ntheta(KIND); ++k) a.th[k] = wave_sum(a.th[k]);
                } else {
                    block_sum_n<MDG_MAX_THETA>(a.th, red);
                }
                if (live && t == 0) {
#pragma unroll
                    for (int k = 0; k < form_ntheta(KIND); ++k)
                        A.partial[(size_t)f * A.K + term.theta_off + k] = -0.5f * gw * a.th[k];
                }
            }
        });
    }
    if (!BWD) {
        w = TPF == MDG_WAVE ? wave_sum(w) : block_sum(w, red);
        if (live && t == 0) A.W[f] = 0.f - w;
    }
}

// ---------------------------------------------------------------------------------- tiles (N > 1024)
// thread-owned atom i against the staged atoms [jlo, nj) of the tile that starts at atom j0 (sj: one array per component)
template <int KIND, bool BWD>
__device__ __forceinline__ void tile_rows(const MdgCell& cell, const TermConst& tc, const uint8_t* mrow, const float* sj, int j0,
                                          int jlo, int nj, float xi, float yi, float zi, Acc& a) {
    for (int jj = jlo; jj < nj; ++jj) {
        if (mrow && !mrow[j0 + jj]) continue;
        float dx = sj[jj] - xi, dy = sj[VIR_TILE + jj] - yi, dz = sj[2 * VIR_TILE + jj] - zi, d2;
        if (!pair_in(cell, tc.rc2, dx, dy, dz, d2)) continue;
        visit<KIND, BWD>(tc, dx, dy, dz, d2, a);
    }
}

__device__ __forceinline__ void stage_tile(float* sj, const float* p, int j0, int nj) {
    for (int e = threadIdx.x; e < 3 * nj; e += VIR_BLOCK) sj[(e % 3) * VIR_TILE + e / 3] = p[3 * (size_t)j0 + e];
}

// grid (F, nb * (nb / 2 + 1)): tile id = ib + nb * k pairs the i-block ib with the j-block (ib + k) mod nb; k = 0 is the
// diagonal tile (j > i), and for even nb the shell k = nb / 2 belongs to the first half of the i-blocks
__global__ __launch_bounds__(VIR_BLOCK) void virial_tile_fwd_kernel(const VirArgs A, int nb) {
    __shared__ float sj[3 * VIR_TILE];
    __shared__ float red[16];
    const int f = blockIdx.x, id = blockIdx.y, ib = id % nb, k = id / nb, t = threadIdx.x, N = A.N;
    float w = 0.f;
    if ((nb & 1) || k != (nb >> 1) || ib < (nb >> 1)) {
        int jb = ib + k;
        if (jb >= nb) jb -= nb;
        const float* p = A.pos + (size_t)f * N * 3;
        const int i = ib * VIR_TILE + t, j0 = jb * VIR_TILE, nj = min(VIR_TILE, N - j0);
        stage_tile(sj, p, j0, nj);
        __syncthreads();
        if (i < N) {
            const float xi = p[3 * i], yi = p[3 * i + 1], zi = p[3 * i + 2];
            for (int m = 0; m < A.terms.n_terms; ++m) {
                const MdgPairTerm& term = A.terms.t[m];
                const TermConst tc = term_prepare(term, A.theta);
                const uint8_t* mrow = term.mask ? term.mask + (size_t)i * N : nullptr;
                with_form(tc, [&](auto form) {
                    Acc a{};
                    tile_rows<decltype(form)::value, false>(A.cell, tc, mrow, sj, j0, k == 0 ? t + 1 : 0, nj, xi, yi, zi, a);
                    w += a.w;
                });
            }
        }
    }
    w = block_sum(w, red);
    if (t == 0) A.partial[(size_t)f * gridDim.y + id] = w;
}

// grid (F, nb): the i-block against every j-block
__global__ __launch_bounds__(VIR_BLOCK) void virial_tile_bwd_kernel(const VirArgs A, int nb) {
    __shared__ float sj[3 * VIR_TILE];
    __shared__ float red[16];
    const int f = blockIdx.x, ib = blockIdx.y, t = threadIdx.x, N = A.N;
    const float* p = A.pos + (size_t)f * N * 3;
    const int i = ib * VIR_TILE + t;
    const bool live = i < N;
    const float xi = live ? p[3 * i] : 0.f, yi = live ? p[3 * i + 1] : 0.f, zi = live ? p[3 * i + 2] : 0.f;
    const float gw = A.gW[f];
    for (int m = 0; m < A.terms.n_terms; ++m) {
        const MdgPairTerm& term = A.terms.t[m];
        const TermConst tc = term_prepare(term, A.theta);
        const uint8_t* mrow = (term.mask && live) ? term.mask + (size_t)i * N : nullptr;
        with_form(tc, [&](auto form) {
            constexpr int KIND = decltype(form)::value;
            Acc a{};
            for (int jb = 0; jb < nb; ++jb) {
                const int j0 = jb * VIR_TILE, nj = min(VIR_TILE, N - j0);
                __syncthreads();                       // the previous tile has been read
                stage_tile(sj, p, j0, nj);
                __syncthreads();
                if (live) tile_rows<KIND, true>(A.cell, tc, mrow, sj, j0, 0, nj, xi, yi, zi, a);
            }
            if (live) put_grad(A.g_pos + ((size_t)f * N + i) * 3, a, gw, m == 0);
            if constexpr (form_ntheta(KIND) > 0) {
                block_sum_n<MDG_MAX_THETA>(a.th, red);
                if (t == 0) {
#pragma unroll
                    for (int k = 0; k < form_ntheta(KIND); ++k)
                        A.partial[((size_t)f * nb + ib) * A.K + term.theta_off + k] = -0.5f * gw * a.th[k];
                }
            }
        });
    }
}

// ---------------------------------------------------------------------------------- second stage: partials in index order
// out[r] = - sum_c in[r, c]: a wave per row
__global__ __launch_bounds__(VIR_BLOCK) void virial_row_sum_kernel(const float* __restrict__ in, int nrow, int ncol,
                                                                   float* __restrict__ out) {
    const int r = blockIdx.x * (VIR_BLOCK / MDG_WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= nrow) return;
    float s = 0.f;
    for (int c = lane; c < ncol; c += MDG_WAVE) s += in[(size_t)r * ncol + c];
    s = wave_sum(s);
    if (lane == 0) out[r] = 0.f - s;
}

// out[k] = sum_r in[r, k]: a workgroup per column
__global__ __launch_bounds__(VIR_BLOCK) void virial_col_sum_kernel(const float* __restrict__ in, long long nrow, int K,
                                                                   float* __restrict__ out) {
    __shared__ float red[16];
    const int k = blockIdx.x;
    float s = 0.f;
    for (long long r = threadIdx.x; r < nrow; r += VIR_BLOCK) s += in[r * K + k];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[k] = s;
}

int tile_blocks(int n_atoms) { return (n_atoms + VIR_TILE - 1) / VIR_TILE; }
int tile_count(int n_atoms) { const int nb = tile_blocks(n_atoms); return nb * (nb / 2 + 1); }
long long bwd_rows(int n_frames, int n_atoms) {
    return n_atoms > VIR_GROUP_ATOMS ? (long long)n_frames * tile_blocks(n_atoms) : n_frames;
}

int vir_args(VirArgs& A, const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const MdgTerms* terms,
             const float* theta) {
    MDG_CHECK_ARG(pos && cell && terms, "virial: null argument");
    MDG_CHECK_ARG(n_frames > 0 && n_atoms > 0, "virial: empty trajectory");
    MDG_CHECK_ARG(n_atoms <= VIR_MAX_ATOMS, "virial: at most %d atoms per frame, got %d", VIR_MAX_ATOMS, n_atoms);
    MDG_CHECK_ARG(n_frames < (1 << 24), "virial: fewer than 2^24 frames in one call (chunk the frames)");
    MDG_CHECK_ARG(cell->diag, "virial: the cell must be diagonal (triclinic cells are not supported)");
    MDG_CHECK_ARG(terms->n_terms >= 1 && terms->n_terms <= MDG_MAX_TERMS, "virial: 1..%d pair terms, got %d", MDG_MAX_TERMS,
                  terms->n_terms);
    int off = 0;
    for (int m = 0; m < terms->n_terms; ++m) {
        const MdgPairTerm& t = terms->t[m];
        MDG_CHECK_ARG(t.kind >= MDG_PAIR_LJ && t.kind <= MDG_PAIR_YUKAWA,
                      "virial: term %d is not a built-in pair form (LJ family, Morse, Buckingham, Yukawa)", m);
        MDG_CHECK_ARG(t.n_theta == kind_ntheta(t.kind) && t.theta_off == off,
                      "virial: term %d must hold its form's %d parameters at offset %d of theta", m, kind_ntheta(t.kind), off);
        MDG_CHECK_ARG(t.cutoff > 0.f, "virial: term %d has no positive cutoff", m);
        MDG_CHECK_ARG(t.kind != MDG_PAIR_LJ || (t.p >= 0 && t.q >= 0), "virial: term %d has negative LJ powers", m);
        off += t.n_theta;
    }
    MDG_CHECK_ARG(off == terms->n_theta_total, "virial: n_theta_total = %d, the terms hold %d parameters", terms->n_theta_total, off);
    MDG_CHECK_ARG(off == 0 || theta, "virial: theta is null");
    A.pos = pos; A.theta = theta; A.gW = nullptr; A.W = nullptr; A.g_pos = nullptr; A.partial = nullptr;
    A.F = n_frames; A.N = n_atoms; A.K = off;
    A.cell = *cell; A.terms = *terms;
    return MDG_OK;
}

}  // namespace

extern "C" int64_t mdg_virial_workspace(int n_frames, int n_atoms, int n_theta_total) {
    if (n_frames <= 0 || n_atoms <= 0) return 1;
    const long long fwd = n_atoms > VIR_GROUP_ATOMS ? (long long)n_frames * tile_count(n_atoms) : 0;
    const long long bwd = bwd_rows(n_frames, n_atoms) * (n_theta_total > 0 ? n_theta_total : 0);
    const long long n = fwd > bwd ? fwd : bwd;
    return n > 0 ? n : 1;
}

extern "C" int mdg_virial_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const MdgTerms* terms,
                              const float* theta, float* W, float* workspace, void* stream) {
    VirArgs A;
    const int rc = vir_args(A, pos, n_frames, n_atoms, cell, terms, theta);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(W && workspace, "virial_fwd: null output or workspace");
    A.W = W; A.partial = workspace;
    hipStream_t st = (hipStream_t)stream;
    if (n_atoms <= VIR_WAVE_ATOMS) {
        constexpr int FPB = VIR_BLOCK / MDG_WAVE;
        hipLaunchKernelGGL((virial_frame_kernel<MDG_WAVE, false>), dim3((n_frames + FPB - 1) / FPB), dim3(VIR_BLOCK), 0, st, A);
    } else if (n_atoms <= VIR_GROUP_ATOMS) {
        hipLaunchKernelGGL((virial_frame_kernel<VIR_BLOCK, false>), dim3(n_frames), dim3(VIR_BLOCK), 0, st, A);
    } else {
        const int nt = tile_count(n_atoms);
        hipLaunchKernelGGL(virial_tile_fwd_kernel, dim3(n_frames, nt), dim3(VIR_BLOCK), 0, st, A, tile_blocks(n_atoms));
        MDG_CHECK_LAUNCH("virial_tile_fwd_kernel");
        constexpr int RPB = VIR_BLOCK / MDG_WAVE;
        hipLaunchKernelGGL(virial_row_sum_kernel, dim3((n_frames + RPB - 1) / RPB), dim3(VIR_BLOCK), 0, st, workspace, n_frames, nt,
                           W);
    }
    MDG_CHECK_LAUNCH("virial_fwd");
    return MDG_OK;
}

extern "C" int mdg_virial_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const MdgTerms* terms,
                              const float* theta, const float* gW, float* g_pos, float* g_theta, float* workspace, void* stream) {
    VirArgs A;
    const int rc = vir_args(A, pos, n_frames, n_atoms, cell, terms, theta);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(gW && g_pos && workspace, "virial_bwd: null gW, g_pos or workspace");
    MDG_CHECK_ARG(A.K == 0 || g_theta, "virial_bwd: g_theta is null");
    A.gW = gW; A.g_pos = g_pos; A.partial = workspace;
    hipStream_t st = (hipStream_t)stream;
    if (n_atoms <= VIR_WAVE_ATOMS) {
        constexpr int FPB = VIR_BLOCK / MDG_WAVE;
        hipLaunchKernelGGL((virial_frame_kernel<MDG_WAVE, true>), dim3((n_frames + FPB - 1) / FPB), dim3(VIR_BLOCK), 0, st, A);
    } else if (n_atoms <= VIR_GROUP_ATOMS) {
        hipLaunchKernelGGL((virial_frame_kernel<VIR_BLOCK, true>), dim3(n_frames), dim3(VIR_BLOCK), 0, st, A);
    } else {
        hipLaunchKernelGGL(virial_tile_bwd_kernel, dim3(n_frames, tile_blocks(n_atoms)), dim3(VIR_BLOCK), 0, st, A,
                           tile_blocks(n_atoms));
    }
    MDG_CHECK_LAUNCH("virial_bwd");
    if (A.K > 0) {
        hipLaunchKernelGGL(virial_col_sum_kernel, dim3(A.K), dim3(VIR_BLOCK), 0, st, workspace, bwd_rows(n_frames, n_atoms), A.K,
                           g_theta);
        MDG_CHECK_LAUNCH("virial_col_sum_kernel");
    }
    return MDG_OK;
}
