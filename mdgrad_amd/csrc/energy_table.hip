// K33: tabulated pair energy of every frame of a trajectory, and its gradient -- thermo.TabulatedEnergy, the energy side of
// trajectory reweighting (mdgrad_amd/reweight.py) for learned pair potentials (pairMLP ...), whose energy K31 refuses.
//
//   U[f] = sum_pairs phi~(d^2)
//
// phi~ = the cubic-Hermite interpolant of ONE table on the uniform grid u_g = u0 + g du, g = 0 .. p - 1, in u = r^2, with
// u_{p-1} = cutoff^2 and node entries (phi_g, du dphi/du_g) packed as [2 p] floats: the layout, the grid arithmetic and the
// four basis values of pair_eval's MDG_PAIR_TABLE case (common.hpp), applied to the energy.  A pair below the first node
// (d^2 < u0) takes the constant n_0.x: no position gradient, its whole node gradient into n_0.x, and it is counted once in the
// device word n_below by the forward pass.
//
// Pair set, the three shapes by frame size (a wave per frame up to 128 atoms, a workgroup per frame up to 1 024, tiles of
// 256 x 256 atoms up to 32 768) and the fixed-order sums of U are those of csrc/frame_pairs.hpp; positions AND the table are
// staged in LDS (the lookups are random gathers).  The sweeps themselves are written out here, not put on that header's
// pair walk (says why).  Three sweeps:
//   ET_VALUE    U[f], every unordered pair once
//   ET_NODES    (frames detached: the reweighting case) gT[2 p] = sum_f gU[f] sum_pairs basis, once per pair, no position written
//   ET_ROWS     full rows: dL/dx_i = -gU[f] sum_j 2 (dphi~/du) D (D = x_j - x_i), the exact derivative of the interpolant; the
//               node gradient, when wanted too, takes half of each of a pair's two visits
// Node gradient: a scatter into 2 p words, as csrc/eam_table.hip does it -- fx64 fixed point (common.hpp) into int64 LDS words
// with integer atomics, the non-zero words flushed with 64-bit integer atomics into a zeroed [2 p] global buffer, a final
// kernel turns the words into floats.  The power-of-two scale is taken on the device (etab_prepare_kernel) from max |gU| and
// the number of contributions a word can receive, F N (N - 1) (both visits of the full rows, each entered at full weight and
// halved by the final kernel, so both sweeps add the same integers per pair): every |basis| <= 1, so no word can leave int64.
// No host read, no floating-point atomics: two launches give the same bits, and so does any order of the frames.
//
// LDS (derived, not measured): a frame of <= 1 024 atoms 12 KB, the table <= 32 KB, the gradient words <= 64 KB: <= 108 KB of the
// 160 KiB of a CU.  docs/KERNELS.md K33.
#include "frame_pairs.hpp"

namespace {

using namespace frame_pairs;

constexpr int ET_VALUE = 0, ET_NODES = 1, ET_ROWS = 2;
constexpr int ET_MIN_NODES = 4, ET_MAX_NODES = 4096;
constexpr int ET_GRID_CAP = 512;           // workgroups of the whole-frame shapes: each walks its share of the frame groups
constexpr int ET_HEAD = 4;                 // floats in front of the workspace's words: [0] = the fixed-point scale

struct TabArgs {
    const float* pos;            // [F, N, 3]
    const float* tab;            // [2 p]
    const float* g;              // ET_NODES, ET_ROWS: upstream gradient [F]
    const uint8_t* mask;         // nullable [N, N]
    float* out;                  // ET_VALUE: [F]
    float* g_pos;                // ET_ROWS: [F, N, 3]
    float* partial;              // tiled ET_VALUE: [F, tiles]
    unsigned long long* words;   // [2 p] fixed-point node gradient (zeroed by etab_prepare_kernel); null: not wanted
    const float* scale;          // device: the power-of-two scale of the words
    unsigned int* below;         // ET_VALUE: pairs with d^2 < u0
    int F, N, p;
    float u0, inv_du, pm1, rc2;
    MdgCell cell;
};

struct TabAcc {
    float w;                     // ET_VALUE: sum of phi~
    float gx, gy, gz;            // ET_ROWS: sum c D of one atom
    int nb;                      // ET_VALUE: pairs below the first node
};

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one pair: st = the table in LDS, sw = this workgroup's gradient words in LDS (null: none), gs = gU[f] * scale
template <int MODE>
__device__ __forceinline__ void tab_visit(const TabArgs& A, const float* st, unsigned long long* sw, float gs, float dx, float dy,
                                          float dz, float d2, TabAcc& a) {
    // (grid coordinate clamped to the nodes [0, p - 1], cell index to the last cell: no index leaves the table)
    const float tt = fminf(fmaxf((d2 - A.u0) * A.inv_du, 0.f), A.pm1);
    const int g = min((int)tt, A.p - 2);
    const float fr = tt - (float)g;
    const float2 n0 = *reinterpret_cast<const float2*>(st + 2 * g);
    const float2 n1 = *reinterpret_cast<const float2*>(st + 2 * g + 2);
    const float om = 1.f - fr, fr2 = fr * fr, om2 = om * om;
    const float b0 = (1.f + 2.f * fr) * om2, b1 = fr * om2, b2 = fr2 * (3.f - 2.f * fr), b3 = fr2 * (fr - 1.f);
    const bool below = d2 < A.u0;                    // (tt = 0 there: b = (1, 0, 0, 0), the constant n_0.x)
    if (MODE == ET_VALUE) {
        a.w += b0 * n0.x + b1 * n0.y + b2 * n1.x + b3 * n1.y;
        a.nb += below ? 1 : 0;
    } else {
        if (MODE == ET_ROWS) {
            const float pu = (6.f * fr * (fr - 1.f) * (n0.x - n1.x) + ((3.f * fr - 4.f) * fr + 1.f) * n0.y +
                              (3.f * fr - 2.f) * fr * n1.y) * A.inv_du;
            const float c = below ? 0.f : -2.f * pu;
            a.gx = fmaf(c, dx, a.gx); a.gy = fmaf(c, dy, a.gy); a.gz = fmaf(c, dz, a.gz);
        }
        if (sw) {
            const float v0 = gs * b0, v1 = gs * b1, v2 = gs * b2, v3 = gs * b3;
            unsigned long long* w = sw + 2 * g;
            if (v0 != 0.f) atomicAdd(w, fx64(v0));
            if (v1 != 0.f) atomicAdd(w + 1, fx64(v1));
            if (v2 != 0.f) atomicAdd(w + 2, fx64(v2));
            if (v3 != 0.f) atomicAdd(w + 3, fx64(v3));
        }
    }
}

// the dynamic LDS of every kernel here: [gradient words (2 p, when wanted)] [table (2 p floats)] [positions]
struct TabLds { unsigned long long* sw; float* st; float* sp; };

extern __shared__ unsigned long long etab_lds[];

template <int MODE>
__device__ __forceinline__ TabLds tab_lds_open(const TabArgs& A) {
    const bool nodes = MODE != ET_VALUE && A.words != nullptr;
    const int nw = nodes ? 2 * A.p : 0;
    TabLds L;
    L.sw = nodes ? etab_lds : nullptr;
    L.st = reinterpret_cast<float*>(etab_lds + nw);
    L.sp = L.st + 2 * A.p;
    for (int k = threadIdx.x; k < 2 * A.p; k += FP_BLOCK) L.st[k] = A.tab[k];
    for (int k = threadIdx.x; k < nw; k += FP_BLOCK) L.sw[k] = 0ull;
    return L;                                        // (the caller's next barrier publishes both)
}

// the words this workgroup touched, one integer atomic each
__device__ __forceinline__ void tab_lds_flush(const TabArgs& A, const TabLds& L) {
    if (!L.sw) return;                               // (block-uniform)
    __syncthreads();
    for (int k = threadIdx.x; k < 2 * A.p; k += FP_BLOCK) {
        const unsigned long long v = L.sw[k];
        if (v != 0ull) atomicAdd(A.words + k, v);
    }
}

__device__ __forceinline__ void tab_count_below(const TabArgs& A, int nb) {
    nb = wave_sum_int(nb);
    if ((threadIdx.x & 63) == 0 && nb > 0) atomicAdd(A.below, (unsigned int)nb);
}

// ---------------------------------------------------------------------------------- whole frame in LDS (N <= 1024)
// TPF threads share a frame (frame_pairs.hpp: lane t owns the atoms t, t + TPF, ...); a workgroup walks the frame groups
// blockIdx.x, blockIdx.x + gridDim.x, ... so the table is staged, and the words flushed, once per workgroup
template <int TPF, int MODE>
__global__ __launch_bounds__(FP_BLOCK) void etab_frame_kernel(const TabArgs A, int ngroups) {
    constexpr int CAP = TPF == MDG_WAVE ? FP_WAVE_ATOMS : FP_GROUP_ATOMS, FPB = FP_BLOCK / TPF;
    static_assert(TPF == MDG_WAVE || TPF == FP_BLOCK, "a wave or the whole workgroup per frame");
    __shared__ float red[17];
    const TabLds L = tab_lds_open<MODE>(A);
    const int t = threadIdx.x % TPF, g = threadIdx.x / TPF, N = A.N, half = (N - 1) >> 1;
    float* sx = L.sp + g * 3 * CAP;
    float* sy = sx + CAP;
    float* sz = sy + CAP;
    const float scale = L.sw ? A.scale[0] : 0.f;
    int nb = 0;
    for (int fg = blockIdx.x; fg < ngroups; fg += gridDim.x) {
        const long long f = (long long)fg * FPB + g;
        const bool live = f < A.F;
        __syncthreads();                             // the previous frames have been read (first pass: nothing yet)
        if (live) {
            const float* p = A.pos + (size_t)f * N * 3;
            for (int e = t; e < 3 * N; e += TPF) L.sp[g * 3 * CAP + (e % 3) * CAP + e / 3] = p[e];
        }
        __syncthreads();
        const float gw = (MODE != ET_VALUE && live) ? A.g[f] : 0.f;
        const float gs = gw * scale;
        TabAcc a{};
        if (live) {
            for (int i = t; i < N; i += TPF) {
                const float xi = sx[i], yi = sy[i], zi = sz[i];
                // once per pair: the partners (i + k) mod N, k = 1 .. (N - 1) / 2, for even N also k = N / 2 on the first half
                const int kmax = MODE == ET_ROWS ? N - 1 : half + ((!(N & 1) && i < (N >> 1)) ? 1 : 0);
                if (MODE == ET_ROWS) a.gx = a.gy = a.gz = 0.f;
                for (int k = 1; k <= kmax; ++k) {
                    int j = i + k;
                    if (j >= N) j -= N;
                    if (A.mask && !A.mask[(size_t)i * N + j]) continue;
                    float dx = sx[j] - xi, dy = sy[j] - yi, dz = sz[j] - zi, d2;
                    if (!pair_in(A.cell, A.rc2, dx, dy, dz, d2)) continue;
                    tab_visit<MODE>(A, L.st, L.sw, gs, dx, dy, dz, d2, a);
                }
                if (MODE == ET_ROWS) {
                    float* o = A.g_pos + ((size_t)f * N + i) * 3;
                    o[0] = gw * a.gx; o[1] = gw * a.gy; o[2] = gw * a.gz;
                }
            }
        }
        if (MODE == ET_VALUE) {
            const float w = TPF == MDG_WAVE ? wave_sum(a.w) : block_sum(a.w, red);
            if (live && t == 0) A.out[f] = w;
            nb += a.nb;
        }
    }
    if (MODE == ET_VALUE) tab_count_below(A, nb);
    tab_lds_flush(A, L);
}

// ---------------------------------------------------------------------------------- tiles (N > 1024)
template <int MODE>
__device__ __forceinline__ void etab_tile_rows(const TabArgs& A, const TabLds& L, const uint8_t* mrow, int j0, int jlo, int nj,
                                               float gs, float xi, float yi, float zi, TabAcc& a) {
    const float* sj = L.sp;
    for (int jj = jlo; jj < nj; ++jj) {
        if (mrow && !mrow[j0 + jj]) continue;
        float dx = sj[jj] - xi, dy = sj[FP_TILE + jj] - yi, dz = sj[2 * FP_TILE + jj] - zi, d2;
        if (!pair_in(A.cell, A.rc2, dx, dy, dz, d2)) continue;
        tab_visit<MODE>(A, L.st, L.sw, gs, dx, dy, dz, d2, a);
    }
}

// grid (F, nb * (nb / 2 + 1)): the tiles of fp_tile_once_kernel.  MODE = ET_VALUE or ET_NODES.
template <int MODE>
__global__ __launch_bounds__(FP_BLOCK) void etab_tile_once_kernel(const TabArgs A, int nb) {
    __shared__ float red[17];
    const TabLds L = tab_lds_open<MODE>(A);
    const int f = blockIdx.x, id = blockIdx.y, ib = id % nb, k = id / nb, t = threadIdx.x, N = A.N;
    const bool tile_on = (nb & 1) || k != (nb >> 1) || ib < (nb >> 1);
    int jb = ib + k;
    if (jb >= nb) jb -= nb;
    const float* p = A.pos + (size_t)f * N * 3;
    const int i = ib * FP_TILE + t, j0 = jb * FP_TILE, nj = min(FP_TILE, N - j0);
    const bool live = tile_on && i < N;
    if (tile_on) stage_tile(L.sp, p, j0, nj);
    __syncthreads();
    const float xi = live ? p[3 * i] : 0.f, yi = live ? p[3 * i + 1] : 0.f, zi = live ? p[3 * i + 2] : 0.f;
    const float gs = (MODE == ET_NODES && L.sw) ? A.g[f] * A.scale[0] : 0.f;
    const uint8_t* mrow = (A.mask && live) ? A.mask + (size_t)i * N : nullptr;
    TabAcc a{};
    if (live) etab_tile_rows<MODE>(A, L, mrow, j0, k == 0 ? t + 1 : 0, nj, gs, xi, yi, zi, a);
    if (MODE == ET_VALUE) {
        const float w = block_sum(a.w, red);
        if (t == 0) A.partial[(size_t)f * gridDim.y + id] = w;
        tab_count_below(A, a.nb);
    }
    tab_lds_flush(A, L);
}

// grid (F, nb): the i-block against every j-block (ET_ROWS)
__global__ __launch_bounds__(FP_BLOCK) void etab_tile_rows_kernel(const TabArgs A, int nb) {
    const TabLds L = tab_lds_open<ET_ROWS>(A);
    const int f = blockIdx.x, ib = blockIdx.y, t = threadIdx.x, N = A.N;
    const float* p = A.pos + (size_t)f * N * 3;
    const int i = ib * FP_TILE + t;
    const bool live = i < N;
    const float xi = live ? p[3 * i] : 0.f, yi = live ? p[3 * i + 1] : 0.f, zi = live ? p[3 * i + 2] : 0.f;
    const float gw = A.g[f];
    const float gs = L.sw ? gw * A.scale[0] : 0.f;
    const uint8_t* mrow = (A.mask && live) ? A.mask + (size_t)i * N : nullptr;
    TabAcc a{};
    for (int jb = 0; jb < nb; ++jb) {
        const int j0 = jb * FP_TILE, nj = min(FP_TILE, N - j0);
        __syncthreads();                             // the previous tile has been read (first pass: table and words are set)
        stage_tile(L.sp, p, j0, nj);
        __syncthreads();
        if (live) etab_tile_rows<ET_ROWS>(A, L, mrow, j0, 0, nj, gs, xi, yi, zi, a);
    }
    if (live) {
        float* o = A.g_pos + ((size_t)f * N + i) * 3;
        o[0] = gw * a.gx; o[1] = gw * a.gy; o[2] = gw * a.gz;
    }
    tab_lds_flush(A, L);
}

// ---------------------------------------------------------------------------------- the fixed-point words: before and after
// one workgroup: zeroes the words and takes the scale, the largest power of two s with s max|gU| <= limit (max|gU| = 0 or not
// finite: s = 1 -- every contribution is then zero, or the result is not finite whatever the scale)
__global__ __launch_bounds__(FP_BLOCK) void etab_prepare_kernel(const float* __restrict__ gU, int F, float limit,
                                                                unsigned long long* words, int nwords, float* scale) {
    __shared__ float red[4];
    for (int k = threadIdx.x; k < nwords; k += FP_BLOCK) words[k] = 0ull;
    float m = 0.f;
    for (int f = threadIdx.x; f < F; f += FP_BLOCK) m = fmaxf(m, fabsf(gU[f]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        float s = 1.f;
        if (m > 0.f && m <= 3.0e38f) {
            int e;
            frexpf(limit / m, &e);                   // limit / m = x 2^e, x in [1/2, 1): 2^(e - 1) <= limit / m
            s = ldexpf(1.f, min(max(e - 1, -120), 120));
        }
        scale[0] = s;
    }
}

__global__ __launch_bounds__(FP_BLOCK) void etab_finish_kernel(const unsigned long long* __restrict__ words, int nwords,
                                                               const float* __restrict__ scale, float weight, float* out) {
    const int k = blockIdx.x * FP_BLOCK + threadIdx.x;
    if (k >= nwords) return;
    out[k] = (float)((double)(long long)words[k] * ((double)weight / (double)scale[0]));     // (powers of two: exact)
}

// ---------------------------------------------------------------------------------- host side
inline size_t lds_bytes(int n_atoms, int p, bool nodes) {
    const size_t pos = n_atoms <= FP_WAVE_ATOMS ? (size_t)(FP_BLOCK / MDG_WAVE) * 3 * FP_WAVE_ATOMS
                                                : (n_atoms <= FP_GROUP_ATOMS ? (size_t)3 * FP_GROUP_ATOMS : (size_t)3 * FP_TILE);
    return (pos + 2 * (size_t)p) * sizeof(float) + (nodes ? 2 * (size_t)p * sizeof(unsigned long long) : 0);
}

// beyond 64 KB of dynamic LDS a kernel's limit has to be raised before the launch
template <class K>
inline int allow_lds(K kernel, size_t bytes) {
    if (bytes > 65536)
        MDG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return MDG_OK;
}

#define ETAB_LAUNCH(kernel, grid, bytes, ...)                                                         \
    do { const int rc_ = allow_lds(kernel, bytes);                                                      \
         if (rc_ != MDG_OK) return rc_;                                                                 \
         hipLaunchKernelGGL(kernel, grid, dim3(FP_BLOCK), bytes, st, __VA_ARGS__);                      \
         MDG_CHECK_LAUNCH(who); } while (0)

inline int64_t words_floats(int p) { return ET_HEAD + 4 * (int64_t)p; }      // the head, then 2 p int64 words

inline int make_tab_args(const char* who, TabArgs& A, const float* pos, int n_frames, int n_atoms, const MdgCell* cell,
                         const float* table, int p, float u0, float du, float cutoff, const uint8_t* mask) {
    int rc = check_frames(who, pos, cell, table, n_frames, n_atoms, FP_MAX_ATOMS);
    if (rc == MDG_OK) rc = check_frame_count(who, n_frames);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(p >= ET_MIN_NODES && p <= ET_MAX_NODES, "%s: the table needs %d..%d nodes, got %d", who, ET_MIN_NODES,
                  ET_MAX_NODES, p);
    MDG_CHECK_ARG(du > 0.f && cutoff > 0.f && u0 >= 0.f, "%s: the grid needs du > 0, u0 >= 0 and a positive cutoff", who);
    const double last = (double)u0 + (double)(p - 1) * (double)du, rc2 = (double)cutoff * (double)cutoff;
    // (u0, du and cutoff are float32 roundings of the caller's grid: a few ulps of cutoff^2 per node at the most)
    MDG_CHECK_ARG(fabs(last - rc2) <= 1e-6 * rc2, "%s: the last node u0 + (p - 1) du = %.9g is not cutoff^2 = %.9g", who, last, rc2);
    A.pos = pos; A.tab = table; A.g = nullptr; A.mask = mask; A.out = nullptr; A.g_pos = nullptr; A.partial = nullptr;
    A.words = nullptr; A.scale = nullptr; A.below = nullptr;
    A.F = n_frames; A.N = n_atoms; A.p = p;
    A.u0 = u0; A.inv_du = 1.f / du; A.pm1 = (float)(p - 1); A.rc2 = cutoff * cutoff;
    A.cell = *cell;
    return MDG_OK;
}

inline int frame_grid(const TabArgs& A, int fpb) {
    const int groups = (A.F + fpb - 1) / fpb;
    return groups < ET_GRID_CAP ? groups : ET_GRID_CAP;
}

}  // namespace

extern "C" int64_t mdg_energy_table_workspace(int n_frames, int n_atoms, int n_nodes) {
    if (n_frames <= 0 || n_atoms <= 0 || n_nodes < ET_MIN_NODES || n_nodes > ET_MAX_NODES) return 1;
    const int64_t tiles = n_atoms > FP_GROUP_ATOMS ? (int64_t)n_frames * tile_count(n_atoms) : 0;
    return words_floats(n_nodes) + tiles;
}

extern "C" int mdg_energy_table_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const float* table,
                                    int n_nodes, float u0, float du, float cutoff, const uint8_t* mask, float* U,
                                    int32_t* n_below, float* workspace, void* stream) {
    const char* who = "energy_table_fwd";
    TabArgs A;
    const int rc = make_tab_args("energy_table", A, pos, n_frames, n_atoms, cell, table, n_nodes, u0, du, cutoff, mask);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(U && n_below && workspace, "energy_table_fwd: null output, n_below or workspace");
    hipStream_t st = (hipStream_t)stream;
    A.out = U; A.below = reinterpret_cast<unsigned int*>(n_below); A.partial = workspace + words_floats(n_nodes);
    MDG_HIP(hipMemsetAsync(n_below, 0, sizeof(int32_t), st));
    const size_t bytes = lds_bytes(A.N, A.p, false);
    if (A.N <= FP_WAVE_ATOMS) {
        constexpr int FPB = FP_BLOCK / MDG_WAVE;
        ETAB_LAUNCH((etab_frame_kernel<MDG_WAVE, ET_VALUE>), dim3(frame_grid(A, FPB)), bytes, A, (A.F + FPB - 1) / FPB);
    } else if (A.N <= FP_GROUP_ATOMS) {
        ETAB_LAUNCH((etab_frame_kernel<FP_BLOCK, ET_VALUE>), dim3(frame_grid(A, 1)), bytes, A, A.F);
    } else {
        const int nt = tile_count(A.N);
        ETAB_LAUNCH((etab_tile_once_kernel<ET_VALUE>), dim3(A.F, nt), bytes, A, tile_blocks(A.N));
        constexpr int RPB = FP_BLOCK / MDG_WAVE;
        hipLaunchKernelGGL(fp_row_sum_kernel, dim3((A.F + RPB - 1) / RPB), dim3(FP_BLOCK), 0, st, A.partial, A.F, nt, 1.f, A.out);
        MDG_CHECK_LAUNCH(who);
    }
    return MDG_OK;
}

extern "C" int mdg_energy_table_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const float* table,
                                    int n_nodes, float u0, float du, float cutoff, const uint8_t* mask, const float* gU,
                                    float* g_pos, float* g_table, float* workspace, void* stream) {
    const char* who = "energy_table_bwd";
    TabArgs A;
    const int rc = make_tab_args("energy_table", A, pos, n_frames, n_atoms, cell, table, n_nodes, u0, du, cutoff, mask);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(gU && workspace, "energy_table_bwd: null gU or workspace");
    MDG_CHECK_ARG(g_pos || g_table, "energy_table_bwd: g_pos and g_table are both null (nothing to compute)");
    hipStream_t st = (hipStream_t)stream;
    A.g = gU; A.g_pos = g_pos;
    const int nwords = 2 * n_nodes;
    if (g_table) {
        A.scale = workspace;
        A.words = reinterpret_cast<unsigned long long*>(workspace + ET_HEAD);
        // a word receives at most F N (N - 1) contributions (both visits of the full rows), each |gU| |basis| <= max |gU|
        const float limit = fx64_limit((double)n_frames * (double)n_atoms * (double)(n_atoms > 1 ? n_atoms - 1 : 1));
        hipLaunchKernelGGL(etab_prepare_kernel, dim3(1), dim3(FP_BLOCK), 0, st, gU, n_frames, limit, A.words, nwords, workspace);
        MDG_CHECK_LAUNCH(who);
    }
    const size_t bytes = lds_bytes(A.N, A.p, g_table != nullptr);
    if (A.N <= FP_WAVE_ATOMS) {
        constexpr int FPB = FP_BLOCK / MDG_WAVE;
        const dim3 grid(frame_grid(A, FPB));
        const int groups = (A.F + FPB - 1) / FPB;
        if (g_pos) ETAB_LAUNCH((etab_frame_kernel<MDG_WAVE, ET_ROWS>), grid, bytes, A, groups);
        else ETAB_LAUNCH((etab_frame_kernel<MDG_WAVE, ET_NODES>), grid, bytes, A, groups);
    } else if (A.N <= FP_GROUP_ATOMS) {
        const dim3 grid(frame_grid(A, 1));
        if (g_pos) ETAB_LAUNCH((etab_frame_kernel<FP_BLOCK, ET_ROWS>), grid, bytes, A, A.F);
        else ETAB_LAUNCH((etab_frame_kernel<FP_BLOCK, ET_NODES>), grid, bytes, A, A.F);
    } else {
        const int nb = tile_blocks(A.N);
        if (g_pos) ETAB_LAUNCH(etab_tile_rows_kernel, dim3(A.F, nb), bytes, A, nb);
        else ETAB_LAUNCH((etab_tile_once_kernel<ET_NODES>), dim3(A.F, tile_count(A.N)), bytes, A, nb);
    }
    if (g_table) {
        hipLaunchKernelGGL(etab_finish_kernel, dim3((nwords + FP_BLOCK - 1) / FP_BLOCK), dim3(FP_BLOCK), 0, st, A.words, nwords,
                           A.scale, g_pos ? 0.5f : 1.f, g_table);
        MDG_CHECK_LAUNCH(who);
    }
    return MDG_OK;
}
