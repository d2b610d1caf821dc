// K16: static structure factor S(k) of every frame of a trajectory, and its gradient (mdgrad_amd/observable.py
// structure_factor; the reference has no S(k), the definition is this project's).
//
//   rho_f(k) = sum_i w_i exp(i k.x_fi)      S_f(k) = |rho_f(k)|^2 / sum_i w_i^2      S_f[b] = mean of S_f(k) over the bin's vectors
//   dS_f(k)/dx_fi = (2 w_i / sum w^2) [ Im rho cos(k.x_fi) - Re rho sin(k.x_fi) ] k
//
// k(n) = 2 pi (nx / Lx, ny / Ly, nz / Lz) on a diagonal cell.  The integer vectors n arrive sorted by bin as int32 [M, 3] with
// the segment offsets int32 [B + 1]: a bin's sum is a walk over a contiguous segment.  No pair search: O(F N M) independent
// phase sums, list-free like K15 (csrc/virial.hip).  Three shapes by frame size, positions staged in LDS in all of them:
//   N <= 128     a wave per frame, four frames per workgroup; vectors in chunks of 64
//   N <= 1024    a workgroup per frame; vectors in chunks of 256
//   larger       (atom block of 1024) x (chunk of 256 vectors) tiles write rho partials, summed over the atom blocks in index
//                order by a second small kernel
// LDS holds the frame (or atom block), the segment table and one chunk of vectors: it does not grow with M.
//
// Phases are formed in turns, never in radians: per atom and axis u = x / L - rint(x / L) (the remainder x - q L is one fma,
// exact), split into uh = a multiple of 2^-12 and ul = the rest, the division's own remainder included.  For integer n the
// sum n.uh is exact in float32 (|n_d| <= 1024), so t = n.uh - rint(n.uh) + n.ul carries ~3e-8 turns whatever the size of n or
// of x: fused trajectories are not wrapped, and an atom fifty boxes away costs nothing.  sin / cos of 2 pi t: reduction to an
// eighth turn and the Cephes float minimax polynomials (1 ulp), one sine / cosine pair per (atom, vector).
//
// Backward: recomputes rho of the frame chunk by chunk (no [F, M] complex tensor survives the forward), then every thread
// owns up to two (four) atoms and sums the chunk's vectors into them.
// Every sum runs in a fixed order: per lane over the atoms / the chunk's vectors, the xor-shuffle tree of common.hpp per bin
// run of a wave pass, passes in ascending order, waves in index order.  No floating-point read-modify-write to global memory
// by more than one thread: two launches give the same bits.
#include "common.hpp"
#include "sk_phase.hpp"

namespace {

constexpr int SK_BLOCK = 256;
constexpr int SK_WAVE_ATOMS = 128;       // up to here a wave per frame
constexpr int SK_GROUP_ATOMS = 1024;     // up to here a workgroup per frame
constexpr int SK_TILE_ATOMS = 1024;      // beyond: atom blocks of SK_TILE_ATOMS x vector chunks of SK_BLOCK
constexpr int SK_MAX_ATOMS = 32768;
constexpr int SK_MAX_VECS = 65536;
constexpr int SK_MAX_BINS = 1024;
constexpr int SK_WAVES = SK_BLOCK / MDG_WAVE;

// (SkArgs and the phase helpers turns, load_atom, phase, sincos_turns, rho_sweep, grad_chunk, load_n, bin_of: sk_phase.hpp,
// shared with csrc/isf.hip)

// one pass of a wave: val of lane's vector (bin b, ignored unless valid) added to the wave's bin sums; a shuffle tree per run
// of equal bins, lane 0 adds
__device__ __forceinline__ void bin_add(float* sbin, float val, int b, bool valid) {
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int bb = __shfl(b, __ffsll((long long)todo) - 1, MDG_WAVE);
        const bool mine = valid && b == bb;
        const float s = wave_sum(mine ? val : 0.f);
        if ((threadIdx.x & 63) == 0) sbin[bb] += s;
        todo &= ~__ballot(mine);
    }
}

// S[b] = (sum over the nw waves' bin sums, in index order) / (norm count_b); an empty bin gives 0
__device__ __forceinline__ void bins_out(const float* sbin, int nw, const int32_t* sseg, int B, float inv_norm, float* S, int t,
                                         int stride) {
    for (int b = t; b < B; b += stride) {
        float s = 0.f;
        for (int w = 0; w < nw; ++w) s += sbin[w * SK_MAX_BINS + b];
        const int cnt = sseg[b + 1] - sseg[b];
        S[b] = cnt > 0 ? s * inv_norm / (float)cnt : 0.f;
    }
}

// dS/dx of atom i: the sum in turns times 2 w_i / norm times 2 pi / L
__device__ __forceinline__ void put_grad(const SkArgs& A, long long f, int i, float w, const float (&g)[3]) {
    const float c = 2.f * A.inv_norm * w * 6.283185307179586f;
    float* o = A.g_pos + ((size_t)f * A.N + i) * 3;
    o[0] = c * g[0] / A.L[0]; o[1] = c * g[1] / A.L[1]; o[2] = c * g[2] / A.L[2];
}

// ---------------------------------------------------------------------------------- whole frame in LDS (N <= 1024)
// TPF threads share a frame; vectors in chunks of TPF, thread t of the frame takes vector m0 + t
template <int TPF, bool BWD>
__global__ __launch_bounds__(SK_BLOCK) void sk_frame_kernel(const SkArgs A) {
    constexpr int CAP = TPF == MDG_WAVE ? SK_WAVE_ATOMS : SK_GROUP_ATOMS, FPB = SK_BLOCK / TPF, APT = CAP / TPF, WPF = TPF / MDG_WAVE;
    static_assert(TPF == MDG_WAVE || TPF == SK_BLOCK, "a wave or the whole workgroup per frame");
    __shared__ float4 sa[FPB * CAP], sb[FPB * CAP];
    __shared__ int32_t sseg[SK_MAX_BINS + 1];
    __shared__ float sbin[BWD ? 1 : SK_WAVES * SK_MAX_BINS];    // forward: bin sums per wave
    __shared__ float4 snv[BWD ? SK_BLOCK : 1];                  // backward: the chunk of every frame of the workgroup
    __shared__ float2 sab[BWD ? SK_BLOCK : 1];
    const int t = threadIdx.x % TPF, g = threadIdx.x / TPF, wv = threadIdx.x >> 6, N = A.N, M = A.M, B = A.B;
    const long long f0 = (long long)blockIdx.x * FPB + g;
    const bool live = f0 < A.F;
    const long long f = live ? f0 : A.F - 1;                     // (a spare wave repeats the last frame and writes nothing)
    float4* fa = sa + g * CAP;
    float4* fb = sb + g * CAP;
    const float* p = A.pos + (size_t)f * N * 3;
    for (int i = t; i < N; i += TPF) {
        float4 a, b;
        load_atom(A, p, i, a, b);
        fa[i] = a; fb[i] = b;
    }
    for (int b = threadIdx.x; b <= B; b += SK_BLOCK) sseg[b] = A.seg[b];
    if (!BWD)
        for (int b = threadIdx.x & 63; b < B; b += MDG_WAVE) sbin[wv * SK_MAX_BINS + b] = 0.f;
    __syncthreads();

    float4 oa[APT], ob[APT];                                     // backward: the atoms t, t + TPF, ... of this thread
    float gacc[APT][3];
    if (BWD) {
#pragma unroll
        for (int k = 0; k < APT; ++k) {
            const int i = min(t + k * TPF, N - 1);
            oa[k] = fa[i]; ob[k] = fb[i];
            gacc[k][0] = gacc[k][1] = gacc[k][2] = 0.f;
        }
    }
    for (int m0 = 0; m0 < M; m0 += TPF) {
        const int m = m0 + t;
        const bool valid = m < M;
        const float4 n = load_n(A.kvec, valid ? m : M - 1);
        float re, im;
        rho_sweep(fa, fb, N, n.x, n.y, n.z, re, im);
        const int b = bin_of(sseg, B, valid ? m : M - 1);
        if (!BWD) {
            bin_add(sbin + wv * SK_MAX_BINS, fmaf(re, re, im * im), b, valid);
        } else {
            const float coef = valid ? A.gS[(size_t)f * B + b] / (float)(sseg[b + 1] - sseg[b]) : 0.f;
            __syncthreads();                                     // the previous chunk has been read
            snv[threadIdx.x] = n;
            sab[threadIdx.x] = make_float2(coef * im, coef * re);
            __syncthreads();
            const int kc = min(TPF, M - m0);
#pragma unroll
            for (int k = 0; k < APT; ++k)
                if (t + k * TPF < N) grad_chunk(snv + g * TPF, sab + g * TPF, kc, oa[k], ob[k], gacc[k]);
        }
    }
    if (!BWD) {
        __syncthreads();
        if (live) bins_out(sbin + g * WPF * SK_MAX_BINS, WPF, sseg, B, A.inv_norm, A.S + (size_t)f * B, t, TPF);
    } else if (live) {
#pragma unroll
        for (int k = 0; k < APT; ++k)
            if (t + k * TPF < N) put_grad(A, f, t + k * TPF, oa[k].w, gacc[k]);
    }
}

// ---------------------------------------------------------------------------------- tiles (N > 1024)
__host__ __device__ inline int atom_blocks(int n_atoms) { return (n_atoms + SK_TILE_ATOMS - 1) / SK_TILE_ATOMS; }
__host__ __device__ inline int vec_chunks(int n_vecs) { return (n_vecs + SK_BLOCK - 1) / SK_BLOCK; }

// grid (F, nb * nc): tile id = ib + nb * ic; partial rho of the chunk's vectors over the block's atoms -> ws [F, nb, M] float2
__global__ __launch_bounds__(SK_BLOCK) void sk_tile_rho_kernel(const SkArgs A) {
    __shared__ float4 sa[SK_TILE_ATOMS], sb[SK_TILE_ATOMS];
    const int nb = atom_blocks(A.N), f = blockIdx.x, ib = blockIdx.y % nb, ic = blockIdx.y / nb, t = threadIdx.x;
    const int i0 = ib * SK_TILE_ATOMS, na = min(SK_TILE_ATOMS, A.N - i0);
    const float* p = A.pos + (size_t)f * A.N * 3;
    for (int i = t; i < na; i += SK_BLOCK) {
        float4 a, b;
        load_atom(A, p, i0 + i, a, b);
        sa[i] = a; sb[i] = b;
    }
    __syncthreads();
    const int m = ic * SK_BLOCK + t;
    if (m >= A.M) return;
    const float4 n = load_n(A.kvec, m);
    float re, im;
    rho_sweep(sa, sb, na, n.x, n.y, n.z, re, im);
    reinterpret_cast<float2*>(A.ws)[((size_t)f * nb + ib) * A.M + m] = make_float2(re, im);
}

// rho of vector m of frame f: the atom blocks' partials in index order
__device__ __forceinline__ float2 rho_total(const SkArgs& A, int nb, int f, int m) {
    const float2* part = reinterpret_cast<const float2*>(A.ws) + (size_t)f * nb * A.M + m;
    float2 r = make_float2(0.f, 0.f);
    for (int ib = 0; ib < nb; ++ib) { const float2 q = part[(size_t)ib * A.M]; r.x += q.x; r.y += q.y; }
    return r;
}

// forward second stage, a workgroup per frame: |rho|^2 into the bins
__global__ __launch_bounds__(SK_BLOCK) void sk_tile_bins_kernel(const SkArgs A) {
    __shared__ int32_t sseg[SK_MAX_BINS + 1];
    __shared__ float sbin[SK_WAVES * SK_MAX_BINS];
    const int nb = atom_blocks(A.N), f = blockIdx.x, t = threadIdx.x, wv = t >> 6, B = A.B, M = A.M;
    for (int b = t; b <= B; b += SK_BLOCK) sseg[b] = A.seg[b];
    for (int b = t & 63; b < B; b += MDG_WAVE) sbin[wv * SK_MAX_BINS + b] = 0.f;
    __syncthreads();
    for (int m0 = 0; m0 < M; m0 += SK_BLOCK) {
        const int m = m0 + t;
        const bool valid = m < M;
        const float2 r = rho_total(A, nb, f, valid ? m : M - 1);
        bin_add(sbin + wv * SK_MAX_BINS, fmaf(r.x, r.x, r.y * r.y), bin_of(sseg, B, valid ? m : M - 1), valid);
    }
    __syncthreads();
    bins_out(sbin, SK_WAVES, sseg, B, A.inv_norm, A.S + (size_t)f * B, t, SK_BLOCK);
}

// backward second stage, grid (F, nc): (coef Im rho, coef Re rho) of every vector -> ws behind the partials, [F, M] float2
__global__ __launch_bounds__(SK_BLOCK) void sk_tile_coef_kernel(const SkArgs A) {
    const int nb = atom_blocks(A.N), f = blockIdx.x, m = blockIdx.y * SK_BLOCK + threadIdx.x;
    if (m >= A.M) return;
    const float2 r = rho_total(A, nb, f, m);
    const int b = bin_of(A.seg, A.B, m);
    const float coef = A.gS[(size_t)f * A.B + b] / (float)(A.seg[b + 1] - A.seg[b]);
    float2* out = reinterpret_cast<float2*>(A.ws) + (size_t)A.F * nb * A.M;
    out[(size_t)f * A.M + m] = make_float2(coef * r.y, coef * r.x);
}

// backward third stage, grid (F, nb): every thread owns four atoms of the block and walks all vectors, a chunk at a time
__global__ __launch_bounds__(SK_BLOCK) void sk_tile_bwd_kernel(const SkArgs A) {
    constexpr int APT = SK_TILE_ATOMS / SK_BLOCK;
    __shared__ float4 snv[SK_BLOCK];
    __shared__ float2 sab[SK_BLOCK];
    const int nb = atom_blocks(A.N), f = blockIdx.x, ib = blockIdx.y, t = threadIdx.x, N = A.N, M = A.M;
    const float* p = A.pos + (size_t)f * N * 3;
    const float2* coef = reinterpret_cast<const float2*>(A.ws) + (size_t)A.F * nb * M + (size_t)f * M;
    float4 oa[APT], ob[APT];
    float gacc[APT][3];
#pragma unroll
    for (int k = 0; k < APT; ++k) {
        load_atom(A, p, min(ib * SK_TILE_ATOMS + t + k * SK_BLOCK, N - 1), oa[k], ob[k]);
        gacc[k][0] = gacc[k][1] = gacc[k][2] = 0.f;
    }
    for (int m0 = 0; m0 < M; m0 += SK_BLOCK) {
        const int m = m0 + t;
        __syncthreads();                                         // the previous chunk has been read
        snv[t] = load_n(A.kvec, m < M ? m : M - 1);
        sab[t] = m < M ? coef[m] : make_float2(0.f, 0.f);
        __syncthreads();
        const int kc = min(SK_BLOCK, M - m0);
#pragma unroll
        for (int k = 0; k < APT; ++k)
            if (ib * SK_TILE_ATOMS + t + k * SK_BLOCK < N) grad_chunk(snv, sab, kc, oa[k], ob[k], gacc[k]);
    }
#pragma unroll
    for (int k = 0; k < APT; ++k) {
        const int i = ib * SK_TILE_ATOMS + t + k * SK_BLOCK;
        if (i < N) put_grad(A, f, i, oa[k].w, gacc[k]);
    }
}

int sk_args(SkArgs& A, const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const float* weights, float norm,
            const int32_t* kvec, int n_vecs, const int32_t* seg, int n_bins) {
    MDG_CHECK_ARG(pos && cell && kvec && seg, "sk: null argument");
    MDG_CHECK_ARG(n_frames > 0 && n_atoms > 0, "sk: empty trajectory");
    MDG_CHECK_ARG(n_atoms <= SK_MAX_ATOMS, "sk: at most %d atoms per frame, got %d", SK_MAX_ATOMS, n_atoms);
    MDG_CHECK_ARG(n_frames < (1 << 24), "sk: fewer than 2^24 frames in one call (chunk the frames)");
    MDG_CHECK_ARG(n_vecs >= 1 && n_vecs <= SK_MAX_VECS, "sk: 1..%d wave vectors, got %d (max_per_bin thins them)", SK_MAX_VECS,
                  n_vecs);
    MDG_CHECK_ARG(n_bins >= 1 && n_bins <= SK_MAX_BINS, "sk: 1..%d bins, got %d", SK_MAX_BINS, n_bins);
    MDG_CHECK_ARG(cell->diag, "sk: the cell must be diagonal (triclinic cells are not supported)");
    MDG_CHECK_ARG(cell->h[0] > 0.f && cell->h[4] > 0.f && cell->h[8] > 0.f, "sk: the cell lengths must be positive");
    MDG_CHECK_ARG(norm > 0.f, "sk: norm = sum of the squared weights must be positive, got %g", (double)norm);
    A.pos = pos; A.w = weights; A.kvec = kvec; A.seg = seg; A.gS = nullptr; A.S = nullptr; A.g_pos = nullptr; A.ws = nullptr;
    A.F = n_frames; A.N = n_atoms; A.M = n_vecs; A.B = n_bins;
    A.inv_norm = 1.f / norm;
    A.L[0] = cell->h[0]; A.L[1] = cell->h[4]; A.L[2] = cell->h[8];
    return MDG_OK;
}

}  // namespace

extern "C" int64_t mdg_sk_workspace(int n_frames, int n_atoms, int n_vecs) {
    if (n_frames <= 0 || n_atoms <= SK_GROUP_ATOMS || n_vecs <= 0) return 1;
    return 2LL * n_frames * n_vecs * (atom_blocks(n_atoms) + 1);          // rho partials [F, nb, M] + coefficients [F, M], float2
}

extern "C" int mdg_sk_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const float* weights, float norm,
                          const int32_t* kvec, int n_vecs, const int32_t* seg, int n_bins, float* S, float* workspace,
                          void* stream) {
    SkArgs A;
    const int rc = sk_args(A, pos, n_frames, n_atoms, cell, weights, norm, kvec, n_vecs, seg, n_bins);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(S && workspace, "sk_fwd: null output or workspace");
    A.S = S; A.ws = workspace;
    hipStream_t st = (hipStream_t)stream;
    if (n_atoms <= SK_WAVE_ATOMS) {
        constexpr int FPB = SK_BLOCK / MDG_WAVE;
        hipLaunchKernelGGL((sk_frame_kernel<MDG_WAVE, false>), dim3((n_frames + FPB - 1) / FPB), dim3(SK_BLOCK), 0, st, A);
    } else if (n_atoms <= SK_GROUP_ATOMS) {
        hipLaunchKernelGGL((sk_frame_kernel<SK_BLOCK, false>), dim3(n_frames), dim3(SK_BLOCK), 0, st, A);
    } else {
        hipLaunchKernelGGL(sk_tile_rho_kernel, dim3(n_frames, atom_blocks(n_atoms) * vec_chunks(n_vecs)), dim3(SK_BLOCK), 0, st, A);
        MDG_CHECK_LAUNCH("sk_tile_rho_kernel");
        hipLaunchKernelGGL(sk_tile_bins_kernel, dim3(n_frames), dim3(SK_BLOCK), 0, st, A);
    }
    MDG_CHECK_LAUNCH("sk_fwd");
    return MDG_OK;
}

extern "C" int mdg_sk_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const float* weights, float norm,
                          const int32_t* kvec, int n_vecs, const int32_t* seg, int n_bins, const float* gS, float* g_pos,
                          float* workspace, void* stream) {
    SkArgs A;
    const int rc = sk_args(A, pos, n_frames, n_atoms, cell, weights, norm, kvec, n_vecs, seg, n_bins);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(gS && g_pos && workspace, "sk_bwd: null gS, g_pos or workspace");
    A.gS = gS; A.g_pos = g_pos; A.ws = workspace;
    hipStream_t st = (hipStream_t)stream;
    if (n_atoms <= SK_WAVE_ATOMS) {
        constexpr int FPB = SK_BLOCK / MDG_WAVE;
        hipLaunchKernelGGL((sk_frame_kernel<MDG_WAVE, true>), dim3((n_frames + FPB - 1) / FPB), dim3(SK_BLOCK), 0, st, A);
    } else if (n_atoms <= SK_GROUP_ATOMS) {
        hipLaunchKernelGGL((sk_frame_kernel<SK_BLOCK, true>), dim3(n_frames), dim3(SK_BLOCK), 0, st, A);
    } else {
        const int nb = atom_blocks(n_atoms), nc = vec_chunks(n_vecs);
        hipLaunchKernelGGL(sk_tile_rho_kernel, dim3(n_frames, nb * nc), dim3(SK_BLOCK), 0, st, A);
        MDG_CHECK_LAUNCH("sk_tile_rho_kernel");
        hipLaunchKernelGGL(sk_tile_coef_kernel, dim3(n_frames, nc), dim3(SK_BLOCK), 0, st, A);
        MDG_CHECK_LAUNCH("sk_tile_coef_kernel");
        hipLaunchKernelGGL(sk_tile_bwd_kernel, dim3(n_frames, nb), dim3(SK_BLOCK), 0, st, A);
    }
    MDG_CHECK_LAUNCH("sk_bwd");
    return MDG_OK;
}
