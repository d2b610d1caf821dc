// K21: the reciprocal-space part of the Ewald sum for point charges (mdgrad_amd/interface.py EwaldReciprocal; the reference
// has no Ewald sum, the definition is this project's).  For one replica on a diagonal cell L, V = Lx Ly Lz, charges q_i, wave
// vectors k(n) = 2 pi (nx / Lx, ny / Ly, nz / Lz) of a half space and a host table coef(k) (the class passes
// (4 pi / V) exp(-k^2 / (4 alpha^2)) / k^2, prepared in double):
//
//   rho(k) = A + iB = sum_j q_j exp(i k.x_j)            sigma(k) = sum_j q_j (k.w_j) exp(i k.x_j)
//   energy  = sum_replicas sum_k coef(k) (A^2 + B^2)
//   dU/dx_i = sum_k 2 coef q_i k (B c_i - A s_i)                                       c_i = cos k.x_i, s_i = sin k.x_i
//   pot_i   = sum_k 2 coef (A c_i + B s_i)                                             (= dU/dq_i)
//   (H w)_i = sum_k 2 coef q_i k [ Re sigma c_i + Im sigma s_i - (k.w_i) (A c_i + B s_i) ]
//   potw_i  = sum_k 2 coef [ (k.w_i) (B c_i - A s_i) + Re sigma s_i - Im sigma c_i ]   (= d(w.dU/dx)/dq_i)
//
// The conversion factor, the neutralising background and the self term are the caller's (ops.py / CoulombPotentials).
//
// Two phases per evaluation, on the phase arithmetic of sk_phase.hpp (positions in turns, 1-ulp sine / cosine, so unwrapped
// positions many cells away cost nothing):
//   mode phase  one thread per (replica, vector); the replica's atoms pass through LDS in blocks of EW_MODE_ATOMS as
//               (uh, q), (ul, -), (2 pi w / L, -) and every thread walks them in index order: one sine / cosine pair per
//               (atom, vector) feeds rho and sigma.  All lanes read the same atom (an LDS broadcast).  (A, B, Re sigma,
//               Im sigma) -> workspace [R, M] float4.
//   atom phase  a workgroup of 1024 threads owns EW_SLICE_ATOMS = 64 atoms of a replica, lane = atom; its sixteen waves are
//               sixteen slices of every staged chunk of EW_CHUNK vectors (n, coef A, coef B, coef sigma as two float4
//               arrays), so a single 64-atom replica -- one workgroup -- walks ~M / 16 vectors per lane instead of M.  A
//               wave reads one vector at a time: broadcast reads, no bank conflicts.  The slices' partial sums meet in LDS
//               (the staging arrays again, as [slice][component][lane]: conflict-free) and are added in slice order.
//   energy      one workgroup sums coef (A^2 + B^2) over the workspace in double: a fixed stride per thread, then a fixed tree.
// Every sum runs in a fixed order and every output word has one writer: two launches give the same bits.  No atomics.
#include "common.hpp"
#include "sk_phase.hpp"

namespace {

constexpr int EW_BLOCK = 256;
constexpr int EW_MODE_ATOMS = 512;       // atoms per LDS block of the mode phase
constexpr int EW_SLICE_ATOMS = 64;       // atoms per workgroup of the atom phase: lane = atom
constexpr int EW_ATOM_BLOCK = 1024;      // threads of an atom-phase workgroup
constexpr int EW_SLICES = EW_ATOM_BLOCK / EW_SLICE_ATOMS;
constexpr int EW_CHUNK = EW_ATOM_BLOCK;  // vectors staged at a time in the atom phase, EW_CHUNK / EW_SLICES per slice
constexpr int EW_SLICE_VECS = EW_CHUNK / EW_SLICES;
constexpr int EW_MAX_ATOMS = 32768;
constexpr int EW_MAX_VECS = 65536;
constexpr float EW_TWO_PI = 6.283185307179586f;

struct EwArgs {
    const float* pos;        // [R, N, 3]
    const float* q;          // [R, N]
    const float* w;          // [R, N, 3] or null
    const int32_t* kvec;     // [M, 3]
    const float* coef;       // [M]
    float4* ws;              // [R, M] (A, B, Re sigma, Im sigma)
    float* grad; float* hw; float* pot; float* potw;
    int R, N, M;
    float L[3];
    float oscale; int oacc;  // grad / hw: out = (oacc ? out : 0) + oscale * value
};

// atom at row `at` of pos / q = (uh.xyz, q), (ul.xyz, -)
__device__ __forceinline__ void ew_atom(const EwArgs& A, size_t at, float4& a, float4& b) {
    turns(A.pos[3 * at], A.L[0], a.x, b.x);
    turns(A.pos[3 * at + 1], A.L[1], a.y, b.y);
    turns(A.pos[3 * at + 2], A.L[2], a.z, b.z);
    a.w = A.q[at];
    b.w = 0.f;
}

// 2 pi w / L: n . (this) = k . w
__device__ __forceinline__ float4 ew_wt(const EwArgs& A, size_t at) {
    return make_float4(EW_TWO_PI * A.w[3 * at] / A.L[0], EW_TWO_PI * A.w[3 * at + 1] / A.L[1],
                       EW_TWO_PI * A.w[3 * at + 2] / A.L[2], 0.f);
}

// ---------------------------------------------------------------------------------- mode phase
// grid R * ceil(M / EW_BLOCK): block = (replica, chunk of vectors)
template <bool HASW>
__global__ __launch_bounds__(EW_BLOCK) void ewald_mode_kernel(const EwArgs A) {
    __shared__ float4 sa[EW_MODE_ATOMS], sb[EW_MODE_ATOMS];
    __shared__ float4 sw[HASW ? EW_MODE_ATOMS : 1];
    const int nc = (A.M + EW_BLOCK - 1) / EW_BLOCK;
    const int r = blockIdx.x / nc, m = (blockIdx.x % nc) * EW_BLOCK + threadIdx.x;
    const bool valid = m < A.M;
    const float4 n = load_n(A.kvec, valid ? m : A.M - 1);
    const size_t base = (size_t)r * A.N;
    float re = 0.f, im = 0.f, sr = 0.f, si = 0.f;
    for (int i0 = 0; i0 < A.N; i0 += EW_MODE_ATOMS) {
        const int na = min(EW_MODE_ATOMS, A.N - i0);
        __syncthreads();                                         // the previous block has been read
        for (int i = threadIdx.x; i < na; i += EW_BLOCK) {
            float4 a, b;
            ew_atom(A, base + i0 + i, a, b);
            sa[i] = a; sb[i] = b;
            if (HASW) sw[i] = ew_wt(A, base + i0 + i);
        }
        __syncthreads();
        for (int i = 0; i < na; ++i) {
            const float4 a = sa[i], b = sb[i];
            float s, c;
            sincos_turns(phase(n.x, n.y, n.z, a, b), s, c);
            re = fmaf(a.w, c, re);
            im = fmaf(a.w, s, im);
            if (HASW) {
                const float4 wt = sw[i];
                const float qk = a.w * fmaf(n.z, wt.z, fmaf(n.y, wt.y, n.x * wt.x));
                sr = fmaf(qk, c, sr);
                si = fmaf(qk, s, si);
            }
        }
    }
    if (valid) A.ws[(size_t)r * A.M + m] = make_float4(re, im, sr, si);
}

// ---------------------------------------------------------------------------------- atom phase
// grid R * ceil(N / EW_SLICE_ATOMS), EW_ATOM_BLOCK threads: block = (replica, 64 atoms); wave = slice of every chunk
template <bool HASW>
__global__ __launch_bounds__(EW_ATOM_BLOCK) void ewald_atom_kernel(const EwArgs A) {
    constexpr int NV = HASW ? 8 : 4;                              // g.xyz, pot (, h.xyz, potw)
    __shared__ float4 stage[2 * EW_CHUNK];
    float4* snv = stage;
    float4* scf = stage + EW_CHUNK;
    float* part = reinterpret_cast<float*>(stage);               // (after the last chunk: the slices' partial sums)
    static_assert((EW_SLICES - 1) * NV * EW_SLICE_ATOMS <= 8 * EW_CHUNK, "the partial sums fit the staging arrays");
    const int nb = (A.N + EW_SLICE_ATOMS - 1) / EW_SLICE_ATOMS;
    const int r = blockIdx.x / nb, ib = blockIdx.x % nb, t = threadIdx.x, lane = t & 63, sl = t >> 6, M = A.M;
    const int i = ib * EW_SLICE_ATOMS + lane;
    const bool live = i < A.N;
    const size_t at = (size_t)r * A.N + (live ? i : A.N - 1);    // (a spare lane repeats the last atom and writes nothing)
    float4 a, b, wt = make_float4(0.f, 0.f, 0.f, 0.f);
    ew_atom(A, at, a, b);
    if (HASW) wt = ew_wt(A, at);
    const float4* ws = A.ws + (size_t)r * M;
    float v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = 0.f;
    for (int m0 = 0; m0 < M; m0 += EW_CHUNK) {
        const int m = m0 + t;
        __syncthreads();                                         // the previous chunk has been read
        if (m < M) {
            const float cf = A.coef[m];
            const float4 md = ws[m];
            snv[t] = load_n(A.kvec, m);
            scf[t] = make_float4(cf * md.x, cf * md.y, cf * md.z, cf * md.w);
        }
        __syncthreads();
        const int k1 = min(min(EW_CHUNK, M - m0), (sl + 1) * EW_SLICE_VECS);
        for (int k = sl * EW_SLICE_VECS; k < k1; ++k) {
            const float4 n = snv[k], cf = scf[k];
            float s, c;
            sincos_turns(phase(n.x, n.y, n.z, a, b), s, c);
            const float P = fmaf(cf.x, c, cf.y * s);              // coef (A c_i + B s_i)
            const float Q = fmaf(cf.y, c, -(cf.x * s));           // coef (B c_i - A s_i)
            v[0] = fmaf(n.x, Q, v[0]); v[1] = fmaf(n.y, Q, v[1]); v[2] = fmaf(n.z, Q, v[2]);
            v[3] += P;
            if (HASW) {
                const float kw = fmaf(n.z, wt.z, fmaf(n.y, wt.y, n.x * wt.x));
                const float T = fmaf(cf.z, c, fmaf(cf.w, s, -(kw * P)));
                v[4] = fmaf(n.x, T, v[4]); v[5] = fmaf(n.y, T, v[5]); v[6] = fmaf(n.z, T, v[6]);
                v[7] += fmaf(kw, Q, fmaf(cf.z, s, -(cf.w * c)));
            }
        }
    }
    __syncthreads();                                             // the last chunk has been read
    if (sl > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) part[((sl - 1) * NV + j) * EW_SLICE_ATOMS + lane] = v[j];
    }
    __syncthreads();
    if (sl != 0 || !live) return;
#pragma unroll 2                                                 // (all fifteen slices' loads in flight cost registers)
    for (int s = 1; s < EW_SLICES; ++s) {
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] += part[((s - 1) * NV + j) * EW_SLICE_ATOMS + lane];
    }
    // sums in turns -> 2 q_i (2 pi / L_d) per axis
    const float os = A.oscale, c2 = 2.f * a.w * EW_TWO_PI;
    if (A.grad) store3(A.grad + 3 * at, 0, os, A.oacc, c2 * v[0] / A.L[0], c2 * v[1] / A.L[1], c2 * v[2] / A.L[2]);
    if (A.pot) A.pot[at] = 2.f * v[3];
    if (HASW) {
        if (A.hw) store3(A.hw + 3 * at, 0, os, A.oacc, c2 * v[NV - 4] / A.L[0], c2 * v[NV - 3] / A.L[1], c2 * v[NV - 2] / A.L[2]);
        if (A.potw) A.potw[at] = 2.f * v[NV - 1];
    }
}

// ---------------------------------------------------------------------------------- energy
// one workgroup: thread t sums the entries t, t + EW_BLOCK, ... of the [R, M] workspace in double, then a fixed tree
__global__ __launch_bounds__(EW_BLOCK) void ewald_energy_kernel(const float4* __restrict__ ws, const float* __restrict__ coef,
                                                                int R, int M, float* energy) {
    __shared__ double red[EW_BLOCK];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int r = 0; r < R; ++r) {
        const float4* row = ws + (size_t)r * M;
        double sr = 0.0;
        for (int m = t; m < M; m += EW_BLOCK) {
            const float4 md = row[m];
            const double x = md.x, y = md.y;
            sr += (double)coef[m] * (x * x + y * y);
        }
        s += sr;
    }
    tree_sum<EW_BLOCK>(s, red);
    if (t == 0) energy[0] = (float)red[0];
}

}  // namespace

extern "C" int64_t mdg_ewald_workspace(int n_rep, int n_atoms, int n_vecs) {
    if (n_rep <= 0 || n_atoms <= 0 || n_vecs <= 0) return 4;
    return 4LL * n_rep * n_vecs;                                  // (A, B, Re sigma, Im sigma) per (replica, vector)
}

extern "C" int mdg_ewald_eval(const float* pos, int n_rep, int n_atoms, const MdgCell* cell, const float* q, const int32_t* kvec,
                              const float* coef, int n_vecs, const float* w, float* energy, float* grad, float* hw, float* pot,
                              float* potw, float* workspace, float out_scale, int accumulate, void* stream) {
    MDG_CHECK_ARG(pos && cell && q && kvec && coef, "ewald_eval: null argument (pos, cell, q, kvec or coef)");
    MDG_CHECK_ARG(workspace, "ewald_eval: workspace is null (mdg_ewald_workspace() floats)");
    MDG_CHECK_ARG(n_rep > 0 && n_atoms > 0, "ewald_eval: n_rep and n_atoms must be positive");
    MDG_CHECK_ARG(n_atoms <= EW_MAX_ATOMS, "ewald_eval: at most %d atoms per replica, got %d", EW_MAX_ATOMS, n_atoms);
    MDG_CHECK_ARG(n_vecs >= 1 && n_vecs <= EW_MAX_VECS, "ewald_eval: 1..%d wave vectors, got %d", EW_MAX_VECS, n_vecs);
    MDG_CHECK_ARG((long long)n_rep * n_atoms < (1LL << 31) / 4, "ewald_eval: n_rep * n_atoms too large for one call");
    MDG_CHECK_ARG(cell->diag, "ewald_eval: the cell must be diagonal (triclinic cells are not supported)");
    MDG_CHECK_ARG(cell->h[0] > 0.f && cell->h[4] > 0.f && cell->h[8] > 0.f, "ewald_eval: the cell lengths must be positive");
    MDG_CHECK_ARG(w || !(hw || potw), "ewald_eval: hw / potw need w");
    MDG_CHECK_ARG(!w || hw || potw, "ewald_eval: w given without hw or potw output");
    MDG_CHECK_ARG(energy || grad || hw || pot || potw, "ewald_eval: no output requested");
    const long long nc = (n_vecs + EW_BLOCK - 1) / EW_BLOCK, nb = (n_atoms + EW_SLICE_ATOMS - 1) / EW_SLICE_ATOMS;
    MDG_CHECK_ARG(nc * n_rep < (1LL << 31) && nb * n_rep < (1LL << 31), "ewald_eval: too many replicas for one call");
    EwArgs a{pos, q, w, kvec, coef, reinterpret_cast<float4*>(workspace), grad, hw, pot, potw, n_rep, n_atoms, n_vecs,
             {cell->h[0], cell->h[4], cell->h[8]}, out_scale, accumulate & 1};
    hipStream_t st = (hipStream_t)stream;
    const dim3 gm((unsigned)(nc * n_rep)), ga((unsigned)(nb * n_rep));
    if (w) hipLaunchKernelGGL((ewald_mode_kernel<true>), gm, dim3(EW_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((ewald_mode_kernel<false>), gm, dim3(EW_BLOCK), 0, st, a);
    MDG_CHECK_LAUNCH("ewald_mode_kernel");
    if (grad || hw || pot || potw) {
        if (w) hipLaunchKernelGGL((ewald_atom_kernel<true>), ga, dim3(EW_ATOM_BLOCK), 0, st, a);
        else hipLaunchKernelGGL((ewald_atom_kernel<false>), ga, dim3(EW_ATOM_BLOCK), 0, st, a);
        MDG_CHECK_LAUNCH("ewald_atom_kernel");
    }
    if (energy) {
        hipLaunchKernelGGL(ewald_energy_kernel, dim3(1), dim3(EW_BLOCK), 0, st, reinterpret_cast<const float4*>(workspace), coef,
                           n_rep, n_vecs, energy);
        MDG_CHECK_LAUNCH("ewald_energy_kernel");
    }
    return MDG_OK;
}
