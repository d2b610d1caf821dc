// K18: intermediate scattering functions of a trajectory over all lags, coherent F(k,t) and self F_s(k,t), and their gradients
// (mdgrad_amd/observable.py intermediate_scattering; the reference has no ISF, the definition is this project's).
//
//   rho(k, t)   = sum_i w_i exp(i k.x_i(t))                 W2 = sum_i w_i^2
//   F(k, tau)   = 1 / (|O_tau| W2)  sum_{t0 in O_tau} Re[ rho(k, t0 + tau) conj rho(k, t0) ]
//   F_s(k, tau) = 1 / (|O_tau| W2)  sum_{t0 in O_tau} sum_i w_i^2 cos( k.(x_i(t0 + tau) - x_i(t0)) )
//   O_tau = {t0 = 0, s, 2 s, ... : t0 + tau < T}      |O_tau| = (T - 1 - tau) / s + 1      s = origin_stride
//   F[b, tau], F_s[b, tau] = mean over the vectors of bin b (an empty bin gives 0)
//
// x [n_batch][T][n_cols][3]; the columns are n_cols / group replicas of `group` atoms, a call takes the replicas rep0 ..
// rep0 + n_reps - 1 of every batch: row = batch * n_reps + (replica - rep0).  Wave vectors, bins and the phase arithmetic in
// turns are those of K16 (csrc/sk.hip, sk_phase.hpp).
//
// Coherent.  isf_rho_kernel writes rho of every (frame, vector) as partials per block of 1024 atoms (the tiling of
// sk_tile_rho_kernel), summed in index order by whoever reads them.  Forward: isf_corr_kernel walks the origins of each (row,
// lag, vector) in ascending order in double, isf_bins_kernel takes each bin's mean over its vectors in index order.  Backward:
// isf_coef_kernel forms G(k, t) = sum_tau c[b, tau] / (cnt_b |O_tau| W2) [ (t - tau in O_tau) rho(k, t - tau) + (t in O_tau,
// t + tau < T) rho(k, t + tau) ] in double, isf_sweep_kernel applies grad_chunk with (Im G, Re G): a thread per (frame, atom).
//
// Self forward.  exp(i k.(x(t) - x(t0))) = z(t) conj z(t0), z_i(t) = exp(i k.x_i(t)): one sine / cosine pair per (frame, atom,
// vector) and two fused multiply-adds per (origin, lag, atom, vector).  A workgroup owns P = 16 atoms x P / 16 vectors of one
// row and walks through time once.  The phasors of the last n_lags - 1 + ISF_WINDOW frames of its P pairs live in an LDS ring;
// per window of ISF_WINDOW = 8 new frames thread (pair p, lag class j) holds z_p(t) of the window in registers and takes every
// lag tau = j, j + 256 / P, ... of every frame of the window from the ring.  Every position is read from HBM once per vector
// chunk whatever n_lags is.  Ring layout: [slot][re | im][pair] floats, P = 64, 128 or 256 and pair = thread % P, so the 64
// lanes of a wave read 64 consecutive dwords of one plane of one slot: whichever 32 lanes the LDS serves together fall on 32
// different banks, no conflict; the accumulators [lag][pair] likewise.  Large n_lags shrink P (256, 128, 64) so that ring +
// accumulators + the staged window stay within 64 KiB; ISF_MAX_LAGS is what fits at P = 64.  Partials per (row, vector, lag,
// atom tile) go to the workspace; isf_self_finish_kernel sums tiles, then the bin's vectors, in index order in double.
//
// Self backward.  A workgroup owns 4 atoms x 64 frames of one row, thread = (frame, atom).  It converts the positions of the
// frames [t_lo - (n_lags - 1), t_hi + n_lags - 1] of its atoms to turns once (registers), and per chunk of 8 vectors stages
// their phasors as [frame][re | im][vector][atom] with a frame stride of 2 * 32 + 4 floats: the 32 lanes the LDS serves
// together are 8 frames x 4 atoms, 8 * 4 consecutive dwords modulo 32 banks, no conflict.  The gather looks back and ahead:
//   H(k)    = sum_tau C(k, tau) [ (t - tau in O_tau) z(t - tau) + (t in O_tau, t + tau < T) z(t + tau) ]
//   gx_i(t) = w_i^2 sum_k k [ Re z_i(t) Im H - Im z_i(t) Re H ]          C(k, tau) = c[b, tau] / (cnt_b |O_tau| W2)
// With T <= 64 every phasor is computed once; longer trajectories recompute the n_lags - 1 frames on either side of a window.
// Every gx element is written exactly once (the caller passes uninitialised memory), an atom of weight 0 gets exactly 0.
//
// Order of the sums, the same in every launch (no floating-point read-modify-write to global memory by more than one thread;
// two launches give the same bits).  Self forward: per (pair, lag) over the origins in ascending order in float32 (chain depth
// |O_tau| <= T), the xor-shuffle tree over the 16 atoms of a tile, then tiles and vectors in double.  Self backward: per
// (frame, atom, vector) the lags in ascending order, the 8 vectors of a chunk, the chunks in ascending order.
#include "common.hpp"
#include "sk_phase.hpp"

namespace {

constexpr int ISF_BLOCK = 256;
constexpr int ISF_TILE_SHIFT = 4;        // self forward: atoms per tile = 1 << shift = 16
constexpr int ISF_WINDOW = 8;            // self forward: new frames per step of the ring
constexpr int ISF_PAIR_SHIFT = 8;        // self forward: (atom, vector) pairs per workgroup = 1 << shift = 256 at most ...
constexpr int ISF_MIN_PAIR_SHIFT = 6;    // ... and one wave's worth at least
constexpr int ISF_BWD_ATOMS = 4;         // self backward: atoms x vectors x frames of a workgroup
constexpr int ISF_BWD_VECS = 8;
constexpr int ISF_BWD_FRAMES = ISF_BLOCK / ISF_BWD_ATOMS;
constexpr int ISF_RHO_ATOMS = 1024;      // coherent: atom block of the rho partials
constexpr int ISF_LDS_BYTES = 65536;
constexpr int ISF_MAX_ATOMS = 32768;     // the limits of K16 (csrc/sk.hip)
constexpr int ISF_MAX_VECS = 65536;
constexpr int ISF_MAX_BINS = 1024;
constexpr int ISF_COHERENT = 0, ISF_SELF = 1;

// LDS bytes of the self forward (ring of L - 1 + window slots of 2 P floats, an accumulator per (lag, pair), the window's
// atoms in turns, the chunk's vectors) and of the self backward (2 (L - 1) + 64 frames of 2 * 32 + 4 floats, a coefficient
// per (vector, lag), the chunk's vectors)
constexpr long long isf_fwd_lds(int L, int sh) {
    return 4ll * ((long long)(L - 1 + ISF_WINDOW) * (2 << sh) + ((long long)L << sh) + ISF_WINDOW * (8 << ISF_TILE_SHIFT) +
                  4 * (1 << (sh - ISF_TILE_SHIFT)));
}
constexpr int ISF_BWD_PAIRS = ISF_BWD_ATOMS * ISF_BWD_VECS, ISF_BWD_SLOT = 2 * ISF_BWD_PAIRS + ISF_BWD_ATOMS;
constexpr long long isf_bwd_lds(int L) {
    return 4ll * ((long long)(2 * (L - 1) + ISF_BWD_FRAMES) * ISF_BWD_SLOT + (long long)ISF_BWD_VECS * L + 4 * ISF_BWD_VECS);
}
constexpr int isf_max_lags() {
    int L = 1;
    while (isf_fwd_lds(L + 1, ISF_MIN_PAIR_SHIFT) <= ISF_LDS_BYTES && isf_bwd_lds(L + 1) <= ISF_LDS_BYTES) ++L;
    return L;
}
constexpr int ISF_MAX_LAGS = isf_max_lags();
static_assert((2 * (ISF_MAX_LAGS - 1) + ISF_BWD_FRAMES) * ISF_BWD_ATOMS <= 4 * ISF_BLOCK, "self backward: four staged atoms per thread");
// the largest pair tile whose LDS fits
inline int isf_fwd_shift(int L) {
    for (int sh = ISF_PAIR_SHIFT; sh >= ISF_MIN_PAIR_SHIFT; --sh) if (isf_fwd_lds(L, sh) <= ISF_LDS_BYTES) return sh;
    return -1;
}

struct IsfArgs {
    SkArgs s;                // w, kvec, seg, M, B, L of the shared phase code
    const float* x;          // [n_batch, T, C, 3]
    const float* gF;         // backward: [rows, B, L]
    float* F;                // forward:  [rows, B, L]
    float* gx;               // backward: [n_batch, T, C, 3]
    float* ws;
    int T, C, group, rep0, reps, L, stride;
    int sh, ring, tiles;     // self forward: pairs = 1 << sh, ring slots, atom tiles of a row
    int nb;                  // coherent: atom blocks of the rho partials
    long long rows;
    double norm;             // W2
};

__host__ __device__ inline int isf_atom_blocks(int n) { return (n + ISF_RHO_ATOMS - 1) / ISF_RHO_ATOMS; }
__device__ __forceinline__ double isf_origins(int T, int tau, int stride) { return (double)((T - 1 - tau) / stride + 1); }
// offset of atom 0 of frame 0 of a row in x / gx
__device__ __forceinline__ size_t isf_base(const IsfArgs& A, long long row) {
    const long long b = row / A.reps;
    const int r = (int)(row - b * A.reps);
    return ((size_t)b * A.T * A.C + (size_t)(A.rep0 + r) * A.group) * 3;
}

// ---------------------------------------------------------------------------------- coherent
// grid (rows T, nb nc): partial rho of the chunk's 256 vectors over the block's atoms -> ws [rows T, nb, M] float2
__global__ __launch_bounds__(ISF_BLOCK) void isf_rho_kernel(const IsfArgs A) {
    __shared__ float4 sa[ISF_RHO_ATOMS], sb[ISF_RHO_ATOMS];
    const int nb = A.nb, ib = blockIdx.y % nb, ic = blockIdx.y / nb, t = threadIdx.x, M = A.s.M;
    const long long f = blockIdx.x, row = f / A.T;
    const int fr = (int)(f - row * A.T);
    const int i0 = ib * ISF_RHO_ATOMS, na = min(ISF_RHO_ATOMS, A.group - i0);
    const float* p = A.x + isf_base(A, row) + (size_t)fr * A.C * 3;
    for (int i = t; i < na; i += ISF_BLOCK) {
        float4 a, b;
        load_atom(A.s, p, i0 + i, a, b);
        sa[i] = a; sb[i] = b;
    }
    __syncthreads();
    const int m = ic * ISF_BLOCK + t;
    if (m >= M) return;
    const float4 n = load_n(A.s.kvec, m);
    float re, im;
    rho_sweep(sa, sb, na, n.x, n.y, n.z, re, im);
    reinterpret_cast<float2*>(A.ws)[((size_t)f * nb + ib) * M + m] = make_float2(re, im);
}

// rho of vector m of frame f: the atom blocks' partials in index order
__device__ __forceinline__ float2 isf_rho_total(const IsfArgs& A, long long f, int m) {
    const float2* part = reinterpret_cast<const float2*>(A.ws) + (size_t)f * A.nb * A.s.M + m;
    float2 r = make_float2(0.f, 0.f);
    for (int ib = 0; ib < A.nb; ++ib) { const float2 q = part[(size_t)ib * A.s.M]; r.x += q.x; r.y += q.y; }
    return r;
}
__device__ __forceinline__ double* isf_corr(const IsfArgs& A) {          // behind the partials: [rows, L, M] double
    return reinterpret_cast<double*>(A.ws + 2 * (size_t)A.rows * A.T * A.nb * A.s.M);
}

// a thread per (row, lag, vector): sum over the origins in ascending order of Re rho(t0 + tau) conj rho(t0), in double
__global__ __launch_bounds__(ISF_BLOCK) void isf_corr_kernel(const IsfArgs A) {
    const long long i = (long long)blockIdx.x * ISF_BLOCK + threadIdx.x;
    const int M = A.s.M;
    if (i >= A.rows * A.L * M) return;
    const int m = (int)(i % M), tau = (int)((i / M) % A.L);
    const long long f0 = (i / ((long long)M * A.L)) * A.T;
    double s = 0.0;
    for (int t0 = 0; t0 + tau < A.T; t0 += A.stride) {
        const float2 a = isf_rho_total(A, f0 + t0, m), b = isf_rho_total(A, f0 + t0 + tau, m);
        s += (double)a.x * (double)b.x + (double)a.y * (double)b.y;
    }
    isf_corr(A)[i] = s;
}

// a thread per (row, bin, lag): the bin's vectors in index order, then 1 / (cnt |O_tau| W2)
__global__ __launch_bounds__(ISF_BLOCK) void isf_bins_kernel(const IsfArgs A) {
    const long long i = (long long)blockIdx.x * ISF_BLOCK + threadIdx.x;
    const int B = A.s.B, M = A.s.M;
    if (i >= A.rows * B * A.L) return;
    const int tau = (int)(i % A.L), b = (int)((i / A.L) % B);
    const long long row = i / ((long long)A.L * B);
    const int m_lo = A.s.seg[b], m_hi = A.s.seg[b + 1];
    const double* c = isf_corr(A) + ((size_t)row * A.L + tau) * M;
    double s = 0.0;
    for (int m = m_lo; m < m_hi; ++m) s += c[m];
    A.F[i] = m_hi > m_lo ? (float)(s / ((double)(m_hi - m_lo) * isf_origins(A.T, tau, A.stride) * A.norm)) : 0.f;
}

// backward, a thread per (frame, vector): (Im G, Re G) -> ws behind the partials, [rows T, M] float2
__global__ __launch_bounds__(ISF_BLOCK) void isf_coef_kernel(const IsfArgs A) {
    const long long i = (long long)blockIdx.x * ISF_BLOCK + threadIdx.x;
    const int M = A.s.M, T = A.T;
    if (i >= A.rows * T * M) return;
    const int m = (int)(i % M);
    const long long f = i / M, row = f / T, f0 = row * T;
    const int t = (int)(f - f0);
    const int b = bin_of(A.s.seg, A.s.B, m);
    const double inv = 1.0 / ((double)(A.s.seg[b + 1] - A.s.seg[b]) * A.norm);
    const float* g = A.gF + ((size_t)row * A.s.B + b) * A.L;
    const bool origin = t % A.stride == 0;
    double gre = 0.0, gim = 0.0;
    for (int tau = 0; tau < A.L; ++tau) {
        const double c = (double)g[tau] * inv / isf_origins(T, tau, A.stride);
        if (t - tau >= 0 && (t - tau) % A.stride == 0) {
            const float2 r = isf_rho_total(A, f0 + t - tau, m);
            gre += c * (double)r.x; gim += c * (double)r.y;
        }
        if (origin && t + tau < T) {
            const float2 r = isf_rho_total(A, f0 + t + tau, m);
            gre += c * (double)r.x; gim += c * (double)r.y;
        }
    }
    float2* out = reinterpret_cast<float2*>(A.ws) + (size_t)A.rows * T * A.nb * M;
    out[i] = make_float2((float)gim, (float)gre);
}

// gx of one atom: the sum in turns times w 2 pi / L; weight 0 gives exactly 0
__device__ __forceinline__ void isf_put_grad(const IsfArgs& A, float* o, float w, const float (&g)[3]) {
    const float c = w * 6.283185307179586f;
    const bool on = w != 0.f;
    o[0] = on ? c * g[0] / A.s.L[0] : 0.f; o[1] = on ? c * g[1] / A.s.L[1] : 0.f; o[2] = on ? c * g[2] / A.s.L[2] : 0.f;
}

// backward, grid (rows T, ceil(group / 256)): a thread per atom walks all vectors, a chunk of 256 at a time
__global__ __launch_bounds__(ISF_BLOCK) void isf_sweep_kernel(const IsfArgs A) {
    __shared__ float4 snv[ISF_BLOCK];
    __shared__ float2 sab[ISF_BLOCK];
    const int t = threadIdx.x, M = A.s.M, i = blockIdx.y * ISF_BLOCK + t;
    const long long f = blockIdx.x, row = f / A.T;
    const size_t off = isf_base(A, row) + (size_t)(f - row * A.T) * A.C * 3;
    const float2* coef = reinterpret_cast<const float2*>(A.ws) + (size_t)A.rows * A.T * A.nb * M + (size_t)f * M;
    float4 oa, ob;
    load_atom(A.s, A.x + off, min(i, A.group - 1), oa, ob);
    float g[3] = {0.f, 0.f, 0.f};
    for (int m0 = 0; m0 < M; m0 += ISF_BLOCK) {
        const int m = m0 + t;
        __syncthreads();                                         // the previous chunk has been read
        snv[t] = load_n(A.s.kvec, m < M ? m : M - 1);
        sab[t] = m < M ? coef[m] : make_float2(0.f, 0.f);
        __syncthreads();
        if (i < A.group) grad_chunk(snv, sab, min(ISF_BLOCK, M - m0), oa, ob, g);
    }
    if (i < A.group) isf_put_grad(A, A.gx + off + (size_t)i * 3, oa.w, g);
}

// ---------------------------------------------------------------------------------- self
// block = (row, atom tile, vector chunk).  thread = (pair p = tid % P, lag class j = tid / P); pair = (vector p / 16, atom p % 16)
__global__ __launch_bounds__(ISF_BLOCK) void isf_self_fwd_kernel(const IsfArgs A) {
    extern __shared__ float sm[];
    constexpr int TA = 1 << ISF_TILE_SHIFT, W = ISF_WINDOW;
    const int P = 1 << A.sh, KC = P >> ISF_TILE_SHIFT, J = ISF_BLOCK >> A.sh, RB = A.ring, L = A.L, T = A.T, M = A.s.M;
    float* ring = sm;                                            // [RB][2][P]
    float* acc = ring + (size_t)RB * 2 * P;                      // [L][P]
    float4* sa = reinterpret_cast<float4*>(acc + (size_t)L * P); // [W][TA] the window's atoms in turns
    float4* sb = sa + W * TA;
    float4* snv = sb + W * TA;                                   // [KC]
    const int tid = threadIdx.x, p = tid & (P - 1), j = tid >> A.sh, a = p & (TA - 1);
    const int nch = (M + KC - 1) / KC;
    const long long bid = blockIdx.x, rt = bid / nch, row = rt / A.tiles;
    const int chunk = (int)(bid - rt * nch), tile = (int)(rt - row * A.tiles);
    const int a0 = tile << ISF_TILE_SHIFT, n_valid = min(TA, A.group - a0), m0 = chunk * KC;
    const float* xt = A.x + isf_base(A, row);

    if (tid < KC) snv[tid] = load_n(A.s.kvec, min(m0 + tid, M - 1));
    for (int tau = j; tau < L; tau += J) acc[tau * P + p] = 0.f;      // this thread's own accumulators
    for (int tw = 0; tw < T; tw += W) {
        const int slot_w = tw % RB;
        __syncthreads();                                         // the previous window's reads are done (and snv is there)
        if (tid < W * TA && tw + (tid >> ISF_TILE_SHIFT) < T)
            load_atom(A.s, xt + (size_t)(tw + (tid >> ISF_TILE_SHIFT)) * A.C * 3, a0 + min(tid & (TA - 1), n_valid - 1), sa[tid],
                      sb[tid]);
        __syncthreads();
        for (int i = tid; i < W * P; i += ISF_BLOCK) {           // the window's phasors into their ring slots
            const int fr = i >> A.sh, pp = i & (P - 1);
            if (tw + fr < T) {
                const float4 n = snv[pp >> ISF_TILE_SHIFT];
                const int at = fr * TA + (pp & (TA - 1));
                float s, c;
                sincos_turns(phase(n.x, n.y, n.z, sa[at], sb[at]), s, c);
                int slot = slot_w + fr;
                if (slot >= RB) slot -= RB;
                ring[(size_t)slot * 2 * P + pp] = c;
                ring[(size_t)slot * 2 * P + P + pp] = s;
            }
        }
        __syncthreads();
        float zc[W], zs[W];
        {
            int slot = slot_w;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const float* q = ring + (size_t)slot * 2 * P + p;    // (frames past T: stale slots, never used below)
                zc[w] = q[0]; zs[w] = q[P];
                slot = slot + 1 == RB ? 0 : slot + 1;
            }
        }
        for (int tau = j; tau < L; tau += J) {
            const int e = tw - tau;                              // the earlier frame of the window's first frame; > -RB
            int slot = (e + RB) % RB;
            int rs = A.stride > 1 ? ((e % A.stride) + A.stride) % A.stride : 0;
            float s = acc[tau * P + p];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const float* q = ring + (size_t)slot * 2 * P + p;
                const float term = fmaf(zc[w], q[0], zs[w] * q[P]);
                if (e + w >= 0 && tw + w < T && rs == 0) s += term;   // t0 = e + w is an origin of this lag
                slot = slot + 1 == RB ? 0 : slot + 1;
                rs = rs + 1 >= A.stride ? 0 : rs + 1;
            }
            acc[tau * P + p] = s;
        }
    }
    // over the tile's atoms with w^2: xor-shuffle tree inside each group of 16 lanes (the loop bound is uniform)
    float wa = 0.f;
    if (a < n_valid) { wa = A.s.w ? A.s.w[a0 + a] : 1.f; wa *= wa; }
    const int m = m0 + (p >> ISF_TILE_SHIFT);
    for (int tb = 0; tb < L; tb += J) {
        const int tau = tb + j;
        float v = tau < L ? wa * acc[tau * P + p] : 0.f;
        v = group_sum_rt(v, TA);
        if (a == 0 && tau < L && m < M) A.ws[(((size_t)row * M + m) * L + tau) * A.tiles + tile] = v;
    }
}

// a thread per (row, bin, lag): tiles, then the bin's vectors, in index order in double; then 1 / (cnt |O_tau| W2)
__global__ __launch_bounds__(ISF_BLOCK) void isf_self_finish_kernel(const IsfArgs A) {
    const long long i = (long long)blockIdx.x * ISF_BLOCK + threadIdx.x;
    const int B = A.s.B, M = A.s.M, L = A.L;
    if (i >= A.rows * B * L) return;
    const int tau = (int)(i % L), b = (int)((i / L) % B);
    const long long row = i / ((long long)L * B);
    const int m_lo = A.s.seg[b], m_hi = A.s.seg[b + 1];
    double s = 0.0;
    for (int m = m_lo; m < m_hi; ++m) {
        const float* part = A.ws + (((size_t)row * M + m) * L + tau) * A.tiles;
        double sm = 0.0;
        for (int k = 0; k < A.tiles; ++k) sm += (double)part[k];
        s += sm;
    }
    A.F[i] = m_hi > m_lo ? (float)(s / ((double)(m_hi - m_lo) * isf_origins(A.T, tau, A.stride) * A.norm)) : 0.f;
}

// block = (row, tile of 4 atoms, window of 64 frames).  thread = (atom a = tid % 4, frame w = tid / 4)
__global__ __launch_bounds__(ISF_BLOCK) void isf_self_bwd_kernel(const IsfArgs A) {
    extern __shared__ float sm[];
    constexpr int TA = ISF_BWD_ATOMS, KC = ISF_BWD_VECS, WB = ISF_BWD_FRAMES, P = ISF_BWD_PAIRS, FS = ISF_BWD_SLOT;
    const int L = A.L, T = A.T, M = A.s.M, B = A.s.B;
    float* ring = sm;                                            // [frames][re | im][vector][atom], frame stride FS
    float* ctab = ring + (size_t)(2 * (L - 1) + WB) * FS;        // [KC][L]
    float4* snv = reinterpret_cast<float4*>(ctab + KC * L);      // [KC]
    const int tid = threadIdx.x, a = tid & (TA - 1), w = tid / TA;
    const int nwin = (T + WB - 1) / WB, tiles = (A.group + TA - 1) / TA;
    const long long bid = blockIdx.x, rt = bid / nwin, row = rt / tiles;
    const int win = (int)(bid - rt * nwin), tile = (int)(rt - row * tiles);
    const int a0 = tile * TA, n_valid = min(TA, A.group - a0);
    const int tw = win * WB, lo = max(0, tw - (L - 1)), hi = min(T, tw + WB + L - 1), nf = hi - lo;
    const size_t base = isf_base(A, row);

    float4 ra[4], rb[4];                                         // the staged (frame, atom) items of this thread, in turns
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int item = tid + q * ISF_BLOCK, fr = item / TA;
        if (fr < nf) load_atom(A.s, A.x + base + (size_t)(lo + fr) * A.C * 3, a0 + min(item & (TA - 1), n_valid - 1), ra[q], rb[q]);
        else ra[q] = rb[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int t = tw + w;
    const bool live = t < T && a < n_valid;
    const bool origin = t % A.stride == 0;
    float g[3] = {0.f, 0.f, 0.f};
    for (int m0 = 0; m0 < M; m0 += KC) {
        const int kc = min(KC, M - m0);
        __syncthreads();                                         // the previous chunk has been read
        if (tid < KC) snv[tid] = load_n(A.s.kvec, min(m0 + tid, M - 1));
        for (int i = tid; i < KC * L; i += ISF_BLOCK) {
            const int k = i / L, tau = i - k * L, m = m0 + k;
            float c = 0.f;
            if (m < M) {
                const int b = bin_of(A.s.seg, B, m);
                c = (float)((double)A.gF[((size_t)row * B + b) * L + tau] /
                            ((double)(A.s.seg[b + 1] - A.s.seg[b]) * isf_origins(T, tau, A.stride) * A.norm));
            }
            ctab[i] = c;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int item = tid + q * ISF_BLOCK, fr = item / TA, aa = item & (TA - 1);
            if (fr < nf) {
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const float4 n = snv[k];
                    float s, c;
                    sincos_turns(phase(n.x, n.y, n.z, ra[q], rb[q]), s, c);
                    ring[fr * FS + k * TA + aa] = c;
                    ring[fr * FS + P + k * TA + aa] = s;
                }
            }
        }
        __syncthreads();
        if (live) {
            const int s0 = t - lo;
            float lx = 0.f, ly = 0.f, lz = 0.f;
            for (int k = 0; k < kc; ++k) {
                const float* z = ring + s0 * FS + k * TA + a;
                const float* ck = ctab + k * L;
                float hre = 0.f, him = 0.f;
                int rs = A.stride > 1 ? t % A.stride : 0;        // (t - tau) % stride, tau = 0
                for (int tau = 1; tau < L; ++tau) {
                    rs = rs == 0 ? A.stride - 1 : rs - 1;
                    const float c = ck[tau];
                    if (t - tau >= 0 && rs == 0) {
                        const float* q = z - tau * FS;
                        hre = fmaf(c, q[0], hre); him = fmaf(c, q[P], him);
                    }
                    if (origin && t + tau < T) {
                        const float* q = z + tau * FS;
                        hre = fmaf(c, q[0], hre); him = fmaf(c, q[P], him);
                    }
                }
                const float v = fmaf(z[0], him, -(z[P] * hre));
                const float4 n = snv[k];
                lx = fmaf(n.x, v, lx); ly = fmaf(n.y, v, ly); lz = fmaf(n.z, v, lz);
            }
            g[0] += lx; g[1] += ly; g[2] += lz;
        }
    }
    if (live) {
        const float wa = A.s.w ? A.s.w[a0 + a] : 1.f;
        isf_put_grad(A, A.gx + base + ((size_t)t * A.C + a0 + a) * 3, wa * wa, g);
    }
}

// ---------------------------------------------------------------------------------- host
int isf_args(IsfArgs& A, const char* who, int kind, const float* x, int n_batch, int n_frames, int n_cols, int group, int rep0,
             int n_reps, const MdgCell* cell, const float* weights, double norm, const int32_t* kvec, int n_vecs,
             const int32_t* seg, int n_bins, int n_lags, int origin_stride, const float* workspace) {
    MDG_CHECK_ARG(kind == ISF_COHERENT || kind == ISF_SELF, "%s: kind must be 0 (coherent) or 1 (self), got %d", who, kind);
    MDG_CHECK_ARG(x && cell && kvec && seg && workspace, "%s: null argument", who);
    MDG_CHECK_ARG(n_batch > 0 && n_frames > 0 && n_cols > 0 && group > 0, "%s: empty input (batch %d, frames %d, columns %d, "
                  "group %d)", who, n_batch, n_frames, n_cols, group);
    MDG_CHECK_ARG(n_cols % group == 0, "%s: the columns (%d) must be a multiple of the group (%d)", who, n_cols, group);
    MDG_CHECK_ARG(rep0 >= 0 && n_reps >= 1 && rep0 + (long long)n_reps <= n_cols / group, "%s: replicas %d .. %d + %d are not "
                  "among the %d of the columns", who, rep0, rep0, n_reps, n_cols / group);
    MDG_CHECK_ARG(kind == ISF_SELF || group <= ISF_MAX_ATOMS, "%s: at most %d atoms per replica, got %d", who, ISF_MAX_ATOMS, group);
    MDG_CHECK_ARG(n_lags >= 1 && n_lags <= n_frames, "%s: 1 <= lags <= frames (got %d, %d)", who, n_lags, n_frames);
    MDG_CHECK_ARG(n_lags <= ISF_MAX_LAGS, "%s: at most %d lags (got %d)", who, ISF_MAX_LAGS, n_lags);
    MDG_CHECK_ARG(origin_stride >= 1, "%s: origin_stride must be >= 1 (got %d)", who, origin_stride);
    MDG_CHECK_ARG(n_vecs >= 1 && n_vecs <= ISF_MAX_VECS, "%s: 1..%d wave vectors, got %d (max_per_bin thins them)", who,
                  ISF_MAX_VECS, n_vecs);
    MDG_CHECK_ARG(n_bins >= 1 && n_bins <= ISF_MAX_BINS, "%s: 1..%d bins, got %d", who, ISF_MAX_BINS, n_bins);
    MDG_CHECK_ARG(cell->diag, "%s: the cell must be diagonal (triclinic cells are not supported)", who);
    MDG_CHECK_ARG(cell->h[0] > 0.f && cell->h[4] > 0.f && cell->h[8] > 0.f, "%s: the cell lengths must be positive", who);
    MDG_CHECK_ARG(norm > 0.0, "%s: norm = sum of the squared weights must be positive, got %g", who, norm);
    A = IsfArgs{};
    A.s.w = weights; A.s.kvec = kvec; A.s.seg = seg; A.s.M = n_vecs; A.s.B = n_bins;
    A.s.L[0] = cell->h[0]; A.s.L[1] = cell->h[4]; A.s.L[2] = cell->h[8];
    A.x = x; A.ws = const_cast<float*>(workspace);
    A.T = n_frames; A.C = n_cols; A.group = group; A.rep0 = rep0; A.reps = n_reps; A.L = n_lags;
    A.stride = origin_stride < n_frames ? origin_stride : n_frames;          // beyond T - 1 only origin 0 is left either way
    A.rows = (long long)n_batch * n_reps;
    A.nb = isf_atom_blocks(group);
    A.norm = norm;
    const long long frames = A.rows * n_frames;
    MDG_CHECK_ARG(frames < (1ll << 31) && frames * n_vecs < (1ll << 31) * ISF_BLOCK && A.rows * n_bins * n_lags < (1ll << 31) *
                  ISF_BLOCK && A.rows * n_lags * n_vecs < (1ll << 31) * ISF_BLOCK, "%s: %lld frames x %d vectors exceed the "
                  "grid (chunk the rows)", who, frames, n_vecs);
    return MDG_OK;
}

inline unsigned isf_blocks(long long n) { return (unsigned)((n + ISF_BLOCK - 1) / ISF_BLOCK); }

void isf_rho(const IsfArgs& A, hipStream_t st) {
    const int nc = (A.s.M + ISF_BLOCK - 1) / ISF_BLOCK;
    hipLaunchKernelGGL(isf_rho_kernel, dim3((unsigned)(A.rows * A.T), A.nb * nc), dim3(ISF_BLOCK), 0, st, A);
}

}  // namespace

// floats of workspace of one call on n_rows = n_batch * n_reps rows (the larger of forward and backward)
extern "C" int64_t mdg_isf_workspace(int kind, int64_t n_rows, int n_frames, int group, int n_vecs, int n_lags) {
    if (n_rows <= 0 || n_frames <= 0 || group <= 0 || n_vecs <= 0 || n_lags < 1 || n_lags > ISF_MAX_LAGS) return 0;
    if (kind == ISF_SELF) {
        const int64_t tiles = (group + (1 << ISF_TILE_SHIFT) - 1) >> ISF_TILE_SHIFT;
        return n_rows * n_vecs * n_lags * tiles;                                  // partials [rows, M, L, tiles]
    }
    const int64_t nb = isf_atom_blocks(group);
    const int64_t part = 2 * n_rows * n_frames * nb * n_vecs;                    // rho partials [rows T, nb, M] float2
    const int64_t fwd = 2 * n_rows * n_lags * n_vecs, bwd = 2 * n_rows * n_frames * n_vecs;   // [rows, L, M] double | [rows T, M] float2
    return part + (fwd > bwd ? fwd : bwd);
}

extern "C" int mdg_isf_fwd(int kind, const float* x, int n_batch, int n_frames, int n_cols, int group, int rep0, int n_reps,
                           const MdgCell* cell, const float* weights, double norm, const int32_t* kvec, int n_vecs,
                           const int32_t* seg, int n_bins, int n_lags, int origin_stride, float* F, float* workspace,
                           void* stream) {
    IsfArgs A;
    if (int rc = isf_args(A, "isf_fwd", kind, x, n_batch, n_frames, n_cols, group, rep0, n_reps, cell, weights, norm, kvec, n_vecs,
                          seg, n_bins, n_lags, origin_stride, workspace)) return rc;
    MDG_CHECK_ARG(F, "isf_fwd: null argument");
    A.F = F;
    hipStream_t st = (hipStream_t)stream;
    const long long n_out = A.rows * n_bins * n_lags;
    if (kind == ISF_COHERENT) {
        isf_rho(A, st);
        MDG_CHECK_LAUNCH("isf_rho_kernel");
        hipLaunchKernelGGL(isf_corr_kernel, dim3(isf_blocks(A.rows * n_lags * n_vecs)), dim3(ISF_BLOCK), 0, st, A);
        MDG_CHECK_LAUNCH("isf_corr_kernel");
        hipLaunchKernelGGL(isf_bins_kernel, dim3(isf_blocks(n_out)), dim3(ISF_BLOCK), 0, st, A);
    } else {
        A.sh = isf_fwd_shift(n_lags);
        A.ring = n_lags - 1 + ISF_WINDOW;
        A.tiles = (group + (1 << ISF_TILE_SHIFT) - 1) >> ISF_TILE_SHIFT;
        const int kc = 1 << (A.sh - ISF_TILE_SHIFT);
        const long long blocks = A.rows * A.tiles * ((n_vecs + kc - 1) / kc);
        MDG_CHECK_ARG(blocks < (1ll << 31), "isf_fwd: %lld (replica, atom tile, vector chunk) workgroups exceed the grid (chunk "
                      "the rows)", blocks);
        hipLaunchKernelGGL(isf_self_fwd_kernel, dim3((unsigned)blocks), dim3(ISF_BLOCK), (size_t)isf_fwd_lds(n_lags, A.sh), st, A);
        MDG_CHECK_LAUNCH("isf_self_fwd_kernel");
        hipLaunchKernelGGL(isf_self_finish_kernel, dim3(isf_blocks(n_out)), dim3(ISF_BLOCK), 0, st, A);
    }
    MDG_CHECK_LAUNCH("isf forward kernels");
    return MDG_OK;
}

extern "C" int mdg_isf_bwd(int kind, const float* x, int n_batch, int n_frames, int n_cols, int group, int rep0, int n_reps,
                           const MdgCell* cell, const float* weights, double norm, const int32_t* kvec, int n_vecs,
                           const int32_t* seg, int n_bins, int n_lags, int origin_stride, const float* gF, float* gx,
                           float* workspace, void* stream) {
    IsfArgs A;
    if (int rc = isf_args(A, "isf_bwd", kind, x, n_batch, n_frames, n_cols, group, rep0, n_reps, cell, weights, norm, kvec, n_vecs,
                          seg, n_bins, n_lags, origin_stride, workspace)) return rc;
    MDG_CHECK_ARG(gF && gx, "isf_bwd: null argument");
    A.gF = gF; A.gx = gx;
    hipStream_t st = (hipStream_t)stream;
    if (kind == ISF_COHERENT) {
        isf_rho(A, st);
        MDG_CHECK_LAUNCH("isf_rho_kernel");
        hipLaunchKernelGGL(isf_coef_kernel, dim3(isf_blocks(A.rows * n_frames * n_vecs)), dim3(ISF_BLOCK), 0, st, A);
        MDG_CHECK_LAUNCH("isf_coef_kernel");
        hipLaunchKernelGGL(isf_sweep_kernel, dim3((unsigned)(A.rows * n_frames), (group + ISF_BLOCK - 1) / ISF_BLOCK),
                           dim3(ISF_BLOCK), 0, st, A);
    } else {
        const long long blocks = A.rows * ((group + ISF_BWD_ATOMS - 1) / ISF_BWD_ATOMS) *
                                 ((n_frames + ISF_BWD_FRAMES - 1) / ISF_BWD_FRAMES);
        MDG_CHECK_ARG(blocks < (1ll << 31), "isf_bwd: %lld (replica, atom tile, frame window) workgroups exceed the grid (chunk "
                      "the rows)", blocks);
        hipLaunchKernelGGL(isf_self_bwd_kernel, dim3((unsigned)blocks), dim3(ISF_BLOCK), (size_t)isf_bwd_lds(n_lags), st, A);
    }
    MDG_CHECK_LAUNCH("isf backward kernels");
    return MDG_OK;
}

// the tile constants, for callers that size their inputs around them (tests, tools)
extern "C" int mdg_isf_max_lags(void) { return ISF_MAX_LAGS; }
extern "C" int mdg_isf_tile_atoms(void) { return 1 << ISF_TILE_SHIFT; }
extern "C" int mdg_isf_window(void) { return ISF_WINDOW; }
