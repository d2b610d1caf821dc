// K8: soft-histogram radial distribution function and its gradient.
// Replaces rdf.forward (torchmd/observable.py:62-76: generate_nbr_list with cutoff end+0.5
// over all frames -> GaussianSmearing nff/nn/layers.py:14-31 -> sum) and the autograd
// backward through it.  The [pairs, bins] exp matrix of the reference is never
// materialised.
//
// forward : rdf_fwd_plan (host side, end of this file) picks, in this order: fine -- >= 1024 frames of 64 .. 1024 atoms,
//           equally spaced centres: pairs counted on a fine integer histogram per workgroup, smeared onto the centres once
//           (rdf_fwd_fine_kernel); half / lane -- >= 1024 frames, equally spaced centres: one wave per frame, one lane per
//           pair, lane-private LDS histogram columns of half or full width (rdf_fwd_half_kernel, rdf_fwd_lane_kernel);
//           block8 / direct -- few frames or arbitrary centres: persistent blocks stride over (frame, candidate chunk) work
//           items, compact the accepted i<j distances into LDS in a fixed order, a thread owns an 8-bin block with the
//           Gaussian recurrence (rdf_fwd_block8_kernel) or bin k (rdf_fwd_kernel).  Partial histograms are added by a
//           second kernel in a fixed order, integer counts commute => no float atomics, reproducible.  exp is v_exp_f32.
// backward: each accepted pair contributes dL/dd = sum_k g_raw[k] * 2 coeff (d - mu_k) e_k along +/- its unit separation
//           vector.  rdf_bwd_plan: table / frame -- many frames, one wave per frame, dL/dd from a fine table, cyclic pair
//           order with one end's gradient in registers (rdf_bwd_fine_kernel) or the bin recurrence in round-robin-
//           tournament order (rdf_bwd_kernel); atom -- few frames, (frame, atom) gather (rdf_bwd_atom_kernel).  LDS
//           accumulation without atomics.  mdg_rdf_fwd_variant / mdg_rdf_bwd_variant report the plan of a shape.
#include "common.hpp"
#include <type_traits>

namespace {

constexpr int RDF_BLOCK = 512;
constexpr int RDF_MAX_BLOCKS = 2048;     // persistent blocks: each strides over (frame, chunk) work items
constexpr int RDF_CHUNK = 8192;          // candidate pairs per work item
constexpr float LOG2E = 1.4426950408889634f;

// flat index c in [0, N(N-1)/2) -> (i, j), i < j, row-major (the order torch.nonzero yields)
__device__ __forceinline__ void pair_from_flat(long long c, int N, int& i, int& j) {
    const double b = 2.0 * N - 1.0;
    int ii = (int)((b - sqrt(b * b - 8.0 * (double)c)) * 0.5);
    while ((long long)ii * (2LL * N - ii - 1) / 2 > c) --ii;
    while ((long long)(ii + 1) * (2LL * N - ii - 2) / 2 <= c) ++ii;
    i = ii;
    j = (int)(c - (long long)ii * (2LL * N - ii - 1) / 2) + ii + 1;
}

// exp(coeff (d - mu)^2) = exp2(-(s d - s mu)^2) with s = sqrt(-coeff log2 e): distances and
// the sweep costs sub, mul, mul, v_exp_f32, add per (pair, bin).
//
// Thread layout: nbins <= RDF_BLOCK.  G = RDF_BLOCK / nbins thread groups; thread (g, k) owns
// bin k and sweeps the compacted distances 4g..4g+3, 4(g+G).., ... (ds_read_b128); the groups
// are combined in group order at the end.  More than RDF_BLOCK bins are refused (rdf_fwd_impl).
template <bool DIAG>
__global__ __launch_bounds__(RDF_BLOCK) void rdf_fwd_kernel(
    const float* __restrict__ xyz, int nF, int N, MdgCell cell, float rc2, const uint8_t* __restrict__ mask,
    const float* __restrict__ mu, float coeff, int nbins, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float dist[RDF_BLOCK + 4];
    __shared__ int wcnt[RDF_BLOCK / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    constexpr int nw = RDF_BLOCK / 64;
    const float sc = sqrtf(-coeff * LOG2E);
    const int G = RDF_BLOCK / nbins;
    const int grp = threadIdx.x / nbins;
    const bool active = grp < G;
    const int k = threadIdx.x - grp * nbins;
    const float ms = active ? mu[k] : 0.f;
    float acc = 0.f;
    const long long npair = (long long)N * (N - 1) / 2;
    const int chunks = (int)((npair + RDF_CHUNK - 1) / RDF_CHUNK);
    const long long items = (long long)nF * chunks;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int fr = (int)(it / chunks), ch = (int)(it % chunks);
        const float* pos = xyz + (size_t)fr * N * 3;
        const long long c_end = min(npair, (long long)(ch + 1) * RDF_CHUNK);
        long long c = (long long)ch * RDF_CHUNK + threadIdx.x;
        int i = 0, j = 0;
        if (c < c_end) pair_from_flat(c, N, i, j);
        for (long long cb = (long long)ch * RDF_CHUNK; cb < c_end; cb += RDF_BLOCK) {
            float d = -1.f;
            if (c < c_end) {
                float dx = pos[3 * j] - pos[3 * i], dy = pos[3 * j + 1] - pos[3 * i + 1],
                      dz = pos[3 * j + 2] - pos[3 * i + 2];
                min_image<DIAG>(cell, dx, dy, dz);
                const float d2 = norm2_ref(dx, dy, dz);
                bool ok = (d2 < rc2) && (d2 != 0.f);
                if (ok && mask) ok = mask[(size_t)i * N + j] != 0;
                if (ok) d = sqrtf(d2);
                // advance to the candidate RDF_BLOCK further on
                c += RDF_BLOCK;
                j += RDF_BLOCK;
                while (j >= N && i < N - 1) { ++i; j = j - N + i + 1; }
            }
            const unsigned long long b = __ballot(d >= 0.f);
            __syncthreads();                                   // previous sweep done with dist[]
            if (lane == 0) wcnt[wid] = __popcll(b);
            __syncthreads();
            int base = 0, total = 0;
#pragma unroll
            for (int w = 0; w < nw; ++w) { if (w < wid) base += wcnt[w]; total += wcnt[w]; }
            if (d >= 0.f) dist[base + __popcll(b & ((1ull << lane) - 1ull))] = d;
            if (threadIdx.x < 4) dist[total + threadIdx.x] = 3.0e18f;   // pad: exp2(-x^2) == 0
            __syncthreads();
            if (active) {
                for (int p = 4 * grp; p < total; p += 4 * G) {
                    const float4 dd = *reinterpret_cast<const float4*>(&dist[p]);
                    // (d - mu) first, then scale: no cancellation error on the scaled values
                    const float x0 = (dd.x - ms) * sc, x1 = (dd.y - ms) * sc, x2 = (dd.z - ms) * sc,
                                x3 = (dd.w - ms) * sc;
                    acc += __builtin_amdgcn_exp2f(-x0 * x0);
                    acc += __builtin_amdgcn_exp2f(-x1 * x1);
                    acc += __builtin_amdgcn_exp2f(-x2 * x2);
                    acc += __builtin_amdgcn_exp2f(-x3 * x3);
                }
            }
        }
    }
    __syncthreads();
    if (active) dist[threadIdx.x] = acc;                        // [g][k], G * nbins <= RDF_BLOCK
    __syncthreads();
    if (threadIdx.x < nbins) {
        float s = 0.f;
        for (int g = 0; g < G; ++g) s += dist[g * nbins + threadIdx.x];
        partial[(size_t)blockIdx.x * nbins + threadIdx.x] = s;
    }
}

// Variant for equally spaced centres with Ds = s * spacing <= 1 (the default width == spacing gives
// Ds = 0.85): a thread owns a block of 8 consecutive bins and gets their 8 Gaussians of one distance
// from ONE centre evaluation and a two-term recurrence outwards from the block's middle bin
//     e_{j+1} = e_j rho_j , rho_{j+1} = rho_j exp2(-2 Ds^2) , rho = exp2(+-2 Ds x - Ds^2)
// i.e. 3 v_exp_f32 + 14 multiplies per 8 (pair, bin) values instead of 8 exps + 16 multiplies.  The
// recurrence runs at most 4 steps (relative error ~1e-6); a block whose middle bin is farther than the
// exp2 underflow reach from the distance can only miss terms below 2^-60.
constexpr int RDF_KB = 8;

template <bool DIAG>
__global__ __launch_bounds__(RDF_BLOCK) void rdf_fwd_block8_kernel(
    const float* __restrict__ xyz, int nF, int N, MdgCell cell, float rc2, const uint8_t* __restrict__ mask,
    const float* __restrict__ mu, float coeff, int nbins, float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* dist = sm;                                   // [RDF_BLOCK]
    int* wcnt = (int*)(sm + RDF_BLOCK);                 // [nw]
    float* comb = sm + RDF_BLOCK + 16;                  // [G][nblk*8] final combine
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    constexpr int nw = RDF_BLOCK / 64;
    const float sc = sqrtf(-coeff * LOG2E);
    const int nblk = (nbins + RDF_KB - 1) / RDF_KB;     // bin blocks
    const int G = RDF_BLOCK / nblk;                     // thread groups sharing the sweep
    const int grp = threadIdx.x / nblk;
    const bool active = grp < G;
    const int kb = threadIdx.x - grp * nblk;            // this thread's bin block
    const float mu0 = mu[0];
    const float dmu = (mu[nbins - 1] - mu0) / (float)(nbins - 1);
    const float Ds = dmu * sc;
    const float c2 = __builtin_amdgcn_exp2f(-2.f * Ds * Ds);
    const int kmid = min(nbins - 1, kb * RDF_KB + 4);
    const float mum = active ? mu[kmid] : 0.f;          // centre of the block's middle bin (exact value)
    const float off = (float)(kb * RDF_KB + 4 - kmid) * dmu;   // 0 unless the last block is partial
    float acc[RDF_KB];
#pragma unroll
    for (int j = 0; j < RDF_KB; ++j) acc[j] = 0.f;
    const long long npair = (long long)N * (N - 1) / 2;
    const int chunks = (int)((npair + RDF_CHUNK - 1) / RDF_CHUNK);
    const long long items = (long long)nF * chunks;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int fr = (int)(it / chunks), ch = (int)(it % chunks);
        const float* pos = xyz + (size_t)fr * N * 3;
        const long long c_end = min(npair, (long long)(ch + 1) * RDF_CHUNK);
        long long c = (long long)ch * RDF_CHUNK + threadIdx.x;
        int i = 0, j = 0;
        if (c < c_end) pair_from_flat(c, N, i, j);
        for (long long cb = (long long)ch * RDF_CHUNK; cb < c_end; cb += RDF_BLOCK) {
            float d = -1.f;
            if (c < c_end) {
                float dx = pos[3 * j] - pos[3 * i], dy = pos[3 * j + 1] - pos[3 * i + 1],
                      dz = pos[3 * j + 2] - pos[3 * i + 2];
                min_image<DIAG>(cell, dx, dy, dz);
                const float d2 = norm2_ref(dx, dy, dz);
                bool ok = (d2 < rc2) && (d2 != 0.f);
                if (ok && mask) ok = mask[(size_t)i * N + j] != 0;
                if (ok) d = sqrtf(d2);
                c += RDF_BLOCK;
                j += RDF_BLOCK;
                while (j >= N && i < N - 1) { ++i; j = j - N + i + 1; }
            }
            const unsigned long long b = __ballot(d >= 0.f);
            __syncthreads();                                   // previous sweep done with dist[]
            if (lane == 0) wcnt[wid] = __popcll(b);
            __syncthreads();
            int base = 0, total = 0;
#pragma unroll
            for (int w = 0; w < nw; ++w) { if (w < wid) base += wcnt[w]; total += wcnt[w]; }
            if (d >= 0.f) dist[base + __popcll(b & ((1ull << lane) - 1ull))] = d;
            __syncthreads();
            if (active) {
                for (int p = grp; p < total; p += G) {
                    const float x4 = (dist[p] - mum - off) * sc;          // x at block bin 4
                    // beyond 12 the block's nearest bin is > 12 - 4 Ds >= 8 away: all eight terms are
                    // below 2^-64 (and the ratio below would overflow against an underflowed e4)
                    if (fabsf(x4) >= 12.f) continue;
                    const float e4 = __builtin_amdgcn_exp2f(-x4 * x4);
                    float eu = e4, ed = e4;
                    float ru = __builtin_amdgcn_exp2f(2.f * Ds * x4 - Ds * Ds);     // towards larger mu
                    float rd = __builtin_amdgcn_exp2f(-2.f * Ds * x4 - Ds * Ds);    // towards smaller mu
                    acc[4] += e4;
                    eu *= ru; ru *= c2; acc[5] += eu;
                    ed *= rd; rd *= c2; acc[3] += ed;
                    eu *= ru; ru *= c2; acc[6] += eu;
                    ed *= rd; rd *= c2; acc[2] += ed;
                    eu *= ru;           acc[7] += eu;
                    ed *= rd; rd *= c2; acc[1] += ed;
                    ed *= rd;           acc[0] += ed;
                }
            }
        }
    }
    __syncthreads();
    const int nk = nblk * RDF_KB;
    if (active) {
#pragma unroll
        for (int j = 0; j < RDF_KB; ++j) comb[grp * nk + kb * RDF_KB + j] = acc[j];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nbins; k += RDF_BLOCK) {
        float s = 0.f;
        for (int g = 0; g < G; ++g) s += comb[g * nk + k];
        partial[(size_t)blockIdx.x * nbins + k] = s;
    }
}


// Equally spaced centres, many frames (the replica-batched training shape): one WAVE per frame, one LANE
// per pair.  Each lane owns a private column of a wave-private LDS histogram [rows][64], so a pair's
// Gaussians are deposited with plain (conflict-free, order-fixed) LDS adds -- no bin-owner sweep, every
// pair is looked at exactly once.  Only the 2R+1 bins around the nearest centre kc are touched: the
// centre value and two outward recurrences (as in the block-of-8 kernel); the nearest bin left out is
// (R + 1/2) Ds >= 4.65 away, where the Gaussian is below 2^-21.6 of the peak: a relative 3e-7 of a bin's count
// in the worst case, under the fp32 rounding of a sum of thousands of terms.  Real bin k lives in row
// k + 2R; rows outside [2R, 2R + nbins) are write-only padding so that no deposit needs a bounds test.
// The recurrence places the neighbours of bin kc at mu[kc] +- s dmu; every deposited value is taken to the centre as given
// by a first-order factor (rdf_centre_offset below).
// The columns are summed in a fixed order at the end => bitwise reproducible.
//
// The pairs come from a table built once per call (it stays in L1/L2): entry = (4 i) | (4 j2) << 16 stands for
// the TWO pairs (i, j2), (i, j2 + 1) with j2 even, rows in order, j2 from (i + 1) & ~1.  No index arithmetic in
// the loop (the closed-form round-robin order this replaces spent 27 of its 95 VALU instructions per pair on
// it); the i coordinates are an LDS broadcast, the two j's one aligned ds_read_b64 per component, already in
// packed-fp32 register pairs.  Slots that are not pairs need no flags: (i, i) -- the first slot of an even
// row -- is rejected by the d2 != 0 test of topology.py:67, column N of an odd N and the columns the padding
// entries point at hold NaN, and NaN < cutoff^2 is false.
__host__ __device__ inline int rdf_row_entries(int i, int N) { return (N + 1 - ((i + 1) & ~1)) >> 1; }

__global__ __launch_bounds__(256) void rdf_pair_table_kernel(uint32_t* __restrict__ tab, int N, int n_entries,
                                                             int n_padded, uint32_t pad_entry) {
    __shared__ int off_s;
    const int i = blockIdx.x;
    if (i < N - 1) {
        if (threadIdx.x == 0) off_s = 0;
        __syncthreads();
        int part = 0;
        for (int k = threadIdx.x; k < i; k += blockDim.x) part += rdf_row_entries(k, N);
        if (part) atomicAdd(&off_s, part);
        __syncthreads();
        const int off = off_s, j0 = (i + 1) & ~1, cnt = rdf_row_entries(i, N);
        for (int e = threadIdx.x; e < cnt; e += blockDim.x)
            tab[off + e] = (uint32_t)(4 * i) | ((uint32_t)(4 * (j0 + 2 * e)) << 16);
    } else {
        for (int p_ = n_entries + threadIdx.x; p_ < n_padded; p_ += blockDim.x) tab[p_] = pad_entry;
    }
}

constexpr int RDF_TABLE_MAX_ATOMS = 4096;      // 4 j < 2^16 and a table of at most 16 MB

// Constants of the deposit: e_{+-s} = e0 r^s K_s with r = exp2(+-2 Ds x0 - Ds^2) <= 1 and K_s = c2^(s(s-1)/2),
// K_0 = K_1 = 1.  Bins are handled two adjacent rows at a time (one ds_read2st64 / ds_write2st64 and one packed
// fma per two bins): the packed power {r^s, r^(s+1)} advances by r^2.  Outward chain s = 0 (the centre) .. R,
// inward chain s = 1 .. R.
// The recurrences of the lane and half kernels step from a centre to its neighbours by Ds = s dmu: they take the centres as
// exactly equidistant.  The float32 linspace centres are that to an ulp only, and a centre's shift is the same for every pair
// of its bin, so it does not average out (1.3e-6 .. 8e-6 of the largest bin against the float64 sum, growing like 1 / sigma).
// Per row, 2 ln 2 x the scaled offset of the centre as given from the grid the recurrence walks, delta_k = s (mu_k - mu_0) -
// k Ds: a value reached from anchor row a belongs to x + (delta_k - delta_a) and is multiplied by 1 + x 2 ln 2 (delta_k -
// delta_a), the first order of exp2(-(x - eps)^2) / exp2(-x^2) (eps < 1e-4: the second order is below 1e-8).
__device__ __forceinline__ float rdf_centre_offset(float centre, float mu0, float sc, float Ds, int k) {
    return (float)(1.3862943611198906 * (((double)centre - (double)mu0) * (double)sc - (double)k * (double)Ds));
}

template <int R>
struct RdfLane {
    static constexpr int NPO = (R + 1) / 2, NPI = R / 2;
    static constexpr bool TAIL_O = ((R + 1) & 1) != 0, TAIL_I = (R & 1) != 0;   // one unpaired row at the far end
    float sc, mu0, inv_dmu, dmu, Ds, Ds2, Klast;
    f32x2 Ko[NPO], Ki[NPI > 0 ? NPI : 1];                       // outward {K_2m, K_2m+1}, inward {K_2m+2, K_2m+1}
    struct Rows { f32x2 vo[NPO]; f32x2 vi[NPI > 0 ? NPI : 1]; float vlo, vli; float* h; };

    __device__ __forceinline__ void init(const float* __restrict__ mu, float coeff, int nbins) {
        sc = sqrtf(-coeff * LOG2E);
        mu0 = mu[0];
        dmu = (mu[nbins - 1] - mu0) / (float)(nbins - 1);
        inv_dmu = 1.f / dmu;
        Ds = dmu * sc; Ds2 = Ds * Ds;
        const float c2 = __builtin_amdgcn_exp2f(-2.f * Ds2);
        float cp = 1.f, K = 1.f, Ks[R + 2];
        Ks[0] = 1.f; Ks[1] = 1.f;
#pragma unroll
        for (int s_ = 2; s_ <= R; ++s_) { cp *= c2; K *= cp; Ks[s_] = K; }
#pragma unroll
        for (int m = 0; m < NPO; ++m) Ko[m] = f32x2{Ks[2 * m], Ks[2 * m + 1]};
#pragma unroll
        for (int m = 0; m < NPI; ++m) Ki[m] = f32x2{Ks[2 * m + 2], Ks[2 * m + 1]};
        Klast = Ks[R];
    }
    // the 2R + 1 rows around bin kc of this lane's column (col = hist + lane)
    __device__ __forceinline__ void rows_load(float* col, int kc, Rows& w) const {
        float* h = col + (size_t)(kc + R) * 64;                  // row of bin kc - R
        w.h = h;
#pragma unroll
        for (int m_ = 0; m_ < NPO; ++m_) w.vo[m_] = f32x2{h[(R + 2 * m_) * 64], h[(R + 2 * m_ + 1) * 64]};
#pragma unroll
        for (int m_ = 0; m_ < NPI; ++m_) w.vi[m_] = f32x2{h[(R - 2 * m_ - 2) * 64], h[(R - 2 * m_ - 1) * 64]};
        w.vlo = 0.f; w.vli = 0.f;
        if (TAIL_O) w.vlo = h[2 * R * 64];
        if (TAIL_I) w.vli = h[0];
    }
    // branch-free: a rejected pair adds +0 (a bitwise no-op) around bin 0.  Plain read-add-write on the
    // lane-private column: ds_add_f32 is serialised per lane in the LDS atomic unit (measured 9x slower).
    // dl = the offsets of rdf_centre_offsets at the window's first row (bin kc - R): the value the recurrence gives for the
    // bin s rows from kc belongs to a centre at mu[kc] +- s dmu; the factor 1 + x eps takes it to the centre as given.
    __device__ __forceinline__ void rows_add_store(Rows& w, float d, float m, bool ok, const float* dl) const {
        const float x0 = ok ? (d - m) * sc : 0.f;
        const float a_ = 2.f * Ds * x0;
        const float e0 = ok ? __builtin_amdgcn_exp2f(-x0 * x0) : 0.f;
        const float rp = __builtin_amdgcn_exp2f(a_ - Ds2), rm = __builtin_amdgcn_exp2f(-a_ - Ds2);
        const float rp2 = rp * rp, rm2 = rm * rm;
        const float dc = dl[R];
        auto fix = [&](int s_) { return fmaf(x0 - (float)s_ * Ds, dl[R + s_] - dc, 1.f); };      // s_ < 0: towards smaller mu
        f32x2 Po = e0 * f32x2{1.f, rp}, Pi = e0 * f32x2{rm2, rm};
#pragma unroll
        for (int m_ = 0; m_ < NPO; ++m_) {
            w.vo[m_] += Ko[m_] * Po * f32x2{fix(2 * m_), fix(2 * m_ + 1)};
            if (m_ + 1 < NPO || TAIL_O) Po *= rp2;
        }
#pragma unroll
        for (int m_ = 0; m_ < NPI; ++m_) {
            w.vi[m_] += Ki[m_] * Pi * f32x2{fix(-2 * m_ - 2), fix(-2 * m_ - 1)};
            if (m_ + 1 < NPI || TAIL_I) Pi *= rm2;
        }
        if (TAIL_O) w.vlo += Klast * Po.x * fix(R);              // Po = {e0 r^R, .} after NPO steps (R even)
        if (TAIL_I) w.vli += Klast * Pi.y * fix(-R);             // Pi = {., e0 r^R} after NPI steps (R odd)
        float* h = w.h;
#pragma unroll
        for (int m_ = 0; m_ < NPO; ++m_) { h[(R + 2 * m_) * 64] = w.vo[m_].x; h[(R + 2 * m_ + 1) * 64] = w.vo[m_].y; }
#pragma unroll
        for (int m_ = 0; m_ < NPI; ++m_) { h[(R - 2 * m_ - 2) * 64] = w.vi[m_].x; h[(R - 2 * m_ - 1) * 64] = w.vi[m_].y; }
        if (TAIL_O) h[2 * R * 64] = w.vlo;
        if (TAIL_I) h[0] = w.vli;
    }
};

// the table entry's two pairs: squared minimum-image distances in packed fp32 (px: SoA rows of stride PXLD)
template <bool DIAG, bool NEAR>
__device__ __forceinline__ f32x2 rdf_entry_d2(const float* px, int PXLD, const MdgCell& cell, float ivx, float ivy, float ivz,
                                              uint32_t t, int& i4, int& j4) {
    i4 = (int)(t & 0xffffu); j4 = (int)(t >> 16);
    const float* pi = reinterpret_cast<const float*>(reinterpret_cast<const char*>(px) + i4);
    const float* pj = reinterpret_cast<const float*>(reinterpret_cast<const char*>(px) + j4);
    f32x2 dx = *reinterpret_cast<const f32x2*>(pj) - pi[0], dy = *reinterpret_cast<const f32x2*>(pj + PXLD) - pi[PXLD],
          dz = *reinterpret_cast<const f32x2*>(pj + 2 * PXLD) - pi[2 * PXLD];
    if constexpr (NEAR) {
        dx = min_image_diag2_near(dx, ivx, cell.h[0]);
        dy = min_image_diag2_near(dy, ivy, cell.h[4]);
        dz = min_image_diag2_near(dz, ivz, cell.h[8]);
    } else if constexpr (DIAG) {
        dx = min_image_diag2(dx, ivx, cell.h[0]);
        dy = min_image_diag2(dy, ivy, cell.h[4]);
        dz = min_image_diag2(dz, ivz, cell.h[8]);
    } else {
        float ax_ = dx.x, ay_ = dy.x, az_ = dz.x, bx_ = dx.y, by_ = dy.y, bz_ = dz.y;
        min_image<false>(cell, ax_, ay_, az_);
        min_image<false>(cell, bx_, by_, bz_);
        dx = f32x2{ax_, bx_}; dy = f32x2{ay_, by_}; dz = f32x2{az_, bz_};
    }
    return norm2_ref2(dx, dy, dz);
}

// a frame's coordinates into SoA LDS rows; true when every atom is within [-0.24, 1.24] cell lengths
// (trajectories are wrapped at every epoch, md.py:66): the image shift is then a plain rint, see
// min_image_diag2_near
template <bool DIAG>
__device__ __forceinline__ bool rdf_load_frame(float* px, int PXLD, const float* __restrict__ pos, int N, int lane,
                                               float ivx, float ivy, float ivz) {
    bool out = false;
    for (int e = lane; e < 3 * N; e += 64) {
        const int c = e % 3;
        const float v = pos[e];
        px[c * PXLD + e / 3] = v;
        if (DIAG) {
            const float s_ = v * (c == 0 ? ivx : c == 1 ? ivy : ivz);
            out |= !(s_ > -0.24f && s_ < 1.24f);
        }
    }
    return DIAG && !__any(out);
}

template <bool DIAG, int R, bool MASKED, int PXC>
__global__ __launch_bounds__(256) void rdf_fwd_lane_kernel(
    const float* __restrict__ xyz, int nF, int N, MdgCell cell, float rc2, const uint8_t* __restrict__ mask,
    const float* __restrict__ mu, float coeff, int nbins, const uint32_t* __restrict__ tab, int iters, int pxld,
    float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int rows = nbins + 4 * R;
    const int PXLD = PXC ? PXC : pxld;                          // row stride of the SoA coordinates (even, >= N + 2)
    float* hist = sm + (size_t)wid * ((size_t)rows * 64 + 3 * PXLD);
    float* px = hist + (size_t)rows * 64;                       // [3][PXLD]   (8-byte aligned: rows * 64 and PXLD are even)
    float* smu = sm + (size_t)nw * ((size_t)rows * 64 + 3 * PXLD);   // [nbins + 2R] centres incl. extrapolated pads
    float* sdl = smu + nbins + 2 * R;                           // [nbins + 4R] rdf_centre_offset of every histogram row
    RdfLane<R> K;
    K.init(mu, coeff, nbins);
    for (int k = threadIdx.x; k < nbins + 2 * R; k += blockDim.x) {
        const int kk = k - R;
        smu[k] = (kk >= 0 && kk < nbins) ? mu[kk] : fmaf((float)kk, K.dmu, K.mu0);
    }
    for (int k = threadIdx.x; k < rows; k += blockDim.x) {
        const int kk = k - 2 * R;
        sdl[k] = rdf_centre_offset((kk >= 0 && kk < nbins) ? mu[kk] : fmaf((float)kk, K.dmu, K.mu0), K.mu0, K.sc, K.Ds, kk);
    }
    for (int e = lane; e < rows * 64; e += 64) hist[e] = 0.f;
    for (int e = lane; e < 3 * PXLD; e += 64) px[e] = (e >= N && e < PXLD) ? __builtin_nanf("") : 0.f;
    __syncthreads();
    const float ivx = cell.inv[0], ivy = cell.inv[4], ivz = cell.inv[8];
    const int gw = blockIdx.x * nw + wid, nwaves = gridDim.x * nw;
    float* col = hist + lane;
    for (int fr = gw; fr < nF; fr += nwaves) {
        const bool near = rdf_load_frame<DIAG>(px, PXLD, xyz + (size_t)fr * N * 3, N, lane, ivx, ivy, ivz);
        f32x2 dd, mm;                 // distances and nearest centres of the two pairs of the current entry
        int kA, kB;
        bool okA, okB;
        // (measured: a single row of fixed-point counters per wave updated with ds_add_u32 -- 2 KB of LDS
        //  instead of 32 KB, many waves per SIMD -- is 3.5x SLOWER: the lanes of a wave hit the same few
        //  bins around the g(r) peak and the atomics serialise; the lane-private columns never conflict.)
        auto sweep = [&](auto near_c) {
            constexpr bool NEAR = decltype(near_c)::value;
            f32x2 d2;
            int mi = 0, mj = 0;
            auto locate_a = [&](uint32_t t) {
                int i4, j4;
                d2 = rdf_entry_d2<DIAG, NEAR>(px, PXLD, cell, ivx, ivy, ivz, t, i4, j4);
                if constexpr (MASKED) { mi = i4 >> 2; mj = j4 >> 2; }
            };
            auto locate_b = [&]() {
                okA = (d2.x < rc2) & (d2.x != 0.f);                              // (bitwise: no short-circuit branches)
                okB = (d2.y < rc2) & (d2.y != 0.f);
                if constexpr (MASKED) {                                          // unconditional loads: no branch
                    okA = okA & (mask[(size_t)mi * N + min(mj, N - 1)] != 0);
                    okB = okB & (mask[(size_t)mi * N + min(mj + 1, N - 1)] != 0);
                }
                // correctly rounded: an error of v_sqrt_f32 (1 ulp) that does not average to zero moves every distance like a
                // shift of the centres, 1 / sigma times as much in the histogram (see rdf_centre_offset)
                dd = f32x2{sqrtf(d2.x), sqrtf(d2.y)};
                const f32x2 tk = (dd - K.mu0) * K.inv_dmu;
                kA = (int)rintf(tk.x); kB = (int)rintf(tk.y);
                okA = okA & (kA >= -R) & (kA <= nbins - 1 + R);
                okB = okB & (kB >= -R) & (kB <= nbins - 1 + R);
                kA = okA ? kA : 0; kB = okB ? kB : 0;
                mm = f32x2{smu[kA + R], smu[kB + R]};
            };
            // software pipeline, unrolled by four so that no register rotates.  Each step deposits the entry
            // located by the previous step and locates the one of the next iteration in the shadow of the row
            // reads: first pair's rows | coordinates, squared distances | first deposit | second pair's rows
            // (after the first pair's stores: the two windows may overlap) | distances, bins | second deposit;
            // the table register is reloaded for four iterations later.
            const uint32_t* tp = tab + lane;
            uint32_t t0 = tp[64], t1 = tp[128], t2 = tp[192], t3 = tp[256];
            locate_a(tp[0]);
            locate_b();
            auto step = [&](uint32_t& t, const uint32_t* next) {
                const f32x2 d_ = dd, m_ = mm; const int ka = kA, kb = kB; const bool oa = okA, ob = okB;
                typename RdfLane<R>::Rows w;
                K.rows_load(col, kA, w);
                locate_a(t);
                t = *next;
                K.rows_add_store(w, d_.x, m_.x, oa, sdl + ka + R);
                K.rows_load(col, kb, w);
                locate_b();
                K.rows_add_store(w, d_.y, m_.y, ob, sdl + kb + R);
            };
            for (int it = 0; it < iters; it += 4) {
                tp += 256;
                step(t0, tp + 64);
                step(t1, tp + 128);
                step(t2, tp + 192);
                step(t3, tp + 256);
            }
        };
        if (near) sweep(std::true_type{});
        else sweep(std::false_type{});
    }
    // column sums in a fixed (lane-rotated) order; one partial histogram per wave
    for (int k = lane; k < nbins; k += 64) {
        const float* row = hist + (size_t)(k + 2 * R) * 64;
        float s = 0.f;
        for (int t = 0; t < 64; ++t) s += row[(t + lane) & 63];
        partial[(size_t)gw * nbins + k] = s;
    }
}

// Half-width columns: EIGHT depositing waves per CU (two per SIMD, so one wave's LDS round trips and
// transcendentals hide behind the other's arithmetic).  A wave's histogram is [rows][32]: lanes l and l + 32
// share column l & 31 and split every deposit -- lane l adds the R + 1 rows from the nearest bin upwards, lane
// l + 32 the R + 1 rows below it -- so the two never touch the same row.  Each lane still locates its own table
// entry (two pairs); v_permlane32_swap hands both entries of the lane pair to both lanes (4 instructions for 2 x
// {distance, bin}), and the four pairs are deposited in the same order on both.  One instruction stream for
// both roles: a deposit is R + 1 ascending rows from a per-lane base row, the Gaussian values by the two-term
// recurrence E_(t+1) = E_t rho_t, rho_(t+1) = rho_t c2 (packed: two rows per step, multiplier {rho_t rho_(t+1)}
// advancing by c2^4), anchored at the base row -- for the lower half that is 2^-26 growing towards the centre.
// +46 % VALU instructions per pair against the full-column kernel, at twice the occupancy.
template <bool DIAG, int R, bool MASKED, int PXC>
__global__ __launch_bounds__(512) void rdf_fwd_half_kernel(
    const float* __restrict__ xyz, int nF, int N, MdgCell cell, float rc2, const uint8_t* __restrict__ mask,
    const float* __restrict__ mu, float coeff, int nbins, const uint32_t* __restrict__ tab, int iters, int pxld,
    float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int HR = R + 1;                                   // rows per half deposit
    static_assert(HR % 2 == 0, "rows are handled in adjacent pairs");
    constexpr int PADL = 2 * R + 1;                             // rows below bin 0
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int col = lane & 31;
    const int boff = (lane >> 5) ? -HR : 0;                     // this lane's rows start at bin k + boff
    const int rows = (nbins + PADL + 2 * R + 2) & ~1;
    const int PXLD = PXC ? PXC : pxld;
    float* hist = sm + (size_t)wid * ((size_t)rows * 32 + 3 * PXLD);
    float* px = hist + (size_t)rows * 32;                       // [3][PXLD]
    float* smu = sm + (size_t)nw * ((size_t)rows * 32 + 3 * PXLD);   // [rows] centre of every row
    float* sdl = smu + rows;                                    // [rows] rdf_centre_offset of every row
    const float sc = sqrtf(-coeff * LOG2E);
    const float mu0 = mu[0];
    const float dmu = (mu[nbins - 1] - mu0) / (float)(nbins - 1), inv_dmu = 1.f / dmu;
    const float Ds = dmu * sc, Ds2 = Ds * Ds, twoDs = 2.f * Ds;
    const float c2 = __builtin_amdgcn_exp2f(-2.f * Ds2), c4 = (c2 * c2) * (c2 * c2);
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        const int kk = r - PADL;
        const float c_ = (kk >= 0 && kk < nbins) ? mu[kk] : fmaf((float)kk, dmu, mu0);
        smu[r] = c_;
        sdl[r] = rdf_centre_offset(c_, mu0, sc, Ds, kk);
    }
    for (int e = lane; e < rows * 32; e += 64) hist[e] = 0.f;
    for (int e = lane; e < 3 * PXLD; e += 64) px[e] = (e >= N && e < PXLD) ? __builtin_nanf("") : 0.f;
    __syncthreads();
    const float ivx = cell.inv[0], ivy = cell.inv[4], ivz = cell.inv[8];
    const int gw = blockIdx.x * nw + wid, nwaves = gridDim.x * nw;
    float* hcol = hist + col + (size_t)(boff + PADL) * 32;      // row of bin boff
    const float* smub = smu + boff + PADL;
    const float* sdlb = sdl + boff + PADL;
    // R + 1 rows upwards from bin k + boff.  A rejected pair comes in as (1e4, bin 0): y0 clamps to 20, E0
    // underflows to an exact 0 and every product with the (finite) multipliers stays 0.
    // In two parts: the values of all four deposits of a step are computed first, so that the four dependent
    // read-add-write round trips that follow carry one packed add per row pair and nothing else -- that stretch
    // is where the SIMD's other wave runs its arithmetic.
    struct Half { float* h; f32x2 P[HR / 2]; };
    auto half_values = [&](float d, int k, Half& w) {
        w.h = hcol + k * 32;
        const float y0 = fminf((d - smub[k]) * sc, 20.f);
        const float E0 = __builtin_amdgcn_exp2f(-y0 * y0), r0 = __builtin_amdgcn_exp2f(fmaf(y0, twoDs, -Ds2));
        const float r1 = r0 * c2, r2 = r1 * c2;
        f32x2 P = {E0, E0 * r0}, M = f32x2{r0, r1} * f32x2{r1, r2};     // {rho_0 rho_1, rho_1 rho_2}
        // row t above the base row sits at y0 - t Ds on the recurrence's grid: to the centre as given (rdf_centre_offset)
        const float* dl = sdlb + k;
        const float d0 = dl[0];
#pragma unroll
        for (int m_ = 0; m_ < HR / 2; ++m_) {
            const f32x2 fx = {fmaf(y0 - (float)(2 * m_) * Ds, dl[2 * m_] - d0, 1.f),
                              fmaf(y0 - (float)(2 * m_ + 1) * Ds, dl[2 * m_ + 1] - d0, 1.f)};
            w.P[m_] = P * fx;
            if (m_ + 1 < HR / 2) { P *= M; M *= c4; }
        }
    };
    auto half_add = [&](const Half& w) {
        float* h = w.h;
        f32x2 v[HR / 2];
#pragma unroll
        for (int m_ = 0; m_ < HR / 2; ++m_) v[m_] = f32x2{h[(2 * m_) * 32], h[(2 * m_ + 1) * 32]};
#pragma unroll
        for (int m_ = 0; m_ < HR / 2; ++m_) v[m_] += w.P[m_];
#pragma unroll
        for (int m_ = 0; m_ < HR / 2; ++m_) { h[(2 * m_) * 32] = v[m_].x; h[(2 * m_ + 1) * 32] = v[m_].y; }
    };
    for (int fr = gw; fr < nF; fr += nwaves) {
        const bool near = rdf_load_frame<DIAG>(px, PXLD, xyz + (size_t)fr * N * 3, N, lane, ivx, ivy, ivz);
        auto sweep = [&](auto near_c) {
            constexpr bool NEAR = decltype(near_c)::value;
            const uint32_t* tp = tab + lane;
            uint32_t t0 = tp[0], t1 = tp[64], t2 = tp[128], t3 = tp[192];
            // software pipeline over steps: the four read-add-writes of the previous entry pair are spread
            // between the pieces of this one's arithmetic (two register sets, no rotation)
            Half A[4], B[4];
#pragma unroll
            for (int q_ = 0; q_ < 4; ++q_) {
                A[q_].h = hcol;
#pragma unroll
                for (int m_ = 0; m_ < HR / 2; ++m_) A[q_].P[m_] = f32x2{0.f, 0.f};
            }
            auto step = [&](uint32_t& t, const uint32_t* next, const Half (&prev)[4], Half (&cur)[4]) {
                half_add(prev[0]);
                int i4, j4;
                const f32x2 d2 = rdf_entry_d2<DIAG, NEAR>(px, PXLD, cell, ivx, ivy, ivz, t, i4, j4);
                t = *next;
                bool okA = (d2.x < rc2) & (d2.x != 0.f), okB = (d2.y < rc2) & (d2.y != 0.f);
                if constexpr (MASKED) {
                    const int mi = i4 >> 2, mj = j4 >> 2;
                    okA = okA & (mask[(size_t)mi * N + min(mj, N - 1)] != 0);
                    okB = okB & (mask[(size_t)mi * N + min(mj + 1, N - 1)] != 0);
                }
                half_add(prev[1]);
                const f32x2 dd = {sqrtf(d2.x), sqrtf(d2.y)};                     // correctly rounded: see rdf_fwd_lane_kernel
                const f32x2 tk = (dd - mu0) * inv_dmu;
                int kA = (int)rintf(tk.x), kB = (int)rintf(tk.y);
                okA = okA & (kA >= -R) & (kA <= nbins - 1 + R);
                okB = okB & (kB >= -R) & (kB <= nbins - 1 + R);
                const uint32_t uda = __float_as_uint(okA ? dd.x : 1e4f), udb = __float_as_uint(okB ? dd.y : 1e4f);
                const uint32_t uka = (uint32_t)(okA ? kA : 0), ukb = (uint32_t)(okB ? kB : 0);
                // [0]: the value of the lower lane of the pair on both lanes, [1]: the upper lane's
                const auto sda = __builtin_amdgcn_permlane32_swap(uda, uda, false, false);
                const auto sdb = __builtin_amdgcn_permlane32_swap(udb, udb, false, false);
                const auto ska = __builtin_amdgcn_permlane32_swap(uka, uka, false, false);
                const auto skb = __builtin_amdgcn_permlane32_swap(ukb, ukb, false, false);
                half_values(__uint_as_float(sda[0]), (int)ska[0], cur[0]);
                half_values(__uint_as_float(sdb[0]), (int)skb[0], cur[1]);
                half_add(prev[2]);
                half_values(__uint_as_float(sda[1]), (int)ska[1], cur[2]);
                half_add(prev[3]);
                half_values(__uint_as_float(sdb[1]), (int)skb[1], cur[3]);
            };
            for (int it = 0; it < iters; it += 4) {
                tp += 256;
                step(t0, tp, A, B);
                step(t1, tp + 64, B, A);
                step(t2, tp + 128, A, B);
                step(t3, tp + 192, B, A);
            }
#pragma unroll
            for (int q_ = 0; q_ < 4; ++q_) half_add(A[q_]);
        };
        if (near) sweep(std::true_type{});
        else sweep(std::false_type{});
    }
    // column sums in a fixed (lane-rotated) order; one partial histogram per wave
    for (int k = lane; k < nbins; k += 64) {
        const float* row = hist + (size_t)(k + PADL) * 32;
        float s_ = 0.f;
        for (int t = 0; t < 32; ++t) s_ += row[(t + lane) & 31];
        partial[(size_t)gw * nbins + k] = s_;
    }
}

// (measured: the same sweep with the two halves of the work on different waves -- four producer waves turning
//  table entries into distances through a double-buffered LDS ring, four consumer waves in the SIMDs' second
//  slots depositing them, one barrier per four entries -- gives the same bits and is 6 % SLOWER, 18.3 vs 17.3 ms:
//  the wave that deposits is bound by the LDS pipe itself, not by the exposed round trips.  Removed.)

// ---------------------------------------------------------------------------------------------------------
// Fine-grid backward for equally spaced centres (width ~ spacing): dL/dd(d) = sum_k g_k 2 coeff (d - mu_k) e_k(d)
// is ONE smooth function of the distance.  A tiny kernel tabulates it -- value and hf * slope on RDF_SUB nodes
// per centre spacing, x_n = xlo + n hf -- and the per-pair work shrinks from a 13-bin Gaussian sum to the
// evaluation of the cell's cubic Hermite interpolant from LDS (interpolation error (hf/sigma)^4 / 384 * 5.8 -- the largest
// fourth derivative of t exp(-t^2 / 2), at t = 0.6 -- = 1.5e-6 of a unit contribution g / sigma for hf = sigma / 10, i.e.
// width = spacing; tests/test_rdf_ref_host.py holds the float64 restatement of the table below 2e-6.  With eight nodes
// per spacing, and 3 taken for that derivative, it measured 3.6e-6.)
// (The transposed idea for the forward pass -- every pair deposits its four Hermite weights into per-wave
//  node accumulators with fixed-point ds_add_u32, Gaussians evaluated once per wave at the end -- halves the
//  arithmetic but is bound by the LDS atomic unit, ~15 cycles per wave instruction and CU plus 2-3-way address
//  conflicts: 13.5 ms against 11.6 ms for the lane-private columns of rdf_fwd_lane_kernel.  Measured, removed.)
constexpr int RDF_SUB = 10;      // nodes per centre spacing of this table (the u-space table of the ring adjoint: RDF_SUB_U)
constexpr int RDF_SUB_U = 8;     // rdf_u_grid (common.hpp)

struct FineGrid { float xlo, hf, inv_hf; int nn; };

__host__ __device__ inline int fine_nodes(int nbins, int R) { return (nbins - 1 + 2 * (R + 1)) * RDF_SUB + 1; }

// (the centres live in device memory: the grid is derived from them inside the kernels)
__device__ __forceinline__ FineGrid fine_grid(const float* __restrict__ mu, int nbins, int R) {
    FineGrid G;
    const float mu0 = mu[0], dmu = (mu[nbins - 1] - mu0) / (float)(nbins - 1);
    G.xlo = mu0 - (float)(R + 1) * dmu;
    G.hf = dmu / (float)RDF_SUB;
    G.inv_hf = (float)RDF_SUB / dmu;
    G.nn = fine_nodes(nbins, R);
    return G;
}

// S = dL/dd = sum_k sg_k x e and S' = dS/dd at the distance r, x = s (r - mu_k), e = exp2(-x^2), over the 2R + 3 centres
// around the nearest one: the node value of both derivative tables
__device__ __forceinline__ float2 rdf_node_sum(const float* __restrict__ mu, float coeff, int nbins,
                                               const float* __restrict__ g_raw, int R, float r) {
    const float sc = sqrtf(-coeff * LOG2E);
    const float mu0 = mu[0], dmu = (mu[nbins - 1] - mu0) / (float)(nbins - 1);
    const int kc = (int)rintf((r - mu0) / dmu);
    float val = 0.f, der = 0.f;
    for (int k = max(0, kc - R - 1); k <= min(nbins - 1, kc + R + 1); ++k) {
        const float xs = (r - mu[k]) * sc;
        const float e = __builtin_amdgcn_exp2f(-xs * xs);
        const float sg = g_raw[k] * 2.f * coeff / sc;
        val = fmaf(sg * xs, e, val);
        der = fmaf(sg * sc * (1.f - 2.f * 0.69314718056f * xs * xs), e, der);
    }
    return make_float2(val, der);
}
// node table of dL/dd: tab[n] = (S, hf S') at x_n
__device__ __forceinline__ float2 rdf_fine_node(const FineGrid& G, const float* __restrict__ mu, float coeff, int nbins,
                                                const float* __restrict__ g_raw, int R, int n) {
    const float2 s_ = rdf_node_sum(mu, coeff, nbins, g_raw, R, fmaf((float)n, G.hf, G.xlo));
    return make_float2(s_.x, s_.y * G.hf);
}
// cell n = nodes n and n + 1: the cubic Hermite interpolant of {value, hf slope} at both ends, stored as its
// monomial coefficients in the cell coordinate f in [0, 1) (c0 + f (c1 + f (c2 + f c3)): three fma per pair)
__global__ void rdf_bwd_table_kernel(const float* __restrict__ mu, float coeff, int nbins,
                                     const float* __restrict__ g_raw, int R, float4* __restrict__ tab) {
    const FineGrid G = fine_grid(mu, nbins, R);
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= G.nn - 1) return;
    const float2 a_ = rdf_fine_node(G, mu, coeff, nbins, g_raw, R, n), b_ = rdf_fine_node(G, mu, coeff, nbins, g_raw, R, n + 1);
    tab[n] = make_float4(a_.x, a_.y, 3.f * (b_.x - a_.x) - 2.f * a_.y - b_.y, 2.f * (a_.x - b_.x) + a_.y + b_.y);
}

// The u-space variant (rdf_u_grid in common.hpp): node n at u_n = ulo + n hu, r = sqrt(u_n), holds
// W = (dL/dd)(r) / r and hu dW/du = hu (S' / r - S / r^2) / (2 r)  with S = dL/dd, S' = dS/dd.
__global__ void rdf_bwd_table_u_kernel(const float* __restrict__ mu, float coeff, int nbins,
                                       const float* __restrict__ g_raw, int R, float4* __restrict__ tab) {
    float ulo, hu;
    int ncell;
    rdf_u_grid(mu, nbins, R, ulo, hu, ncell);
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= ncell) return;
    auto node = [&](int m) {
        const float r = sqrtf(fmaf((float)m, hu, ulo));
        const float2 s_ = rdf_node_sum(mu, coeff, nbins, g_raw, R, r);
        const float ir = 1.0f / r;
        return make_float2(s_.x * ir, hu * (s_.y * ir - s_.x * ir * ir) * (0.5f * ir));
    };
    const float2 a_ = node(n), b_ = node(n + 1);
    tab[n] = make_float4(a_.x, a_.y, 3.f * (b_.x - a_.x) - 2.f * a_.y - b_.y, 2.f * (a_.x - b_.x) + a_.y + b_.y);
}

// Fine-grid backward, one wave per frame.  Pair order: lane <-> atom i (64 at a time), step s <-> partner
// j = (i + s) mod N, s = 1 .. N/2 (for an even N the last step only for i < N/2): every unordered pair once, and
// in one step the partners of the 64 lanes are all different, so the partners' gradient read-add-writes never
// collide, while atom i's own gradient accumulates in registers (half the LDS traffic of a pair order that
// scatters both ends).  Positions and partner gradients live in index-doubled arrays (entry k and k + N are the
// same atom; the two gradient halves are folded at the end): the partner address is affine in s, no modulo.
// Two steps per iteration in packed fp32; the stores of step s precede the reads of step s + 1 (lane l's second
// partner is lane l + 1's first).  The table holds one float4 per cell: the cell's cubic in monomial form.
template <bool DIAG>
__global__ __launch_bounds__(256) void rdf_bwd_fine_kernel(
    const float* __restrict__ xyz, int nF, int N, MdgCell cell, float rc2, const uint8_t* __restrict__ mask,
    const float* __restrict__ mu, int nbins, int R, const float4* __restrict__ tab_g, int LDW,
    float* __restrict__ g_xyz) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const FineGrid G = fine_grid(mu, nbins, R);
    float4* tab = reinterpret_cast<float4*>(sm);                     // [nn - 1] cells
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float* px = sm + 4 * (size_t)(G.nn - 1) + (size_t)wid * 6 * LDW; // positions [3][LDW] then gradient [3][LDW]
    float* gx = px + 3 * LDW;
    for (int n = threadIdx.x; n < G.nn - 1; n += blockDim.x) tab[n] = tab_g[n];
    for (int e = lane; e < 6 * LDW; e += 64) px[e] = 0.f;
    __syncthreads();
    const int fr = blockIdx.x * (blockDim.x >> 6) + wid;
    if (fr >= nF) return;
    const float* pos = xyz + (size_t)fr * N * 3;
    const float ivx = cell.inv[0], ivy = cell.inv[4], ivz = cell.inv[8];
    bool out = false;
    for (int e = lane; e < 3 * N; e += 64) {
        const int c = e % 3, a = e / 3;
        const float v = pos[e];
        px[c * LDW + a] = v;
        px[c * LDW + a + N] = v;
        if (DIAG) {
            const float s_ = v * (c == 0 ? ivx : c == 1 ? ivy : ivz);
            out |= !(s_ > -0.24f && s_ < 1.24f);
        }
    }
    const bool near = DIAG && !__any(out);                           // see rdf_fwd_lane_kernel
    const float tmax = (float)(G.nn - 1);
    const int smax = N / 2;                                          // steps (the last one is the half step of an even N)
    auto sweep = [&](auto near_c) {
        constexpr bool NEAR = decltype(near_c)::value;
        for (int i0 = 0; i0 < N; i0 += 64) {
            const int i = i0 + lane;                                 // (lanes past N run on zeros and add +-0)
            const bool live = i < N;
            const int lim = !live ? 0 : ((N & 1) ? (N - 1) / 2 : (i >= N / 2 ? smax - 1 : smax));
            const float xi = px[i], yi = px[LDW + i], zi = px[2 * LDW + i];
            f32x2 ax = {0.f, 0.f}, ay = ax, az = ax;                 // - gradient of atom i, two partial sums
            const float* pj = px + i;
            float* gj = gx + i;
            for (int s_ = 1; s_ <= smax; s_ += 2) {
                pj += 2; gj += 2;                                    // -> partner i + s_ + 1 (the first one is at [-1])
                f32x2 dx = f32x2{pj[-1], pj[0]} - xi, dy = f32x2{pj[LDW - 1], pj[LDW]} - yi,
                      dz = f32x2{pj[2 * LDW - 1], pj[2 * LDW]} - zi;   // D = x_j - x_i
                if constexpr (NEAR) {
                    dx = min_image_diag2_near(dx, ivx, cell.h[0]);
                    dy = min_image_diag2_near(dy, ivy, cell.h[4]);
                    dz = min_image_diag2_near(dz, ivz, cell.h[8]);
                } else if constexpr (DIAG) {
                    dx = min_image_diag2(dx, ivx, cell.h[0]);
                    dy = min_image_diag2(dy, ivy, cell.h[4]);
                    dz = min_image_diag2(dz, ivz, cell.h[8]);
                } else {
                    float ax_ = dx.x, ay_ = dy.x, az_ = dz.x, bx_ = dx.y, by_ = dy.y, bz_ = dz.y;
                    min_image<false>(cell, ax_, ay_, az_);
                    min_image<false>(cell, bx_, by_, bz_);
                    dx = f32x2{ax_, bx_}; dy = f32x2{ay_, by_}; dz = f32x2{az_, bz_};
                }
                const f32x2 d2 = norm2_ref2(dx, dy, dz);
                bool okA = (s_ <= lim) & (d2.x < rc2) & (d2.x != 0.f), okB = (s_ + 1 <= lim) & (d2.y < rc2) & (d2.y != 0.f);
                if (mask) {                                                  // (uniform)
                    const int ii = live ? i : 0;
                    int ja = ii + s_, jb = ii + s_ + 1;
                    ja = ja >= N ? ja - N : ja; jb = jb >= N ? jb - N : jb;
                    jb = jb >= N ? jb - N : jb;
                    okA = okA & (mask[(size_t)min(ii, ja) * N + max(ii, ja)] != 0);
                    okB = okB & (mask[(size_t)min(ii, jb) * N + max(ii, jb)] != 0);
                }
                const f32x2 id = {__builtin_amdgcn_rsqf(okA ? d2.x : 1.f), __builtin_amdgcn_rsqf(okB ? d2.y : 1.f)};
                f32x2 t = (d2 * id - G.xlo) * G.inv_hf;
                okA = okA & (t.x >= 0.f) & (t.x < tmax);
                okB = okB & (t.y >= 0.f) & (t.y < tmax);
                t = f32x2{okA ? t.x : 0.f, okB ? t.y : 0.f};
                const int gA = (int)t.x, gB = (int)t.y;
                const f32x2 f = t - f32x2{(float)gA, (float)gB};
                const float4 ca = tab[gA], cb = tab[gB];
                const float sdA = fmaf(f.x, fmaf(f.x, fmaf(f.x, ca.w, ca.z), ca.y), ca.x);
                const float sdB = fmaf(f.y, fmaf(f.y, fmaf(f.y, cb.w, cb.z), cb.y), cb.x);
                // d(dist)/dx_j = +D/d, d(dist)/dx_i = -D/d; a rejected pair adds +-0
                const f32x2 cw = f32x2{okA ? sdA : 0.f, okB ? sdB : 0.f} * id;
                const f32x2 cx = cw * dx, cy = cw * dy, cz = cw * dz;
                ax += cx; ay += cy; az += cz;
                {
                    const float g0 = gj[-1], g1 = gj[LDW - 1], g2 = gj[2 * LDW - 1];
                    gj[-1] = g0 + cx.x; gj[LDW - 1] = g1 + cy.x; gj[2 * LDW - 1] = g2 + cz.x;
                }
                {
                    const float g0 = gj[0], g1 = gj[LDW], g2 = gj[2 * LDW];
                    gj[0] = g0 + cx.y; gj[LDW] = g1 + cy.y; gj[2 * LDW] = g2 + cz.y;
                }
            }
            if (live) {
                gx[i] -= ax.x + ax.y; gx[LDW + i] -= ay.x + ay.y; gx[2 * LDW + i] -= az.x + az.y;
            }
        }
    };
    if (near) sweep(std::true_type{});
    else sweep(std::false_type{});
    float* out_g = g_xyz + (size_t)fr * N * 3;
    for (int e = lane; e < 3 * N; e += 64) {
        const int c = e % 3, a = e / 3;
        out_g[e] = gx[c * LDW + a] + gx[c * LDW + a + N];
    }
}

// ---------------------------------------------------------------------------------------------
// Forward for many frames and equally spaced centres through a FINE INTEGER histogram.
// The soft histogram  raw[k] = sum_pairs exp2(-(s (d - mu_k))^2)  is a smooth function of every pair distance, so
// the pairs are first COUNTED on a grid M times finer than the centres (one integer LDS atomic per pair: a
// `ds_add_u32` instead of the 11 float read-add-writes of the lane-private columns), and the fine counts are smeared
// onto the centres once at the end:  raw[k] = sum_m H[m] exp2(-(s (x_m - mu_k))^2),  x_m = centre of fine bin m.
// Error: moving a pair to its bin centre changes its Gaussian by (delta^2 / 2) G'' on average (the first-order
// term averages out over the bin): relative (s h)^2 [(2 ln2 u)^2 - 2 ln2] / 24 at u = s |d - mu|, i.e. 9e-7 at the
// peak and 1.1e-5 three widths out (where the Gaussian is 2^-9 of its peak) for s h = 0.004 -- the tests allow 2e-5
// per bin.  Integer counts commute, so the result is independent of the order in which waves and workgroups
// deposit: bitwise reproducible without lane-private columns -- the sixteen waves of a workgroup share ONE histogram
// (~24 000 fine bins = 95 KB at 100 centres) and the workgroups merge into a global integer histogram.
// Pairs come from a table (i | j << 16), row-major in (i, j): the lanes of one step share atom i (LDS broadcast) and
// read consecutive j (conflict-free), and masked (species-selected) histograms simply have a shorter table.
constexpr int RDF_FINE_MAX = 36864;       // fine bins that fit the workgroup's LDS histogram (144 KB)
constexpr int RDF_FINE_WAVES = 16;
constexpr int RDF_FINE_ATOMS = 1024;

__global__ __launch_bounds__(1024) void rdf_fine_table_kernel(int N, const uint8_t* __restrict__ mask,
                                                              uint32_t* __restrict__ tab, int32_t* __restrict__ count) {
    __shared__ int32_t cnt[RDF_FINE_ATOMS + 1];
    const int i = threadIdx.x;
    int c = 0;
    if (i < N) {
        if (mask) { for (int j = i + 1; j < N; ++j) c += mask[(size_t)i * N + j] != 0; }
        else c = N - 1 - i;
    }
    cnt[i] = c;
    __syncthreads();
    if (threadIdx.x == 0) {                          // N <= 1024: a serial scan is a few microseconds
        int run = 0;
        for (int k = 0; k < N; ++k) { const int v = cnt[k]; cnt[k] = run; run += v; }
        cnt[N] = run;
        *count = run;
    }
    __syncthreads();
    if (i < N) {
        int o = cnt[i];
        for (int j = i + 1; j < N; ++j)                   // entries hold BYTE offsets (4 i | 4 j << 16): no shifts in the loop
            if (!mask || mask[(size_t)i * N + j]) tab[o++] = (uint32_t)(4 * i) | ((uint32_t)(4 * j) << 16);
    }
    // padding up to the next multiple of 128 entries: the pair (0, 0) has distance 0, which lies below the fine grid
    const int total = cnt[N], padded = (total + 127) & ~127;
    for (int o = total + threadIdx.x; o < padded; o += blockDim.x) tab[o] = 0u;
}

// One frame of one wave.  SAFE: the fine grid starts above 0 and ends inside the cutoff (checked once per kernel), so
// `0 <= t < nfine` alone accepts exactly the pairs of topology.py:67 that can contribute -- a zero distance (padding
// entries, coincident atoms) falls below the grid, a distance beyond the cutoff above it.
template <bool DIAG, bool SAFE>
__device__ __forceinline__ void rdf_fine_frame(const MdgCell& cell, const uint32_t* __restrict__ tab, int P, float rc2,
                                               float inv_h, float tlo, float fmax, const float* px, const float* py,
                                               const float* pz, uint32_t* hist, int lane) {
    const char* bx = reinterpret_cast<const char*>(px);
    const char* by = reinterpret_cast<const char*>(py);
    const char* bz = reinterpret_cast<const char*>(pz);
#define LDF(base, off) (*reinterpret_cast<const float*>((base) + (off)))
    if constexpr (DIAG) {
        // two table entries per lane and step in packed fp32 (the same image arithmetic as min_image<true>)
        const float iv0 = cell.inv[0], iv1 = cell.inv[4], iv2 = cell.inv[8];
        const float h0 = cell.h[0], h1 = cell.h[4], h2 = cell.h[8];
        for (int p0 = 0; p0 < P; p0 += 128) {
            const uint32_t ea = tab[p0 + lane], eb = tab[p0 + 64 + lane];
            const int ia = (int)(ea & 0xFFFFu), ja = (int)(ea >> 16), ib = (int)(eb & 0xFFFFu), jb = (int)(eb >> 16);
            f32x2 dx = f32x2{LDF(bx, ja), LDF(bx, jb)} - f32x2{LDF(bx, ia), LDF(bx, ib)};
            f32x2 dy = f32x2{LDF(by, ja), LDF(by, jb)} - f32x2{LDF(by, ia), LDF(by, ib)};
            f32x2 dz = f32x2{LDF(bz, ja), LDF(bz, jb)} - f32x2{LDF(bz, ia), LDF(bz, ib)};
            dx = min_image_diag2(dx, iv0, h0); dy = min_image_diag2(dy, iv1, h1); dz = min_image_diag2(dz, iv2, h2);
            const f32x2 d2 = norm2_ref2(dx, dy, dz);
            const float ta = fmaf(__builtin_amdgcn_sqrtf(d2.x), inv_h, tlo), tb = fmaf(__builtin_amdgcn_sqrtf(d2.y), inv_h, tlo);
            bool oka = ta >= 0.f && ta < fmax, okb = tb >= 0.f && tb < fmax;
            if (!SAFE) { oka = oka && d2.x < rc2 && d2.x != 0.f; okb = okb && d2.y < rc2 && d2.y != 0.f; }
            if (oka) atomicAdd(&hist[(int)ta], 1u);
            if (okb) atomicAdd(&hist[(int)tb], 1u);
        }
    } else {
        for (int p0 = 0; p0 < P; p0 += 64) {
            const uint32_t ent = tab[p0 + lane];
            const int i = (int)(ent & 0xFFFFu), j = (int)(ent >> 16);
            float dx = LDF(bx, j) - LDF(bx, i), dy = LDF(by, j) - LDF(by, i), dz = LDF(bz, j) - LDF(bz, i);
            min_image<DIAG>(cell, dx, dy, dz);
            const float d2 = norm2_ref(dx, dy, dz);
            const float t = fmaf(__builtin_amdgcn_sqrtf(d2), inv_h, tlo);
            bool ok = t >= 0.f && t < fmax;
            if (!SAFE) ok = ok && d2 < rc2 && d2 != 0.f;
            if (ok) atomicAdd(&hist[(int)t], 1u);
        }
    }
#undef LDF
}

template <bool DIAG>
__global__ __launch_bounds__(64 * RDF_FINE_WAVES) void rdf_fwd_fine_kernel(
    const float* __restrict__ xyz, int nF, int N, MdgCell cell, float rc2, const uint32_t* __restrict__ tab,
    const int32_t* __restrict__ count, const float* __restrict__ mu, float reach, float inv_h, int nfine, int ld,
    uint32_t* __restrict__ ghist) {
    extern __shared__ __attribute__((aligned(16))) float smf[];
    const float lo = mu[0] - reach;                             // lower edge of the fine grid
    uint32_t* hist = reinterpret_cast<uint32_t*>(smf);          // [nfine] shared by the workgroup's waves
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float* px = smf + nfine + wid * 3 * ld;                     // wave-private SoA frame
    float* py = px + ld;
    float* pz = py + ld;
    for (int m = threadIdx.x; m < nfine; m += blockDim.x) hist[m] = 0u;
    __syncthreads();
    const int P = *count;                                       // (the table is padded to a multiple of 128 entries)
    const float fmax = (float)nfine, tlo = -lo * inv_h;
    const float hi = lo + fmax / inv_h;
    const bool safe = lo > 0.f && hi * hi <= rc2;
    for (int fr = blockIdx.x * RDF_FINE_WAVES + wid; fr < nF; fr += gridDim.x * RDF_FINE_WAVES) {
        const float* pos = xyz + (size_t)fr * N * 3;
        for (int e = lane; e < 3 * N; e += 64) {                // AoS -> SoA (coalesced read)
            const int a = e / 3, c = e - 3 * a;
            px[c * ld + a] = pos[e];
        }
        // (px is private to the wave: program order + the LDS counter suffice)
        if (safe) rdf_fine_frame<DIAG, true>(cell, tab, P, rc2, inv_h, tlo, fmax, px, py, pz, hist, lane);
        else rdf_fine_frame<DIAG, false>(cell, tab, P, rc2, inv_h, tlo, fmax, px, py, pz, hist, lane);
    }
    __syncthreads();
    for (int m = threadIdx.x; m < nfine; m += blockDim.x) {
        const uint32_t v = hist[m];
        if (v) atomicAdd(&ghist[m], v);
    }
}

// The same fine histogram fed from a neighbour list (large systems, few frames: config #4's 4 096-atom liquid):
// thread per (atom, slot) of the per-atom list, every pair counted once (slot's neighbour index above the atom's).
// Frames are stacked as groups of the list (mdg_nbr_build_cell_groups), so one launch covers all of them.
__global__ __launch_bounds__(1024) void rdf_fwd_ell_kernel(
    const float* __restrict__ pos, long long n_slots, MdgCell cell, const int32_t* __restrict__ col,
    const int32_t* __restrict__ shift, const int32_t* __restrict__ cnt, int max_nbr, const float* __restrict__ mu,
    float reach, float inv_h, int nfine, uint32_t* __restrict__ ghist) {
    extern __shared__ __attribute__((aligned(16))) float smf[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(smf);
    for (int m = threadIdx.x; m < nfine; m += blockDim.x) hist[m] = 0u;
    __syncthreads();
    const float lo = mu[0] - reach, tlo = -lo * inv_h, fmax = (float)nfine;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n_slots; t += (long long)gridDim.x * blockDim.x) {
        const int i = (int)(t / max_nbr), k = (int)(t - (long long)i * max_nbr);
        if (k >= cnt[i]) continue;
        const int j = col[t];
        if (j <= i) continue;
        float dx = pos[3 * i] - pos[3 * j], dy = pos[3 * i + 1] - pos[3 * j + 1], dz = pos[3 * i + 2] - pos[3 * j + 2];
        apply_shift(cell, shift[t], dx, dy, dz);
        const float tt = fmaf(__builtin_amdgcn_sqrtf(norm2_ref(dx, dy, dz)), inv_h, tlo);
        if (tt >= 0.f && tt < fmax) atomicAdd(&hist[(int)tt], 1u);
    }
    __syncthreads();
    for (int m = threadIdx.x; m < nfine; m += blockDim.x) {
        const uint32_t v = hist[m];
        if (v) atomicAdd(&ghist[m], v);
    }
}

// raw[k] = sum_m H[m] exp2(-(s (x_m - mu_k))^2): one wave per centre over the fine bins within reach
__global__ void rdf_fine_finish_kernel(const uint32_t* __restrict__ ghist, int nfine, float h,
                                       const float* __restrict__ mu, float sc, float reach, int nbins,
                                       float* __restrict__ raw) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const float m_k = mu[k], lo = mu[0] - reach;
    int m0 = (int)floorf((m_k - reach - lo) / h), m1 = (int)ceilf((m_k + reach - lo) / h);
    m0 = m0 < 0 ? 0 : m0;
    m1 = m1 > nfine ? nfine : m1;
    double s = 0.0;
    for (int m = m0 + lane; m < m1; m += 64) {
        const uint32_t c = ghist[m];
        if (c) {
            const float x = (lo + ((float)m + 0.5f) * h - m_k) * sc;
            s += (double)c * (double)__builtin_amdgcn_exp2f(-x * x);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) raw[k] = (float)s;
}

// raw[k] = sum_b partial[b][k] in fixed order; one wave per bin
__global__ void rdf_finish_kernel(const float* __restrict__ partial, int nblocks, int nbins,
                                  float* __restrict__ raw) {
    const int k = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int b = lane; b < nblocks; b += 64) s += partial[(size_t)b * nbins + k];
    s = wave_sum(s);
    if (lane == 0) raw[k] = s;
}

// Backward: one WAVE per frame, every unordered pair visited once.  The pairs are walked in
// round-robin-tournament order (circle method): round r holds floor(N'/2) DISJOINT pairs, so
// the lanes of one instruction never touch the same atom and the +/- contributions go into a
// wave-private LDS gradient with plain read-modify-writes -- no atomics, and the rounds are
// sequential within the wave => fixed summation order, bitwise reproducible.
// R > 0: equally spaced centres, dL/dd from the 2R+1 bins around the nearest centre with the forward
// kernel's recurrence (tables padded so that no bin needs a bounds test); R == 0: direct sum, `uniform`
// only narrows the bin range.
template <bool DIAG, int R>
__global__ __launch_bounds__(256) void rdf_bwd_kernel(
    const float* __restrict__ xyz, int nF, int N, MdgCell cell, float rc2, const uint8_t* __restrict__ mask,
    const float* __restrict__ mu, float coeff, int nbins, const float* __restrict__ g_raw,
    float* __restrict__ g_xyz, int uniform) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* smu = sm;                         // [nbins + 2R]  centre of bin k at k + R
    float* sg = sm + nbins + 2 * R;          // [nbins + 4R]  g_k * 2 coeff / s at k + 2R, zero padding
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float* px = sg + nbins + 4 * R + (size_t)wid * 6 * N;   // positions [3][N] then gradient [3][N] of this wave's frame
    float* gx = px + 3 * N;
    const float sc = sqrtf(-coeff * LOG2E);
    {
        const float m0 = mu[0], dm = nbins > 1 ? (mu[nbins - 1] - m0) / (float)(nbins - 1) : 0.f;
        for (int k = threadIdx.x; k < nbins + 2 * R; k += blockDim.x) {
            const int kk = k - R;
            smu[k] = (kk >= 0 && kk < nbins) ? mu[kk] : fmaf((float)kk, dm, m0);
        }
        for (int k = threadIdx.x; k < nbins + 4 * R; k += blockDim.x) {
            const int kk = k - 2 * R;
            sg[k] = (kk >= 0 && kk < nbins) ? g_raw[kk] * 2.f * coeff / sc : 0.f;
        }
    }
    __syncthreads();
    const int fr = blockIdx.x * (blockDim.x >> 6) + wid;
    if (fr >= nF) return;
    const float* pos = xyz + (size_t)fr * N * 3;
    for (int e = lane; e < 3 * N; e += 64) { px[(e % 3) * N + e / 3] = pos[e]; gx[e] = 0.f; }
    const float mu0 = smu[R];
    const float dmu = nbins > 1 ? (smu[R + nbins - 1] - mu0) / (float)(nbins - 1) : 0.f;
    const float reach = 11.3f / sc;          // exp2 argument below -126 beyond this
    const float inv_dmu = dmu > 0.f ? 1.f / dmu : 0.f;
    const float Ds = dmu * sc, Ds2 = Ds * Ds;
    const float c2 = __builtin_amdgcn_exp2f(-2.f * Ds2);
    const int Np = N + (N & 1);              // even number of tournament slots (one dummy when N is odd)
    const int M = Np - 1, half = Np / 2;
    for (int r = 0; r < M; ++r) {
        for (int p0 = 0; p0 < half; p0 += 64) {
            const int p = p0 + lane;
            int a = -1, b = -1;
            if (p < half) {
                if (p == 0) { a = M; b = r; }
                else { a = r + p; if (a >= M) a -= M; b = r - p; if (b < 0) b += M; }
                if (a >= N || b >= N) a = -1;                     // pair with the dummy slot
            }
            if (a >= 0) {
                const int i = min(a, b), j = max(a, b);
                float dx = px[j] - px[i], dy = px[N + j] - px[N + i], dz = px[2 * N + j] - px[2 * N + i];
                min_image<DIAG>(cell, dx, dy, dz);               // D = x_j - x_i as the forward pass
                const float d2 = norm2_ref(dx, dy, dz);
                bool ok = (d2 < rc2) && (d2 != 0.f);
                if (ok && mask) ok = mask[(size_t)i * N + j] != 0;
                if (ok) {
                    const float id = __builtin_amdgcn_rsqf(d2);
                    const float d = d2 * id;
                    // dL/dd = sum_k g_k 2 coeff (d - mu_k) e_k = sum_k sg_k x_k exp2(-x_k^2), x_k = s (d - mu_k)
                    float sd = 0.f;
                    if constexpr (R > 0) {
                        const int kc = (int)rintf((d - mu0) * inv_dmu);
                        if (kc >= -R && kc <= nbins - 1 + R) {
                            const float x0 = (d - smu[kc + R]) * sc;
                            const float a = 2.f * Ds * x0;
                            float eu = __builtin_amdgcn_exp2f(-x0 * x0), ed = eu, xu = x0, xd = x0;
                            float ru = __builtin_amdgcn_exp2f(a - Ds2), rd = __builtin_amdgcn_exp2f(-a - Ds2);
                            const float* gk = sg + kc + R;        // gk[R] is bin kc
                            sd = gk[R] * x0 * eu;
#pragma unroll
                            for (int s = 1; s <= R; ++s) {
                                eu *= ru; ru *= c2; xu -= Ds; sd = fmaf(gk[R + s] * xu, eu, sd);
                                ed *= rd; rd *= c2; xd += Ds; sd = fmaf(gk[R - s] * xd, ed, sd);
                            }
                        }
                    } else {
                        int klo = 0, khi = nbins - 1;
                        if (uniform && dmu > 0.f) {
                            klo = max(0, (int)floorf((d - reach - mu0) / dmu));
                            khi = min(nbins - 1, (int)ceilf((d + reach - mu0) / dmu));
                        }
                        for (int k = klo; k <= khi; ++k) {
                            const float x = (d - smu[k]) * sc;
                            sd = fmaf(sg[k] * x, __builtin_amdgcn_exp2f(-x * x), sd);
                        }
                    }
                    const float c = sd * id;                      // d(dist)/dx_j = +D/d, d(dist)/dx_i = -D/d
                    gx[j] += c * dx; gx[N + j] += c * dy; gx[2 * N + j] += c * dz;
                    gx[i] -= c * dx; gx[N + i] -= c * dy; gx[2 * N + i] -= c * dz;
                }
            }
        }
    }
    float* out = g_xyz + (size_t)fr * N * 3;
    for (int e = lane; e < 3 * N; e += 64) out[e] = gx[(e % 3) * N + e / 3];
}

// Backward, few-frames / large-N variant: LPA lanes per (frame, atom) gather (each pair visited from
// both ends; used when there are too few frames to fill the chip with one wave per frame).
template <bool DIAG, int LPA>
__global__ void rdf_bwd_atom_kernel(const float* __restrict__ xyz, int nF, int N, MdgCell cell, float rc2,
                               const uint8_t* __restrict__ mask, const float* __restrict__ mu, float coeff,
                               int nbins, const float* __restrict__ g_raw, float* __restrict__ g_xyz, int uniform) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* smu = sm;             // [nbins]
    float* sg = sm + nbins;      // [nbins]
    const float sc = sqrtf(-coeff * LOG2E);
    for (int k = threadIdx.x; k < nbins; k += blockDim.x) { smu[k] = mu[k]; sg[k] = g_raw[k] * 2.f * coeff / sc; }
    __syncthreads();
    const int apb = blockDim.x / LPA;
    const long long gi = (long long)blockIdx.x * apb + threadIdx.x / LPA;
    const int sub = threadIdx.x % LPA;
    if (gi >= (long long)nF * N) return;
    const int fr = (int)(gi / N), i = (int)(gi % N);
    const float* pos = xyz + (size_t)fr * N * 3;
    const float xi = pos[3 * i], yi = pos[3 * i + 1], zi = pos[3 * i + 2];
    // bins whose Gaussian is non-negligible (exp2 argument > -126) around a distance
    const float dmu = nbins > 1 ? (smu[nbins - 1] - smu[0]) / (float)(nbins - 1) : 0.f;
    const float reach = 11.3f / sc;                                       // sqrt(126) in scaled units
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int j = sub; j < N; j += LPA) {
        if (j == i) continue;
        float dx = pos[3 * j] - xi, dy = pos[3 * j + 1] - yi, dz = pos[3 * j + 2] - zi;
        // the half list holds (min(i,j), max(i,j)) with D = x_hi - x_lo: evaluate in that
        // orientation so the accepted set is the forward pass's
        const bool flip = j < i;
        if (flip) { dx = -dx; dy = -dy; dz = -dz; }
        min_image<DIAG>(cell, dx, dy, dz);
        const float d2 = norm2_ref(dx, dy, dz);
        if (!((d2 < rc2) && (d2 != 0.f))) continue;
        if (mask && !mask[(size_t)(flip ? j : i) * N + (flip ? i : j)]) continue;
        const float id = __builtin_amdgcn_rsqf(d2);
        const float ds = d2 * id;
        int klo = 0, khi = nbins - 1;
        if (uniform && dmu > 0.f) {
            klo = max(0, (int)floorf((ds - reach - smu[0]) / dmu));
            khi = min(nbins - 1, (int)ceilf((ds + reach - smu[0]) / dmu));
        }
        // dL/dd = sum_k g_k 2 coeff (d - mu_k) e_k = sum_k sg_k x_k exp2(-x_k^2),
        //   x_k = s (d - mu_k), sg_k = g_k * 2 coeff / s
        float s = 0.f;
        for (int k = klo; k <= khi; ++k) {
            const float x = (ds - smu[k]) * sc;
            s = fmaf(sg[k] * x, __builtin_amdgcn_exp2f(-x * x), s);
        }
        // d(dist)/dx_i = -(D)/d for D = x_j - x_i (unflipped); with flip, D was negated
        const float c = (flip ? s : -s) * id;
        gx = fmaf(c, dx, gx); gy = fmaf(c, dy, gy); gz = fmaf(c, dz, gz);
    }
    gx = group_sum<LPA>(gx); gy = group_sum<LPA>(gy); gz = group_sum<LPA>(gz);
    if (sub == 0) {
        float* o = g_xyz + ((size_t)fr * N + i) * 3;
        o[0] = gx; o[1] = gy; o[2] = gz;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// Host side.  Every entry point checks its arguments, plans and launches.  A plan (RdfFwdPlan, RdfBwdPlan) is a pure
// function of the shape -- no HIP call -- that names the kernel variant and holds everything its launch needs.  What a
// variant cannot do (LDS, table sizes) is kept apart from what is merely preferred (many frames, enough atoms).
constexpr size_t RDF_LDS_BUDGET = 156 * 1024;    // dynamic LDS a forward plan may ask for
constexpr size_t RDF_LDS_MAX = 160 * 1024;       // the CU's LDS
constexpr int RDF_MANY_FRAMES = 1024;            // from here on one wave per frame fills the chip

struct RdfFrames {                               // the leading arguments of every frame kernel
    const float* xyz; int nF, N; const MdgCell* cell; float rc2; const uint8_t* mask; const float* mu; float coeff; int nbins;
    hipStream_t st;
};
template <class K, class... Tail>
static void rdf_launch(K kernel, int grid, int block, size_t lds, const RdfFrames& a, Tail... tail) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, a.st, a.xyz, a.nF, a.N, *a.cell, a.rc2, a.mask, a.mu, a.coeff,
                       a.nbins, tail...);
}

// f(DIAG, MASKED, PX, R) with compile-time constants, for exactly the combinations the kernels are built for: a reach
// out of Rs; 128-column coordinate rows (PX = 128: immediate LDS offsets) for the common shape, orthorhombic without a
// mask, and the run-time stride (PX = 0) for the four (DIAG, MASKED) cases otherwise.  Kernels that only distinguish
// the cell go through rdf_dispatch<0>(diag, false, false, 0, ...).
template <int V> using RdfInt = std::integral_constant<int, V>;
template <int... Rs, class F>
static void rdf_dispatch(bool diag, bool masked, bool px128, int R, F&& f) {
    auto with_r = [&](auto d, auto m, auto px) { (void)((R == Rs && (f(d, m, px, RdfInt<Rs>{}), true)) || ...); };
    if (px128) with_r(std::true_type{}, std::false_type{}, RdfInt<128>{});
    else if (diag && masked) with_r(std::true_type{}, std::true_type{}, RdfInt<0>{});
    else if (diag) with_r(std::true_type{}, std::false_type{}, RdfInt<0>{});
    else if (masked) with_r(std::false_type{}, std::true_type{}, RdfInt<0>{});
    else with_r(std::false_type{}, std::false_type{}, RdfInt<0>{});
}

static int rdf_grid(int n_frames, int n_atoms) {
    const long long npair = (long long)n_atoms * (n_atoms - 1) / 2;
    const long long items = (long long)n_frames * ((npair + RDF_CHUNK - 1) / RDF_CHUNK);
    return (int)(items < RDF_MAX_BLOCKS ? items : RDF_MAX_BLOCKS);
}

extern "C" int64_t mdg_rdf_partial_size(int n_frames, int n_atoms, int nbins) {
    (void)n_frames; (void)n_atoms;
    return (int64_t)RDF_MAX_BLOCKS * nbins;      // one partial histogram per persistent block / wave
}

// scaled spacing Ds = s * spacing of equally spaced centres, s = sqrt(-coeff log2 e); 0: the caller makes no such statement
static float rdf_spacing_s(float spacing, float coeff) {
    return spacing > 0.f && coeff < 0.f ? spacing * sqrtf(-coeff * LOG2E) : 0.f;
}

// lane-per-pair kernel: reach R (bins) for the scaled spacing Ds, waves per workgroup that fit the LDS
static int rdf_lane_reach(float spacing_s) {
    // the nearest uncovered bin is R + 1/2 spacings from the distance: (R + 1/2) Ds >= 5.3 => below 2^-28
    if (spacing_s >= 0.82f) return 6;
    if (spacing_s >= 0.465f) return 11;
    return 0;
}
// reach of the forward lane kernel (the 2R+1 rows a pair touches are its LDS traffic, so it is cut closer than
// the backward table's): (R + 1/2) Ds >= 4.65
static int rdf_fwd_reach(float spacing_s) {
    if (spacing_s >= 0.8455f) return 5;
    if (spacing_s >= 0.405f) return 11;
    return 0;
}
static size_t rdf_lane_lds(int nw, int R, int pxld, int nbins) {
    return sizeof(float) * ((size_t)(nbins + 2 * R) + (size_t)(nbins + 4 * R) + (size_t)nw * ((size_t)(nbins + 4 * R) * 64 + 3 * (size_t)pxld));
}

// ---- shared with the fused observable of the trajectory kernels and csrc/rdf_cell.hip (common.hpp): the one sizing of
// the fine grids for centres mu0 + k spacing and exp(coeff x^2)
RdfFinePlan mdg_rdf_fine_plan(float spacing, float coeff, int nbins) {
    RdfFinePlan P{};
    if (!(spacing > 0.f) || !(coeff < 0.f) || nbins < 2) return P;
    P.sc = sqrtf(-coeff * LOG2E);                                 // exp(coeff x^2) = exp2(-(sc x)^2)
    P.reach = 5.3f / P.sc;                                        // beyond: below 2^-28 of the peak
    P.h = 0.004f / P.sc;                                          // sc h = 0.004 (error bound: see rdf_fwd_fine_kernel)
    const double span = (double)(nbins - 1) * spacing + 2.0 * P.reach;
    const long long nfine = (long long)ceil(span / P.h) + 1;
    P.nfine = nfine <= RDF_FINE_MAX ? nfine : 0;                  // 0: does not fit the workgroup's LDS histogram
    const float spacing_s = spacing * P.sc;
    const int R = rdf_lane_reach(spacing_s);
    // (the u-space table of the ring adjoint: RDF_SUB_U cells per spacing, rdf_u_grid)
    const int ncell_u = (nbins - 1 + 2 * (R + 1)) * RDF_SUB_U;
    if (R && spacing_s <= 1.0f && ncell_u + 1 <= 4096) { P.reach_bins = R; P.ncell = ncell_u; }
    return P;
}

enum class RdfFwd { direct = MDG_RDF_FWD_DIRECT, block8 = MDG_RDF_FWD_BLOCK8, lane = MDG_RDF_FWD_LANE,
                    half = MDG_RDF_FWD_HALF, fine = MDG_RDF_FWD_FINE };
struct RdfFwdPlan {
    RdfFwd variant;
    int R, waves, grid;                  // reach in bins (lane, half), waves per workgroup, workgroups
    size_t lds, scratch_words;           // dynamic LDS bytes; stream-ordered scratch, 32-bit words
    int pxld; bool px128;                // lane, half, fine: row stride of the LDS coordinates; it is the compile-time 128
    int n_entries, iters, n_padded; uint32_t pad_entry;   // lane, half: pair table entries, sweep iterations, padding
    RdfFinePlan fine;                    // fine: nfine, h, reach of the integer histogram
};
static RdfFwdPlan rdf_fwd_plan(int n_frames, int n_atoms, int nbins, float spacing, float coeff, bool diag, bool masked) {
    RdfFwdPlan P{};
    // spacing_s is the caller's statement that mu is a linspace; 0 selects the direct kernel
    const float spacing_s = rdf_spacing_s(spacing, coeff);
    const bool many = n_frames >= RDF_MANY_FRAMES;
    // ---- many frames, equally spaced centres: fine integer histogram (see rdf_fwd_fine_kernel) when it fits the LDS
    // (the first-order term of the binning error averages out statistically, ~ (s h) 0.4 / sqrt(pairs near a centre):
    //  small systems -- cheap anyway -- keep the exact lane-private kernels below)
    P.fine = mdg_rdf_fine_plan(spacing, coeff, nbins);
    const int ld = (n_atoms + 1) & ~1;
    const size_t lds_fine = sizeof(float) * ((size_t)P.fine.nfine + RDF_FINE_WAVES * 3 * (size_t)ld);
    const bool fine_can = P.fine.nfine > 0 && n_atoms <= RDF_FINE_ATOMS && lds_fine <= RDF_LDS_BUDGET;
    if (fine_can && many && n_atoms >= 64) {
        P.variant = RdfFwd::fine; P.waves = RDF_FINE_WAVES; P.lds = lds_fine; P.pxld = ld;
        P.grid = min((n_frames + RDF_FINE_WAVES - 1) / RDF_FINE_WAVES, 256);   // one resident workgroup (16 waves) per CU
        const long long npair = (long long)n_atoms * (n_atoms - 1) / 2;
        P.scratch_words = (size_t)P.fine.nfine + 4 + (size_t)npair + 128;   // [nfine] global histogram | count | pair table
        return P;
    }
    // ---- many frames, equally spaced centres: one wave per frame, one lane per pair
    const int R = nbins >= 2 && n_atoms <= RDF_TABLE_MAX_ATOMS ? rdf_fwd_reach(spacing_s) : 0;
    if (R && many) {
        // coordinate stride: even, with at least two NaN columns after the atoms for the padding entries;
        // compile-time (immediate LDS offsets) for the common shape: orthorhombic, no mask
        const int npad_col = (n_atoms + 1) & ~1;
        P.px128 = npad_col + 2 <= 128 && diag && !masked;
        P.pxld = P.px128 ? 128 : npad_col + 2;
        int nw = 4;
        while (nw > 1 && rdf_lane_lds(nw, R, P.pxld, nbins) > RDF_LDS_BUDGET) nw >>= 1;
        const size_t lds = rdf_lane_lds(nw, R, P.pxld, nbins);
        if (lds <= RDF_LDS_BUDGET) {
            P.R = R;
            // sum of rdf_row_entries(i, N) over the rows i < N - 1: row i holds ceil(N / 2) - floor((i + 1) / 2)
            const int N = n_atoms;
            P.n_entries = (N - 1) * ((N + 1) / 2) - ((N - 1) / 2) * (N / 2);
            P.iters = (((P.n_entries + 63) / 64) + 3) & ~3;                   // (the loop is unrolled by four)
            P.n_padded = (P.iters + 5) * 64;
            P.pad_entry = (uint32_t)(4 * npad_col) | ((uint32_t)(4 * npad_col) << 16);
            P.scratch_words = (size_t)P.n_padded;
            // half-width columns, eight waves per workgroup, when they fit (R = 5, 100 bins: 137 KB)
            const size_t rows_h = (size_t)((nbins + 4 * R + 3) & ~1);
            const size_t lds_half = sizeof(float) * (2 * rows_h + 8 * (rows_h * 32 + 3 * (size_t)P.pxld));
            // (spacing_s <= 1.5: the recurrence multipliers of a rejected pair, y0 clamped to 20, stay finite)
            const bool half = R == 5 && spacing_s <= 1.5f && lds_half <= RDF_LDS_BUDGET;
            P.variant = half ? RdfFwd::half : RdfFwd::lane;
            P.waves = half ? 8 : nw;
            P.lds = half ? lds_half : lds;
            P.grid = min((n_frames + P.waves - 1) / P.waves, RDF_MAX_BLOCKS / P.waves);
            return P;
        }
    }
    // ---- few frames or arbitrary centres: persistent blocks over (frame, candidate chunk) work items.
    // Equally spaced centres with Ds = s * spacing <= 1: 8-bin blocks + recurrence
    const int nblk = (nbins + RDF_KB - 1) / RDF_KB;
    const bool block8 = spacing_s > 0.f && spacing_s <= 1.0f && nbins >= 2 * RDF_KB && nblk <= RDF_BLOCK;
    P.variant = block8 ? RdfFwd::block8 : RdfFwd::direct;
    P.waves = RDF_BLOCK / 64;
    P.grid = rdf_grid(n_frames, n_atoms);
    P.lds = block8 ? sizeof(float) * (RDF_BLOCK + 16 + (size_t)(RDF_BLOCK / nblk) * nblk * RDF_KB) : 0;
    return P;
}

// stream-ordered scratch (no state, re-entrant); a failed allocation is an error in both directions
template <class T>
static T* rdf_scratch(size_t count, hipStream_t st, const char* who) {
    T* p = nullptr;
    if (hipMallocAsync((void**)&p, sizeof(T) * count, st) == hipSuccess && p) return p;
    mdg_set_error("%s: scratch allocation failed", who);
    return nullptr;
}
static void rdf_fine_finish_launch(const uint32_t* ghist, const RdfFinePlan& G, const float* mu, int nbins, float* raw,
                                   hipStream_t st) {
    hipLaunchKernelGGL(rdf_fine_finish_kernel, dim3(nbins), dim3(64), 0, st, ghist, (int)G.nfine, G.h, mu, G.sc, G.reach,
                       nbins, raw);
}

static int rdf_launch_fine(const RdfFwdPlan& P, const RdfFrames& a, float* raw) {
    const int nfine = (int)P.fine.nfine;
    uint32_t* ghist = rdf_scratch<uint32_t>(P.scratch_words, a.st, "rdf_fwd");    // [nfine] | count | pair table
    if (!ghist) return MDG_ELAUNCH;
    int32_t* count = reinterpret_cast<int32_t*>(ghist + nfine);
    uint32_t* tab = ghist + nfine + 4;
    MDG_HIP(hipMemsetAsync(ghist, 0, sizeof(uint32_t) * (size_t)(nfine + 4), a.st));
    hipLaunchKernelGGL(rdf_fine_table_kernel, dim3(1), dim3(1024), 0, a.st, a.N, a.mask, tab, count);
    // (the fine grid starts at mu[0] - reach; the kernels read mu[0] themselves: no host copy)
    rdf_dispatch<0>(a.cell->diag, false, false, 0, [&](auto d, auto...) {
        hipLaunchKernelGGL(rdf_fwd_fine_kernel<decltype(d)::value>, dim3(P.grid), dim3(64 * RDF_FINE_WAVES), P.lds, a.st, a.xyz,
                           a.nF, a.N, *a.cell, a.rc2, tab, count, a.mu, P.fine.reach, 1.0f / P.fine.h, nfine, P.pxld, ghist);
    });
    rdf_fine_finish_launch(ghist, P.fine, a.mu, a.nbins, raw, a.st);
    (void)hipFreeAsync(ghist, a.st);
    MDG_CHECK_LAUNCH("rdf_fwd_fine_kernel");
    return MDG_OK;
}
// half, lane: the pair table, the sweep, the sum over the waves' partial histograms
static int rdf_launch_pairs(const RdfFwdPlan& P, const RdfFrames& a, float* raw, float* partial) {
    uint32_t* tab = rdf_scratch<uint32_t>(P.scratch_words, a.st, "rdf_fwd");
    if (!tab) return MDG_ELAUNCH;
    hipLaunchKernelGGL(rdf_pair_table_kernel, dim3(a.N), dim3(256), 0, a.st, tab, a.N, P.n_entries, P.n_padded, P.pad_entry);
    const bool half = P.variant == RdfFwd::half;
    if (half)
        rdf_dispatch<5>(a.cell->diag, a.mask != nullptr, P.px128, P.R, [&](auto d, auto m, auto px, auto r) {
            rdf_launch(rdf_fwd_half_kernel<decltype(d)::value, decltype(r)::value, decltype(m)::value, decltype(px)::value>,
                       P.grid, 64 * P.waves, P.lds, a, tab, P.iters, P.pxld, partial);
        });
    else
        rdf_dispatch<5, 11>(a.cell->diag, a.mask != nullptr, P.px128, P.R, [&](auto d, auto m, auto px, auto r) {
            rdf_launch(rdf_fwd_lane_kernel<decltype(d)::value, decltype(r)::value, decltype(m)::value, decltype(px)::value>,
                       P.grid, 64 * P.waves, P.lds, a, tab, P.iters, P.pxld, partial);
        });
    hipLaunchKernelGGL(rdf_finish_kernel, dim3(a.nbins), dim3(64), 0, a.st, partial, P.grid * P.waves, a.nbins, raw);
    (void)hipFreeAsync(tab, a.st);
    MDG_CHECK_LAUNCH(half ? "rdf_fwd_half_kernel" : "rdf_fwd_lane_kernel");
    return MDG_OK;
}
// block8, direct: the persistent blocks, the sum over their partial histograms
static int rdf_launch_blocks(const RdfFwdPlan& P, const RdfFrames& a, float* raw, float* partial) {
    rdf_dispatch<0>(a.cell->diag, false, false, 0, [&](auto d, auto...) {
        if (P.variant == RdfFwd::block8) rdf_launch(rdf_fwd_block8_kernel<decltype(d)::value>, P.grid, RDF_BLOCK, P.lds, a, partial);
        else rdf_launch(rdf_fwd_kernel<decltype(d)::value>, P.grid, RDF_BLOCK, P.lds, a, partial);
    });
    hipLaunchKernelGGL(rdf_finish_kernel, dim3(a.nbins), dim3(64), 0, a.st, partial, P.grid, a.nbins, raw);
    MDG_CHECK_LAUNCH("rdf_fwd_kernel");
    return MDG_OK;
}

static int rdf_fwd_impl(const float* xyz, int n_frames, int n_atoms, const MdgCell* cell, float cutoff,
                        const uint8_t* mask, const float* mu, float coeff, int nbins, float* raw,
                        float* partial, float spacing, void* stream) {
    MDG_CHECK_ARG(xyz && cell && mu && raw && partial, "rdf_fwd: null buffer");
    MDG_CHECK_ARG(n_frames > 0 && n_atoms > 1 && nbins > 0, "rdf_fwd: bad sizes");
    MDG_CHECK_ARG(nbins <= RDF_BLOCK, "rdf_fwd: nbins > %d not supported", RDF_BLOCK);
    MDG_CHECK_ARG(coeff < 0.f, "rdf_fwd: coeff must be negative (-0.5 / width^2)");
    const RdfFwdPlan P = rdf_fwd_plan(n_frames, n_atoms, nbins, spacing, coeff, cell->diag != 0, mask != nullptr);
    const RdfFrames a{xyz, n_frames, n_atoms, cell, cutoff * cutoff, mask, mu, coeff, nbins, (hipStream_t)stream};
    switch (P.variant) {
    case RdfFwd::fine: return rdf_launch_fine(P, a, raw);
    case RdfFwd::half: case RdfFwd::lane: return rdf_launch_pairs(P, a, raw, partial);
    default: return rdf_launch_blocks(P, a, raw, partial);
    }
}
extern "C" int mdg_rdf_fwd(const float* xyz, int n_frames, int n_atoms, const MdgCell* cell, float cutoff,
                           const uint8_t* mask, const float* mu, float coeff, int nbins, float* raw,
                           float* partial, void* stream) {
    return rdf_fwd_impl(xyz, n_frames, n_atoms, cell, cutoff, mask, mu, coeff, nbins, raw, partial, 0.f, stream);
}

extern "C" int mdg_rdf_fwd_uniform(const float* xyz, int n_frames, int n_atoms, const MdgCell* cell, float cutoff,
                                   const uint8_t* mask, const float* mu, float spacing, float coeff, int nbins,
                                   float* raw, float* partial, void* stream) {
    return rdf_fwd_impl(xyz, n_frames, n_atoms, cell, cutoff, mask, mu, coeff, nbins, raw, partial, spacing, stream);
}

enum class RdfBwd { atom = MDG_RDF_BWD_ATOM, table = MDG_RDF_BWD_TABLE, frame = MDG_RDF_BWD_FRAME };
struct RdfBwdPlan {
    RdfBwd variant;
    int R, waves, grid;                  // reach in bins (table: of the tabulated sum), waves per workgroup, workgroups
    size_t lds;                          // dynamic LDS bytes
    int ldw, cells;                      // table: length of the index-doubled rows, cells of the cubic-Hermite table
    bool fits;                           // false: no variant holds this shape
};

// waves (= frames) per workgroup of the wave-per-frame kernels, limited by the `per_wave` floats of LDS each one needs
static void rdf_bwd_waves(RdfBwdPlan& P, int n_frames, size_t shared, size_t per_wave) {
    P.waves = 4;
    while (P.waves > 1 && sizeof(float) * (shared + P.waves * per_wave) > 150 * 1024) P.waves >>= 1;
    P.lds = sizeof(float) * (shared + P.waves * per_wave);
    P.grid = (n_frames + P.waves - 1) / P.waves;
    P.fits = P.lds <= RDF_LDS_MAX;
}
static RdfBwdPlan rdf_bwd_plan(int n_frames, int n_atoms, int nbins, float spacing, float coeff) {
    RdfBwdPlan P{};
    // few frames or frames too large for LDS: (frame, atom) gather variant, 16 lanes per atom
    if (n_frames < RDF_MANY_FRAMES || n_atoms > 4096) {
        P.variant = RdfBwd::atom; P.waves = 4; P.lds = sizeof(float) * 2 * nbins; P.fits = true;
        P.grid = (int)(((long long)n_frames * n_atoms + 15) / 16);
        return P;
    }
    P.R = nbins >= 2 ? rdf_lane_reach(rdf_spacing_s(spacing, coeff)) : 0;
    // table of dL/dd on the fine nodes, then the wave-per-frame kernel with a table lookup per pair: for width ~ spacing
    // (Ds <= 1) and at most 4096 nodes
    {
        const float spacing_s = rdf_spacing_s(spacing, coeff);
        P.cells = P.R && spacing_s <= 1.0f && fine_nodes(nbins, P.R) <= 4096 ? fine_nodes(nbins, P.R) - 1 : 0;
    }
    if (P.cells) {
        // index-doubled rows: the last lane group's idle lanes reach index 64 ceil(N/64) - 1 + N/2 + 1
        P.ldw = (max(2 * n_atoms, 64 * ((n_atoms + 63) / 64) + n_atoms / 2 + 1) + 2) & ~1;
        rdf_bwd_waves(P, n_frames, 4 * (size_t)P.cells, 6 * (size_t)P.ldw);
        P.variant = RdfBwd::table;
        if (P.fits) return P;
    }
    // the bin recurrence (R > 0) or the direct sum, one wave per frame with the 6N floats of its frame
    P.ldw = P.cells = 0;
    rdf_bwd_waves(P, n_frames, 2 * (size_t)nbins + 6 * (size_t)P.R, 6 * (size_t)n_atoms);
    P.variant = RdfBwd::frame;
    return P;
}

static int rdf_launch_bwd_atom(const RdfBwdPlan& P, const RdfFrames& a, const float* g_raw, float* g_xyz, int uniform) {
    rdf_dispatch<0>(a.cell->diag, false, false, 0, [&](auto d, auto...) {
        rdf_launch(rdf_bwd_atom_kernel<decltype(d)::value, 16>, P.grid, 64 * P.waves, P.lds, a, g_raw, g_xyz, uniform);
    });
    MDG_CHECK_LAUNCH("rdf_bwd_atom_kernel");
    return MDG_OK;
}
static int rdf_launch_bwd_table(const RdfBwdPlan& P, const RdfFrames& a, const float* g_raw, float* g_xyz) {
    float4* tab = rdf_scratch<float4>((size_t)P.cells, a.st, "rdf_bwd");
    if (!tab) return MDG_ELAUNCH;
    hipLaunchKernelGGL(rdf_bwd_table_kernel, dim3((P.cells + 255) / 256), dim3(256), 0, a.st, a.mu, a.coeff, a.nbins, g_raw, P.R, tab);
    rdf_dispatch<0>(a.cell->diag, false, false, 0, [&](auto d, auto...) {
        hipLaunchKernelGGL(rdf_bwd_fine_kernel<decltype(d)::value>, dim3(P.grid), dim3(64 * P.waves), P.lds, a.st, a.xyz, a.nF,
                           a.N, *a.cell, a.rc2, a.mask, a.mu, a.nbins, P.R, tab, P.ldw, g_xyz);
    });
    (void)hipFreeAsync(tab, a.st);
    MDG_CHECK_LAUNCH("rdf_bwd_fine_kernel");
    return MDG_OK;
}
static int rdf_launch_bwd_frame(const RdfBwdPlan& P, const RdfFrames& a, const float* g_raw, float* g_xyz, int uniform) {
    rdf_dispatch<6, 11, 0>(a.cell->diag, false, false, P.R, [&](auto d, auto, auto, auto r) {
        rdf_launch(rdf_bwd_kernel<decltype(d)::value, decltype(r)::value>, P.grid, 64 * P.waves, P.lds, a, g_raw, g_xyz, uniform);
    });
    MDG_CHECK_LAUNCH("rdf_bwd_kernel");
    return MDG_OK;
}

static int rdf_bwd_impl(const float* xyz, int n_frames, int n_atoms, const MdgCell* cell, float cutoff,
                        const uint8_t* mask, const float* mu, float coeff, int nbins, const float* g_raw,
                        float* g_xyz, float spacing, void* stream) {
    MDG_CHECK_ARG(xyz && cell && mu && g_raw && g_xyz, "rdf_bwd: null buffer");
    MDG_CHECK_ARG(n_frames > 0 && n_atoms > 1 && nbins > 0, "rdf_bwd: bad sizes");
    MDG_CHECK_ARG(coeff < 0.f, "rdf_bwd: coeff must be negative (-0.5 / width^2)");
    const RdfBwdPlan P = rdf_bwd_plan(n_frames, n_atoms, nbins, spacing, coeff);
    MDG_CHECK_ARG(P.fits, "rdf_bwd: N=%d does not fit the LDS-resident frame kernel", n_atoms);
    const RdfFrames a{xyz, n_frames, n_atoms, cell, cutoff * cutoff, mask, mu, coeff, nbins, (hipStream_t)stream};
    const int uniform = rdf_spacing_s(spacing, coeff) > 0.f;
    switch (P.variant) {
    case RdfBwd::atom: return rdf_launch_bwd_atom(P, a, g_raw, g_xyz, uniform);
    case RdfBwd::table: return rdf_launch_bwd_table(P, a, g_raw, g_xyz);
    default: return rdf_launch_bwd_frame(P, a, g_raw, g_xyz, uniform);
    }
}

extern "C" int mdg_rdf_bwd(const float* xyz, int n_frames, int n_atoms, const MdgCell* cell, float cutoff,
                           const uint8_t* mask, const float* mu, float coeff, int nbins, const float* g_raw,
                           float* g_xyz, void* stream) {
    return rdf_bwd_impl(xyz, n_frames, n_atoms, cell, cutoff, mask, mu, coeff, nbins, g_raw, g_xyz, 0.f, stream);
}

extern "C" int mdg_rdf_bwd_uniform(const float* xyz, int n_frames, int n_atoms, const MdgCell* cell, float cutoff,
                                   const uint8_t* mask, const float* mu, float spacing, float coeff, int nbins,
                                   const float* g_raw, float* g_xyz, void* stream) {
    return rdf_bwd_impl(xyz, n_frames, n_atoms, cell, cutoff, mask, mu, coeff, nbins, g_raw, g_xyz, spacing, stream);
}

// The plans' answers without a launch: MDG_RDF_FWD_* / MDG_RDF_BWD_*, or -1 where the launch would refuse the shape.
// info (may be null): MDG_RDF_PLAN_INFO words {R, waves per workgroup, workgroups, LDS bytes, row stride (forward: of the
// coordinates, backward: ldw), forward: 1 for 128-column rows / backward: table cells}
static int rdf_report(int variant, int32_t* info, const int32_t (&v)[MDG_RDF_PLAN_INFO]) {
    for (int k = 0; info && k < MDG_RDF_PLAN_INFO; ++k) info[k] = v[k];
    return variant;
}
extern "C" int mdg_rdf_fwd_variant(int n_frames, int n_atoms, int nbins, float spacing, float coeff, int diag, int masked,
                                   int32_t* info) {
    if (!(n_frames > 0 && n_atoms > 1 && nbins > 0 && nbins <= RDF_BLOCK && coeff < 0.f)) return -1;
    const RdfFwdPlan P = rdf_fwd_plan(n_frames, n_atoms, nbins, spacing, coeff, diag != 0, masked != 0);
    return rdf_report((int)P.variant, info, {P.R, P.waves, P.grid, (int32_t)P.lds, P.pxld, P.px128});
}
extern "C" int mdg_rdf_bwd_variant(int n_frames, int n_atoms, int nbins, float spacing, float coeff, int, int, int32_t* info) {
    if (!(n_frames > 0 && n_atoms > 1 && nbins > 0 && coeff < 0.f)) return -1;
    const RdfBwdPlan P = rdf_bwd_plan(n_frames, n_atoms, nbins, spacing, coeff);      // (neither the cell nor a mask matters)
    return P.fits ? rdf_report((int)P.variant, info, {P.R, P.waves, P.grid, (int32_t)P.lds, P.ldw, P.cells}) : -1;
}
// The grids of mdg_rdf_fine_plan for these centres, host only: the fine integer histogram of the FINE variant, of
// mdg_rdf_fwd_ell and of mdg_rdf_fwd_cell (bins -- 0: it does not fit --, bin width h, reach: it starts at mu[0] - reach) and
// the nodes per centre spacing of the backward's derivative table.  Returns 0, or -1 for centres without a grid.
extern "C" int mdg_rdf_fine_grid(float spacing, float coeff, int nbins, int32_t* bins, float* h, float* reach, int32_t* table_sub) {
    const RdfFinePlan P = mdg_rdf_fine_plan(spacing, coeff, nbins);
    if (!(P.sc > 0.f)) return -1;
    if (bins) *bins = (int32_t)P.nfine;
    if (h) *h = P.h;
    if (reach) *reach = P.reach;
    if (table_sub) *table_sub = RDF_SUB;
    return 0;
}

int mdg_rdf_fine_finish(const uint32_t* ghist, const RdfFinePlan& P, const float* mu, int nbins, float* raw, hipStream_t st) {
    rdf_fine_finish_launch(ghist, P, mu, nbins, raw, st);
    MDG_CHECK_LAUNCH("rdf_fine_finish_kernel");
    return MDG_OK;
}
int mdg_rdf_bwd_table(const float* mu, float coeff, int nbins, const float* g_raw, const RdfFinePlan& P, float4* tab,
                      hipStream_t st) {
    const int nn = fine_nodes(nbins, P.reach_bins);                   // (this table's own grid: RDF_SUB nodes per spacing)
    hipLaunchKernelGGL(rdf_bwd_table_kernel, dim3((nn + 254) / 256), dim3(256), 0, st, mu, coeff, nbins, g_raw, P.reach_bins, tab);
    MDG_CHECK_LAUNCH("rdf_bwd_table_kernel");
    return MDG_OK;
}

int mdg_rdf_bwd_table_u(const float* mu, float coeff, int nbins, const float* g_raw, const RdfFinePlan& P, float4* tab,
                        hipStream_t st) {
    hipLaunchKernelGGL(rdf_bwd_table_u_kernel, dim3((P.ncell + 255) / 256), dim3(256), 0, st, mu, coeff, nbins, g_raw,
                       P.reach_bins, tab);
    MDG_CHECK_LAUNCH("rdf_bwd_table_u_kernel");
    return MDG_OK;
}

extern "C" int mdg_rdf_ell_supported(float spacing, float coeff, int nbins) {
    return mdg_rdf_fine_plan(spacing, coeff, nbins).nfine > 0;
}

extern "C" int mdg_rdf_fwd_ell(const float* pos, int64_t n_atoms_total, const MdgCell* cell, const int32_t* col,
                               const int32_t* shift, const int32_t* cnt, int max_nbr, const float* mu, float spacing,
                               float coeff, int nbins, float* raw, void* stream) {
    MDG_CHECK_ARG(pos && cell && col && shift && cnt && mu && raw && n_atoms_total > 0 && max_nbr > 0, "rdf_fwd_ell: bad arguments");
    const RdfFinePlan G = mdg_rdf_fine_plan(spacing, coeff, nbins);
    const long long nfine = G.nfine;
    MDG_CHECK_ARG(nfine > 0,"rdf_fwd_ell: the fine grid for these centres does not fit (see mdg_rdf_ell_supported)");
    hipStream_t st = (hipStream_t)stream;
    uint32_t* ghist = nullptr;
    MDG_HIP(hipMallocAsync((void**)&ghist, sizeof(uint32_t) * (size_t)nfine, st));
    MDG_HIP(hipMemsetAsync(ghist, 0, sizeof(uint32_t) * (size_t)nfine, st));
    const long long n_slots = (long long)n_atoms_total * max_nbr;
    long long grid = (n_slots + 1023) / 1024;
    if (grid > 256) grid = 256;
    hipLaunchKernelGGL(rdf_fwd_ell_kernel, dim3((unsigned)grid), dim3(1024), sizeof(uint32_t) * (size_t)nfine, st, pos, n_slots,
                       *cell, col, shift, cnt, max_nbr, mu, G.reach, 1.0f / G.h, (int)nfine, ghist);
    rdf_fine_finish_launch(ghist, G, mu, nbins, raw, st);
    (void)hipFreeAsync(ghist, st);
    MDG_CHECK_LAUNCH("rdf_fwd_ell_kernel");
    return MDG_OK;
}
