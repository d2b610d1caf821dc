// Bond-angle distribution (torchmd/observable.py:120-151, angle_distribution with compute_angle :166-179 and the triplet list
// of torchmd/topology.py:83-122) as a soft histogram over a per-atom neighbour list, and its gradient.
//
//   triplets   every ordered (i, j, k) of one frame with j the centre, (i, j) and (j, k) neighbour pairs of the list, k != i;
//              the two orders of one unordered (i, k) pair give the same angle, so each is evaluated once with weight 2
//   vectors    u = x_i - x_j, v = x_k - x_j, each re-imaged with topology.get_offsets on the diagonal cell
//              (o = -[u >= L/2] + [u < -L/2] per component, NON-strict on the upper side; piecewise constant, no derivative)
//   angle      theta = atan2(|u x v|, u.v): the reference's acos(u.v / sqrt(|u|^2 |v|^2)) without its loss of precision
//              near 0 and pi (where f32 acos of a rounded cosine is off by up to ~3e-4 rad)
//   histogram  raw[b] = sum 2 exp(coeff (theta - mu_b)^2),  mu_b = mu_0 + b h  (linspace centres, h = spacing)
//
// Reach: only the centres within R = 5.3 / s of theta are summed, s = sqrt(-coeff log2 e), so exp(coeff x^2) = exp2(-(s x)^2);
// a dropped term is <= exp2(-5.3^2) = 2^-28.1 of a peak term (the bound of the RDF list kernels, ops.RdfRawFn), and R follows
// the caller's width.  Inside the window, one exp2 at the nearest centre and two ratio recurrences outward
// (e_{b+1} = e_b r, r <- r q with q = exp2(-2 s^2 h^2)) replace one exp per bin.  The relative error of the recurrence grows
// as ~k^2/2 ulp over k steps, so it restarts from two direct exp2 every ADF_ANCHOR = 8 centres (<= ~28 ulp): with a width
// far above the spacing the window spans a hundred centres or more.
//
// Forward determinism: every contribution is a fixed-point integer (fx64, common.hpp) added into a per-workgroup LDS
// histogram and then into one global int64 word per bin -- integer sums do not depend on the order, so two launches are
// bitwise equal.  The scale is S = fx64_limit(n) / 2 with n = frames * atoms * max_nbr (max_nbr - 1) / 2, an upper bound on
// the unordered triplets of the launch, i.e. on the contributions one word can receive; every contribution is <= 2, so no
// word can leave int64.  A non-finite angle (non-finite positions) sets a flag word and the histogram comes out NaN.
//
// Backward: g_xyz[n] = d(sum_b g_raw[b] raw[b]) / dx_n, atom-centric like csrc/bonded.hip: thread n sums, in a fixed order,
// its centre-role triplets (unordered neighbour pairs of its own row) and its end-role triplets (for each neighbour b, every
// other neighbour k of b) -- no atomics, bitwise reproducible.  d theta / du = u x w / (|u|^2 |w|) and
// d theta / dv = -v x w / (|v|^2 |w|), w = u x v: no cancellation near collinearity.
// Degenerate triplets: when |w| <= ADF_EPS |u| |v| (ADF_EPS = 2^-20, i.e. sin theta below ~1e-6, under the f32 rounding of w
// itself) the triplet contributes zero gradient -- theta has a kink at 0 and pi, and zero is its symmetric subgradient.
#include <math.h>
#include "common.hpp"

namespace {

constexpr int ADF_BLOCK = 256;
constexpr int ADF_MAX_BLOCKS = 2048;     // persistent forward grid: one LDS histogram flush per workgroup
constexpr int ADF_MAX_BINS = 4096;
constexpr float ADF_EPS = 9.5367431640625e-07f;   // 2^-20
constexpr float ADF_REACH = 5.3f;
constexpr int ADF_ANCHOR = 8;            // the recurrence restarts from a direct exp2 every 8 centres

struct AdfArgs {
    const float* pos;
    const int32_t* col;
    const int32_t* cnt;
    const float* mu;
    long long n_total;       // frames * atoms (rows of the list)
    int max_nbr, nbins;
    float L[3];
    float s2;                // s^2 = -coeff log2 e
    float h, inv_h, q;       // spacing, 1 / spacing (0 when nbins == 1), exp2(-2 s^2 h^2)
    float reach, reach_b;    // R and R / |h| in bins
};

// topology.get_offsets (topology.py:75-80) on one component
__device__ __forceinline__ float reimage(float b, float L) {
    return b + ((b < -0.5f * L ? 1.f : 0.f) - (b >= 0.5f * L ? 1.f : 0.f)) * L;
}

__device__ __forceinline__ float3 bond(const float* __restrict__ pos, long long a, float3 xc, const float* L) {
    return make_float3(reimage(pos[3 * a] - xc.x, L[0]), reimage(pos[3 * a + 1] - xc.y, L[1]), reimage(pos[3 * a + 2] - xc.z, L[2]));
}

__device__ __forceinline__ float dot3(float3 a, float3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ float3 cross3(float3 a, float3 b) {
    return make_float3(fmaf(a.y, b.z, -a.z * b.y), fmaf(a.z, b.x, -a.x * b.z), fmaf(a.x, b.y, -a.y * b.x));
}

// re-anchor the recurrence at a centre at distance db from theta: e = exp2(-s^2 db^2) directly, and the next ratio
// (dir = -1: towards higher bins, db decreasing by h; dir = +1: towards lower bins)
__device__ __forceinline__ void anchor(const AdfArgs& A, float db, float dir, float& eb, float& r) {
    eb = exp2f(-A.s2 * db * db);
    r = exp2f(A.s2 * A.h * (-dir * 2.f * db - A.h));
}

// the window of centres within the reach of theta: [lo, hi] and the nearest centre c (false: none)
__device__ __forceinline__ bool window(const AdfArgs& A, const float* mu_s, float th, int& lo, int& hi, int& c) {
    if (A.nbins == 1) {
        lo = hi = c = 0;
        return fabsf(th - mu_s[0]) <= A.reach;
    }
    const float t = (th - mu_s[0]) * A.inv_h;
    const float tl = fmaxf(ceilf(t - A.reach_b), 0.f), th_ = fminf(floorf(t + A.reach_b), (float)(A.nbins - 1));
    if (!(tl <= th_)) return false;
    lo = (int)tl;
    hi = (int)th_;
    c = min(max((int)rintf(t), lo), hi);
    return true;
}

// FRAMES = false: a persistent grid over all list rows, one LDS histogram per workgroup flushed into the global words (K14).
// FRAMES = true (K35): workgroup f walks the n_atoms rows of frame f alone and writes its LDS histogram straight to
// raw[f, :] -- no global atomics; a non-finite angle makes that row NaN and no other.
template <bool FRAMES>
__global__ __launch_bounds__(ADF_BLOCK) void adf_fwd_kernel(AdfArgs A, float scale, unsigned long long* __restrict__ words,
                                                            int n_atoms, double inv_scale, float* __restrict__ raw) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long hist[];
    float* mu_s = reinterpret_cast<float*>(hist + A.nbins);
    __shared__ int bad;
    for (int b = threadIdx.x; b < A.nbins; b += ADF_BLOCK) {
        hist[b] = 0ull;
        mu_s[b] = A.mu[b];
    }
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const float w2 = 2.f * scale;                                  // weight 2: both orders of the unordered pair
    const long long j_lo = FRAMES ? (long long)blockIdx.x * n_atoms : (long long)blockIdx.x * ADF_BLOCK;
    const long long j_hi = FRAMES ? j_lo + n_atoms : A.n_total;
    const long long j_step = FRAMES ? ADF_BLOCK : (long long)gridDim.x * ADF_BLOCK;
    for (long long j = j_lo + threadIdx.x; j < j_hi; j += j_step) {
        const int n = A.cnt[j];
        const int32_t* row = A.col + j * A.max_nbr;
        const float3 xc = make_float3(A.pos[3 * j], A.pos[3 * j + 1], A.pos[3 * j + 2]);
        for (int p = 0; p + 1 < n; ++p) {
            const float3 u = bond(A.pos, row[p], xc, A.L);
            for (int qq = p + 1; qq < n; ++qq) {
                const float3 v = bond(A.pos, row[qq], xc, A.L);
                const float3 w = cross3(u, v);
                const float th = atan2f(sqrtf(dot3(w, w)), dot3(u, v));
                if (!(th == th)) { bad = 1; continue; }
                int lo, hi, c;
                if (!window(A, mu_s, th, lo, hi, c)) continue;
                const float d = th - mu_s[c];
                const float e = exp2f(-A.s2 * d * d);
                atomicAdd(&hist[c], fx64(w2 * e));
                float eb = e, r = exp2f(A.s2 * A.h * (2.f * d - A.h));         // e_{b+1} / e_b at b = c
                for (int b = c + 1; b <= hi; ++b) {
                    if (((b - c) & (ADF_ANCHOR - 1)) == 0) anchor(A, d - (float)(b - c) * A.h, -1.f, eb, r);
                    else { eb *= r; r *= A.q; }
                    atomicAdd(&hist[b], fx64(w2 * eb));
                }
                eb = e; r = exp2f(-A.s2 * A.h * (2.f * d + A.h));                // e_{b-1} / e_b at b = c
                for (int b = c - 1; b >= lo; --b) {
                    if (((c - b) & (ADF_ANCHOR - 1)) == 0) anchor(A, d + (float)(c - b) * A.h, 1.f, eb, r);
                    else { eb *= r; r *= A.q; }
                    atomicAdd(&hist[b], fx64(w2 * eb));
                }
            }
        }
    }
    __syncthreads();
    if (FRAMES) {
        const bool nan = bad != 0;
        float* out = raw + (size_t)blockIdx.x * A.nbins;
        for (int b = threadIdx.x; b < A.nbins; b += ADF_BLOCK)
            out[b] = nan ? __int_as_float(0x7fc00000) : (float)((double)(long long)hist[b] * inv_scale);
        return;
    }
    for (int b = threadIdx.x; b < A.nbins; b += ADF_BLOCK)
        if (hist[b]) atomicAdd(&words[b], hist[b]);
    if (threadIdx.x == 0 && bad) atomicOr(reinterpret_cast<unsigned int*>(words + A.nbins), 1u);
}

__global__ void adf_finish_kernel(const unsigned long long* __restrict__ words, int nbins, double inv_scale, float* __restrict__ raw) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbins) return;
    const bool bad = reinterpret_cast<const unsigned int*>(words + nbins)[0] != 0u;
    raw[b] = bad ? __int_as_float(0x7fc00000) : (float)((double)(long long)words[b] * inv_scale);
}

// dL/dtheta of one unordered triplet: 2 sum_b g_b d e_b / d theta,  d e_b / d theta = -2 ln2 s^2 (theta - mu_b) e_b
__device__ __forceinline__ float dl_dtheta(const AdfArgs& A, const float* mu_s, const float* g_s, float th) {
    int lo, hi, c;
    if (!window(A, mu_s, th, lo, hi, c)) return 0.f;
    const float d = th - mu_s[c];
    const float e = exp2f(-A.s2 * d * d);
    float acc = g_s[c] * d * e;
    float eb = e, r = exp2f(A.s2 * A.h * (2.f * d - A.h)), db = d;
    for (int b = c + 1; b <= hi; ++b) {
        db = d - (float)(b - c) * A.h;
        if (((b - c) & (ADF_ANCHOR - 1)) == 0) anchor(A, db, -1.f, eb, r);
        else { eb *= r; r *= A.q; }
        acc = fmaf(g_s[b] * db, eb, acc);
    }
    eb = e; r = exp2f(-A.s2 * A.h * (2.f * d + A.h));
    for (int b = c - 1; b >= lo; --b) {
        db = d + (float)(c - b) * A.h;
        if (((c - b) & (ADF_ANCHOR - 1)) == 0) anchor(A, db, 1.f, eb, r);
        else { eb *= r; r *= A.q; }
        acc = fmaf(g_s[b] * db, eb, acc);
    }
    return -4.f * 0.69314718055994531f * A.s2 * acc;
}

// FRAMES = false: one g_raw [nbins] for every row (K14), grid = blocks of rows.
// FRAMES = true (K35): grid (frames, blocks of the atoms of a frame); a thread reads the g_raw row of its own frame.
template <bool FRAMES>
__global__ __launch_bounds__(ADF_BLOCK) void adf_bwd_kernel(AdfArgs A, const float* __restrict__ g_raw, float* __restrict__ g_xyz,
                                                            int n_atoms) {
    extern __shared__ __attribute__((aligned(16))) float smb[];
    float* mu_s = smb;
    float* g_s = smb + A.nbins;
    for (int b = threadIdx.x; b < A.nbins; b += ADF_BLOCK) {
        mu_s[b] = A.mu[b];
        g_s[b] = g_raw[(FRAMES ? (size_t)blockIdx.x * A.nbins : (size_t)0) + b];
    }
    __syncthreads();
    const int a_in = blockIdx.y * ADF_BLOCK + threadIdx.x;           // FRAMES: the atom inside its frame
    const long long a = FRAMES ? (long long)blockIdx.x * n_atoms + a_in : (long long)blockIdx.x * ADF_BLOCK + threadIdx.x;
    if (FRAMES ? a_in >= n_atoms : a >= A.n_total) return;
    const int n = A.cnt[a];
    const int32_t* row = A.col + a * A.max_nbr;
    const float3 xa = make_float3(A.pos[3 * a], A.pos[3 * a + 1], A.pos[3 * a + 2]);
    float gx = 0.f, gy = 0.f, gz = 0.f;
    // centre role: u, v from a to two of its neighbours
    for (int p = 0; p + 1 < n; ++p) {
        const float3 u = bond(A.pos, row[p], xa, A.L);
        const float uu = dot3(u, u);
        for (int qq = p + 1; qq < n; ++qq) {
            const float3 v = bond(A.pos, row[qq], xa, A.L);
            const float vv = dot3(v, v);
            const float3 w = cross3(u, v);
            const float ww = sqrtf(dot3(w, w));
            if (ww <= ADF_EPS * sqrtf(uu * vv)) continue;
            const float G = dl_dtheta(A, mu_s, g_s, atan2f(ww, dot3(u, v)));
            if (G == 0.f) continue;
            const float3 cu = cross3(u, w), cv = cross3(v, w);
            const float su = G / (uu * ww), sv = G / (vv * ww);
            // d theta/dx_a = -(d theta/du + d theta/dv) = -(u x w / (|u|^2 |w|) - v x w / (|v|^2 |w|))
            gx -= su * cu.x - sv * cv.x;
            gy -= su * cu.y - sv * cv.y;
            gz -= su * cu.z - sv * cv.z;
        }
    }
    // end role: for each neighbour b of a, the triplets (a, b, k) centred on b
    for (int p = 0; p < n; ++p) {
        const long long b = row[p];
        const float3 xb = make_float3(A.pos[3 * b], A.pos[3 * b + 1], A.pos[3 * b + 2]);
        const float3 u = make_float3(reimage(xa.x - xb.x, A.L[0]), reimage(xa.y - xb.y, A.L[1]), reimage(xa.z - xb.z, A.L[2]));
        const float uu = dot3(u, u);
        const int m = A.cnt[b];
        const int32_t* rb = A.col + b * A.max_nbr;
        for (int qq = 0; qq < m; ++qq) {
            const long long k = rb[qq];
            if (k == a) continue;
            const float3 v = bond(A.pos, k, xb, A.L);
            const float vv = dot3(v, v);
            const float3 w = cross3(u, v);
            const float ww = sqrtf(dot3(w, w));
            if (ww <= ADF_EPS * sqrtf(uu * vv)) continue;
            const float G = dl_dtheta(A, mu_s, g_s, atan2f(ww, dot3(u, v)));
            if (G == 0.f) continue;
            const float3 cu = cross3(u, w);
            const float su = G / (uu * ww);
            gx = fmaf(su, cu.x, gx);
            gy = fmaf(su, cu.y, gy);
            gz = fmaf(su, cu.z, gz);
        }
    }
    g_xyz[3 * a] = gx;
    g_xyz[3 * a + 1] = gy;
    g_xyz[3 * a + 2] = gz;
}

int adf_args(AdfArgs& A, const float* pos, int n_frames, int n_atoms, const MdgCell* cell, float cutoff, const int32_t* col,
             const int32_t* cnt, int max_nbr, const float* mu, float spacing, float coeff, int nbins) {
    MDG_CHECK_ARG(pos && cell && col && cnt && mu, "adf: null argument");
    MDG_CHECK_ARG(n_frames > 0 && n_atoms > 0 && max_nbr > 0, "adf: empty system or list");
    MDG_CHECK_ARG((long long)n_frames * n_atoms < (1ll << 31), "adf: more than 2^31 list rows in one call (chunk the frames)");
    MDG_CHECK_ARG(cell->diag, "adf: the angle observable takes the diagonal of the cell (torchmd/observable.py:30)");
    MDG_CHECK_ARG(cutoff > 0.f, "adf: cutoff must be positive");
    MDG_CHECK_ARG(nbins >= 1 && nbins <= ADF_MAX_BINS, "adf: nbins must be in [1, %d], got %d", ADF_MAX_BINS, nbins);
    MDG_CHECK_ARG(coeff < 0.f && isfinite(coeff), "adf: coeff must be finite and negative (width > 0), got %g", (double)coeff);
    MDG_CHECK_ARG(nbins == 1 || (spacing != 0.f && isfinite(spacing)), "adf: the centres must be distinct");
    A.pos = pos; A.col = col; A.cnt = cnt; A.mu = mu;
    A.n_total = (long long)n_frames * n_atoms;
    A.max_nbr = max_nbr; A.nbins = nbins;
    A.L[0] = cell->h[0]; A.L[1] = cell->h[4]; A.L[2] = cell->h[8];
    A.s2 = -coeff * 1.4426950408889634f;
    A.h = nbins > 1 ? spacing : 0.f;
    A.inv_h = nbins > 1 ? 1.f / spacing : 0.f;
    A.q = exp2f(-2.f * A.s2 * A.h * A.h);
    A.reach = ADF_REACH / sqrtf(A.s2);
    A.reach_b = nbins > 1 ? A.reach / fabsf(spacing) : 0.f;
    return MDG_OK;
}

}  // namespace

extern "C" int64_t mdg_adf_partial_size(int n_frames, int n_atoms, int max_nbr, int nbins) {
    (void)n_frames; (void)n_atoms; (void)max_nbr;
    return (int64_t)nbins + 2;          // one int64 word per bin, then the flag word (and one spare, 16-byte multiple)
}

extern "C" int mdg_adf_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, float cutoff, const int32_t* col,
                           const int32_t* cnt, int max_nbr, const float* mu, float spacing, float coeff, int nbins, float* raw,
                           int64_t* scratch, void* stream) {
    AdfArgs A;
    const int rc = adf_args(A, pos, n_frames, n_atoms, cell, cutoff, col, cnt, max_nbr, mu, spacing, coeff, nbins);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(raw && scratch, "adf_fwd: null output or scratch");
    hipStream_t st = (hipStream_t)stream;
    const double n_contrib = (double)A.n_total * (double)max_nbr * (double)(max_nbr - 1) * 0.5;
    const float scale = 0.5f * fx64_limit(n_contrib);            // contributions <= 2: 2 S = the per-contribution limit
    MDG_HIP(hipMemsetAsync(scratch, 0, sizeof(int64_t) * mdg_adf_partial_size(n_frames, n_atoms, max_nbr, nbins), st));
    const long long blocks = (A.n_total + ADF_BLOCK - 1) / ADF_BLOCK;
    const int grid = (int)(blocks < ADF_MAX_BLOCKS ? blocks : ADF_MAX_BLOCKS);
    const size_t lds = (size_t)nbins * (sizeof(unsigned long long) + sizeof(float));
    hipLaunchKernelGGL(adf_fwd_kernel<false>, dim3(grid), dim3(ADF_BLOCK), lds, st, A, scale,
                       reinterpret_cast<unsigned long long*>(scratch), n_atoms, 0.0, (float*)nullptr);
    MDG_CHECK_LAUNCH("adf_fwd_kernel");
    hipLaunchKernelGGL(adf_finish_kernel, dim3((nbins + 255) / 256), dim3(256), 0, st,
                       reinterpret_cast<const unsigned long long*>(scratch), nbins, 1.0 / (double)scale, raw);
    MDG_CHECK_LAUNCH("adf_finish_kernel");
    return MDG_OK;
}

extern "C" int mdg_adf_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, float cutoff, const int32_t* col,
                           const int32_t* cnt, int max_nbr, const float* mu, float spacing, float coeff, int nbins,
                           const float* g_raw, float* g_xyz, void* stream) {
    AdfArgs A;
    const int rc = adf_args(A, pos, n_frames, n_atoms, cell, cutoff, col, cnt, max_nbr, mu, spacing, coeff, nbins);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(g_raw && g_xyz, "adf_bwd: null g_raw or g_xyz");
    const long long blocks = (A.n_total + ADF_BLOCK - 1) / ADF_BLOCK;
    hipLaunchKernelGGL(adf_bwd_kernel<false>, dim3((unsigned)blocks), dim3(ADF_BLOCK), (size_t)nbins * 2 * sizeof(float),
                       (hipStream_t)stream, A, g_raw, g_xyz, n_atoms);
    MDG_CHECK_LAUNCH("adf_bwd_kernel");
    return MDG_OK;
}

// ---------------------------------------------------------------------------------- K35: the rows of the sum above
// raw [n_frames, nbins]: the histogram of every frame on its own.  The fixed-point scale comes from the triplet bound of ONE
// frame, n_atoms max_nbr (max_nbr - 1) / 2, so no word of a frame's LDS histogram can leave int64.
extern "C" int mdg_adf_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, float cutoff, const int32_t* col,
                                  const int32_t* cnt, int max_nbr, const float* mu, float spacing, float coeff, int nbins,
                                  float* raw, void* stream) {
    AdfArgs A;
    const int rc = adf_args(A, pos, n_frames, n_atoms, cell, cutoff, col, cnt, max_nbr, mu, spacing, coeff, nbins);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(raw, "adf_frames_fwd: null output");
    const double n_contrib = (double)n_atoms * (double)max_nbr * (double)(max_nbr - 1) * 0.5;
    const float scale = 0.5f * fx64_limit(n_contrib);
    const size_t lds = (size_t)nbins * (sizeof(unsigned long long) + sizeof(float));
    hipLaunchKernelGGL(adf_fwd_kernel<true>, dim3(n_frames), dim3(ADF_BLOCK), lds, (hipStream_t)stream, A, scale,
                       (unsigned long long*)nullptr, n_atoms, 1.0 / (double)scale, raw);
    MDG_CHECK_LAUNCH("adf_frames_fwd_kernel");
    return MDG_OK;
}

// g_xyz [n_frames * n_atoms, 3] = d(sum_fb g_raw[f, b] raw[f, b]) / d pos, g_raw [n_frames, nbins]
extern "C" int mdg_adf_frames_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, float cutoff, const int32_t* col,
                                  const int32_t* cnt, int max_nbr, const float* mu, float spacing, float coeff, int nbins,
                                  const float* g_raw, float* g_xyz, void* stream) {
    AdfArgs A;
    const int rc = adf_args(A, pos, n_frames, n_atoms, cell, cutoff, col, cnt, max_nbr, mu, spacing, coeff, nbins);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(g_raw && g_xyz, "adf_frames_bwd: null g_raw or g_xyz");
    hipLaunchKernelGGL(adf_bwd_kernel<true>, dim3(n_frames, (n_atoms + ADF_BLOCK - 1) / ADF_BLOCK), dim3(ADF_BLOCK),
                       (size_t)nbins * 2 * sizeof(float), (hipStream_t)stream, A, g_raw, g_xyz, n_atoms);
    MDG_CHECK_LAUNCH("adf_frames_bwd_kernel");
    return MDG_OK;
}
