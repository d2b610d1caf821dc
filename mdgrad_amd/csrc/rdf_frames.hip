// K32: the smeared pair count of EVERY frame (observable.rdf.per_frame), and its gradient -- the rows a weighted average over
// frames needs (mdgrad_amd/reweight.py); csrc/rdf.hip returns only their sum.
//
//   raw[f, k] = sum_{i<j, 0<d<cutoff} exp(coeff (d - mu_k)^2)        mu_k = mu_0 + k h  (linspace centres, h = spacing)
//
// Pair set (strict +-1/2 minimum image on the diagonal cell, 0 < d^2 < cutoff^2 with the un-contracted d^2, the observable's
// [N, N] selection mask), the staging of a frame in LDS and the walk over a row's partners are those of csrc/frame_pairs.hpp, in
// its two whole-frame shapes: one frame per wave (N <= 128, four frames per workgroup) or per workgroup (N <= 1024).  This file
// holds what a visit does with d = sqrt(d^2): the window, the exp2f terms and the fixed-point histogram.
//
// Reach: only the 2R + 1 centres around the nearest one, kc = rint((d - mu_0) / h), are summed, R = ceil(5.3 / (s h)) with
// s = sqrt(-coeff log2 e), so exp(coeff x^2) = exp2(-(s x)^2): a dropped term is <= exp2(-5.3^2) = 2^-28.1 of a peak term (the
// bound of csrc/adf.hip and of the RDF list kernels).
//
// Forward determinism (the idiom of csrc/adf.hip): every contribution is a fixed-point integer (fx64, common.hpp) added into the
// LDS histogram of its frame -- integer sums do not depend on the order, so two launches are bitwise equal.  Every contribution
// is <= 1 and a word receives at most N (N - 1) / 2 of them: scale = fx64_limit(N (N - 1) / 2), no word can leave int64.  A frame
// belongs to one wave or workgroup, which converts and writes its row: no global atomics at all.
//
// Backward: g_xyz[f, i] = d(sum_k g_raw[f, k] raw[f, k]) / dx_i, atom-centric full rows with the frame's g_raw row in LDS:
//   dL/dd = sum_k g_raw[f, k] 2 coeff (d - mu_k) e_k  over the window,      g_x_i = -sum_j (dL/dd) D / d
// summed per thread in a fixed order, no atomics.  A frame whose upstream row is all zero gets exact zeros.
#include <math.h>
#include "frame_pairs.hpp"

namespace {

using namespace frame_pairs;

constexpr int RF_MAX_BINS = 1024;
constexpr float RF_REACH = 5.3f;

struct RfArgs {
    const float* pos;        // [F, N, 3]
    const uint8_t* mask;     // [N, N] or null
    const float* mu;         // [nbins]
    const float* g_raw;      // backward: [F, nbins]
    float* raw;              // forward:  [F, nbins]
    float* g_xyz;            // backward: [F, N, 3]
    int F, N, nbins, R;
    float rc2, s2, coeff2;   // cutoff^2, s^2 = -coeff log2 e, 2 coeff
    float inv_h;             // 1 / spacing
    float scale;             // fixed-point scale of the forward
    double inv_scale;
    MdgCell cell;
};

// the window [lo, hi] of centres summed for a pair at distance d (empty when lo > hi)
__device__ __forceinline__ void rf_window(const RfArgs& A, float mu0, float d, int& lo, int& hi) {
    const float t = fminf(fmaxf((d - mu0) * A.inv_h, -1.0e9f), 1.0e9f);
    const int kc = (int)rintf(t);
    lo = max(kc - A.R, 0);
    hi = min(kc + A.R, A.nbins - 1);
}

template <int TPF>
__global__ __launch_bounds__(FP_BLOCK) void rdf_frames_fwd_kernel(const RfArgs A) {
    constexpr int CAP = TPF == MDG_WAVE ? FP_WAVE_ATOMS : FP_GROUP_ATOMS, FPB = FP_BLOCK / TPF;
    __shared__ float sp[FPB * 3 * CAP];
    extern __shared__ __attribute__((aligned(16))) unsigned long long rf_dyn[];       // [FPB, nbins] words, then mu [nbins]
    float* mu_s = reinterpret_cast<float*>(rf_dyn + (size_t)FPB * A.nbins);
    const int t = threadIdx.x % TPF, g = threadIdx.x / TPF, N = A.N, B = A.nbins;
    const long long f = (long long)blockIdx.x * FPB + g;
    const bool live = f < A.F;
    unsigned long long* hist = rf_dyn + (size_t)g * B;
    for (int b = threadIdx.x; b < FPB * B; b += FP_BLOCK) rf_dyn[b] = 0ull;
    for (int b = threadIdx.x; b < B; b += FP_BLOCK) mu_s[b] = A.mu[b];
    float* sf = sp + g * 3 * CAP;
    if (live) stage_frame<TPF, CAP>(sf, A.pos + (size_t)f * N * 3, N, t);
    __syncthreads();
    if (live) {
        const float mu0 = mu_s[0];
        // every unordered pair once
        for (int i = t; i < N; i += TPF)
            walk_row<CAP>(A.cell, A.rc2, A.mask, sf, N, i, once_partners(N, i), [&](float, float, float, float d2) {
                const float d = sqrtf(d2);
                int lo, hi;
                rf_window(A, mu0, d, lo, hi);
                for (int b = lo; b <= hi; ++b) {
                    const float x = d - mu_s[b];
                    atomicAdd(&hist[b], fx64(A.scale * exp2f(-A.s2 * x * x)));
                }
            });
    }
    __syncthreads();
    if (live)
        for (int b = t; b < B; b += TPF) A.raw[(size_t)f * B + b] = (float)((double)(long long)hist[b] * A.inv_scale);
}

template <int TPF>
__global__ __launch_bounds__(FP_BLOCK) void rdf_frames_bwd_kernel(const RfArgs A) {
    constexpr int CAP = TPF == MDG_WAVE ? FP_WAVE_ATOMS : FP_GROUP_ATOMS, FPB = FP_BLOCK / TPF;
    __shared__ float sp[FPB * 3 * CAP];
    extern __shared__ __attribute__((aligned(16))) float rf_dynf[];                   // g_raw rows [FPB, nbins], then mu [nbins]
    float* mu_s = rf_dynf + (size_t)FPB * A.nbins;
    const int t = threadIdx.x % TPF, g = threadIdx.x / TPF, N = A.N, B = A.nbins;
    const long long f = (long long)blockIdx.x * FPB + g;
    const bool live = f < A.F;
    float* g_s = rf_dynf + (size_t)g * B;
    for (int b = threadIdx.x; b < B; b += FP_BLOCK) mu_s[b] = A.mu[b];
    if (live)
        for (int b = t; b < B; b += TPF) g_s[b] = A.g_raw[(size_t)f * B + b];
    float* sf = sp + g * 3 * CAP;
    if (live) stage_frame<TPF, CAP>(sf, A.pos + (size_t)f * N * 3, N, t);
    __syncthreads();
    if (!live) return;
    const float mu0 = mu_s[0];
    for (int i = t; i < N; i += TPF) {
        float gx = 0.f, gy = 0.f, gz = 0.f;
        walk_row<CAP>(A.cell, A.rc2, A.mask, sf, N, i, N - 1, [&](float dx, float dy, float dz, float d2) {
            const float d = sqrtf(d2);
            int lo, hi;
            rf_window(A, mu0, d, lo, hi);
            float acc = 0.f;
            for (int b = lo; b <= hi; ++b) {
                const float x = d - mu_s[b];
                acc = fmaf(g_s[b] * x, exp2f(-A.s2 * x * x), acc);
            }
            const float c = -(A.coeff2 * acc) / d;                  // -(dL/dd) / d
            gx = fmaf(c, dx, gx); gy = fmaf(c, dy, gy); gz = fmaf(c, dz, gz);
        });
        float* o = A.g_xyz + ((size_t)f * N + i) * 3;
        o[0] = gx; o[1] = gy; o[2] = gz;
    }
}

int rf_args(RfArgs& A, const float* pos, int n_frames, int n_atoms, const MdgCell* cell, float cutoff, const uint8_t* mask,
            const float* mu, float spacing, float coeff, int nbins) {
    const int rc = check_frames("rdf_frames", pos, cell, mu, n_frames, n_atoms, FP_GROUP_ATOMS);    // (no tiles)
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(cutoff > 0.f && isfinite(cutoff), "rdf_frames: cutoff must be positive");
    MDG_CHECK_ARG(nbins >= 2 && nbins <= RF_MAX_BINS, "rdf_frames: nbins must be in [2, %d], got %d", RF_MAX_BINS, nbins);
    MDG_CHECK_ARG(coeff < 0.f && isfinite(coeff), "rdf_frames: coeff must be finite and negative (width > 0), got %g", (double)coeff);
    MDG_CHECK_ARG(spacing > 0.f && isfinite(spacing), "rdf_frames: the centres must ascend with a finite spacing, got %g",
                  (double)spacing);
    A.pos = pos; A.mask = mask; A.mu = mu; A.g_raw = nullptr; A.raw = nullptr; A.g_xyz = nullptr;
    A.F = n_frames; A.N = n_atoms; A.nbins = nbins;
    A.rc2 = cutoff * cutoff;
    A.s2 = -coeff * 1.4426950408889634f;
    A.coeff2 = 2.f * coeff;
    A.inv_h = 1.f / spacing;
    const float rb = ceilf(RF_REACH / (sqrtf(A.s2) * spacing));
    A.R = rb < (float)nbins ? (int)rb : nbins;                   // (the window is clipped to the centres anyway)
    A.scale = fx64_limit(0.5 * (double)n_atoms * (double)(n_atoms - 1));
    A.inv_scale = 1.0 / (double)A.scale;
    A.cell = *cell;
    return MDG_OK;
}

template <class K64, class K256>
int rf_launch(const char* name, const RfArgs& A, size_t word, K64 k64, K256 k256, hipStream_t st) {
    if (A.N <= FP_WAVE_ATOMS) {
        constexpr int FPB = FP_BLOCK / MDG_WAVE;
        hipLaunchKernelGGL(k64, dim3((A.F + FPB - 1) / FPB), dim3(FP_BLOCK), (size_t)A.nbins * (FPB * word + sizeof(float)), st, A);
    } else {
        hipLaunchKernelGGL(k256, dim3(A.F), dim3(FP_BLOCK), (size_t)A.nbins * (word + sizeof(float)), st, A);
    }
    MDG_CHECK_LAUNCH(name);
    return MDG_OK;
}

}  // namespace

extern "C" int mdg_rdf_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, float cutoff,
                                  const uint8_t* mask, const float* mu, float spacing, float coeff, int nbins, float* raw,
                                  void* stream) {
    RfArgs A;
    const int rc = rf_args(A, pos, n_frames, n_atoms, cell, cutoff, mask, mu, spacing, coeff, nbins);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(raw, "rdf_frames_fwd: null output");
    A.raw = raw;
    return rf_launch("rdf_frames_fwd_kernel", A, sizeof(unsigned long long), rdf_frames_fwd_kernel<MDG_WAVE>,
                     rdf_frames_fwd_kernel<FP_BLOCK>, (hipStream_t)stream);
}

extern "C" int mdg_rdf_frames_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, float cutoff,
                                  const uint8_t* mask, const float* mu, float spacing, float coeff, int nbins, const float* g_raw,
                                  float* g_xyz, void* stream) {
    RfArgs A;
    const int rc = rf_args(A, pos, n_frames, n_atoms, cell, cutoff, mask, mu, spacing, coeff, nbins);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(g_raw && g_xyz, "rdf_frames_bwd: null g_raw or g_xyz");
    A.g_raw = g_raw; A.g_xyz = g_xyz;
    return rf_launch("rdf_frames_bwd_kernel", A, sizeof(float), rdf_frames_bwd_kernel<MDG_WAVE>, rdf_frames_bwd_kernel<FP_BLOCK>,
                     (hipStream_t)stream);
}
