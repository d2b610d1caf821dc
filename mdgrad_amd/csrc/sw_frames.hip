// K34: Stillinger-Weber energy of every frame of a trajectory, list-free -- thermo.StillingerWeberEnergy, the energy side of
// trajectory reweighting (mdgrad_amd/reweight.py) for the one-species three-body model of csrc/sw.hip (K23).
//
//   U[f]         = 1/2 sum_i sum_j phi2(r_ij) + sum_i sum_{j<k} phi3(j, i, k)       exactly K23's definition and formulas
//   dU_dtheta[f] = dU[f] / d(eps, sigma, lam)                                        from the same pass, when asked for
//
// over the neighbours of i in its own frame: D = x_j - x_i re-imaged with the strict minimum image on the diagonal cell
// (csrc/frame_pairs.hpp), r = sqrtf(d2) with the un-contracted d2, 0 < r < a sigma with the LIVE device sigma.  Nothing is
// searched on the host and no list exists: a step of sigma costs nothing, and the value is the one StillingerWeber gives
// for the frame.
//
// Shape: the frame's positions are staged in LDS (a wave per frame up to 128 atoms, four frames per workgroup; a workgroup
// per frame up to 1024 atoms); every thread owns the atoms t, t + TPF, ... and, for each of them,
//   1. walks the frame once and writes the indices of the atoms inside the support into ITS OWN compact row in LDS (uint16,
//      slot-major: lane-consecutive, no bank conflict) -- every lane does the same N - 1 tests;
//   2. walks that row: the pair (i, j) for every slot, the triplet (j, i, k) for every later slot, edges by sw_edge().
// The row belongs to one thread from the first step to the second, so no barrier separates them.
// Row cap: SWF_ROW_CAP = 64 entries (32 KB of LDS for the 256 rows of a workgroup; silicon and mW water hold 4 - 30
// neighbours inside a sigma).  A row is never truncated silently: a frame in which any atom has more neighbours comes out NaN
// in U and dU_dtheta, alone.
//
// Every sum runs in a fixed order: per atom in slot order, per thread in atom order, then the shuffle / LDS trees of
// common.hpp.  No floating-point atomics; a frame's arithmetic does not depend on where it stands in the batch, so permuting
// the frames permutes the outputs bit for bit, and the value part does not depend on whether dU_dtheta is asked for (no
// fused multiply-add is formed in this file).
#include "sw_core.hpp"
#include "frame_pairs.hpp"

namespace {

using namespace frame_pairs;

constexpr int SWF_ROW_CAP = 64;

struct SwfArgs {
    const float* pos; const float* theta;
    float* U; float* dU;
    int F, N;
    MdgCell cell;
    float a, gamma, cos0, A, B; int p, q;
};

template <int TPF, bool DTH>
__global__ __launch_bounds__(FP_BLOCK) void sw_frames_kernel(const SwfArgs A) {
    constexpr int CAP = TPF == MDG_WAVE ? FP_WAVE_ATOMS : FP_GROUP_ATOMS, FPB = FP_BLOCK / TPF;
    static_assert(TPF == MDG_WAVE || TPF == FP_BLOCK, "a wave or the whole workgroup per frame");
    constexpr int NV = 5;                                     // U, dU/d(eps, sigma, lam), overflowing rows
    __shared__ float sp[FPB * 3 * CAP];
    __shared__ uint16_t rows[SWF_ROW_CAP * FP_BLOCK];
    __shared__ float red[(FP_BLOCK / MDG_WAVE) * NV];
    const int t = threadIdx.x % TPF, g = threadIdx.x / TPF, N = A.N;
    const long long f = (long long)blockIdx.x * FPB + g;
    const bool live = f < A.F;
    float* sf = sp + g * 3 * CAP;
    if (live) stage_frame<TPF, CAP>(sf, A.pos + (size_t)f * N * 3, N, t);
    __syncthreads();
    const SwK K = sw_constants(A.theta[0], A.theta[1], A.theta[2], A.a, A.gamma, A.cos0, A.A, A.B, A.p, A.q);
    const float *sx = sf, *sy = sf + CAP, *sz = sf + 2 * CAP;
    uint16_t* row = rows + threadIdx.x;                       // slot s of this thread's row: row[s * FP_BLOCK]
    const float inf = __int_as_float(0x7f800000);
    float v[NV] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
        for (int i = t; i < N; i += TPF) {
            const float xi = sx[i], yi = sy[i], zi = sz[i];
            // ---- 1. the row of atom i
            int n = 0, over = 0;
            for (int j = 0; j < N; ++j) {
                float dx = sx[j] - xi, dy = sy[j] - yi, dz = sz[j] - zi, d2;
                if (j == i || !pair_in(A.cell, inf, dx, dy, dz, d2)) continue;
                const float rv = sqrtf(d2);
                if (!(rv > 0.f && rv < K.rc)) continue;       // sw_edge's support test
                if (n < SWF_ROW_CAP) row[(n++) * FP_BLOCK] = (uint16_t)j;
                else over = 1;
            }
            if (over) { v[4] += 1.f; continue; }
            // ---- 2. pairs and triplets of the row
            float S2 = 0.f, S2s = 0.f, S3 = 0.f, S3s = 0.f;
            for (int s = 0; s < n; ++s) {
                const int j = row[s * FP_BLOCK];
                float dx = sx[j] - xi, dy = sy[j] - yi, dz = sz[j] - zi;
                min_image<true>(A.cell, dx, dy, dz);
                SwEdge<float> ej;
                if (!sw_edge<float>(K, dx, dy, dz, 0.f, 0.f, 0.f, ej)) continue;
                const SwPair<float> pr = sw_pair<float>(K, ej);
                S2 = S2 + pr.e2;
                if (DTH) S2s = S2s + sw_pair_dsigma<float>(K, ej, pr);
                const float q1 = ej.inv * ej.inv;
                for (int u = s + 1; u < n; ++u) {
                    const int k = row[u * FP_BLOCK];
                    float bx = sx[k] - xi, by = sy[k] - yi, bz = sz[k] - zi;
                    min_image<true>(A.cell, bx, by, bz);
                    SwEdge<float> ek;
                    if (!sw_edge<float>(K, bx, by, bz, 0.f, 0.f, 0.f, ek)) continue;
                    const float c = ej.ex * ek.ex + ej.ey * ek.ey + ej.ez * ek.ez;
                    const float dc = c - K.cos0;
                    const float gg = ej.g * ek.g;
                    const float t3 = dc * dc * gg;
                    S3 = S3 + t3;
                    if (DTH) S3s = S3s + K.gamma * (t3 * (ej.r * q1 + ek.r * (ek.inv * ek.inv)));
                }
            }
            // u_i = eps (S2 / 2 + lam S3) and its parameter derivatives (sw_atom's pe, psg, pl)
            const float pe = 0.5f * S2 + K.lam * S3;
            v[0] += K.eps * pe;
            if (DTH) {
                v[1] += pe;
                v[2] += K.eps * (0.5f * S2s + K.lam * S3s);
                v[3] += K.eps * S3;
            }
        }
    }
    if constexpr (TPF == MDG_WAVE) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
    } else {
        block_sum_n<NV>(v, red);
    }
    if (live && t == 0) {
        const float nan = __int_as_float(0x7fc00000);
        const bool bad = v[4] > 0.f;
        A.U[f] = bad ? nan : v[0];
        if (DTH) {
#pragma unroll
            for (int k = 0; k < 3; ++k) A.dU[3 * f + k] = bad ? nan : v[1 + k];
        }
    }
}

// g_theta[k] = sum_f gU[f] dU[f, k]: a workgroup per parameter, fixed order.  The products of a reweighting gradient cancel
// (gU sums to zero over the frames), so the sum runs in double: 3 F multiply-adds in all.
__global__ __launch_bounds__(FP_BLOCK) void sw_frames_reduce_kernel(const float* __restrict__ gU, const float* __restrict__ dU,
                                                                    long long F, float* __restrict__ g_theta) {
    __shared__ double red[FP_BLOCK];
    const int k = blockIdx.x;
    double s = 0.0;
    for (long long f = threadIdx.x; f < F; f += FP_BLOCK) s = s + (double)gU[f] * (double)dU[3 * f + k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = FP_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) g_theta[k] = (float)red[0];
}

}  // namespace

extern "C" int mdg_sw_frames_row_cap(void) { return SWF_ROW_CAP; }

extern "C" int mdg_sw_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const MdgSWConsts* k,
                                 const float* theta, float* U, float* dU_dtheta, void* stream) {
    const int rc = check_frames("sw_frames_fwd", pos, cell, k, n_frames, n_atoms, FP_GROUP_ATOMS);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(theta, "sw_frames_fwd: theta is null (the device buffer (epsilon, sigma, lam) is required)");
    MDG_CHECK_ARG(U, "sw_frames_fwd: null output U");
    MDG_CHECK_ARG(k->a > 0.0 && k->gamma >= 0.0, "sw_frames_fwd: consts need a > 0 and gamma >= 0");
    MDG_CHECK_ARG(k->q >= 0 && k->q < k->p && k->p <= 12, "sw_frames_fwd: exponents need 0 <= q < p <= 12");
    SwfArgs A{pos, theta, U, dU_dtheta, n_frames, n_atoms, *cell,
              (float)k->a, (float)k->gamma, (float)k->cos0, (float)k->A, (float)k->B, (int)k->p, (int)k->q};
    hipStream_t st = (hipStream_t)stream;
    if (n_atoms <= FP_WAVE_ATOMS) {
        constexpr int FPB = FP_BLOCK / MDG_WAVE;
        const dim3 grid((n_frames + FPB - 1) / FPB);
        if (dU_dtheta) hipLaunchKernelGGL((sw_frames_kernel<MDG_WAVE, true>), grid, dim3(FP_BLOCK), 0, st, A);
        else hipLaunchKernelGGL((sw_frames_kernel<MDG_WAVE, false>), grid, dim3(FP_BLOCK), 0, st, A);
    } else {
        if (dU_dtheta) hipLaunchKernelGGL((sw_frames_kernel<FP_BLOCK, true>), dim3(n_frames), dim3(FP_BLOCK), 0, st, A);
        else hipLaunchKernelGGL((sw_frames_kernel<FP_BLOCK, false>), dim3(n_frames), dim3(FP_BLOCK), 0, st, A);
    }
    MDG_CHECK_LAUNCH("sw_frames_kernel");
    return MDG_OK;
}

extern "C" int mdg_sw_frames_theta_bwd(const float* gU, const float* dU_dtheta, int n_frames, float* g_theta, void* stream) {
    MDG_CHECK_ARG(gU && dU_dtheta && g_theta, "sw_frames_theta_bwd: null argument");
    MDG_CHECK_ARG(n_frames > 0, "sw_frames_theta_bwd: empty trajectory");
    hipLaunchKernelGGL(sw_frames_reduce_kernel, dim3(3), dim3(FP_BLOCK), 0, (hipStream_t)stream, gU, dU_dtheta,
                       (long long)n_frames, g_theta);
    MDG_CHECK_LAUNCH("sw_frames_reduce_kernel");
    return MDG_OK;
}
