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
// Shape: the scaffold of csrc/frame_atoms.hpp.  Every thread, for each of its atoms,
//   1. builds the row of the atoms inside the support (build_row) -- every lane does the same N - 1 tests;
//   2. walks that row: the pair (i, j) for every slot, the triplet (j, i, k) for every later slot, edges by sw_edge() and pair
//      terms by sw_pair() of csrc/sw_core.hpp on one pair entry (eps, sigma, a sigma, gamma sigma, ...) built from theta.
// Row cap: SWF_ROW_CAP = 64 entries (32 KB of LDS for the 256 rows of a workgroup; silicon and mW water hold 4 - 30
// neighbours inside a sigma); a frame in which any atom has more neighbours comes out NaN in U and dU_dtheta, alone.
//
// Every sum runs in a fixed order: per atom in slot order, per thread in atom order, then the shuffle / LDS trees of
// common.hpp.  No floating-point atomics; a frame's arithmetic does not depend on where it stands in the batch, so permuting
// the frames permutes the outputs bit for bit, and the value part does not depend on whether dU_dtheta is asked for (no
// fused multiply-add is formed in this file).
#include "sw_core.hpp"
#include "frame_atoms.hpp"

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
    using C = FrameCtx<TPF>;
    constexpr int NV = 5;                                     // U, dU/d(eps, sigma, lam), overflowing rows
    __shared__ float sp[C::FPB * 3 * C::CAP];
    __shared__ uint16_t rows[SWF_ROW_CAP * FP_BLOCK];
    __shared__ float red[(FP_BLOCK / MDG_WAVE) * NV];
    const C fr = open_frame<TPF>(sp, A.pos, A.F, A.N);
    // the one pair entry, from the live (eps, sigma, lam) as csrc/sw.hip derives it
    const float eps = A.theta[0], sigma = A.theta[1], lam = A.theta[2];
    const SwPairE P{eps, sigma, A.a * sigma, A.gamma * sigma, A.gamma, A.A, A.B, (float)A.p, (float)A.q, A.a, eps * A.A, 0.f};
    const float *sx = fr.sx, *sy = fr.sy, *sz = fr.sz;
    uint16_t* row = rows + threadIdx.x;
    float v[NV] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (fr.live) {
        for (int i = fr.t; i < fr.N; i += TPF) {
            const float xi = sx[i], yi = sy[i], zi = sz[i];
            // ---- 1. the row of atom i (sw_edge's support test)
            int over;
            const int n = build_row<SWF_ROW_CAP, C::CAP>(row, A.cell, fr.sf, fr.N, i, over,
                                                         [&](int, float rv) { return rv < P.rc; });
            if (over) { v[4] += 1.f; continue; }
            // ---- 2. pairs and triplets of the row
            float S2 = 0.f, S2s = 0.f, S3 = 0.f, S3s = 0.f;
            for (int s = 0; s < n; ++s) {
                const int j = row_at(row, s);
                float dx = sx[j] - xi, dy = sy[j] - yi, dz = sz[j] - zi;
                min_image<true>(A.cell, dx, dy, dz);
                SwEdge<float> ej;
                if (!sw_edge<float>(P, dx, dy, dz, 0.f, 0.f, 0.f, ej)) continue;
                float e2, e2s = 0.f, du = 0.f;                           // (du: the force, not needed here)
                sw_pair<float, DTH ? 1 : 0>(P, A.p, A.q, ej, e2, e2s, du);
                S2 = S2 + e2;
                if (DTH) S2s = S2s + e2s;
                const float q1 = ej.inv * ej.inv;
                for (int u = s + 1; u < n; ++u) {
                    const int k = row_at(row, u);
                    float bx = sx[k] - xi, by = sy[k] - yi, bz = sz[k] - zi;
                    min_image<true>(A.cell, bx, by, bz);
                    SwEdge<float> ek;
                    if (!sw_edge<float>(P, bx, by, bz, 0.f, 0.f, 0.f, ek)) continue;
                    const float c = ej.ex * ek.ex + ej.ey * ek.ey + ej.ez * ek.ez;
                    const float dc = c - A.cos0;
                    const float gg = ej.g * ek.g;
                    const float t3 = dc * dc * gg;
                    S3 = S3 + t3;
                    if (DTH) S3s = S3s + P.gamma * (t3 * (ej.r * q1 + ek.r * (ek.inv * ek.inv)));
                }
            }
            // u_i = eps (S2 / 2 + lam S3) and its parameter derivatives (this kernel's own sum: K23 / K28 add u_i term by term)
            const float pe = 0.5f * S2 + lam * S3;
            v[0] += eps * pe;
            if (DTH) {
                v[1] += pe;
                v[2] += eps * (0.5f * S2s + lam * S3s);
                v[3] += eps * S3;
            }
        }
    }
    if (frame_sums(fr, v, red)) {
        const bool bad = v[4] > 0.f;
        A.U[fr.f] = nan_if(bad, v[0]);
        if (DTH) {
#pragma unroll
            for (int k = 0; k < 3; ++k) A.dU[3 * fr.f + k] = nan_if(bad, v[1 + k]);
        }
    }
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
    launch_frames(n_frames, n_atoms, dU_dtheta != nullptr, [&](auto tpf, auto dth, dim3 grid) {
        hipLaunchKernelGGL((sw_frames_kernel<decltype(tpf)::value, decltype(dth)::value>), grid, dim3(FP_BLOCK), 0,
                           (hipStream_t)stream, A);
    });
    MDG_CHECK_LAUNCH("sw_frames_kernel");
    return MDG_OK;
}
