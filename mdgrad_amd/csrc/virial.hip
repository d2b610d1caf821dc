// K15: pair virial of every frame of a trajectory, and its gradient -- the configurational part of the pressure observable
// (mdgrad_amd/thermo.py Pressure; the reference's torchmd/thermo.py:17-54 does not run).
//
//   W[f] = - sum_terms sum_pairs r phi'(r)            P = (sum_i m_i |v_i|^2 + W) / (dim V)
//
// List-free: the headline shape is 10^5-10^6 frames of ~100 atoms, where a neighbour list over 10^8 atoms costs more than
// the all-pairs sweep, and at a few thousand atoms the sweep with its early distance test is still a few milliseconds for
// hundreds of frames.  The sweeps are those of csrc/frame_pairs.hpp (pair set, the three shapes by frame size, fixed-order
// sums, no floating-point atomics); this file names what a visit adds:
//   forward      r phi'(r), every unordered pair once, pair_eval level 1
//   backward     full rows at level 2 -- each pair is evaluated from both ends, the parameter gradient takes half of each visit:
//                dW/dx_i = sum_j (phi' + r phi'') D / r  (D = x_j - x_i)          dW/dtheta = - sum_pairs r dphi'/dtheta
//                every frame scaled by its gW[f].  There is no parameters-only route: the pressure is differentiated through
//                the positions of a trajectory.
#include "frame_pairs.hpp"

namespace {

using namespace frame_pairs;

struct VirialVisit {
    static constexpr int FWD_LEVEL = 1, BWD_LEVEL = 2;
    static constexpr float SIGN = -1.f;
    static __device__ __forceinline__ float value(const PairOut& o, float r, float acc) { return fmaf(r, o.du, acc); }
    static __device__ __forceinline__ float radial(const PairOut& o, float r, float ir) { return fmaf(r, o.d2u, o.du) * ir; }
    static __device__ __forceinline__ float dtheta(const PairOut& o, float r, int k, float acc) { return fmaf(r, o.ddu_dth[k], acc); }
};

}  // namespace

// (the backward's parameter partials are those of the full-row sweep: a row per frame, tiled a row per i-block)
extern "C" int64_t mdg_virial_workspace(int n_frames, int n_atoms, int n_theta_total) {
    return frame_pairs::workspace(n_frames, n_atoms, n_theta_total, FP_ROWS);
}

extern "C" int mdg_virial_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const MdgTerms* terms,
                              const float* theta, float* W, float* workspace, void* stream) {
    FpArgs A;
    const int rc = make_args("virial", A, pos, n_frames, n_atoms, cell, terms, theta);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(W && workspace, "virial_fwd: null output or workspace");
    A.out = W; A.partial = workspace;
    return launch_value<VirialVisit>("virial_fwd", A, (hipStream_t)stream);
}

extern "C" int mdg_virial_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const MdgTerms* terms,
                              const float* theta, const float* gW, float* g_pos, float* g_theta, float* workspace, void* stream) {
    FpArgs A;
    const int rc = make_args("virial", A, pos, n_frames, n_atoms, cell, terms, theta);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(gW && g_pos && workspace, "virial_bwd: null gW, g_pos or workspace");
    MDG_CHECK_ARG(A.K == 0 || g_theta, "virial_bwd: g_theta is null");
    A.g = gW; A.g_pos = g_pos; A.partial = workspace;
    return launch_grad<VirialVisit, FP_ROWS>("virial_bwd", A, g_theta, (hipStream_t)stream);
}
