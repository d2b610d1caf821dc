// K31: pair potential energy of every frame of a trajectory, and its gradient -- thermo.PotentialEnergy, the energy side of
// trajectory reweighting (mdgrad_amd/reweight.py; Thaler and Zavadlav, DiffTRe, 2021) and the per-frame thermodynamic
// observable (cohesive energy, heat capacity from its fluctuation).
//
//   U[f] = sum_terms sum_pairs phi(r)           the plain truncated phi (no shift): the value PairPotentials gives for frame f
//
// The sweeps are those of csrc/frame_pairs.hpp (pair set, the three shapes by frame size, fixed-order sums, no floating-point
// atomics); this file names what a visit adds:
//   forward                 phi(r), every unordered pair once, pair_eval level 0
//   backward, positions     dU/dx_i = -sum_j phi'(r) D / r (D = x_j - x_i), full rows, level 1; dU/dtheta = sum_pairs dphi/dtheta
//                           takes half of each visit; every frame scaled by its gU[f]
//   backward, parameters    (g_pos == nullptr: the reweighting case, frames detached) the forward's once-per-pair sweep at
//                           level 1, accumulating gU[f] dphi/dtheta only -- half the pair visits, no position written
#include "frame_pairs.hpp"

namespace {

using namespace frame_pairs;

struct EnergyVisit {
    static constexpr int FWD_LEVEL = 0, BWD_LEVEL = 1;
    static constexpr float SIGN = 1.f;
    static __device__ __forceinline__ float value(const PairOut& o, float, float acc) { return acc + o.u; }
    static __device__ __forceinline__ float radial(const PairOut& o, float, float ir) { return -o.du * ir; }
    static __device__ __forceinline__ float dtheta(const PairOut& o, float, int k, float acc) { return acc + o.du_dth[k]; }
};

}  // namespace

extern "C" int64_t mdg_energy_frames_workspace(int n_frames, int n_atoms, int n_theta_total) {
    return frame_pairs::workspace(n_frames, n_atoms, n_theta_total, FP_THETA);
}

extern "C" int mdg_energy_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const MdgTerms* terms,
                                     const float* theta, float* U, float* workspace, void* stream) {
    FpArgs A;
    const int rc = make_args("energy_frames", A, pos, n_frames, n_atoms, cell, terms, theta);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(U && workspace, "energy_frames_fwd: null output or workspace");
    A.out = U; A.partial = workspace;
    return launch_value<EnergyVisit>("energy_frames_fwd", A, (hipStream_t)stream);
}

extern "C" int mdg_energy_frames_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const MdgTerms* terms,
                                     const float* theta, const float* gU, float* g_pos, float* g_theta, float* workspace,
                                     void* stream) {
    FpArgs A;
    const int rc = make_args("energy_frames", A, pos, n_frames, n_atoms, cell, terms, theta);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(gU && workspace, "energy_frames_bwd: null gU or workspace");
    MDG_CHECK_ARG(g_pos || g_theta, "energy_frames_bwd: g_pos and g_theta are both null (nothing to compute)");
    MDG_CHECK_ARG(g_pos || A.K > 0, "energy_frames_bwd: g_theta without parameters (the terms hold none)");
    A.g = gU; A.g_pos = g_pos; A.partial = workspace;
    return g_pos ? launch_grad<EnergyVisit, FP_ROWS>("energy_frames_bwd", A, g_theta, (hipStream_t)stream)
                 : launch_grad<EnergyVisit, FP_THETA>("energy_frames_bwd", A, g_theta, (hipStream_t)stream);
}
