// The parameter part of a frame energy's backward pass (K34, K37, K38): g_theta[k] = sum_f gU[f] dU_dtheta[f, k] over the
// dU_dtheta [F, P] that the forward launch of csrc/sw_frames.hip, csrc/eam_frames.hip or csrc/tersoff_frames.hip emitted.
// A workgroup per parameter, fixed order: the strided sums per thread, then one LDS tree.  The products of a reweighting
// gradient cancel (gU sums to zero over the frames), so the sum runs in double: P F multiply-adds in all.
#include "frame_pairs.hpp"

namespace {

using namespace frame_pairs;

__global__ __launch_bounds__(FP_BLOCK) void frames_theta_reduce_kernel(const float* __restrict__ gU, const float* __restrict__ dU,
                                                                       long long F, int P, float* __restrict__ g_theta) {
    __shared__ double red[FP_BLOCK];
    const int k = blockIdx.x;
    double s = 0.0;
    for (long long f = threadIdx.x; f < F; f += FP_BLOCK) s = s + (double)gU[f] * (double)dU[(size_t)f * P + k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = FP_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) g_theta[k] = (float)red[0];
}

int reduce(const float* gU, const float* dU, int n_frames, int n_params, float* g_theta, void* stream) {
    hipLaunchKernelGGL(frames_theta_reduce_kernel, dim3(n_params), dim3(FP_BLOCK), 0, (hipStream_t)stream, gU, dU,
                       (long long)n_frames, n_params, g_theta);
    MDG_CHECK_LAUNCH("frames_theta_reduce_kernel");
    return MDG_OK;
}

}  // namespace

extern "C" int mdg_frames_theta_bwd(const float* gU, const float* dU_dtheta, int n_frames, int n_params, float* g_theta,
                                    void* stream) {
    MDG_CHECK_ARG(gU && dU_dtheta && g_theta, "frames_theta_bwd: null argument");
    MDG_CHECK_ARG(n_frames > 0, "frames_theta_bwd: empty trajectory");
    MDG_CHECK_ARG(n_params > 0, "frames_theta_bwd: n_params must be positive (got %d)", n_params);
    return reduce(gU, dU_dtheta, n_frames, n_params, g_theta, stream);
}

// K34's entry point: mdg_frames_theta_bwd with n_params = 3, under its own name in the messages
extern "C" int mdg_sw_frames_theta_bwd(const float* gU, const float* dU_dtheta, int n_frames, float* g_theta, void* stream) {
    MDG_CHECK_ARG(gU && dU_dtheta && g_theta, "sw_frames_theta_bwd: null argument");
    MDG_CHECK_ARG(n_frames > 0, "sw_frames_theta_bwd: empty trajectory");
    return reduce(gU, dU_dtheta, n_frames, 3, g_theta, stream);
}
