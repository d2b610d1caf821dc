// K17: mean-squared displacement (and the fourth moment) of a trajectory over all lags, and its gradient
// (mdgrad_amd/observable.py msd; the reference has no MSD, the definition is this project's).
//
//   M_p[tau] = 1 / (|O_tau| sum_i w_i)  sum_{t0 in O_tau} sum_i w_i |x_i(t0 + tau) - x_i(t0)|^p        p = 2, 4
//   O_tau = {t0 = 0, s, 2 s, ... : t0 + tau < T}       |O_tau| = (T - 1 - tau) / s + 1        s = origin_stride
//
// x [n_batch][T][n_cols][3]; replica c / group of batch b owns output row b (n_cols / group) + c / group.  Positions are taken
// as given: no cell, no re-imaging.
//
// Forward.  Not one pass per lag (the vacf pattern of csrc/observe.hip): a workgroup owns MSD_TILE = 16 atoms of one replica
// and walks through time once.  A ring of the last n_lags - 1 + MSD_WINDOW frames of its atoms lives in LDS; per window of
// MSD_WINDOW = 16 new frames thread (atom a, lag class j) holds x_a(t) of the window in registers and takes every lag
// tau = j, j + 16, ... of every frame of the window from the ring, three LDS reads per term.  Every position is read from HBM
// exactly once whatever n_lags is.  The ring is [slot][component][atom] with an odd slot stride: lanes = atoms, conflict-free.
// Large n_lags shrink the atom tile (8, 4, 2, 1) so that ring + accumulators stay within 64 KiB.
//
// Order of the sums, the same in every launch (no floating-point read-modify-write to global memory by more than one thread;
// two launches give the same bits): per (atom, lag) over the origins in ascending order in float32 (chain depth |O_tau| <= T),
// the xor-shuffle tree over the tile's atoms, then msd_finish_kernel over the row's tiles in index order in double, which also
// applies 1 / (|O_tau| sum w).  Lag 0 subtracts a value from itself: M_p[0] is exactly 0.
//
// Backward.  One thread per (frame, atom) of a window of 256 / tile frames gathers over the lags from the same kind of ring,
// here 2 (n_lags - 1) + window frames long (it looks ahead as well as back):
//   gx_i(t) = w_i sum_tau [ (t - tau in O_tau) f(x_t - x_{t-tau}) - (t in O_tau, t + tau < T) f(x_{t+tau} - x_t) ]
//   f(d)    = c2_tau d + c4_tau |d|^2 d       c2 = 2 g2_tau / (|O_tau| sum w)      c4 = 4 g4_tau / (|O_tau| sum w)
// a sequential chain of 2 (n_lags - 1) terms per element; every gx element is written exactly once (the caller passes
// uninitialised memory), an atom of weight 0 gets exactly 0.
#include "common.hpp"

namespace {

constexpr int MSD_BLOCK = 256;
constexpr int MSD_TILE_SHIFT = 4;        // atom tile = 1 << shift = 16 at most
constexpr int MSD_WINDOW = 16;           // forward: new frames per step of the ring
constexpr int MSD_MAX_LAGS = 1024;
constexpr int MSD_LDS_BYTES = 65536;
constexpr int MSD_WS_HEAD = 2;           // workspace[0..1] = sum of the weights as hi + lo floats

struct MsdArgs {
    const float* x;          // [n_batch, T, C, 3]
    const float* w;          // [group] or null (unit weights)
    const float* g2;         // backward: [rows, L]
    const float* g4;         // backward: [rows, L] or null
    float* gx;               // backward: [n_batch, T, C, 3]
    float* ws;               // head, then forward partials [2][rows][L][tiles]
    int T, C, group, L, stride;
    int reps, tiles;         // C / group, ceil(group / tile)
    int sh;                  // atom tile = 1 << sh
    int ring;                // frames in the LDS ring
    long long rows;
};

__host__ __device__ inline int msd_slot_stride(int sh) { return (3 << sh) + 1; }
// LDS bytes of the forward (ring of L - 1 + window frames + one or two accumulators per (lag, atom)) and of the backward
// (ring of 2 (L - 1) + 256 / tile frames + two coefficients per lag)
inline long long msd_fwd_lds(int L, int sh, bool fourth) {
    return 4ll * ((long long)(L - 1 + MSD_WINDOW) * msd_slot_stride(sh) + (fourth ? 2ll : 1ll) * ((long long)L << sh));
}
inline long long msd_bwd_lds(int L, int sh) {
    return 4ll * ((long long)(2 * (L - 1) + (MSD_BLOCK >> sh)) * msd_slot_stride(sh) + 2ll * L);
}
// the largest atom tile whose LDS fits; -1: none
inline int msd_fwd_shift(int L, bool fourth) {
    for (int sh = MSD_TILE_SHIFT; sh >= 0; --sh) if (msd_fwd_lds(L, sh, fourth) <= MSD_LDS_BYTES) return sh;
    return -1;
}
inline int msd_bwd_shift(int L) {
    for (int sh = MSD_TILE_SHIFT; sh >= 0; --sh) if (msd_bwd_lds(L, sh) <= MSD_LDS_BYTES) return sh;
    return -1;
}

__device__ __forceinline__ double msd_origins(int T, int tau, int stride) { return (double)((T - 1 - tau) / stride + 1); }

// frames [f_lo, f_hi) of this tile into their ring slots as [slot][component][atom]; atoms beyond the replica's end read 0.
// f_hi - f_lo <= ring, slot_lo = f_lo % ring.
__device__ __forceinline__ void msd_stage(const MsdArgs& A, float* __restrict__ ring, const float* __restrict__ xt, int f_lo,
                                          int f_hi, int slot_lo, int n_valid) {
    const int TA = 1 << A.sh, FS = msd_slot_stride(A.sh), per = 3 << A.sh;
    const int n = (f_hi - f_lo) * per;
    for (int i = threadIdx.x; i < n; i += MSD_BLOCK) {
        const int fr = (i / 3) >> A.sh, e = i - fr * per, a = e / 3, c = e - 3 * a;
        int slot = slot_lo + fr;
        if (slot >= A.ring) slot -= A.ring;
        ring[slot * FS + c * TA + a] = a < n_valid ? xt[(size_t)(f_lo + fr) * A.C * 3 + e] : 0.f;
    }
}

// sum of the weights in double, fixed order, as hi + lo floats at ws[0..1] (one workgroup)
__global__ __launch_bounds__(MSD_BLOCK) void msd_wsum_kernel(const float* __restrict__ w, int n, float* __restrict__ ws) {
    __shared__ double red[MSD_BLOCK];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += MSD_BLOCK) s += (double)w[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = MSD_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float hi = (float)red[0];
        ws[0] = hi;
        ws[1] = (float)(red[0] - (double)hi);
    }
}

__device__ __forceinline__ double msd_sum_w(const MsdArgs& A) {
    return A.w ? (double)A.ws[0] + (double)A.ws[1] : (double)A.group;
}

// block = (row, tile).  thread = (atom a = tid % TA, lag class j = tid / TA); lags j, j + J, ... with J = 256 / TA.
template <bool FOURTH>
__global__ __launch_bounds__(MSD_BLOCK) void msd_fwd_kernel(MsdArgs A) {
    extern __shared__ float sm[];
    const int TA = 1 << A.sh, FS = msd_slot_stride(A.sh), J = MSD_BLOCK >> A.sh, RB = A.ring, L = A.L, T = A.T;
    float* ring = sm;
    float* acc2 = ring + RB * FS;
    float* acc4 = acc2 + (L << A.sh);
    const int tid = threadIdx.x, a = tid & (TA - 1), j = tid >> A.sh;
    const long long row = blockIdx.x / A.tiles;
    const int tile = blockIdx.x - (int)(row * A.tiles);
    const long long b = row / A.reps;
    const int rep = (int)(row - b * A.reps);
    const int a0 = tile << A.sh, n_valid = min(TA, A.group - a0);
    const float* xt = A.x + ((size_t)b * T * A.C + (size_t)rep * A.group + a0) * 3;
    const float wa = a < n_valid ? (A.w ? A.w[a0 + a] : 1.f) : 0.f;

    for (int tau = j; tau < L; tau += J) {                      // this thread's own accumulators: no barrier needed
        acc2[(tau << A.sh) + a] = 0.f;
        if (FOURTH) acc4[(tau << A.sh) + a] = 0.f;
    }
    for (int tw = 0; tw < T; tw += MSD_WINDOW) {
        const int slot_w = tw % RB;
        __syncthreads();                                         // the previous window's reads are done
        msd_stage(A, ring, xt, tw, min(tw + MSD_WINDOW, T), slot_w, n_valid);
        __syncthreads();
        float xw[MSD_WINDOW][3];
        {
            int slot = slot_w;
#pragma unroll
            for (int w = 0; w < MSD_WINDOW; ++w) {
                const float* p = ring + slot * FS + a;           // (frames past T: stale slots, never used below)
                xw[w][0] = p[0]; xw[w][1] = p[TA]; xw[w][2] = p[2 * TA];
                slot = slot + 1 == RB ? 0 : slot + 1;
            }
        }
        for (int tau = j; tau < L; tau += J) {
            const int e = tw - tau;                              // the earlier frame of the window's first frame; > -RB
            int slot = (e + RB) % RB;
            int rs = A.stride > 1 ? ((e % A.stride) + A.stride) % A.stride : 0;
            float s2 = acc2[(tau << A.sh) + a], s4 = FOURTH ? acc4[(tau << A.sh) + a] : 0.f;
#pragma unroll
            for (int w = 0; w < MSD_WINDOW; ++w) {
                const float* p = ring + slot * FS + a;
                const float dx = xw[w][0] - p[0], dy = xw[w][1] - p[TA], dz = xw[w][2] - p[2 * TA];
                const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                if (e + w >= 0 && tw + w < T && rs == 0) {       // t0 = e + w is an origin of this lag
                    s2 += d2;
                    if (FOURTH) s4 = fmaf(d2, d2, s4);
                }
                slot = slot + 1 == RB ? 0 : slot + 1;
                rs = rs + 1 >= A.stride ? 0 : rs + 1;
            }
            acc2[(tau << A.sh) + a] = s2;
            if (FOURTH) acc4[(tau << A.sh) + a] = s4;
        }
    }
    // over the tile's atoms: xor-shuffle tree inside each group of TA lanes (the loop bound is uniform)
    float* part2 = A.ws + MSD_WS_HEAD;
    float* part4 = part2 + (size_t)A.rows * L * A.tiles;
    for (int tb = 0; tb < L; tb += J) {
        const int tau = tb + j;
        float v2 = tau < L ? wa * acc2[(tau << A.sh) + a] : 0.f;
        float v4 = (FOURTH && tau < L) ? wa * acc4[(tau << A.sh) + a] : 0.f;
        v2 = group_sum_rt(v2, TA);
        if (FOURTH) v4 = group_sum_rt(v4, TA);
        if (a == 0 && tau < L) {
            const size_t o = ((size_t)row * L + tau) * A.tiles + tile;
            part2[o] = v2;
            if (FOURTH) part4[o] = v4;
        }
    }
}

// out[row][tau] = sum over the row's tiles (index order, double) / (|O_tau| sum w)
__global__ __launch_bounds__(MSD_BLOCK) void msd_finish_kernel(MsdArgs A, float* __restrict__ out2, float* __restrict__ out4) {
    const long long i = (long long)blockIdx.x * MSD_BLOCK + threadIdx.x;
    if (i >= A.rows * A.L) return;
    const int tau = (int)(i % A.L);
    const double norm = 1.0 / (msd_origins(A.T, tau, A.stride) * msd_sum_w(A));
    const float* p2 = A.ws + MSD_WS_HEAD + (size_t)i * A.tiles;
    double s = 0.0;
    for (int k = 0; k < A.tiles; ++k) s += (double)p2[k];
    out2[i] = (float)(s * norm);
    if (out4) {
        const float* p4 = p2 + (size_t)A.rows * A.L * A.tiles;
        s = 0.0;
        for (int k = 0; k < A.tiles; ++k) s += (double)p4[k];
        out4[i] = (float)(s * norm);
    }
}

// block = (row, tile).  thread = (atom a = tid % TA, frame w = tid / TA of the window of WB = 256 / TA frames).
template <bool FOURTH>
__global__ __launch_bounds__(MSD_BLOCK) void msd_bwd_kernel(MsdArgs A) {
    extern __shared__ float sm[];
    const int TA = 1 << A.sh, FS = msd_slot_stride(A.sh), WB = MSD_BLOCK >> A.sh, RB = A.ring, L = A.L, T = A.T;
    float* ring = sm;
    float* c2 = ring + RB * FS;
    float* c4 = c2 + L;
    const int tid = threadIdx.x, a = tid & (TA - 1), w = tid >> A.sh;
    const long long row = blockIdx.x / A.tiles;
    const int tile = blockIdx.x - (int)(row * A.tiles);
    const long long b = row / A.reps;
    const int rep = (int)(row - b * A.reps);
    const int a0 = tile << A.sh, n_valid = min(TA, A.group - a0);
    const size_t base = ((size_t)b * T * A.C + (size_t)rep * A.group + a0) * 3;
    const float* xt = A.x + base;
    const float wa = a < n_valid ? (A.w ? A.w[a0 + a] : 1.f) : 0.f;

    const double sw = msd_sum_w(A);
    for (int tau = tid; tau < L; tau += MSD_BLOCK) {
        const double c = 1.0 / (msd_origins(T, tau, A.stride) * sw);
        c2[tau] = (float)(2.0 * (double)A.g2[row * L + tau] * c);
        c4[tau] = FOURTH ? (float)(4.0 * (double)A.g4[row * L + tau] * c) : 0.f;
    }
    int loaded = 0;                                              // frames [0, loaded) have been staged
    for (int tw = 0; tw < T; tw += WB) {
        const int hi = min(T, tw + WB + L - 1);
        __syncthreads();                                         // the previous window's reads are done
        msd_stage(A, ring, xt, loaded, hi, loaded % RB, n_valid);
        loaded = hi;
        __syncthreads();
        const int t = tw + w;
        if (t < T && a < n_valid) {
            const int s0 = t % RB;
            const float* p = ring + s0 * FS + a;
            const float x0 = p[0], x1 = p[TA], x2 = p[2 * TA];
            const bool origin = A.stride == 1 || t % A.stride == 0;
            int rs = A.stride > 1 ? t % A.stride : 0;            // (t - tau) % stride, tau = 0
            int sb = s0, sf = s0;
            float gxx = 0.f, gxy = 0.f, gxz = 0.f;
            for (int tau = 1; tau < L; ++tau) {
                sb = sb == 0 ? RB - 1 : sb - 1;
                sf = sf + 1 == RB ? 0 : sf + 1;
                rs = rs == 0 ? A.stride - 1 : rs - 1;
                const float k2 = c2[tau], k4 = c4[tau];
                if (t - tau >= 0 && rs == 0) {
                    const float* q = ring + sb * FS + a;
                    const float dx = x0 - q[0], dy = x1 - q[TA], dz = x2 - q[2 * TA];
                    const float f = FOURTH ? fmaf(k4, fmaf(dz, dz, fmaf(dy, dy, dx * dx)), k2) : k2;
                    gxx = fmaf(f, dx, gxx); gxy = fmaf(f, dy, gxy); gxz = fmaf(f, dz, gxz);
                }
                if (origin && t + tau < T) {
                    const float* q = ring + sf * FS + a;
                    const float dx = q[0] - x0, dy = q[TA] - x1, dz = q[2 * TA] - x2;
                    const float f = FOURTH ? fmaf(k4, fmaf(dz, dz, fmaf(dy, dy, dx * dx)), k2) : k2;
                    gxx = fmaf(-f, dx, gxx); gxy = fmaf(-f, dy, gxy); gxz = fmaf(-f, dz, gxz);
                }
            }
            float* o = A.gx + base + ((size_t)t * A.C + a) * 3;
            const bool on = wa != 0.f;                           // weight 0: exactly 0, whatever the sums hold
            o[0] = on ? wa * gxx : 0.f; o[1] = on ? wa * gxy : 0.f; o[2] = on ? wa * gxz : 0.f;
        }
    }
}

int msd_check(const char* who, const float* x, int n_batch, int n_frames, int n_cols, int group, int n_lags, int origin_stride,
              const float* workspace) {
    MDG_CHECK_ARG(x && workspace, "%s: null pointer", who);
    MDG_CHECK_ARG(n_batch > 0 && n_frames > 0 && n_cols > 0 && group > 0, "%s: empty input (batch %d, frames %d, columns %d, "
                  "group %d)", who, n_batch, n_frames, n_cols, group);
    MDG_CHECK_ARG(n_cols % group == 0, "%s: the columns (%d) must be a multiple of the group (%d)", who, n_cols, group);
    MDG_CHECK_ARG(n_lags >= 1 && n_lags <= n_frames, "%s: 1 <= lags <= frames (got %d, %d)", who, n_lags, n_frames);
    MDG_CHECK_ARG(n_lags <= MSD_MAX_LAGS, "%s: at most %d lags (got %d)", who, MSD_MAX_LAGS, n_lags);
    MDG_CHECK_ARG(origin_stride >= 1, "%s: origin_stride must be >= 1 (got %d)", who, origin_stride);
    return MDG_OK;
}

MsdArgs msd_args(const float* x, int n_batch, int n_frames, int n_cols, int group, const float* weights, int n_lags,
                 int origin_stride, float* workspace, int sh) {
    MsdArgs A{};
    A.x = x; A.w = weights; A.ws = workspace;
    A.T = n_frames; A.C = n_cols; A.group = group; A.L = n_lags;
    A.stride = origin_stride < n_frames ? origin_stride : n_frames;          // beyond T - 1 only origin 0 is left either way
    A.reps = n_cols / group; A.sh = sh;
    A.tiles = (group + (1 << sh) - 1) >> sh;
    A.rows = (long long)n_batch * A.reps;
    return A;
}

}  // namespace

extern "C" int64_t mdg_msd_workspace(int n_batch, int n_cols, int group, int n_lags, int fourth) {
    if (n_batch <= 0 || n_cols <= 0 || group <= 0 || n_cols % group || n_lags < 1 || n_lags > MSD_MAX_LAGS) return 0;
    const int sh = msd_fwd_shift(n_lags, fourth != 0);
    const int64_t tiles = (group + (1 << sh) - 1) >> sh, rows = (int64_t)n_batch * (n_cols / group);
    return MSD_WS_HEAD + (fourth ? 2 : 1) * rows * n_lags * tiles;
}

extern "C" int mdg_msd_fwd(const float* x, int n_batch, int n_frames, int n_cols, int group, const float* weights, int n_lags,
                           int origin_stride, float* out2, float* out4, float* workspace, void* stream) {
    if (int rc = msd_check("msd_fwd", x, n_batch, n_frames, n_cols, group, n_lags, origin_stride, workspace)) return rc;
    MDG_CHECK_ARG(out2, "msd_fwd: null pointer");
    const bool fourth = out4 != nullptr;
    const int sh = msd_fwd_shift(n_lags, fourth);
    MsdArgs A = msd_args(x, n_batch, n_frames, n_cols, group, weights, n_lags, origin_stride, workspace, sh);
    A.ring = n_lags - 1 + MSD_WINDOW;
    const long long blocks = A.rows * A.tiles;
    MDG_CHECK_ARG(blocks < (1ll << 31) && A.rows * n_lags < (1ll << 31) * MSD_BLOCK, "msd_fwd: %lld (replica, atom tile) "
                  "workgroups exceed the grid", blocks);
    hipStream_t st = (hipStream_t)stream;
    if (weights) hipLaunchKernelGGL(msd_wsum_kernel, dim3(1), dim3(MSD_BLOCK), 0, st, weights, group, workspace);
    const size_t lds = (size_t)msd_fwd_lds(n_lags, sh, fourth);
    if (fourth) hipLaunchKernelGGL(msd_fwd_kernel<true>, dim3((unsigned)blocks), dim3(MSD_BLOCK), lds, st, A);
    else        hipLaunchKernelGGL(msd_fwd_kernel<false>, dim3((unsigned)blocks), dim3(MSD_BLOCK), lds, st, A);
    const long long n_out = A.rows * n_lags;
    hipLaunchKernelGGL(msd_finish_kernel, dim3((unsigned)((n_out + MSD_BLOCK - 1) / MSD_BLOCK)), dim3(MSD_BLOCK), 0, st, A, out2,
                       out4);
    MDG_CHECK_LAUNCH("msd forward kernels");
    return MDG_OK;
}

extern "C" int mdg_msd_bwd(const float* x, int n_batch, int n_frames, int n_cols, int group, const float* weights, int n_lags,
                           int origin_stride, const float* g2, const float* g4, float* gx, float* workspace, void* stream) {
    if (int rc = msd_check("msd_bwd", x, n_batch, n_frames, n_cols, group, n_lags, origin_stride, workspace)) return rc;
    MDG_CHECK_ARG(g2 && gx, "msd_bwd: null pointer");
    const int sh = msd_bwd_shift(n_lags);
    MsdArgs A = msd_args(x, n_batch, n_frames, n_cols, group, weights, n_lags, origin_stride, workspace, sh);
    A.g2 = g2; A.g4 = g4; A.gx = gx;
    A.ring = 2 * (n_lags - 1) + (MSD_BLOCK >> sh);
    const long long blocks = A.rows * A.tiles;
    MDG_CHECK_ARG(blocks < (1ll << 31), "msd_bwd: %lld (replica, atom tile) workgroups exceed the grid", blocks);
    hipStream_t st = (hipStream_t)stream;
    if (weights) hipLaunchKernelGGL(msd_wsum_kernel, dim3(1), dim3(MSD_BLOCK), 0, st, weights, group, workspace);
    const size_t lds = (size_t)msd_bwd_lds(n_lags, sh);
    if (g4) hipLaunchKernelGGL(msd_bwd_kernel<true>, dim3((unsigned)blocks), dim3(MSD_BLOCK), lds, st, A);
    else    hipLaunchKernelGGL(msd_bwd_kernel<false>, dim3((unsigned)blocks), dim3(MSD_BLOCK), lds, st, A);
    MDG_CHECK_LAUNCH("msd backward kernels");
    return MDG_OK;
}

// the tile constants, for callers that size their inputs around them (tests, tools)
extern "C" int mdg_msd_tile_atoms(void) { return 1 << MSD_TILE_SHIFT; }
extern "C" int mdg_msd_window(void) { return MSD_WINDOW; }
extern "C" int mdg_msd_max_lags(void) { return MSD_MAX_LAGS; }
