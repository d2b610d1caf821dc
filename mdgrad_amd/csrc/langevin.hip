// Langevin dynamics (BAOAB splitting) for the generic integrator path: the thermostat algebra of one step as one launch
// per half step and of one adjoint interval as one launch, around the force / force-vjp evaluation -- the pattern of the
// mdg_nhv_* kernels (csrc/nhc.hip): time-major frames [T, M, 3], the step / frame index on the device (idx[0], int64: a
// captured HIP graph advances it itself), dt read from the device grid, gamma and T read from device scalars.
//
//   v1 = v + (h/2) F(q)/m ; q1 = q + (h/2) v1 ; v2 = c1 v1 + c2 sqrt(T/m) xi ; qn = q1 + (h/2) v2 ; vn = v2 + (h/2) F(qn)/m
//   c1 = exp(-gamma h), c2 = sqrt(-expm1(-2 gamma h))
//
// The noise is counter based: Philox4x32-10 (Random123's multipliers, Weyl constants and round function) with
// key = (seed lo, seed hi), counter = (atom row, step lo, step hi, 0), step = step0 + k.  One call serves the three
// components of an atom; seed and step0 are device int64 words (rng[0], rng[1]).  Nothing is carried from step to step.
//
// Every array is walked element by element (M atoms = 3 M consecutive floats, 768 per workgroup: coalesced); only the
// noise is per atom: thread a of a workgroup draws the triple of atom (256 block + a) into LDS, the elementwise loop
// reads it from there.
#include "common.hpp"

namespace {

constexpr int LGV_BLOCK = 256;
constexpr int LGV_ELEMS = 3 * LGV_BLOCK;

__host__ __device__ inline int lgv_blocks(int n) { return (n + LGV_BLOCK - 1) / LGV_BLOCK; }

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&x)[4]) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += W0; k1 += W1;
    }
    x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// u = ((x >> 9) + 1/2) 2^-23: exact in float32, never 0 or 1
__device__ __forceinline__ float lgv_uniform(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// xi of (seed, step, atom): two Box-Muller pairs, the fourth normal is dropped
__device__ __forceinline__ void lgv_normals(long long seed, long long step, uint32_t atom, float& x, float& y, float& z) {
    uint32_t o[4];
    const unsigned long long s = (unsigned long long)seed, k = (unsigned long long)step;
    philox4x32_10(atom, (uint32_t)k, (uint32_t)(k >> 32), 0u, (uint32_t)s, (uint32_t)(s >> 32), o);
    const float r0 = sqrtf(-2.f * logf(lgv_uniform(o[0]))), r1 = sqrtf(-2.f * logf(lgv_uniform(o[2])));
    float sn, cs;
    sincospif(2.f * lgv_uniform(o[1]), &sn, &cs);
    x = r0 * cs; y = r0 * sn; z = r1 * cospif(2.f * lgv_uniform(o[3]));
}

// the triple of this thread's atom into xs[3 tid ..]; behind a barrier on return
__device__ __forceinline__ void lgv_stage_noise(float* xs, const long long* rng, long long step_off, int n, bool on) {
    const int a = blockIdx.x * LGV_BLOCK + threadIdx.x;
    float x = 0.f, y = 0.f, z = 0.f;
    if (on && a < n) lgv_normals(rng[0], rng[1] + step_off, (uint32_t)a, x, y, z);
    xs[3 * threadIdx.x] = x; xs[3 * threadIdx.x + 1] = y; xs[3 * threadIdx.x + 2] = z;
    __syncthreads();
}

// idx[0] <- new_idx by the workgroup that finishes last, i.e. after every workgroup has read the old value (each reads it
// before its loop); the ticket goes back to zero for the next launch
__device__ __forceinline__ void lgv_advance(long long* idx, long long new_idx, unsigned* ticket) {
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (gridDim.x == 1) { idx[0] = new_idx; return; }
    __threadfence();
    if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        idx[0] = new_idx;
    }
}

__global__ __launch_bounds__(LGV_BLOCK) void lgv_noise_kernel(const long long* __restrict__ rng, long long step_off, int n,
                                                              float* __restrict__ xi) {
    __shared__ float xs[LGV_ELEMS];
    lgv_stage_noise(xs, rng, step_off, n, true);
    const size_t base = (size_t)blockIdx.x * LGV_ELEMS;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int l = threadIdx.x + LGV_BLOCK * j;
        if (base + l < (size_t)3 * n) xi[base + l] = xs[l];
    }
}

// B, A, O, A with the cached force: v2 (the velocity after O) and qn
__global__ __launch_bounds__(LGV_BLOCK) void lgv_kick_kernel(
    const float* __restrict__ v, const float* __restrict__ q, const float* __restrict__ f, const float* __restrict__ mass,
    const float* __restrict__ gamma, const float* __restrict__ Tp, const float* __restrict__ t,
    const long long* __restrict__ idx, const long long* __restrict__ rng, int n, float* __restrict__ v2, float* __restrict__ qn) {
    __shared__ float xs[LGV_ELEMS];
    const long long k = idx[0];
    const float h = t[k + 1] - t[k], hh = 0.5f * h, g = gamma[0], T = Tp[0];
    const float c1 = expf(-g * h), c2 = sqrtf(-expm1f(-2.f * g * h));
    lgv_stage_noise(xs, rng, k, n, c2 != 0.f);
    const size_t base = (size_t)blockIdx.x * LGV_ELEMS;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int l = threadIdx.x + LGV_BLOCK * j;
        const size_t e = base + l;
        if (e < (size_t)3 * n) {
            const float m = mass[e / 3];
            const float v1 = v[e] + hh * f[e] / m;
            const float q1 = q[e] + hh * v1;
            const float vo = c1 * v1 + c2 * sqrtf(T / m) * xs[l];
            v2[e] = vo;
            qn[e] = q1 + hh * vo;
        }
    }
}

// the closing B with the new force: v = v2 + (h/2) fn/m, q = qn, f = fn; frame k+1 stored
__global__ __launch_bounds__(LGV_BLOCK) void lgv_finish_kernel(
    float* __restrict__ v, float* __restrict__ q, float* __restrict__ f, const float* __restrict__ v2,
    const float* __restrict__ qn, const float* __restrict__ fn, const float* __restrict__ mass, const float* __restrict__ t,
    long long* idx, int advance, int n, float* __restrict__ out_v, float* __restrict__ out_q, unsigned* ticket) {
    const long long k = idx[0];
    const float hh = 0.5f * (t[k + 1] - t[k]);
    const size_t base = (size_t)blockIdx.x * LGV_ELEMS, fo = (size_t)(k + 1) * n * 3;      // frames are time-major: [T, M, 3]
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const size_t e = base + threadIdx.x + LGV_BLOCK * j;
        if (e < (size_t)3 * n) {
            const float fe = fn[e], vn = v2[e] + hh * fe / mass[e / 3], qe = qn[e];
            v[e] = vn; q[e] = qe; f[e] = fe;
            out_v[fo + e] = vn; out_q[fo + e] = qe;
        }
    }
    if (advance) lgv_advance(idx, k + 1, ticket);
}

// adjoint, before the first force-vjp (frame i = idx[0], the last one): q <- frame i, w = (h/2) lam_v / m
__global__ __launch_bounds__(LGV_BLOCK) void lgv_adj_pre_kernel(
    const float* __restrict__ q_t, const float* __restrict__ lv, const float* __restrict__ mass, const float* __restrict__ t,
    const long long* __restrict__ idx, int n, float* __restrict__ q, float* __restrict__ w) {
    const long long i = idx[0];
    const float hh = 0.5f * (t[i] - t[i - 1]);
    const size_t base = (size_t)blockIdx.x * LGV_ELEMS, fo = (size_t)i * n * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const size_t e = base + threadIdx.x + LGV_BLOCK * j;
        if (e < (size_t)3 * n) {
            q[e] = q_t[fo + e];
            w[e] = hh * lv[e] / mass[e / 3];
        }
    }
}

// adjoint, between the force-vjp at frame i and the one at frame i-1 (f = F(q_i), dwf = H(q_i) w):
//   lam_q += dwf ;  A+: lam_v += (h/2) lam_q ;  O+: gamma_bar += lam_v . h (sqrt(T/m) xi / c2 - v2), lam_v *= c1 ;
//   A+: lam_v += (h/2) lam_q ;  w = (h/2) lam_v / m  (the opening B of this interval, at q_{i-1}) ;  lam += g[i-1] ;
//   w += (h'/2) lam_v / m  (the closing B of interval i-1, h' = t[i-1] - t[i-2]; not at frame 0) ;  q <- frame i-1
// v2 = v_i - (h/2) f / m is the velocity after O of the forward step.
template <bool GAMMA>
__global__ __launch_bounds__(LGV_BLOCK) void lgv_adj_step_kernel(
    const float* __restrict__ v_t, const float* __restrict__ q_t, const float* __restrict__ f, const float* __restrict__ dwf,
    const float* __restrict__ mass, const float* __restrict__ gamma, const float* __restrict__ Tp, const float* __restrict__ t,
    long long* idx, int advance, const long long* __restrict__ rng, const float* __restrict__ g_v,
    const float* __restrict__ g_q, int n, float* __restrict__ lv, float* __restrict__ lq, float* __restrict__ q,
    float* __restrict__ w, float* __restrict__ gpart, unsigned* ticket) {
    __shared__ float xs[GAMMA ? LGV_ELEMS : 1];
    __shared__ float red[32];
    const long long i = idx[0];
    const float h = t[i] - t[i - 1], hh = 0.5f * h, g = gamma[0], T = Tp[0];
    const float hp = i >= 2 ? 0.5f * (t[i - 1] - t[i - 2]) : 0.f;
    const float c1 = expf(-g * h), c2 = sqrtf(-expm1f(-2.f * g * h));
    if (GAMMA) lgv_stage_noise(xs, rng, i - 1, n, true);
    const size_t base = (size_t)blockIdx.x * LGV_ELEMS, fo = (size_t)i * n * 3, go = (size_t)(i - 1) * n * 3;
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int l = threadIdx.x + LGV_BLOCK * j;
        const size_t e = base + l;
        if (e < (size_t)3 * n) {
            const float m = mass[e / 3];
            float lqe = lq[e] + dwf[e];
            float lve = lv[e] + hh * lqe;
            if (GAMMA) {
                const float vo = v_t[fo + e] - hh * f[e] / m;
                part += lve * (h * (sqrtf(T / m) * xs[l] / c2 - vo));
            }
            lve = c1 * lve;
            lve = lve + hh * lqe;
            float we = hh * lve / m;
            lve += g_v[go + e];
            lqe += g_q[go + e];
            if (i >= 2) we += hp * lve / m;
            lv[e] = lve; lq[e] = lqe; w[e] = we;
            q[e] = q_t[go + e];
        }
    }
    if (GAMMA) {
        // per-workgroup partial in its own slot, added to over the intervals of a sweep by this workgroup alone
        const float s = block_sum(part, red);
        if (threadIdx.x == 0) gpart[blockIdx.x] += s;
    }
    if (advance) lgv_advance(idx, i - 1, ticket);
}

// gamma_bar = the slots added in slot order by one workgroup
__global__ __launch_bounds__(LGV_BLOCK) void lgv_gamma_sum_kernel(const float* __restrict__ gpart, int nb, float* __restrict__ out) {
    __shared__ float red[32];
    float s = 0.f;
    for (int b = threadIdx.x; b < nb; b += LGV_BLOCK) s += gpart[b];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

}  // namespace

#define LGV_GRID(n) dim3(lgv_blocks(n)), dim3(LGV_BLOCK), 0, (hipStream_t)stream
#define LGV_SIZE_OK(n) ((n) > 0 && (n) <= (1 << 30))

extern "C" int mdg_lgv_blocks(int n_total) { return n_total > 0 ? lgv_blocks(n_total) : 0; }

extern "C" int mdg_lgv_noise(const int64_t* rng, int64_t step_off, int n_total, float* xi, void* stream) {
    MDG_CHECK_ARG(rng && xi, "lgv_noise: null buffer");
    MDG_CHECK_ARG(LGV_SIZE_OK(n_total), "lgv_noise: bad size n=%d", n_total);
    hipLaunchKernelGGL(lgv_noise_kernel, LGV_GRID(n_total), reinterpret_cast<const long long*>(rng), (long long)step_off,
                       n_total, xi);
    MDG_CHECK_LAUNCH("lgv_noise_kernel");
    return MDG_OK;
}

extern "C" int mdg_lgv_kick(const float* v, const float* q, const float* f, const float* mass, const float* gamma,
                            const float* T, const float* t, const int64_t* idx, const int64_t* rng, int n_total, float* v2,
                            float* qn, void* stream) {
    MDG_CHECK_ARG(v && q && f && mass && gamma && T && t && idx && rng && v2 && qn, "lgv_kick: null buffer");
    MDG_CHECK_ARG(LGV_SIZE_OK(n_total), "lgv_kick: bad size n=%d", n_total);
    hipLaunchKernelGGL(lgv_kick_kernel, LGV_GRID(n_total), v, q, f, mass, gamma, T, t, reinterpret_cast<const long long*>(idx),
                       reinterpret_cast<const long long*>(rng), n_total, v2, qn);
    MDG_CHECK_LAUNCH("lgv_kick_kernel");
    return MDG_OK;
}

extern "C" int mdg_lgv_finish(float* v, float* q, float* f, const float* v2, const float* qn, const float* fn,
                              const float* mass, const float* t, int64_t* idx, int advance, int n_total, float* out_v,
                              float* out_q, uint32_t* ticket, void* stream) {
    MDG_CHECK_ARG(v && q && f && v2 && qn && fn && mass && t && idx && out_v && out_q && ticket, "lgv_finish: null buffer");
    MDG_CHECK_ARG(LGV_SIZE_OK(n_total), "lgv_finish: bad size n=%d", n_total);
    hipLaunchKernelGGL(lgv_finish_kernel, LGV_GRID(n_total), v, q, f, v2, qn, fn, mass, t, reinterpret_cast<long long*>(idx),
                       advance, n_total, out_v, out_q, ticket);
    MDG_CHECK_LAUNCH("lgv_finish_kernel");
    return MDG_OK;
}

extern "C" int mdg_lgv_adj_pre(const float* q_t, const float* lv, const float* mass, const float* t, const int64_t* idx,
                               int n_total, float* q, float* w, void* stream) {
    MDG_CHECK_ARG(q_t && lv && mass && t && idx && q && w, "lgv_adj_pre: null buffer");
    MDG_CHECK_ARG(LGV_SIZE_OK(n_total), "lgv_adj_pre: bad size n=%d", n_total);
    hipLaunchKernelGGL(lgv_adj_pre_kernel, LGV_GRID(n_total), q_t, lv, mass, t, reinterpret_cast<const long long*>(idx), n_total,
                       q, w);
    MDG_CHECK_LAUNCH("lgv_adj_pre_kernel");
    return MDG_OK;
}

extern "C" int mdg_lgv_adj_step(const float* v_t, const float* q_t, const float* f, const float* dwf, const float* mass,
                                const float* gamma, const float* T, const float* t, int64_t* idx, int advance,
                                const int64_t* rng, const float* g_v, const float* g_q, int want_gamma, int n_total, float* lv,
                                float* lq, float* q, float* w, float* gpart, uint32_t* ticket, void* stream) {
    MDG_CHECK_ARG(v_t && q_t && f && dwf && mass && gamma && T && t && idx && rng && g_v && g_q && lv && lq && q && w && ticket,
                  "lgv_adj_step: null buffer");
    MDG_CHECK_ARG(!want_gamma || gpart, "lgv_adj_step: the friction gradient needs its partial-sum slots");
    MDG_CHECK_ARG(LGV_SIZE_OK(n_total), "lgv_adj_step: bad size n=%d", n_total);
    if (want_gamma)
        hipLaunchKernelGGL(lgv_adj_step_kernel<true>, LGV_GRID(n_total), v_t, q_t, f, dwf, mass, gamma, T, t,
                           reinterpret_cast<long long*>(idx), advance, reinterpret_cast<const long long*>(rng), g_v, g_q, n_total,
                           lv, lq, q, w, gpart, ticket);
    else
        hipLaunchKernelGGL(lgv_adj_step_kernel<false>, LGV_GRID(n_total), v_t, q_t, f, dwf, mass, gamma, T, t,
                           reinterpret_cast<long long*>(idx), advance, reinterpret_cast<const long long*>(rng), g_v, g_q, n_total,
                           lv, lq, q, w, gpart, ticket);
    MDG_CHECK_LAUNCH("lgv_adj_step_kernel");
    return MDG_OK;
}

extern "C" int mdg_lgv_gamma_sum(const float* gpart, int n_total, float* out, void* stream) {
    MDG_CHECK_ARG(gpart && out, "lgv_gamma_sum: null buffer");
    MDG_CHECK_ARG(LGV_SIZE_OK(n_total), "lgv_gamma_sum: bad size n=%d", n_total);
    hipLaunchKernelGGL(lgv_gamma_sum_kernel, dim3(1), dim3(LGV_BLOCK), 0, (hipStream_t)stream, gpart, lgv_blocks(n_total), out);
    MDG_CHECK_LAUNCH("lgv_gamma_sum_kernel");
    return MDG_OK;
}
