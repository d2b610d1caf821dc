// Steinhardt bond-orientational order (Steinhardt, Nelson, Ronchetti, Phys. Rev. B 28, 784 (1983)) with a smooth neighbour
// weight: the per-atom moments A_lm(i), n_i over a per-atom neighbour list, and their gradient (K29, include/mdgrad_hip.h).
//
//   bonds      the entries j of atom i's row of the ELL list (frames = groups of n_atoms rows); u = x_j - x_i re-imaged on the
//              diagonal cell like the list builder (common.hpp min_image: u - L clamp(rint(u / L), -1, 1)), r = |u|, s = u / r
//   weight     w(r) = 1 (r <= r_in), 1/2 [1 + cos(pi (r - r_in) / (cutoff - r_in))] (r_in < r < cutoff), 0 (r >= cutoff): C^1.
//              The list is only the candidate set: an entry at r >= cutoff weighs exactly 0.
//   moments    A_lm(i) = sum_j w(r_ij) Y_lm(s_ij),  n_i = sum_j w(r_ij),  Y_lm the REAL orthonormal harmonics
//
// Harmonics without trigonometry and without a pole singularity: with c = s_z and (x + i y)^m = C_m + i S_m,
//     Y_l0 = N_l0 Q_l^0(c)      Y_l,+m = sqrt2 N_lm Q_l^m(c) C_m      Y_l,-m = sqrt2 N_lm Q_l^m(c) S_m       (m = 1 .. l)
//     N_lm = sqrt((2l+1) / (4 pi) (l-m)! / (l+m)!),     Q_l^m = d^m P_l / dc^m = P_l^m / sin^m theta without the Condon-Shortley phase
// Q_l^m is a polynomial in c by the upward recurrences, run on q = Q / (2m-1)!! so that every start value is 1:
//     q_m^m = 1      q_{m+1}^m = (2m+1) c      q_l^m = [(2l-1) c q_{l-1}^m - (l+m-1) q_{l-2}^m] / (l-m)
// and C_{m+1} = x C_m - y S_m, S_{m+1} = x S_m + y C_m.  The constants sqrt2 N_lm (2m-1)!! come from a constexpr table evaluated
// in double by the compiler and multiply the finished sums once.  A sign convention of the basis does not reach q_l, Q_l or
// any other rotational invariant.
//
// Component order (the last axis of A after the Python reshape): the l of `ls` in the given order, and inside one l the
// 2l+1 entries m = -l .. l: index l - m' holds the S_m' (sine) component, index l the m = 0 one, index l + m' the C_m' (cosine) one.
//
// Layout: A is written COMPONENT-MAJOR, A[k * n_rows + row] with n_rows = n_frames * n_atoms, so that the 64 lanes of a wave
// (64 consecutive rows) store 256 contiguous bytes per component.  The backward reads the cotangent gA ROW-MAJOR,
// gA[row * K + k]: there the traffic is the gather of the 2l+1 entries of every neighbour's row, and one neighbour's entries
// then share one or two cache lines.
//
// Thread mapping: one thread per atom (row), 256-thread workgroups, like csrc/adf.hip's backward: a bond costs ~3 (l+1)(l+2)/2
// multiply-adds against five gathered dwords, so the kernels are VALU-bound and a lane that owns its atom needs no cross-lane
// traffic, no LDS and no atomics.  One l is processed at a time (a wave-uniform switch into a template instantiated for
// l = 1 .. 12, every loop over m unrolled), so at most 2l+1 <= 25 accumulators are live and stay in registers: no scratch.
//
// Backward: the list is symmetric, so thread i covers both of its roles in one loop over its own row.  As centre, bond
// (i, j) enters sum_lm gA_lm(i) w Y_lm(s) + gn(i) w through u; as the end of j's bond (-u) it enters
// sum_lm gA_lm(j) w (-1)^l Y_lm(s) + gn(j) w, and both derivatives with respect to x_i are -d/du.  With
// g_lm = gA_lm(i) + (-1)^l gA_lm(j), T = sum g_lm Y_lm and its polynomial gradient G = dT/ds (dQ_l^m/dc = Q_l^{m+1},
// dC_m/dx = m C_{m-1}, dS_m/dx = m S_{m-1}, dC_m/dy = -m S_{m-1}, dS_m/dy = m C_{m-1}):
//     g_xyz(i) = - sum_j [ w'(r) s (T + gn(i) + gn(j)) + w(r) / r (I - s s^T) G ]
// a fixed-order sum per thread: bitwise reproducible from launch to launch.
//
// Non-finite or coincident positions: an atom whose own position is not finite gets NaN moments and a NaN gradient (the list
// builder gives it an empty row, which would otherwise read as "no neighbours"); two atoms at the same point have no bond
// direction and give NaN through 1 / r.  Row entries are clamped to max_nbr and a column index outside the launch is skipped.
#include <math.h>
#include "common.hpp"

namespace {

constexpr int BO_BLOCK = 256;
constexpr int BO_MAX_L = 12;
constexpr int BO_MAX_NL = 4;

constexpr double bo_sqrt(double x) {               // Newton from above; exact to the last bit or two of a double
    double y = x > 1.0 ? x : 1.0;
    for (int i = 0; i < 256; ++i) y = 0.5 * (y + x / y);
    return y;
}

// na[l][m] = (m ? sqrt2 : 1) N_lm (2m-1)!!  scales q_l^m in Y_lm;  nz[l][m] = (m ? sqrt2 : 1) N_lm (2m+1)!!  scales q_l^{m+1} in dY_lm/dz
// ra[l][m] = (2l-1) / (l-m), rb[l][m] = (l+m-1) / (l-m): the recurrence's coefficients
struct BoTable {
    float na[BO_MAX_L + 1][BO_MAX_L + 1], nz[BO_MAX_L + 1][BO_MAX_L + 1];
    float ra[BO_MAX_L + 1][BO_MAX_L + 1], rb[BO_MAX_L + 1][BO_MAX_L + 1];
    constexpr BoTable() : na{}, nz{}, ra{}, rb{} {
        for (int l = 0; l <= BO_MAX_L; ++l) {
            double df = 1.0;                                  // (2m-1)!!
            for (int m = 0; m <= l; ++m) {
                if (m > 0) df *= (double)(2 * m - 1);
                double ratio = 1.0;                           // (l-m)! / (l+m)!
                for (int k = l - m + 1; k <= l + m; ++k) ratio /= (double)k;
                const double nlm = bo_sqrt((2 * l + 1) / (4.0 * 3.14159265358979323846) * ratio) * (m ? 1.41421356237309504880 : 1.0);
                na[l][m] = (float)(nlm * df);
                nz[l][m] = (float)(nlm * df * (2 * m + 1));
                if (l > m) {
                    ra[l][m] = (float)((2.0 * l - 1.0) / (l - m));
                    rb[l][m] = (float)((l + m - 1.0) / (l - m));
                }
            }
        }
    }
};
constexpr BoTable BO_TAB = BoTable();

struct BoArgs {
    const float* pos;
    const int32_t* col;
    const int32_t* cnt;
    long long n_total;       // frames * atoms (rows of the list)
    int n_atoms, max_nbr, n_l, K;
    unsigned ls_packed;      // 4 bits per l        (a runtime index into an array of a by-value argument would go to scratch)
    unsigned off_packed;     // 8 bits per offset of an l's first component
    float L[3], invL[3];
    float cutoff, r_in, inv_dr;      // 1 / (cutoff - r_in)
};

struct BoBond { float x, y, z, r, w, dw; };          // s, r, w(r), w'(r)

__device__ __forceinline__ float bo_image(float d, float inv, float L) {
    return fmaf(-__builtin_amdgcn_fmed3f(rintf(d * inv), -1.f, 1.f), L, d);
}

__device__ __forceinline__ BoBond bo_bond(const BoArgs& P, long long j, float3 xa) {
    const float dx = bo_image(P.pos[3 * j] - xa.x, P.invL[0], P.L[0]);
    const float dy = bo_image(P.pos[3 * j + 1] - xa.y, P.invL[1], P.L[1]);
    const float dz = bo_image(P.pos[3 * j + 2] - xa.z, P.invL[2], P.L[2]);
    BoBond b;
    b.r = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
    const float inv = 1.f / b.r;
    b.x = dx * inv; b.y = dy * inv; b.z = dz * inv;
    if (b.r <= P.r_in) { b.w = 1.f; b.dw = 0.f; }
    else if (b.r < P.cutoff) {
        const float t = (b.r - P.r_in) * P.inv_dr;
        b.w = fmaf(0.5f, cospif(t), 0.5f);
        b.dw = -0.5f * 3.14159265358979323846f * P.inv_dr * sinpif(t);
    } else {
        b.w = b.dw = (b.r != b.r) ? b.r : 0.f;
    }
    return b;
}

// q_L^M(c) = Q_L^M(c) / (2M-1)!!
template <int L, int M>
__device__ __forceinline__ float bo_q(float c) {
    if (L == M) return 1.f;
    float p2 = 1.f, p1 = (float)(2 * M + 1) * c;
#pragma unroll
    for (int l = M + 2; l <= L; ++l) {
        const float t = fmaf(BO_TAB.ra[l][M] * c, p1, -BO_TAB.rb[l][M] * p2);
        p2 = p1;
        p1 = t;
    }
    return p1;
}

template <int L, int M>
struct BoFwdStep {
    static __device__ __forceinline__ void run(const BoBond& b, float cm, float sm, float* ac, float* as) {
        const float wq = b.w * bo_q<L, M>(b.z);
        ac[M] = fmaf(wq, cm, ac[M]);
        if (M > 0) as[M] = fmaf(wq, sm, as[M]);
        if (M < L) BoFwdStep<L, (M < L ? M + 1 : L)>::run(b, fmaf(cm, b.x, -sm * b.y), fmaf(sm, b.x, cm * b.y), ac, as);
    }
};

template <int L>
__device__ __forceinline__ void bo_fwd_l(const BoArgs& P, long long a, long long lo, int n, const int32_t* __restrict__ row,
                                         float3 xa, float bad, float* __restrict__ A_out, float* __restrict__ n_out) {
    float ac[L + 1], as[L + 1];
#pragma unroll
    for (int m = 0; m <= L; ++m) ac[m] = as[m] = 0.f;
    float nsum = 0.f;
    for (int p = 0; p < n; ++p) {
        const long long j = row[p];
        if ((unsigned long long)(j - lo) >= (unsigned long long)P.n_atoms) continue;
        const BoBond b = bo_bond(P, j, xa);
        if (b.w == 0.f) continue;
        nsum += b.w;
        BoFwdStep<L, 0>::run(b, 1.f, 0.f, ac, as);
    }
    // bad = 0 for a finite own position, NaN otherwise
    A_out[(long long)L * P.n_total] = fmaf(BO_TAB.na[L][0], ac[0], bad);
#pragma unroll
    for (int m = 1; m <= L; ++m) {
        A_out[(long long)(L + m) * P.n_total] = fmaf(BO_TAB.na[L][m], ac[m], bad);
        A_out[(long long)(L - m) * P.n_total] = fmaf(BO_TAB.na[L][m], as[m], bad);
    }
    if (n_out) *n_out = nsum + bad;
}

#define BO_SWITCH(l, CALL)                                                                                   \
    switch (l) {                                                                                             \
        case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;      \
        case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; case 8: CALL(8); break;      \
        case 9: CALL(9); break; case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break; \
        default: break;                                                                                      \
    }

__global__ __launch_bounds__(BO_BLOCK) void bond_order_fwd_kernel(BoArgs P, float* __restrict__ A, float* __restrict__ n_out) {
    const long long a = (long long)blockIdx.x * BO_BLOCK + threadIdx.x;
    if (a >= P.n_total) return;
    const int n = min(max(P.cnt[a], 0), P.max_nbr);
    const int32_t* row = P.col + a * P.max_nbr;
    const long long lo = a / P.n_atoms * P.n_atoms;          // first row of this atom's frame
    const float3 xa = make_float3(P.pos[3 * a], P.pos[3 * a + 1], P.pos[3 * a + 2]);
    const float bad = (xa.x + xa.y + xa.z) * 0.f;            // 0, or NaN for a non-finite position
    for (int t = 0; t < P.n_l; ++t) {
        const int l = (P.ls_packed >> (4 * t)) & 15;
        float* out = A + (long long)((P.off_packed >> (8 * t)) & 255) * P.n_total + a;
        float* no = t == 0 ? n_out + a : nullptr;
#define BO_CALL(LL) bo_fwd_l<LL>(P, a, lo, n, row, xa, bad, out, no)
        BO_SWITCH(l, BO_CALL)
#undef BO_CALL
    }
}

// one m of the backward's sums over a bond: T, (Tx, Ty, Tz) += the terms of the components +-M (value, d/dx, d/dy) and of the
// components +-(M-1) (d/dz, which needs q^M); cm, sm = C_M, S_M; cp, sp = C_{M-1}, S_{M-1}; gcp, gsp = the g of +-(M-1)
template <int L, int M>
struct BoBwdStep {
    static __device__ __forceinline__ void run(const BoBond& b, const float* gi, const float* __restrict__ gj, float sgn, float cm,
                                               float sm, float cp, float sp, float gcp, float gsp, float& T, float& Tx, float& Ty,
                                               float& Tz) {
        const float q = bo_q<L, M>(b.z);
        const float gc = fmaf(sgn, gj[L + M], gi[L + M]);
        const float gs = M > 0 ? fmaf(sgn, gj[L - M], gi[L - M]) : 0.f;
        const float qa = BO_TAB.na[L][M] * q;
        T = fmaf(qa, fmaf(gs, sm, gc * cm), T);
        if (M > 0) {
            const float mq = (float)M * qa;
            Tx = fmaf(mq, fmaf(gs, sp, gc * cp), Tx);
            Ty = fmaf(mq, fmaf(gs, cp, -gc * sp), Ty);
            Tz = fmaf(BO_TAB.nz[L][M - 1] * q, fmaf(gsp, sp, gcp * cp), Tz);
        }
        if (M < L)
            BoBwdStep<L, (M < L ? M + 1 : L)>::run(b, gi, gj, sgn, fmaf(cm, b.x, -sm * b.y), fmaf(sm, b.x, cm * b.y), cm, sm, gc, gs,
                                                   T, Tx, Ty, Tz);
    }
};

template <int L>
__device__ __forceinline__ void bo_bwd_l(const BoArgs& P, long long a, long long lo, int n, const int32_t* __restrict__ row, float3 xa,
                                         const float* __restrict__ gA, const float* __restrict__ gn, int off, bool first, float& gx,
                                         float& gy, float& gz) {
    float gi[2 * L + 1];
#pragma unroll
    for (int k = 0; k <= 2 * L; ++k) gi[k] = gA[a * P.K + off + k];
    const float gni = first ? gn[a] : 0.f;
    const float sgn = (L & 1) ? -1.f : 1.f;
    for (int p = 0; p < n; ++p) {
        const long long j = row[p];
        if ((unsigned long long)(j - lo) >= (unsigned long long)P.n_atoms) continue;
        const BoBond b = bo_bond(P, j, xa);
        if (b.w == 0.f && b.dw == 0.f) continue;
        float T = 0.f, Tx = 0.f, Ty = 0.f, Tz = 0.f;
        BoBwdStep<L, 0>::run(b, gi, gA + j * P.K + off, sgn, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f, T, Tx, Ty, Tz);
        const float radial = b.dw * (T + (first ? gni + gn[j] : 0.f));
        const float wr = b.w / b.r;
        const float sd = fmaf(b.z, Tz, fmaf(b.y, Ty, b.x * Tx));
        gx -= fmaf(wr, fmaf(-b.x, sd, Tx), radial * b.x);
        gy -= fmaf(wr, fmaf(-b.y, sd, Ty), radial * b.y);
        gz -= fmaf(wr, fmaf(-b.z, sd, Tz), radial * b.z);
    }
}

__global__ __launch_bounds__(BO_BLOCK) void bond_order_bwd_kernel(BoArgs P, const float* __restrict__ gA, const float* __restrict__ gn,
                                                                  float* __restrict__ g_xyz) {
    const long long a = (long long)blockIdx.x * BO_BLOCK + threadIdx.x;
    if (a >= P.n_total) return;
    const int n = min(max(P.cnt[a], 0), P.max_nbr);
    const int32_t* row = P.col + a * P.max_nbr;
    const long long lo = a / P.n_atoms * P.n_atoms;
    const float3 xa = make_float3(P.pos[3 * a], P.pos[3 * a + 1], P.pos[3 * a + 2]);
    const float bad = (xa.x + xa.y + xa.z) * 0.f;
    float gx = bad, gy = bad, gz = bad;
    for (int t = 0; t < P.n_l; ++t) {
        const int l = (P.ls_packed >> (4 * t)) & 15;
        const int off = (P.off_packed >> (8 * t)) & 255;
#define BO_CALL(LL) bo_bwd_l<LL>(P, a, lo, n, row, xa, gA, gn, off, t == 0, gx, gy, gz)
        BO_SWITCH(l, BO_CALL)
#undef BO_CALL
    }
    g_xyz[3 * a] = gx;
    g_xyz[3 * a + 1] = gy;
    g_xyz[3 * a + 2] = gz;
}

// the checks that need no pointer come first: a caller can ask what the library accepts without any buffer
int bo_ls(const int32_t* ls, int n_l, unsigned& ls_packed, unsigned& off_packed, int& K) {
    MDG_CHECK_ARG(n_l >= 1 && n_l <= BO_MAX_NL, "bond_order: n_l must be in [1, %d], got %d", BO_MAX_NL, n_l);
    MDG_CHECK_ARG(ls, "bond_order: null ls");
    ls_packed = off_packed = 0u;
    K = 0;
    for (int t = 0; t < n_l; ++t) {
        MDG_CHECK_ARG(ls[t] >= 1 && ls[t] <= BO_MAX_L, "bond_order: every l of ls must be in [1, %d], got %d", BO_MAX_L, ls[t]);
        for (int s = 0; s < t; ++s) MDG_CHECK_ARG(ls[s] != ls[t], "bond_order: the l of ls must be distinct, %d is repeated", ls[t]);
        ls_packed |= (unsigned)ls[t] << (4 * t);
        off_packed |= (unsigned)K << (8 * t);
        K += 2 * ls[t] + 1;
    }
    return MDG_OK;
}

int bo_args(BoArgs& P, const float* pos, int n_frames, int n_atoms, const MdgCell* cell, float cutoff, float r_in, const int32_t* col,
            const int32_t* cnt, int max_nbr, const int32_t* ls, int n_l) {
    const int rc = bo_ls(ls, n_l, P.ls_packed, P.off_packed, P.K);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(pos && cell && col && cnt, "bond_order: null argument");
    MDG_CHECK_ARG(n_frames > 0 && n_atoms > 0 && max_nbr > 0, "bond_order: empty system or list");
    MDG_CHECK_ARG((long long)n_frames * n_atoms < (1ll << 31), "bond_order: more than 2^31 list rows in one call (chunk the frames)");
    MDG_CHECK_ARG(cell->diag, "bond_order: the cell must be diagonal");
    MDG_CHECK_ARG(cutoff > 0.f && isfinite(cutoff) && r_in > 0.f && r_in < cutoff,
                  "bond_order: need 0 < r_in < cutoff, got r_in %g, cutoff %g", (double)r_in, (double)cutoff);
    P.pos = pos; P.col = col; P.cnt = cnt;
    P.n_total = (long long)n_frames * n_atoms;
    P.n_atoms = n_atoms; P.max_nbr = max_nbr; P.n_l = n_l;
    for (int d = 0; d < 3; ++d) { P.L[d] = cell->h[4 * d]; P.invL[d] = cell->inv[4 * d]; }
    P.cutoff = cutoff; P.r_in = r_in; P.inv_dr = 1.f / (cutoff - r_in);
    return MDG_OK;
}

}  // namespace

extern "C" int mdg_bond_order_components(const int32_t* ls, int n_l) {
    unsigned a, b;
    int K = 0;
    return bo_ls(ls, n_l, a, b, K) == MDG_OK ? K : 0;
}

extern "C" int mdg_bond_order_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, float cutoff, float r_in,
                                  const int32_t* col, const int32_t* cnt, int max_nbr, const int32_t* ls, int n_l, float* A, float* n,
                                  void* stream) {
    BoArgs P;
    const int rc = bo_args(P, pos, n_frames, n_atoms, cell, cutoff, r_in, col, cnt, max_nbr, ls, n_l);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(A && n, "bond_order_fwd: null output");
    const long long blocks = (P.n_total + BO_BLOCK - 1) / BO_BLOCK;
    hipLaunchKernelGGL(bond_order_fwd_kernel, dim3((unsigned)blocks), dim3(BO_BLOCK), 0, (hipStream_t)stream, P, A, n);
    MDG_CHECK_LAUNCH("bond_order_fwd_kernel");
    return MDG_OK;
}

extern "C" int mdg_bond_order_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, float cutoff, float r_in,
                                  const int32_t* col, const int32_t* cnt, int max_nbr, const int32_t* ls, int n_l, const float* gA,
                                  const float* gn, float* g_xyz, void* stream) {
    BoArgs P;
    const int rc = bo_args(P, pos, n_frames, n_atoms, cell, cutoff, r_in, col, cnt, max_nbr, ls, n_l);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(gA && gn && g_xyz, "bond_order_bwd: null gA, gn or g_xyz");
    const long long blocks = (P.n_total + BO_BLOCK - 1) / BO_BLOCK;
    hipLaunchKernelGGL(bond_order_bwd_kernel, dim3((unsigned)blocks), dim3(BO_BLOCK), 0, (hipStream_t)stream, P, gA, gn, g_xyz);
    MDG_CHECK_LAUNCH("bond_order_bwd_kernel");
    return MDG_OK;
}
