// K28: Stillinger-Weber two- plus three-body potential for up to four species over the per-atom (ELL) list
// (mdgrad_amd/interface.py StillingerWeberMulti; the LAMMPS `pair_style sw` convention).  Atom i has the species t_i; with
// a = t_i (the centre), b = t_j, c = t_k:
//
//   U      = 1/2 sum_i sum_{j != i} phi2_ab(r_ij) + sum_i sum_{j<k in row(i)} phi3_abc(r_ij, r_ik, cos theta_jik)
//   phi2_ab  = A_ab eps_ab [B_ab (sigma_ab/r)^p_ab - (sigma_ab/r)^q_ab] exp(sigma_ab / (r - rc_ab))    r < rc_ab = a_ab sigma_ab
//   g_ab     = exp(gamma_ab sigma_ab / (r - rc_ab))                                                    r < rc_ab, else exactly 0
//   phi3_abc = K_a{bc} (cos theta - cos0_abc)^2 g_ab(r_ij) g_ac(r_ik),   K_a{bc} = (lam_abc eps3_abc + lam_acb eps3_acb) / 2
//
// The structure is that of csrc/sw.hip (read its header first): LPA lanes walk one atom's row, an atom-centric gather of the
// pair, the triplets centred on i and the triplets centred on j with the ends i and k, wave shuffles, block partials and
// energy_finish; no float atomics => bitwise reproducible; Dual numbers for LEVEL 2; no contraction, so that dU/dx of a
// LEVEL 1 and of a LEVEL 2 launch agree bit for bit.
//
// What is particular to this file:
//  - every constant comes from one flat device table (mdg_sw_multi_table_size floats), staged into LDS once per block:
//      pair entry    tab[12 (a S + b) ...]                 = eps, sigma, a sigma, gamma sigma, gamma, A, B, p, q, a, A eps, 0
//      triplet entry tab[12 S S + 4 ((a S + b) S + c) ...] = K_a{bc}, cos0_abc, w_abc, 0
//    row = the species of the centre.  w_abc = eps3_abc / 2 (eps3_abb for b = c) is the weight with which lam[a, b, c] enters
//    K_a{bc}.  A lane indexes the table with the species of its own atoms; a species read from `types` is clamped into it.
//  - the pair tables need not be symmetric: the force of the pair (i, j) is the derivative of (phi2_ab + phi2_ba) / 2 and both
//    directions are evaluated (once when a = b); the bond i -> j has the support and g of (a, b) as a bond of the centre i and
//    those of (b, a) as a bond of the centre j.
//  - the per-lane sums are kept per end species (4) and per unordered pair of end species (10) in registers, with statically
//    unrolled, predicated adds; a row of pth / pthw is [2 S S + S S S] = d u_i / d(eps [S, S], sigma [S, S], lam [S, S, S]),
//    zero but for eps[a, :], sigma[a, :], lam[a, :, :], where lam[a, b, c] and lam[a, c, b] hold w_abc T and w_acb T of their
//    class's sum T: the column sums over the atoms are dU/d(eps, sigma, lam).
#pragma clang fp contract(off)
#include "dual.hpp"
#include "manybody.hpp"

namespace {

constexpr int SWM_LPA = 16;                   // lanes per atom, block: those of sw.hip
constexpr int SWM_BLOCK = 256;
constexpr int SWM_SMAX = 4;                   // species
constexpr int SWM_NCLS = 10;                  // unordered pairs of end species
constexpr int SWM_PAIR = 12, SWM_TRIP = 4;    // floats per table entry
constexpr int SWM_TABLE_MAX = SWM_PAIR * SWM_SMAX * SWM_SMAX + SWM_TRIP * SWM_SMAX * SWM_SMAX * SWM_SMAX;

struct SwmPairE { float eps, sigma, rc, gs, gamma, A, B, fp, fq, a, Ae, pad; };
struct SwmTripE { float K, cos0, w, pad; };

struct SwmArgs {
    const float* pos; int N; MdgCell cell;
    const int32_t* col; const int32_t* shift; const int32_t* cnt; int max_nbr;
    const int32_t* types; int S; const float* tables;
    const float* w;
    float* grad; float* hw; float* pth; float* pthw; float* partial;
    float oscale; int oacc;
};

// the block's copy of the table in LDS
struct SwmView {
    const int32_t* types; int S; const float* tab;
    __device__ __forceinline__ int species(int i) const { return min(max(types[i], 0), S - 1); }
    __device__ __forceinline__ const SwmPairE& pair(int a, int b) const {
        return reinterpret_cast<const SwmPairE*>(tab)[a * S + b];
    }
    __device__ __forceinline__ const SwmTripE& trip(int a, int b, int c) const {
        return reinterpret_cast<const SwmTripE*>(tab + SWM_PAIR * S * S)[(a * S + b) * S + c];
    }
};

// the class of the unordered pair of end species {b, c}: (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)
__device__ __forceinline__ constexpr int swm_cls(int b, int c) {
    const int lo = b < c ? b : c, hi = b < c ? c : b;
    return lo * (9 - lo) / 2 + (hi - lo);
}

template <class T> __device__ __forceinline__ T swm_pow(T x, int n) {
    T r = mk<T>(1.f, 0.f);
    while (n > 0) { if (n & 1) r = r * x; x = x * x; n >>= 1; }
    return r;
}

// one list entry seen from its centre: unit vector centre -> end, r, 1/r (the geometry), then 1/(r - rc) and g of a pair entry
template <class T> struct SwmEdge { T ex, ey, ez, r, ir, inv, g; };

// (dx, dy, dz) = end - centre with the stored image applied, (ax, ay, az) = w_end - w_centre.  False for r = 0 or r >= rmax.
template <class T>
__device__ __forceinline__ bool swm_geo(float rmax, float dx, float dy, float dz, float ax, float ay, float az, SwmEdge<T>& e) {
    const T x = mk<T>(dx, ax), y = mk<T>(dy, ay), z = mk<T>(dz, az);
    const T one = mk<T>(1.f, 0.f);
    const T d2 = x * x + y * y + z * z;
    const float rv = sqrtf(val(d2));
    if (!(rv > 0.f && rv < rmax)) return false;              // the support test, on the r that r - rc is formed from
    e.r = fsqrt_(d2);
    e.ir = one / e.r;
    e.ex = x * e.ir; e.ey = y * e.ir; e.ez = z * e.ir;
    return true;
}
template <class T>
__device__ __forceinline__ void swm_tail(const SwmPairE& P, SwmEdge<T>& e) {
    const T one = mk<T>(1.f, 0.f);
    e.inv = one / (e.r - P.rc);
    e.g = fexp_(P.gs * e.inv);
}
template <class T>
__device__ __forceinline__ bool swm_edge(const SwmPairE& P, float dx, float dy, float dz, float ax, float ay, float az,
                                         SwmEdge<T>& e) {
    if (!swm_geo<T>(P.rc, dx, dy, dz, ax, ay, az, e)) return false;
    swm_tail<T>(P, e);
    return true;
}

// the pair term of the entry P on an edge inside its support (e.inv of P): e2 = phi2 / eps = A [B s^p - s^q] E with
// E = exp(sigma / (r - rc)), d e2 / d sigma, and du = -phi2'
template <class T, int LEVEL>
__device__ __forceinline__ void swm_pair(const SwmPairE& P, const SwmEdge<T>& e, T& e2, T& e2s, T& du) {
    const T sr = P.sigma * e.ir;
    const T sp = swm_pow(sr, (int)P.fp), sq = swm_pow(sr, (int)P.fq);
    const T E = fexp_(P.sigma * e.inv);
    const T bs = P.B * sp - sq;
    const T ps = (P.fp * P.B) * sp - P.fq * sq;
    const T inv2 = e.inv * e.inv;
    e2 = P.A * (bs * E);
    if (LEVEL >= 1) {
        // d e2 / d sigma = A ps E / sigma + e2 r / (r - rc)^2;  phi2' = -eps A E [ps / r + bs sigma / (r - rc)^2]
        e2s = (P.A / P.sigma) * (ps * E) + e2 * (e.r * inv2);
        du = P.Ae * (E * (ps * e.ir + P.sigma * (bs * inv2)));
    }
}

// acc[q] += x for the one q = idx: statically unrolled and predicated, so that acc stays in registers
template <class T, int NQ>
__device__ __forceinline__ void swm_add(T (&acc)[NQ], int idx, const T& x) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        if (q == idx) acc[q] = acc[q] + x;
}

// out: [0] u_i, then per level (value parts, then dual parts) dU/dx_i (3), 1/2 sum e2 per end species (4),
// d u_i / d sigma[a, :] (4), the class sums of (cos - cos0)^2 g g (10)
constexpr int SWM_NOUT = 3 + 2 * SWM_SMAX + SWM_NCLS;      // 21

template <class T, int LEVEL>
__device__ __forceinline__ void swm_atom(const SwmArgs& A, const SwmView& V, int i, int a, int sub, float (&out)[1 + 2 * SWM_NOUT]) {
    const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
    float wxi = 0.f, wyi = 0.f, wzi = 0.f;
    if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
    const T zero = mk<T>(0.f, 0.f);
    T gx = zero, gy = zero, gz = zero;                       // dU/dx_i
    float u = 0.f;                                           // u_i, added term by term in slot order: the sum does not
                                                             // depend on how the species are numbered
    T S2[SWM_SMAX], S2s[SWM_SMAX], S3s[SWM_SMAX], S3[SWM_NCLS];
#pragma unroll
    for (int q = 0; q < SWM_SMAX; ++q) { S2[q] = zero; S2s[q] = zero; S3s[q] = zero; }
#pragma unroll
    for (int q = 0; q < SWM_NCLS; ++q) S3[q] = zero;
    const int n = min(A.cnt[i], A.max_nbr);
    const size_t row = (size_t)i * A.max_nbr;
    for (int s = sub; s < n; s += SWM_LPA) {
        const int j = A.col[row + s];
        if ((unsigned)j >= (unsigned)A.N) continue;
        const int b = V.species(j);
        const SwmPairE& Pab = V.pair(a, b);
        const SwmPairE& Pba = V.pair(b, a);
        float dx = xi - A.pos[3 * j], dy = yi - A.pos[3 * j + 1], dz = zi - A.pos[3 * j + 2];
        apply_shift(A.cell, A.shift[row + s], dx, dy, dz);                  // x_i - x_j - o.h
        float wxj = 0.f, wyj = 0.f, wzj = 0.f;
        if (LEVEL >= 2) { wxj = A.w[3 * j]; wyj = A.w[3 * j + 1]; wzj = A.w[3 * j + 2]; }
        SwmEdge<T> ej;                                                      // centre i -> end j; inv and g of (a, b)
        if (!swm_geo<T>(fmaxf(Pab.rc, Pba.rc), -dx, -dy, -dz, wxj - wxi, wyj - wyi, wzj - wzi, ej)) continue;
        const bool in_ab = val(ej.r) < Pab.rc, in_ba = val(ej.r) < Pba.rc;
        T du_ab = zero, du_ba = zero;
        if (in_ab) {
            swm_tail<T>(Pab, ej);
            // ---- the pair (i, j) as a bond of the centre i: energy and parameter terms of phi2_ab / 2
            T e2, e2s = zero;
            swm_pair<T, LEVEL>(Pab, ej, e2, e2s, du_ab);
            u += 0.5f * (Pab.eps * val(e2));
            swm_add(S2, b, e2);
            if (LEVEL >= 1) swm_add(S2s, b, e2s);
            // ---- triplets centred on i: the ends j and k = later slots of row(i)
            const T q1 = ej.inv * ej.inv;
            T Xj = zero;                                                    // sum_k K t3
            for (int t = s + 1; t < n; ++t) {
                const int k = A.col[row + t];
                if ((unsigned)k >= (unsigned)A.N) continue;
                const int c = V.species(k);
                const SwmPairE& Pac = V.pair(a, c);
                float bx = xi - A.pos[3 * k], by = yi - A.pos[3 * k + 1], bz = zi - A.pos[3 * k + 2];
                apply_shift(A.cell, A.shift[row + t], bx, by, bz);
                float ax = 0.f, ay = 0.f, az = 0.f;
                if (LEVEL >= 2) { ax = A.w[3 * k] - wxi; ay = A.w[3 * k + 1] - wyi; az = A.w[3 * k + 2] - wzi; }
                SwmEdge<T> ek;
                if (!swm_edge<T>(Pac, -bx, -by, -bz, ax, ay, az, ek)) continue;
                const SwmTripE& Q = V.trip(a, b, c);
                const T cth = ej.ex * ek.ex + ej.ey * ek.ey + ej.ez * ek.ez;
                const T dc = cth - Q.cos0;
                const T gg = ej.g * ek.g;
                const T t3 = dc * dc * gg;
                u += Q.K * val(t3);
                swm_add(S3, swm_cls(b, c), t3);
                if (LEVEL >= 1) {
                    const T q2 = ek.inv * ek.inv;
                    const T kt = Q.K * t3;
                    // d g_ab / d sigma_ab = g_ab gamma_ab r / (r - rc_ab)^2: the end j after the loop, the end k here
                    Xj = Xj + kt;
                    swm_add(S3s, c, Pac.gamma * (kt * (ek.r * q2)));
                    // G1 = d phi3 / d x_j = pre [t1 e_k + (s1 - t1 c) e_j],  t1 = 2 / r_ij,  s1 = -gamma sigma dc / (r_ij - rc)^2
                    const T pre = Q.K * (gg * dc);
                    const T t1 = 2.f * ej.ir, t2 = 2.f * ek.ir;
                    const T m1 = t1 * cth + Pab.gs * (dc * q1), m2 = t2 * cth + Pac.gs * (dc * q2);   // -(s - t c)
                    // d phi3 / d x_i = -(G1 + G2)
                    const T cj = pre * (m1 - t2), ck = pre * (m2 - t1);
                    gx = gx + (cj * ej.ex + ck * ek.ex); gy = gy + (cj * ej.ey + ck * ek.ey); gz = gz + (cj * ej.ez + ck * ek.ez);
                }
            }
            if (LEVEL >= 1) swm_add(S3s, b, Pab.gamma * (Xj * (ej.r * q1)));
        }
        if (LEVEL >= 1) {
            if (in_ba) {
                // ---- the same bond seen from the centre j: inv and g of (b, a)
                if (a != b || !in_ab) {
                    swm_tail<T>(Pba, ej);
                    T e2, e2s = zero;
                    swm_pair<T, LEVEL>(Pba, ej, e2, e2s, du_ba);
                } else {
                    du_ba = du_ab;                                          // (one species: the same entry)
                }
                // ---- triplets centred on j: the ends i and k = every entry of row(j) but i
                const int nj = min(A.cnt[j], A.max_nbr);
                const size_t rowj = (size_t)j * A.max_nbr;
                const float xj = A.pos[3 * j], yj = A.pos[3 * j + 1], zj = A.pos[3 * j + 2];
                const T q1 = ej.inv * ej.inv;
                const T t1 = 2.f * ej.ir;
                for (int t = 0; t < nj; ++t) {
                    const int k = A.col[rowj + t];
                    if (k == i || (unsigned)k >= (unsigned)A.N) continue;
                    const int c = V.species(k);
                    const SwmPairE& Pbc = V.pair(b, c);
                    float bx = xj - A.pos[3 * k], by = yj - A.pos[3 * k + 1], bz = zj - A.pos[3 * k + 2];
                    apply_shift(A.cell, A.shift[rowj + t], bx, by, bz);      // x_j - x_k - o.h
                    float ax = 0.f, ay = 0.f, az = 0.f;
                    if (LEVEL >= 2) { ax = A.w[3 * k] - wxj; ay = A.w[3 * k + 1] - wyj; az = A.w[3 * k + 2] - wzj; }
                    SwmEdge<T> ek;                                           // centre j -> end k
                    if (!swm_edge<T>(Pbc, -bx, -by, -bz, ax, ay, az, ek)) continue;
                    const SwmTripE& Q = V.trip(b, a, c);
                    // the unit vector j -> i is -ej.e
                    const T cth = zero - (ej.ex * ek.ex + ej.ey * ek.ey + ej.ez * ek.ez);
                    const T dc = cth - Q.cos0;
                    const T pre = Q.K * ((ej.g * ek.g) * dc);
                    const T m1 = t1 * cth + Pba.gs * (dc * q1);
                    // G1 = pre [t1 e_jk - m1 e_ji] = pre [t1 e_jk + m1 ej.e]
                    const T ca = pre * t1, cb = pre * m1;
                    gx = gx + (ca * ek.ex + cb * ej.ex); gy = gy + (ca * ek.ey + cb * ej.ey); gz = gz + (ca * ek.ez + cb * ej.ez);
                }
            }
            // ---- the pair force: the derivative of (phi2_ab + phi2_ba) / 2;  d r / d x_i = -e
            const T du = 0.5f * (du_ab + du_ba);
            gx = gx + du * ej.ex; gy = gy + du * ej.ey; gz = gz + du * ej.ez;
        }
    }
    // the parameter derivatives of u_i = sum_b eps_ab S2[b] / 2 + sum_classes K S3
    T pe[SWM_SMAX], ps[SWM_SMAX];
#pragma unroll
    for (int q = 0; q < SWM_SMAX; ++q) {
        pe[q] = 0.5f * S2[q];
        ps[q] = zero;
        if (q < V.S) {
            if (LEVEL >= 1) ps[q] = V.pair(a, q).eps * (0.5f * S2s[q]) + S3s[q];
        }
    }
    out[0] = u;
    if (LEVEL >= 1) {
        out[1] = val(gx); out[2] = val(gy); out[3] = val(gz);
#pragma unroll
        for (int q = 0; q < SWM_SMAX; ++q) { out[4 + q] = val(pe[q]); out[4 + SWM_SMAX + q] = val(ps[q]); }
#pragma unroll
        for (int q = 0; q < SWM_NCLS; ++q) out[4 + 2 * SWM_SMAX + q] = val(S3[q]);
        if (LEVEL >= 2) {
            constexpr int D = SWM_NOUT;
            out[D + 1] = dual_part(gx); out[D + 2] = dual_part(gy); out[D + 3] = dual_part(gz);
#pragma unroll
            for (int q = 0; q < SWM_SMAX; ++q) { out[D + 4 + q] = dual_part(pe[q]); out[D + 4 + SWM_SMAX + q] = dual_part(ps[q]); }
#pragma unroll
            for (int q = 0; q < SWM_NCLS; ++q) out[D + 4 + 2 * SWM_SMAX + q] = dual_part(S3[q]);
        }
    }
}

// row i of a per-atom parameter table [N, 2 S S + S S S] from the group's sums v = (pe[4], ps[4], class sums[10]): the lanes of
// the group zero the entries of the other species' blocks, lane 0 writes eps[a, :], sigma[a, :], lam[a, :, :]
__device__ __forceinline__ void swm_store_theta(const SwmView& V, float* dst, int i, int a, int sub, const float* v) {
    const int S = V.S, S2 = S * S, P = 2 * S2 + S2 * S;
    float* r = dst + (size_t)i * P;
    for (int k = sub; k < P; k += SWM_LPA) {
        const int owner = k < 2 * S2 ? (k < S2 ? k : k - S2) / S : (k - 2 * S2) / S2;
        if (owner != a) r[k] = 0.f;
    }
    if (sub != 0) return;
#pragma unroll
    for (int q = 0; q < SWM_SMAX; ++q) {
        if (q < S) { r[a * S + q] = v[q]; r[S2 + a * S + q] = v[SWM_SMAX + q]; }
    }
    float* l = r + 2 * S2 + a * S2;
#pragma unroll
    for (int bb = 0; bb < SWM_SMAX; ++bb) {
#pragma unroll
        for (int cc = bb; cc < SWM_SMAX; ++cc) {
            if (cc < S) {
                const float t = v[2 * SWM_SMAX + swm_cls(bb, cc)];
                l[bb * S + cc] = V.trip(a, bb, cc).w * t;
                if (cc != bb) l[cc * S + bb] = V.trip(a, cc, bb).w * t;
            }
        }
    }
}

// LEVEL 0: U        1: + grad, pth        2: + hw, pthw
template <int LEVEL>
__global__ void __launch_bounds__(SWM_BLOCK) sw_multi_kernel(const SwmArgs A) {
    __shared__ float red[17];
    __shared__ float tab[SWM_TABLE_MAX];
    {
        const int S = A.S, nt = SWM_PAIR * S * S + SWM_TRIP * S * S * S;
        for (int k = threadIdx.x; k < nt; k += SWM_BLOCK) tab[k] = A.tables[k];
        __syncthreads();
    }
    const SwmView V{A.types, A.S, tab};
    constexpr int apb = SWM_BLOCK / SWM_LPA;
    const int i = blockIdx.x * apb + threadIdx.x / SWM_LPA, sub = threadIdx.x % SWM_LPA;
    float e = 0.f;
    if (i < A.N) {
        const int a = V.species(i);
        float o[1 + 2 * SWM_NOUT];
#pragma unroll
        for (int k = 0; k < 1 + 2 * SWM_NOUT; ++k) o[k] = 0.f;
        if (LEVEL >= 2) swm_atom<Dual, LEVEL>(A, V, i, a, sub, o);
        else swm_atom<float, LEVEL>(A, V, i, a, sub, o);
        constexpr int NV = LEVEL >= 2 ? 1 + 2 * SWM_NOUT : (LEVEL >= 1 ? 1 + SWM_NOUT : 1);
#pragma unroll
        for (int k = 0; k < NV; ++k) o[k] = group_sum<SWM_LPA>(o[k]);
        if (LEVEL >= 1 && A.pth) swm_store_theta(V, A.pth, i, a, sub, o + 4);
        if (LEVEL >= 2 && A.pthw) swm_store_theta(V, A.pthw, i, a, sub, o + SWM_NOUT + 4);
        if (sub == 0) {
            e = o[0];
            if (LEVEL >= 1 && A.grad) store3(A.grad, i, A.oscale, A.oacc, o[1], o[2], o[3]);
            if (LEVEL >= 2 && A.hw) store3(A.hw, i, A.oscale, A.oacc, o[SWM_NOUT + 1], o[SWM_NOUT + 2], o[SWM_NOUT + 3]);
        }
    }
    if (A.partial) {                         // (block-uniform: a force-only evaluation has no scalar to reduce)
        e = block_sum(e, red);
        if (threadIdx.x == 0) A.partial[blockIdx.x] = e;
    }
}

}  // namespace

extern "C" int64_t mdg_sw_multi_partial_size(int n_atoms) { return atom_blocks(n_atoms, SWM_LPA, SWM_BLOCK); }

extern "C" int64_t mdg_sw_multi_table_size(int n_species) {
    if (n_species < 1 || n_species > SWM_SMAX) return 0;
    const int64_t S = n_species;
    return SWM_PAIR * S * S + SWM_TRIP * S * S * S;
}

extern "C" int mdg_sw_multi_eval(const float* pos, int n_atoms, const MdgCell* cell, const int32_t* col, const int32_t* shift,
                                 const int32_t* cnt, int max_nbr, const int32_t* types, int n_species, const float* tables,
                                 const float* w, float* energy, float* grad, float* hw, float* pth, float* pthw, float* partial,
                                 float out_scale, int accumulate, void* stream) {
    MDG_CHECK_ARG(pos && cell && col && shift && cnt, "sw_multi_eval: null buffer (pos, cell or list)");
    MDG_CHECK_ARG(n_atoms > 0 && max_nbr > 0, "sw_multi_eval: bad sizes (n_atoms, max_nbr must be positive)");
    MDG_CHECK_ARG(n_species >= 1 && n_species <= SWM_SMAX, "sw_multi_eval: n_species must lie in [1, %d] (got %d)", SWM_SMAX,
                  n_species);
    MDG_CHECK_ARG(types, "sw_multi_eval: types is null (device int32 [n_atoms])");
    MDG_CHECK_ARG(tables, "sw_multi_eval: tables is null (device float [mdg_sw_multi_table_size(n_species)])");
    MDG_CHECK_ARG(w || !(hw || pthw), "sw_multi_eval: hw / pthw need w");
    MDG_CHECK_ARG(!w || hw || pthw, "sw_multi_eval: w given without hw or pthw output");
    MDG_CHECK_ARG(energy || grad || hw || pth || pthw, "sw_multi_eval: no output requested");
    MDG_CHECK_ARG(!energy || partial, "sw_multi_eval: energy needs the partial buffer");
    const int level = w ? 2 : ((grad || pth) ? 1 : 0);
    // (accumulate bit 2, "the list was searched with a skin", needs nothing here: every entry's own support test is always applied)
    SwmArgs a{pos, n_atoms, *cell, col, shift, cnt, max_nbr, types, n_species, tables, w,
              grad, hw, pth, pthw, energy ? partial : nullptr, out_scale, accumulate & 1};
    const int nblocks = (int)mdg_sw_multi_partial_size(n_atoms);
    dim3 grid(nblocks);
    hipStream_t st = (hipStream_t)stream;
    with_level(level, [&](auto L) { hipLaunchKernelGGL((sw_multi_kernel<decltype(L)::value>), grid, dim3(SWM_BLOCK), 0, st, a); });
    if (energy) hipLaunchKernelGGL(energy_finish, dim3(1), dim3(64), 0, st, partial, nblocks, energy);
    MDG_CHECK_LAUNCH("sw_multi_kernel");
    return MDG_OK;
}
