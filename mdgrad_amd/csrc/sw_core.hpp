// The Stillinger-Weber two- plus three-body potential over the per-atom (ELL) list, written once for the one-species kernels
// (K23, csrc/sw.hip) and the kernels for up to four species (K28, csrc/sw_multi.hip); its entry layout, edge and pair term
// also serve the list-free frame-energy kernel (K34, csrc/sw_frames.hip).  Stillinger and Weber 1985, Molinero and Moore 2009
// for mW water; the LAMMPS `pair_style sw` convention.  With a = t_i (the centre), b = t_j, c = t_k the species of the atoms:
//
//   U        = 1/2 sum_i sum_{j != i} phi2_ab(r_ij) + sum_i sum_{j<k in row(i)} phi3_abc(r_ij, r_ik, cos theta_jik)
//   phi2_ab  = A_ab eps_ab [B_ab (sigma_ab/r)^p_ab - (sigma_ab/r)^q_ab] exp(sigma_ab / (r - rc_ab))    r < rc_ab = a_ab sigma_ab
//   g_ab     = exp(gamma_ab sigma_ab / (r - rc_ab))                                                    r < rc_ab, else exactly 0
//   phi3_abc = K_a{bc} (cos theta - cos0_abc)^2 g_ab(r_ij) g_ac(r_ik),   K_a{bc} = (lam_abc eps3_abc + lam_acb eps3_acb) / 2
//
// Laid out like coulomb_ell_kernel (csrc/coulomb.hip): SW_LPA lanes walk one atom's row, wave shuffles combine the per-atom
// sums, the energy goes through a fixed-order block partial and a finish kernel.  No float atomics => bitwise reproducible.
//
// Atom-centric gather, one writer per output word.  The lane that holds slot s of row(i) (neighbour j) adds
//   - the pair (i, j),
//   - the triplets centred on i with the ends j and k = every later slot of row(i)   (centre part of dU/dx_i),
//   - the triplets centred on j with the ends i and k = every entry of row(j) but i  (end part of dU/dx_i; x_k - x_j is taken
//     with j's own stored image).
// Rows are read from global memory where they are needed (they are short and stay in L1/L2): nothing is staged, so there is no
// row cap.  r - rc is formed from r = sqrtf(d2), the exponentials are expf; every entry's own support test 0 < r < rc is always
// applied, so a list searched with a larger radius (a skin, or a cutoff kept while sigma shrank) is exact.
//
// LEVEL 2 runs the same code on Dual numbers seeded with w: x + t w gives dU/dx + t H w in one pass, and the per-atom
// parameter terms carry d(w . grad)(d u_i / d theta) in their dual parts.  No fused multiply-adds are formed by the compiler
// in a file that includes this one (the pragma below reaches the rest of the translation unit): the float and the Dual
// instantiation round the value parts identically, so dU/dx of a LEVEL 1 launch equals that of a LEVEL 2 launch bit for bit,
// and K34 rounds an edge as the list kernels do.
//
// Every constant is read through a parameter view V, two kinds of entry:
//   pair entry    (a, b)    = eps, sigma, a sigma, gamma sigma, gamma, A, B, p, q, a, A eps, 0        a = centre, b = end
//   triplet entry (a, b, c) = K_a{bc}, cos0_abc, w_abc, 0                                             a = centre, b, c = ends
// The pairs are ordered: (a, b) and (b, a) are separate entries and may differ, also in their supports.  V answers
//   v.species(i)                      the species of atom i, inside [0, v.S)
//   v.pair(a, b), v.trip(a, b, c)     the entries (const SwPairE&, const SwTripE&)
//   v.p(P), v.q(P)                    the integer exponents of the pair entry P
//   V::SMAX, v.S                      the species capacity and count; SMAX sizes the per-lane accumulators: SMAX each for
//                                     sum e2, sum d e2 / d sigma, the sigma terms of the triplets (per end species) and
//                                     SMAX (SMAX + 1) / 2 for the sums of (cos - cos0)^2 g g (per unordered pair of end species)
//   v.store_theta(dst, i, a, sub, s)  row i of a per-atom parameter table from the group's sums s = (1/2 sum e2 [SMAX],
//                                     d u_i / d sigma[a, :] [SMAX], the class sums [SMAX (SMAX + 1) / 2]); every lane of the
//                                     group calls it
// and nothing else; csrc/sw.hip holds the view of one species (one entry of each kind in registers, from the kernel
// arguments), csrc/sw_multi.hip the view of a table in LDS.
//
// Which entry is read where, for the lane on slot s of row(i); atom i has the species a, the end j the species b:
//   the edge i -> j:                          built once, cut at max(rc_ab, rc_ba); inside (a, b) and inside (b, a) are
//                                             tested apart: with rc_ab != rc_ba one directed bond can exist without the other
//   the pair as a bond of the centre i:       pair (a, b): u_i += eps_ab e2 / 2, sum e2 [b], sum d e2 / d sigma [b]
//   a triplet (j, i, k), k a later slot:      pair (a, b) for g and 1/(r - rc) of j, pair (a, c) for those of k, triplet
//                                             (a, b, c) for K and cos0; u_i += K t3; class sum [{b, c}]; the sigma terms to [c]
//                                             in the loop and to [b] after it
//   the bond seen from the centre j:          pair (b, a) for g, 1/(r - rc) and the second pair term (the first one again
//                                             where a = b and the bond lies inside (a, b))
//   a triplet (i, j, k), k in row(j):         pair (b, a) for the edge j -> i, pair (b, c) for j -> k, triplet (b, a, c)
//   the pair force:                           1/2 (du_ab + du_ba), added after the triplets
// u_i is added term by term in slot order, so it does not depend on how the species are numbered.  With a species capacity
// of 1 the view returns the same entry for both directions and a constant species: the second support test, the second pair
// term and the predicated accumulator updates fold away at compile time.
#pragma once
#pragma clang fp contract(off)                // (also set by the including files, ahead of dual.hpp; here for this file's sake)
#include <type_traits>
#include "dual.hpp"
#include "manybody.hpp"

namespace {

constexpr int SW_LPA = 16;                    // lanes per atom (rows hold 4 - 20 neighbours)
constexpr int SW_BLOCK = 256;
constexpr int SW_PAIR = 12, SW_TRIP = 4;      // floats per entry

struct SwPairE { float eps, sigma, rc, gs, gamma, A, B, fp, fq, a, Ae, pad; };
struct SwTripE { float K, cos0, w, pad; };

// what both entry points hand to the kernel beside their constants: positions, list, seed and outputs
struct SwIO {
    const float* pos; int N; MdgCell cell;
    const int32_t* col; const int32_t* shift; const int32_t* cnt; int max_nbr;
    const float* w;
    float* grad; float* hw; float* pth; float* pthw; float* partial;
    float oscale; int oacc;
};

// the class of the unordered pair of end species {b, c}; SMAX = 4: (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)
template <int SMAX> __device__ __forceinline__ constexpr int sw_cls(int b, int c) {
    const int lo = b < c ? b : c, hi = b < c ? c : b;
    return lo * (2 * SMAX + 1 - lo) / 2 + (hi - lo);
}

template <class T> __device__ __forceinline__ T sw_pow(T x, int n) {
    T r = mk<T>(1.f, 0.f);
    while (n > 0) { if (n & 1) r = r * x; x = x * x; n >>= 1; }
    return r;
}

// one list entry seen from its centre: unit vector centre -> end, r, 1/r (the geometry), then 1/(r - rc) and g of a pair entry
template <class T> struct SwEdge { T ex, ey, ez, r, ir, inv, g; };

// (dx, dy, dz) = end - centre with the stored image applied, (ax, ay, az) = w_end - w_centre.  False for r = 0 or r >= rmax.
template <class T>
__device__ __forceinline__ bool sw_geo(float rmax, float dx, float dy, float dz, float ax, float ay, float az, SwEdge<T>& e) {
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
__device__ __forceinline__ void sw_tail(const SwPairE& P, SwEdge<T>& e) {
    const T one = mk<T>(1.f, 0.f);
    e.inv = one / (e.r - P.rc);
    e.g = fexp_(P.gs * e.inv);
}
template <class T>
__device__ __forceinline__ bool sw_edge(const SwPairE& P, float dx, float dy, float dz, float ax, float ay, float az, SwEdge<T>& e) {
    if (!sw_geo<T>(P.rc, dx, dy, dz, ax, ay, az, e)) return false;
    sw_tail<T>(P, e);
    return true;
}

// the pair term of the entry P (exponents p, q) on an edge inside its support (e.inv of P): e2 = phi2 / eps = A [B s^p - s^q] E
// with E = exp(sigma / (r - rc)), d e2 / d sigma, and du = -phi2'
template <class T, int LEVEL>
__device__ __forceinline__ void sw_pair(const SwPairE& P, int p, int q, const SwEdge<T>& e, T& e2, T& e2s, T& du) {
    const T sr = P.sigma * e.ir;
    const T sp = sw_pow(sr, p), sq = sw_pow(sr, q);
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
__device__ __forceinline__ void sw_add(T (&acc)[NQ], int idx, const T& x) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        if (q == idx) acc[q] = acc[q] + x;
}

// per level (value parts, then dual parts): dU/dx_i (3), 1/2 sum e2 per end species, d u_i / d sigma[a, :], the class sums of
// (cos - cos0)^2 g g; out[0] is u_i
template <int SMAX> constexpr int sw_nout() { return 3 + 2 * SMAX + SMAX * (SMAX + 1) / 2; }

template <class T, int LEVEL, class View>
__device__ __forceinline__ void sw_atom(const SwIO& A, const View& V, int i, int a, int sub,
                                        float (&out)[1 + 2 * sw_nout<View::SMAX>()]) {
    constexpr int SMAX = View::SMAX, NCLS = SMAX * (SMAX + 1) / 2;
    const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
    float wxi = 0.f, wyi = 0.f, wzi = 0.f;
    if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
    const T zero = mk<T>(0.f, 0.f);
    T gx = zero, gy = zero, gz = zero;                       // dU/dx_i
    float u = 0.f;                                           // u_i, added term by term in slot order
    T S2[SMAX], S2s[SMAX], S3s[SMAX], S3[NCLS];
#pragma unroll
    for (int q = 0; q < SMAX; ++q) { S2[q] = zero; S2s[q] = zero; S3s[q] = zero; }
#pragma unroll
    for (int q = 0; q < NCLS; ++q) S3[q] = zero;
    const int n = min(A.cnt[i], A.max_nbr);
    const size_t row = (size_t)i * A.max_nbr;
    for (int s = sub; s < n; s += SW_LPA) {
        const int j = A.col[row + s];
        if ((unsigned)j >= (unsigned)A.N) continue;
        const int b = V.species(j);
        const SwPairE& Pab = V.pair(a, b);
        const SwPairE& Pba = V.pair(b, a);
        float dx = xi - A.pos[3 * j], dy = yi - A.pos[3 * j + 1], dz = zi - A.pos[3 * j + 2];
        apply_shift(A.cell, A.shift[row + s], dx, dy, dz);                  // x_i - x_j - o.h
        float wxj = 0.f, wyj = 0.f, wzj = 0.f;
        if (LEVEL >= 2) { wxj = A.w[3 * j]; wyj = A.w[3 * j + 1]; wzj = A.w[3 * j + 2]; }
        SwEdge<T> ej;                                                       // centre i -> end j; inv and g of (a, b)
        const float rmax = SMAX > 1 ? fmaxf(Pab.rc, Pba.rc) : Pab.rc;
        if (!sw_geo<T>(rmax, -dx, -dy, -dz, wxj - wxi, wyj - wyi, wzj - wzi, ej)) continue;
        const bool in_ab = val(ej.r) < Pab.rc, in_ba = SMAX > 1 ? val(ej.r) < Pba.rc : in_ab;
        T du_ab = zero, du_ba = zero;
        if (in_ab) {
            sw_tail<T>(Pab, ej);
            // ---- the pair (i, j) as a bond of the centre i: energy and parameter terms of phi2_ab / 2
            T e2, e2s = zero;
            sw_pair<T, LEVEL>(Pab, V.p(Pab), V.q(Pab), ej, e2, e2s, du_ab);
            u += 0.5f * (Pab.eps * val(e2));
            sw_add(S2, b, e2);
            if (LEVEL >= 1) sw_add(S2s, b, e2s);
            // ---- triplets centred on i: the ends j and k = later slots of row(i)
            const T q1 = ej.inv * ej.inv;
            T Xj = zero;                                                    // sum_k K t3
            for (int t = s + 1; t < n; ++t) {
                const int k = A.col[row + t];
                if ((unsigned)k >= (unsigned)A.N) continue;
                const int c = V.species(k);
                const SwPairE& Pac = V.pair(a, c);
                float bx = xi - A.pos[3 * k], by = yi - A.pos[3 * k + 1], bz = zi - A.pos[3 * k + 2];
                apply_shift(A.cell, A.shift[row + t], bx, by, bz);
                float ax = 0.f, ay = 0.f, az = 0.f;
                if (LEVEL >= 2) { ax = A.w[3 * k] - wxi; ay = A.w[3 * k + 1] - wyi; az = A.w[3 * k + 2] - wzi; }
                SwEdge<T> ek;
                if (!sw_edge<T>(Pac, -bx, -by, -bz, ax, ay, az, ek)) continue;
                const SwTripE& Q = V.trip(a, b, c);
                const T cth = ej.ex * ek.ex + ej.ey * ek.ey + ej.ez * ek.ez;
                const T dc = cth - Q.cos0;
                const T gg = ej.g * ek.g;
                const T t3 = dc * dc * gg;
                u += Q.K * val(t3);
                sw_add(S3, sw_cls<SMAX>(b, c), t3);
                if (LEVEL >= 1) {
                    const T q2 = ek.inv * ek.inv;
                    const T kt = Q.K * t3;
                    // d g_ab / d sigma_ab = g_ab gamma_ab r / (r - rc_ab)^2: the end j after the loop, the end k here
                    Xj = Xj + kt;
                    sw_add(S3s, c, Pac.gamma * (kt * (ek.r * q2)));
                    // G1 = d phi3 / d x_j = pre [t1 e_k + (s1 - t1 c) e_j],  t1 = 2 / r_ij,  s1 = -gamma sigma dc / (r_ij - rc)^2
                    const T pre = Q.K * (gg * dc);
                    const T t1 = 2.f * ej.ir, t2 = 2.f * ek.ir;
                    const T m1 = t1 * cth + Pab.gs * (dc * q1), m2 = t2 * cth + Pac.gs * (dc * q2);   // -(s - t c)
                    // d phi3 / d x_i = -(G1 + G2)
                    const T cj = pre * (m1 - t2), ck = pre * (m2 - t1);
                    gx = gx + (cj * ej.ex + ck * ek.ex); gy = gy + (cj * ej.ey + ck * ek.ey); gz = gz + (cj * ej.ez + ck * ek.ez);
                }
            }
            if (LEVEL >= 1) sw_add(S3s, b, Pab.gamma * (Xj * (ej.r * q1)));
        }
        if (LEVEL >= 1) {
            if (in_ba) {
                // ---- the same bond seen from the centre j: inv and g of (b, a)
                if (a != b || !in_ab) {
                    sw_tail<T>(Pba, ej);
                    T e2, e2s = zero;
                    sw_pair<T, LEVEL>(Pba, V.p(Pba), V.q(Pba), ej, e2, e2s, du_ba);
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
                    const SwPairE& Pbc = V.pair(b, c);
                    float bx = xj - A.pos[3 * k], by = yj - A.pos[3 * k + 1], bz = zj - A.pos[3 * k + 2];
                    apply_shift(A.cell, A.shift[rowj + t], bx, by, bz);      // x_j - x_k - o.h
                    float ax = 0.f, ay = 0.f, az = 0.f;
                    if (LEVEL >= 2) { ax = A.w[3 * k] - wxj; ay = A.w[3 * k + 1] - wyj; az = A.w[3 * k + 2] - wzj; }
                    SwEdge<T> ek;                                            // centre j -> end k
                    if (!sw_edge<T>(Pbc, -bx, -by, -bz, ax, ay, az, ek)) continue;
                    const SwTripE& Q = V.trip(b, a, c);
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
    T pe[SMAX], ps[SMAX];
#pragma unroll
    for (int q = 0; q < SMAX; ++q) {
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
        for (int q = 0; q < SMAX; ++q) { out[4 + q] = val(pe[q]); out[4 + SMAX + q] = val(ps[q]); }
#pragma unroll
        for (int q = 0; q < NCLS; ++q) out[4 + 2 * SMAX + q] = val(S3[q]);
        if (LEVEL >= 2) {
            constexpr int D = sw_nout<SMAX>();
            out[D + 1] = dual_part(gx); out[D + 2] = dual_part(gy); out[D + 3] = dual_part(gz);
#pragma unroll
            for (int q = 0; q < SMAX; ++q) { out[D + 4 + q] = dual_part(pe[q]); out[D + 4 + SMAX + q] = dual_part(ps[q]); }
#pragma unroll
            for (int q = 0; q < NCLS; ++q) out[D + 4 + 2 * SMAX + q] = dual_part(S3[q]);
        }
    }
}

// LEVEL 0: U        1: + grad, pth        2: + hw, pthw
template <class View, int LEVEL>
__global__ void __launch_bounds__(SW_BLOCK) sw_kernel(const SwIO A, const typename View::Args VA) {
    using T = typename std::conditional<LEVEL >= 2, Dual, float>::type;
    __shared__ float red[17];
    const View V(VA);                        // (every thread of the block: the table view stages and synchronises here)
    constexpr int apb = SW_BLOCK / SW_LPA, NOUT = sw_nout<View::SMAX>();
    const int i = blockIdx.x * apb + threadIdx.x / SW_LPA, sub = threadIdx.x % SW_LPA;
    float e = 0.f;
    if (i < A.N) {
        const int a = V.species(i);
        float o[1 + 2 * NOUT];
#pragma unroll
        for (int k = 0; k < 1 + 2 * NOUT; ++k) o[k] = 0.f;
        sw_atom<T, LEVEL>(A, V, i, a, sub, o);
        constexpr int NV = LEVEL >= 2 ? 1 + 2 * NOUT : (LEVEL >= 1 ? 1 + NOUT : 1);
#pragma unroll
        for (int k = 0; k < NV; ++k) o[k] = group_sum<SW_LPA>(o[k]);
        if (LEVEL >= 1 && A.pth) V.store_theta(A.pth, i, a, sub, o + 4);
        if (LEVEL >= 2 && A.pthw) V.store_theta(A.pthw, i, a, sub, o + NOUT + 4);
        if (sub == 0) {
            e = o[0];
            if (LEVEL >= 1 && A.grad) store3(A.grad, i, A.oscale, A.oacc, o[1], o[2], o[3]);
            if (LEVEL >= 2 && A.hw) store3(A.hw, i, A.oscale, A.oacc, o[NOUT + 1], o[NOUT + 2], o[NOUT + 3]);
        }
    }
    if (A.partial) {                         // (block-uniform: a force-only evaluation has no scalar to reduce)
        e = block_sum(e, red);
        if (threadIdx.x == 0) A.partial[blockIdx.x] = e;
    }
}

// the kernel and the energy for the view; `level` as the entry points derive it from the requested outputs
template <class View>
inline void sw_launch(const SwIO& a, const typename View::Args& v, int level, float* energy, float* partial, hipStream_t st) {
    const int nblocks = (int)atom_blocks(a.N, SW_LPA, SW_BLOCK);
    with_level(level, [&](auto L) {
        hipLaunchKernelGGL((sw_kernel<View, decltype(L)::value>), dim3(nblocks), dim3(SW_BLOCK), 0, st, a, v);
    });
    if (energy) hipLaunchKernelGGL(energy_finish, dim3(1), dim3(64), 0, st, partial, nblocks, energy);
}

}  // namespace
