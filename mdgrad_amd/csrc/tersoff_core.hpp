// The Tersoff bond-order potential over the per-atom (ELL) list, written once for the one-species kernels (K25,
// csrc/tersoff.hip) and the kernels for up to four species (K26, csrc/tersoff_multi.hip); Tersoff 1988 for silicon, 1989 for
// carbon and for multicomponent systems; the LAMMPS convention.  With a = t_i, b = t_j, c = t_k the species of the atoms:
//
//   U       = 1/2 sum_i sum_{j in row(i)} fc_ab(r_ij) [ A_ab exp(-lam1_ab r_ij) - b_ij B_ab exp(-lam2_ab r_ij) ]
//   b_ij    = (1 + (beta_a zeta_ij)^n_a)^(-1/(2 n_a))
//   zeta_ij = sum_{k in row(i), k != j} fc_ac(r_ik) g_a(cos theta_jik) exp[(lam3 (r_ij - r_ik))^m]       m = 1 or 3
//   g_a(x)  = gamma_a (1 + c_a^2/d_a^2 - c_a^2/(d_a^2 + (h_a - x)^2))
//   fc_ab   = 1 for r <= R_ab - D_ab;  1/2 - 1/2 sin(pi (r - R_ab) / (2 D_ab)) inside the taper;  exactly 0 for r >= R_ab + D_ab
// (the exponential in zeta: only where the parameter view has HAS_LAM3, see below).
//
// The strength of the bond i -> j depends on zeta_ij, a sum over row(i), and the force on an atom needs dU/dzeta of the bonds
// of its neighbours: two passes, as in csrc/eam.hip, with the intermediate stored per directed bond (list slot), not per atom.
//   1. bond pass:   the lane on slot s of row(i) (neighbour j) forms zeta_is by a loop over row(i), then b and b', adds the
//                   bond's half energy and the per-atom parameter terms d u_i / d(A, B, h), and stores
//                   bond_work[row(i) + s] = (P, dP, b, db),  P = dU/dzeta_is = -1/2 fc(r_ij) B exp(-lam2 r_ij) b'(zeta_is)
//                   (dP, db: the dual parts under LEVEL 2, else 0).  An energy-only call runs this pass alone.
//   2. force pass:  atom-centric gather, one writer per output word.  The lane on slot s of row(i) adds to dU/dx_i
//                   - the pair parts of the bonds i -> j and j -> i (b_ji from i's slot in row(j)),
//                   - P_ij dzeta_ij/dx_i                                       (a loop over row(i)),
//                   - P_ji dzeta_ji/dx_i, i being the end of the bond j -> i,  (one loop over row(j) ...
//                   - P_jk dzeta_jk/dx_i for every other k of row(j), i being the third atom       ... for both).
// Both are laid out like sw_kernel (csrc/sw_core.hpp): LPA lanes walk one atom's row, wave shuffles combine the per-atom sums,
// the energy goes through a fixed-order block partial and a finish kernel.  No float atomics => bitwise reproducible.  Rows
// are read from global memory where they are needed, nothing is staged, so there is no row cap; the cost is O(n^2) per atom.
// The support test 0 < r < R + D of an entry is applied on r = sqrtf(d2) with that entry's own pair constants, so the list may
// have been searched with any radius >= max_ab (R_ab + D_ab) (a skin).  A slot inside cnt that fails the test gets
// (0, 0, 0, 0) in bond_work, so the force pass never reads an unwritten word.
//
// g is evaluated as gamma (1 + (c/d)^2 u^2 / (d^2 + u^2)), u = h - cos theta: the same function without the difference of
// c^2/d^2 (3.8e7 for silicon) and c^2/(d^2 + u^2) that the published form takes.
// A bond with zeta = 0 (no third atom inside the cutoff) has b = 1 and b' = b'' = 0 by definition; (beta zeta)^n is never
// formed there (for n < 1 its derivative diverges at 0).
//
// LEVEL 2 runs the same code on Dual numbers seeded with w: x + t w gives dU/dx + t H w, and the per-atom parameter terms carry
// d(w . grad)(d u_i / d theta) in their dual parts.  No fused multiply-adds are formed by the compiler in this file: the float
// and the Dual instantiation round the value parts identically, so dU/dx of a LEVEL 1 launch equals that of a LEVEL 2 launch bit
// for bit.
//
// Every constant is read through a parameter view P, two entries of eight derived constants each:
//   pair entry   (a, b) = A, B, lam1, lam2, R, R - D, R + D, pi / (2 D)                           a = centre, b = end
//   centre entry (a)    = h, beta, n, -1/(2n), d^2, gamma, gamma (c/d)^2, 2 gamma (c/d)^2 d^2
// The pairs are ordered: (a, b) and (b, a) are separate entries and may differ, also in their cutoffs.  P answers
//   p.species(i)                      the species of atom i, inside [0, p.S)
//   p.pair(a, b), p.centre(a)         the entries (const TersEntry&)
//   P::HAS_LAM3                       whether the exponential of zeta is compiled in; then p.lam3 and p.m hold its constants
//   P::SMAX, p.S                      the species capacity (sizes the per-atom accumulators pa[], pb[]) and count
//   p.store_theta(dst, i, a, va, vb, vh)   row i of a per-atom parameter table from d u_i / d(A[a, :], B[a, :], h[a])
// and nothing else; csrc/tersoff.hip holds the view of one species (constants in registers, from the kernel arguments),
// csrc/tersoff_multi.hip the view of a table in LDS.
//
// Which entry is read where.  Bond pass, atom i of species a on slot s (end j, species b):
//   the edge i -> j:                          pair (a, b)
//   a third atom k of row(i):                 pair (a, t_k) for its taper, centre a for g
//   b_ij and b'(zeta_ij):                     centre a
//   per-atom parameter terms:                 d u_i / dA[a, b], d u_i / dB[a, b], d u_i / dh[a]
// Force pass, the five contributions to dU/dx_i of the lane on slot s of row(i):
//   1. pair part of i -> j at fixed b_ij:                         pair (a, b)
//   2. P_ij dzeta_ij/dx_i (loop over row(i)):                     pair (a, b) for e_ij, pair (a, t_k) for k's taper, centre a
//   3. pair part of j -> i at fixed b_ji (b_ji from row(j)):      pair (b, a)
//   4. P_ji dzeta_ji/dx_i, i the end of the bond j -> i:          pair (b, a) for the edge j -> i, pair (b, t_k) for k's taper,
//                                                                 centre b
//   5. P_jk dzeta_jk/dx_i, i the third atom of the bond j -> k:   pair (b, t_k) for the edge j -> k, pair (b, a) for the taper
//                                                                 of i, centre b
// 1 and 2 need r_ij inside the support of (a, b); 3, 4, 5 need it inside the support of (b, a), which is tested on its own: with
// R_ab + D_ab != R_ba + D_ba one of the two directed bonds can exist without the other.  The edge is built once and cut at the
// larger of the two.  With a species capacity of 1 both entries are the same one: the reverse edge keeps the forward edge's taper.
#pragma once
#pragma clang fp contract(off)                // (also set by the including files, ahead of dual.hpp; here for this file's sake)
#include <type_traits>
#include "common.hpp"
#include "dual.hpp"
#include "manybody.hpp"

namespace {

constexpr int TERS_LPA = 16;                  // lanes per atom: taken over from sw_core.hpp (covalent rows hold 4 - 16 entries);
                                              // the choice has not been measured for these kernels
constexpr int TERS_BLOCK = 256;

struct TersEntry {
    float v[8];
    __device__ __forceinline__ float operator[](int k) const { return v[k]; }
};
// pair entry
constexpr int PA_A = 0, PA_B = 1, PA_L1 = 2, PA_L2 = 3, PA_R = 4, PA_RIN = 5, PA_RC = 6, PA_PD = 7;
// centre entry
constexpr int CE_H = 0, CE_BETA = 1, CE_N = 2, CE_MH = 3, CE_D2 = 4, CE_GAMMA = 5, CE_GCD = 6, CE_GU2 = 7;

// what both entry points hand to the kernels beside their constants: positions, list, seed, scratch and outputs
struct TersIO {
    const float* pos; int N; MdgCell cell;
    const int32_t* col; const int32_t* shift; const int32_t* cnt; int max_nbr;
    const float* w;
    float* work;                               // bond_work [N * max_nbr, 4]
    float* grad; float* hw; float* pth; float* pthw; float* partial;
    float oscale; int oacc;
};

// one list entry seen from its centre: unit vector centre -> end, r, 1/r, fc(r), fc'(r)
template <class T> struct TersEdge { T ex, ey, ez, r, ir, fc, dfc; };

// fc and fc' of the edge under the pair entry pp, from e.r.  False outside the support of that entry.
template <class T>
__device__ __forceinline__ bool ters_taper(const TersEntry& pp, TersEdge<T>& e) {
    const float rv = val(e.r);
    if (!(rv < pp[PA_RC])) return false;
    if (rv <= pp[PA_RIN]) {
        e.fc = mk<T>(1.f, 0.f); e.dfc = mk<T>(0.f, 0.f);
    } else {
        const float pd = pp[PA_PD];
        const T arg = pd * (e.r - pp[PA_R]);
        e.fc = 0.5f - 0.5f * fsin_(arg);
        e.dfc = (-0.5f * pd) * fcos_(arg);
    }
    return true;
}

// (dx, dy, dz) = end - centre with the stored image applied, (ax, ay, az) = w_end - w_centre.  Fills the geometry of e;
// false when r = 0 or r >= rmax (rmax: the largest cutoff the caller can still use)
template <class T>
__device__ __forceinline__ bool ters_geom(float dx, float dy, float dz, float ax, float ay, float az, float rmax, TersEdge<T>& e) {
    const T x = mk<T>(dx, ax), y = mk<T>(dy, ay), z = mk<T>(dz, az);
    const T d2 = x * x + y * y + z * z;
    const float rv = sqrtf(val(d2));
    if (!(rv > 0.f && rv < rmax)) return false;              // the support test, on the r that fc is formed from
    e.r = fsqrt_(d2);
    e.ir = mk<T>(1.f, 0.f) / e.r;
    e.ex = x * e.ir; e.ey = y * e.ir; e.ez = z * e.ir;
    return true;
}

// the entry in slot s of the row of a centre of species tc as an edge centre -> end under the pair entry (tc, t_end);
// returns the end atom, or -1 when there is nothing to add
template <class T, int LEVEL, class P>
__device__ __forceinline__ int ters_entry(const TersIO& A, const P& p, int tc, size_t row, int s, float xc, float yc, float zc,
                                          float wxc, float wyc, float wzc, TersEdge<T>& e) {
    const int j = A.col[row + s];
    if ((unsigned)j >= (unsigned)A.N) return -1;
    float dx = xc - A.pos[3 * j], dy = yc - A.pos[3 * j + 1], dz = zc - A.pos[3 * j + 2];
    apply_shift(A.cell, A.shift[row + s], dx, dy, dz);                      // x_c - x_j - o.h
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (LEVEL >= 2) { ax = A.w[3 * j] - wxc; ay = A.w[3 * j + 1] - wyc; az = A.w[3 * j + 2] - wzc; }
    const TersEntry& pp = p.pair(tc, p.species(j));
    if (!ters_geom<T>(-dx, -dy, -dz, ax, ay, az, pp[PA_RC], e)) return -1;
    return ters_taper<T>(pp, e) ? j : -1;
}

// One third atom k of the bond centre -> j:  t = fc(r_k) g(cos) E,  E = exp[(lam3 (r_j - r_k))^m] (1 without HAS_LAM3),
// th = dt/dh, and the derivatives with respect to the two vectors d_j, d_k (end - centre) as coefficients of the unit vectors:
//   dt/dd_j = cjj e_j + cjk e_k,   dt/dd_k = ckj e_j + ckk e_k
// cc: the centre entry of the centre's species; ek.fc: the taper of the pair entry (centre, k)
template <class T> struct TersTerm { T t, th, cjj, cjk, ckj, ckk; };

template <class T, class P>
__device__ __forceinline__ TersTerm<T> ters_term(const P& p, const TersEntry& cc, const TersEdge<T>& ej, const TersEdge<T>& ek) {
    TersTerm<T> o;
    const T c = ej.ex * ek.ex + ej.ey * ek.ey + ej.ez * ek.ez;
    const T u = cc[CE_H] - c;
    const T u2 = u * u;
    const T iden = mk<T>(1.f, 0.f) / (u2 + cc[CE_D2]);
    const T g = cc[CE_GCD] * (u2 * iden) + cc[CE_GAMMA];
    const T gu = cc[CE_GU2] * (u * (iden * iden));            // dg/du = dg/dh = -dg/dcos
    T gE = g, guE = gu, q = mk<T>(0.f, 0.f);                  // g E, dg/du E, fc(r_k) g dE/dr_j
    if constexpr (P::HAS_LAM3) {
        if (p.lam3 != 0.f) {
            const T a = p.lam3 * (ej.r - ek.r);
            T E, dE;
            if (p.m == 1) { E = fexp_(a); dE = p.lam3 * E; }
            else { const T a2 = a * a; E = fexp_(a2 * a); dE = (3.f * p.lam3) * (a2 * E); }
            gE = g * E; guE = gu * E;
            q = ek.fc * (g * dE);
        }
    }
    o.t = ek.fc * gE;
    o.th = ek.fc * guE;
    // dcos/dd_j = (e_k - c e_j) / r_j, dcos/dd_k = (e_j - c e_k) / r_k, dr_j/dd_j = e_j, dr_k/dd_k = e_k
    const T pj = o.th * ej.ir, pk = o.th * ek.ir;
    o.cjj = pj * c;
    o.cjk = mk<T>(0.f, 0.f) - pj;
    o.ckj = mk<T>(0.f, 0.f) - pk;
    o.ckk = ek.dfc * gE + pk * c;
    if constexpr (P::HAS_LAM3) { o.cjj = o.cjj + q; o.ckk = o.ckk - q; }
    return o;
}

// b(zeta) = (1 + (beta zeta)^n)^(-1/(2n)) and b'(zeta) = -1/2 b (beta zeta)^n / ((1 + (beta zeta)^n) zeta);  zeta = 0: (1, 0)
template <class T>
__device__ __forceinline__ void ters_bond_order(const TersEntry& cc, T zeta, T& b, T& bp) {
    b = mk<T>(1.f, 0.f); bp = mk<T>(0.f, 0.f);
    if (!(val(zeta) > 0.f)) return;
    const T zn = fpow_(cc[CE_BETA] * zeta, cc[CE_N]);
    const T q = zn + 1.f;
    b = fexp_(cc[CE_MH] * flog_(q));
    bp = (-0.5f) * ((b * zn) / (q * zeta));
}

// ---- pass 1: the bonds i -> j of one atom.  e = u_i;  pa[b], pb[b] = d u_i / dA[a, b], dB[a, b];  ph = d u_i / dh[a]
template <class T, int LEVEL, class P>
__device__ __forceinline__ void ters_bonds(const TersIO& A, const P& p, int i, int ti, int sub, float& e, T (&pa)[P::SMAX],
                                           T (&pb)[P::SMAX], T& ph) {
    const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
    float wxi = 0.f, wyi = 0.f, wzi = 0.f;
    if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
    const T zero = mk<T>(0.f, 0.f);
    const TersEntry& cc = p.centre(ti);
    const int n = min(A.cnt[i], A.max_nbr);
    const size_t row = (size_t)i * A.max_nbr;
    for (int s = sub; s < n; s += TERS_LPA) {
        float* wk = (LEVEL >= 1 && A.work) ? A.work + 4 * (row + s) : nullptr;
        TersEdge<T> ej;
        const int j = ters_entry<T, LEVEL>(A, p, ti, row, s, xi, yi, zi, wxi, wyi, wzi, ej);
        if (j < 0) {
            if (wk) { wk[0] = 0.f; wk[1] = 0.f; wk[2] = 0.f; wk[3] = 0.f; }
            continue;
        }
        const int tj = p.species(j);
        const TersEntry& pp = p.pair(ti, tj);
        T zeta = zero, zh = zero;
        for (int t = 0; t < n; ++t) {
            if (t == s) continue;
            TersEdge<T> ek;
            if (ters_entry<T, LEVEL>(A, p, ti, row, t, xi, yi, zi, wxi, wyi, wzi, ek) < 0) continue;
            const TersTerm<T> tt = ters_term<T>(p, cc, ej, ek);
            zeta = zeta + tt.t;
            if (LEVEL >= 1) zh = zh + tt.th;
        }
        T b, bp;
        ters_bond_order<T>(cc, zeta, b, bp);
        const T hR = 0.5f * (ej.fc * fexp_((-pp[PA_L1]) * ej.r));           // 1/2 fc exp(-lam1 r)
        const T hA = 0.5f * (ej.fc * fexp_((-pp[PA_L2]) * ej.r));           // 1/2 fc exp(-lam2 r)
        const T bA = b * hA;
#pragma unroll
        for (int q = 0; q < P::SMAX; ++q) {                                 // (constant indices: the sums stay in registers)
            if (q == tj) { pa[q] = pa[q] + hR; pb[q] = pb[q] - bA; }
        }
        if (LEVEL >= 1) {
            const T Pb = (-pp[PA_B]) * (hA * bp);                           // dU/dzeta of this bond
            ph = ph + Pb * zh;
            if (wk) { wk[0] = val(Pb); wk[1] = dual_part(Pb); wk[2] = val(b); wk[3] = dual_part(b); }
        }
    }
    e = 0.f;
#pragma unroll
    for (int q = 0; q < P::SMAX; ++q) {
        if (q < p.S) {
            const TersEntry& pp = p.pair(ti, q);
            e = e + (pp[PA_A] * val(pa[q]) + pp[PA_B] * val(pb[q]));
        }
    }
}

// LEVEL 0: U        1: + pth, bond_work        2: + pthw, bond_work with dual parts
template <class P, int LEVEL>
__global__ void __launch_bounds__(TERS_BLOCK) tersoff_bond_kernel(const TersIO A, const typename P::Args V) {
    using T = typename std::conditional<LEVEL >= 2, Dual, float>::type;
    __shared__ float red[17];
    const P p(V);                            // (every thread of the block: the table view stages and synchronises here)
    constexpr int apb = TERS_BLOCK / TERS_LPA, SMAX = P::SMAX;
    const int i = blockIdx.x * apb + threadIdx.x / TERS_LPA, sub = threadIdx.x % TERS_LPA;
    float e = 0.f;
    if (i < A.N) {
        const int ti = p.species(i);
        const T zero = mk<T>(0.f, 0.f);
        T pa[SMAX], pb[SMAX], ph = zero;
#pragma unroll
        for (int q = 0; q < SMAX; ++q) { pa[q] = zero; pb[q] = zero; }
        ters_bonds<T, LEVEL>(A, p, i, ti, sub, e, pa, pb, ph);
        e = group_sum<TERS_LPA>(e);
        if (LEVEL >= 1 && (A.pth || A.pthw)) {
            float va[SMAX], vb[SMAX], da[SMAX], db[SMAX];
#pragma unroll
            for (int q = 0; q < SMAX; ++q) {
                va[q] = group_sum<TERS_LPA>(val(pa[q])); vb[q] = group_sum<TERS_LPA>(val(pb[q]));
                da[q] = LEVEL >= 2 ? group_sum<TERS_LPA>(dual_part(pa[q])) : 0.f;
                db[q] = LEVEL >= 2 ? group_sum<TERS_LPA>(dual_part(pb[q])) : 0.f;
            }
            const float vh = group_sum<TERS_LPA>(val(ph));
            const float dh = LEVEL >= 2 ? group_sum<TERS_LPA>(dual_part(ph)) : 0.f;
            if (sub == 0) {
                if (A.pth) p.store_theta(A.pth, i, ti, va, vb, vh);
                if (LEVEL >= 2 && A.pthw) p.store_theta(A.pthw, i, ti, da, db, dh);
            }
        }
        if (sub != 0) e = 0.f;
    }
    if (A.partial) {                         // (block-uniform: a force-only evaluation has no scalar to reduce)
        e = block_sum(e, red);
        if (threadIdx.x == 0) A.partial[blockIdx.x] = e;
    }
}

// ---- pass 2
// the bonds j -> i and j -> k (k in row(j), k != i) seen from atom i; eji is the edge j -> i under the pair entry (t_j, t_i).
// Adds to (gx, gy, gz) what they contribute to dU/dx_i through zeta, and returns b_ji
template <class T, int LEVEL, class P>
__device__ __forceinline__ T ters_around_neighbour(const TersIO& A, const P& p, int i, int j, int tj, const TersEdge<T>& eji,
                                                   T& gx, T& gy, T& gz) {
    const T zero = mk<T>(0.f, 0.f);
    const TersEntry& cc = p.centre(tj);
    const int nj = min(A.cnt[j], A.max_nbr);
    const size_t rowj = (size_t)j * A.max_nbr;
    const float xj = A.pos[3 * j], yj = A.pos[3 * j + 1], zj = A.pos[3 * j + 2];
    float wxj = 0.f, wyj = 0.f, wzj = 0.f;
    if (LEVEL >= 2) { wxj = A.w[3 * j]; wyj = A.w[3 * j + 1]; wzj = A.w[3 * j + 2]; }
    T Pji = zero, bji = zero;
    T sj = zero, sx = zero, sy = zero, sz = zero;                           // dzeta_ji/dd_ji = sj e_ji + (sx, sy, sz)
    for (int t = 0; t < nj; ++t) {
        const float* wk = A.work + 4 * (rowj + t);
        if (A.col[rowj + t] == i) {                                         // the bond j -> i itself
            Pji = mk<T>(wk[0], wk[1]); bji = mk<T>(wk[2], wk[3]);
            continue;
        }
        TersEdge<T> ek;                                                     // centre j -> end k: pair (t_j, t_k), j's stored image
        if (ters_entry<T, LEVEL>(A, p, tj, rowj, t, xj, yj, zj, wxj, wyj, wzj, ek) < 0) continue;
        // the bond j -> i with the third atom k: x_i moves d_ji
        const TersTerm<T> a = ters_term<T>(p, cc, eji, ek);
        sj = sj + a.cjj;
        sx = sx + a.cjk * ek.ex; sy = sy + a.cjk * ek.ey; sz = sz + a.cjk * ek.ez;
        // the bond j -> k with the third atom i (taper of the pair (t_j, t_i)): x_i moves the second vector
        const TersTerm<T> c = ters_term<T>(p, cc, ek, eji);
        const T Pjk = mk<T>(wk[0], wk[1]);
        const T ca = Pjk * c.ckj, cb = Pjk * c.ckk;
        gx = gx + (ca * ek.ex + cb * eji.ex); gy = gy + (ca * ek.ey + cb * eji.ey); gz = gz + (ca * ek.ez + cb * eji.ez);
    }
    gx = gx + Pji * (sj * eji.ex + sx); gy = gy + Pji * (sj * eji.ey + sy); gz = gz + Pji * (sj * eji.ez + sz);
    return bji;
}

// d/dr of 1/2 fc(r) (A exp(-lam1 r) - b B exp(-lam2 r)) at fixed b, under the pair entry pp
template <class T>
__device__ __forceinline__ T ters_pair_slope(const TersEntry& pp, const TersEdge<T>& e, T b) {
    const T eR = pp[PA_A] * fexp_((-pp[PA_L1]) * e.r), eA = pp[PA_B] * fexp_((-pp[PA_L2]) * e.r);
    const T bA = b * eA;
    return 0.5f * (e.dfc * (eR - bA) + e.fc * (pp[PA_L2] * bA - pp[PA_L1] * eR));
}

template <class T, int LEVEL, class P>
__device__ __forceinline__ void ters_atom(const TersIO& A, const P& p, int i, int sub, float (&out)[6]) {
    const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
    float wxi = 0.f, wyi = 0.f, wzi = 0.f;
    if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
    const T zero = mk<T>(0.f, 0.f);
    const int ti = p.species(i);
    const TersEntry& cc = p.centre(ti);
    T gx = zero, gy = zero, gz = zero;                       // dU/dx_i
    const int n = min(A.cnt[i], A.max_nbr);
    const size_t row = (size_t)i * A.max_nbr;
    for (int s = sub; s < n; s += TERS_LPA) {
        const int j = A.col[row + s];
        if ((unsigned)j >= (unsigned)A.N) continue;
        const int tj = p.species(j);
        const TersEntry& pij = p.pair(ti, tj);
        const TersEntry& pji = p.pair(tj, ti);
        float dx = xi - A.pos[3 * j], dy = yi - A.pos[3 * j + 1], dz = zi - A.pos[3 * j + 2];
        apply_shift(A.cell, A.shift[row + s], dx, dy, dz);
        float ax = 0.f, ay = 0.f, az = 0.f;
        if (LEVEL >= 2) { ax = A.w[3 * j] - wxi; ay = A.w[3 * j + 1] - wyi; az = A.w[3 * j + 2] - wzi; }
        TersEdge<T> ej;                                                     // i -> j under (t_i, t_j)
        if (!ters_geom<T>(-dx, -dy, -dz, ax, ay, az, fmaxf(pij[PA_RC], pji[PA_RC]), ej)) continue;
        // One species (SMAX == 1): (b, a) is (a, b), so eji keeps ej's taper and one support test serves both bonds; the two
        // pair slopes then stand in one block, where the compiler merges their exponentials.
        T dV = zero, bij = zero;                                            // dV: d/dr_ij of the pair parts of both bonds
        const bool on_ij = ters_taper<T>(pij, ej);
        if (on_ij) {
            const float* wk = A.work + 4 * (row + s);
            const T Pij = mk<T>(wk[0], wk[1]);
            bij = mk<T>(wk[2], wk[3]);
            // ---- P_ij dzeta_ij/dx_i = -P_ij sum_k (dt/dd_j + dt/dd_k)
            T sj = zero, sx = zero, sy = zero, sz = zero;
            for (int t = 0; t < n; ++t) {
                if (t == s) continue;
                TersEdge<T> ek;
                if (ters_entry<T, LEVEL>(A, p, ti, row, t, xi, yi, zi, wxi, wyi, wzi, ek) < 0) continue;
                const TersTerm<T> tt = ters_term<T>(p, cc, ej, ek);
                const T ck = tt.cjk + tt.ckk;
                sj = sj + (tt.cjj + tt.ckj);
                sx = sx + ck * ek.ex; sy = sy + ck * ek.ey; sz = sz + ck * ek.ez;
            }
            gx = gx - Pij * (sj * ej.ex + sx); gy = gy - Pij * (sj * ej.ey + sy); gz = gz - Pij * (sj * ej.ez + sz);
            if constexpr (P::SMAX > 1) dV = dV + ters_pair_slope<T>(pij, ej, bij);
        }
        TersEdge<T> eji = ej;                                               // j -> i under (t_j, t_i): the unit vector is -e
        eji.ex = (-1.f) * ej.ex; eji.ey = (-1.f) * ej.ey; eji.ez = (-1.f) * ej.ez;
        bool on_ji = on_ij;
        if constexpr (P::SMAX > 1) on_ji = ters_taper<T>(pji, eji);
        if (on_ji) {
            // ---- the bonds of j that x_i enters through zeta, then the pair part of j -> i
            const T bji = ters_around_neighbour<T, LEVEL>(A, p, i, j, tj, eji, gx, gy, gz);
            if constexpr (P::SMAX == 1) dV = dV + ters_pair_slope<T>(pij, ej, bij);
            dV = dV + ters_pair_slope<T>(pji, eji, bji);
        }
        gx = gx - dV * ej.ex; gy = gy - dV * ej.ey; gz = gz - dV * ej.ez;                      // d r / d x_i = -e
    }
    out[0] = val(gx); out[1] = val(gy); out[2] = val(gz);
    if (LEVEL >= 2) { out[3] = dual_part(gx); out[4] = dual_part(gy); out[5] = dual_part(gz); }
}

// LEVEL 1: grad        2: + hw
template <class P, int LEVEL>
__global__ void __launch_bounds__(TERS_BLOCK) tersoff_force_kernel(const TersIO A, const typename P::Args V) {
    using T = typename std::conditional<LEVEL >= 2, Dual, float>::type;
    const P p(V);
    const int i = blockIdx.x * (TERS_BLOCK / TERS_LPA) + threadIdx.x / TERS_LPA, sub = threadIdx.x % TERS_LPA;
    if (i >= A.N) return;
    float o[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = 0.f;
    ters_atom<T, LEVEL>(A, p, i, sub, o);
    constexpr int NV = LEVEL >= 2 ? 6 : 3;
#pragma unroll
    for (int k = 0; k < NV; ++k) o[k] = group_sum<TERS_LPA>(o[k]);
    if (sub != 0) return;
    if (A.grad) store3(A.grad, i, A.oscale, A.oacc, o[0], o[1], o[2]);
    if (LEVEL >= 2 && A.hw) store3(A.hw, i, A.oscale, A.oacc, o[3], o[4], o[5]);
}

// the two passes and the energy for the view P; `level` as the entry points derive it from the requested outputs
template <class P>
inline void tersoff_launch(const TersIO& a, const typename P::Args& v, int level, bool forces, float* energy, float* partial,
                           hipStream_t st) {
    const int nblocks = (int)atom_blocks(a.N, TERS_LPA, TERS_BLOCK);
    const dim3 grid(nblocks), block(TERS_BLOCK);
    with_level(level, [&](auto L) {
        constexpr int LV = decltype(L)::value;
        hipLaunchKernelGGL((tersoff_bond_kernel<P, LV>), grid, block, 0, st, a, v);
        if constexpr (LV >= 1) {
            if (forces) hipLaunchKernelGGL((tersoff_force_kernel<P, LV>), grid, block, 0, st, a, v);
        }
    });
    if (energy) hipLaunchKernelGGL(energy_finish, dim3(1), dim3(64), 0, st, partial, nblocks, energy);
}

// floats of bond_work for a list of n_atoms rows of max_nbr slots
inline int64_t tersoff_work_floats(int n_atoms, int max_nbr) {
    if (n_atoms <= 0 || max_nbr <= 0) return 0;
    return 4 * (int64_t)n_atoms * (int64_t)max_nbr;
}

}  // namespace
