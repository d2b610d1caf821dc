// K26: Tersoff bond-order potential for up to four species over the per-atom (ELL) list
// (mdgrad_amd/interface.py TersoffMulti; Tersoff 1989, "Modeling solid-state chemistry: interatomic potentials for
// multicomponent systems"; the LAMMPS convention with lam3 = 0).  With a = t_i, b = t_j, c = t_k the species of the atoms:
//
//   U       = 1/2 sum_i sum_{j in row(i)} fc_ab(r_ij) [ A_ab exp(-lam1_ab r_ij) - b_ij B_ab exp(-lam2_ab r_ij) ]
//   b_ij    = (1 + (beta_a zeta_ij)^n_a)^(-1/(2 n_a)),      zeta_ij = 0: b = 1 with zero derivatives
//   zeta_ij = sum_{k in row(i), k != j} fc_ac(r_ik) g_a(cos theta_jik)
//   g_a(x)  = gamma_a (1 + c_a^2/d_a^2 - c_a^2/(d_a^2 + (h_a - x)^2))
//   fc_ab   = 1 for r <= R_ab - D_ab;  1/2 - 1/2 sin(pi (r - R_ab) / (2 D_ab)) inside the taper;  exactly 0 for r >= R_ab + D_ab
//
// The passes, the lane layout, the per-slot scratch bond_work = (P, dP, b, db), the Dual-number LEVEL 2 and the absence of
// fused multiply-adds and of atomics are those of csrc/tersoff.hip (K25); read its header first.  What is new is that every
// constant is looked up by species, from one flat device table of derived constants (mdg_tersoff_multi_table_size floats):
//   pair entry   tab[8 (a S + b) ...]   = A, B, lam1, lam2, R, R - D, R + D, pi / (2 D)          row = centre, column = end
//   centre entry tab[8 S S + 8 a ...]   = h, beta, n, -1/(2n), d^2, gamma, gamma (c/d)^2, 2 gamma (c/d)^2 d^2
// (the forms TersK of K25 holds, so g is evaluated without the difference of its two large terms).  The pair table is
// ordered: (a, b) and (b, a) are separate entries and may differ, also in their cutoffs.  The table is staged into LDS once per
// block (at most 160 floats); a lane indexes it with the species of its own atoms, which differ from lane to lane.
//
// Which entry is read where.  Bond pass, atom i of species a on slot s (end j, species b):
//   the edge i -> j:                          pair (a, b)
//   a third atom k of row(i):                 pair (a, t_k) for its taper, centre a for g
//   b_ij and b'(zeta_ij):                     centre a
//   per-atom parameter terms:                 d u_i / dA[a, b], d u_i / dB[a, b], d u_i / dh[a]; every other entry of row i of
//                                             pth is written as 0, so the column sums over the atoms are dU/d(A, B, h)
// Force pass, the five contributions to dU/dx_i of the lane on slot s of row(i):
//   1. pair part of i -> j at fixed b_ij:                         pair (a, b)
//   2. P_ij dzeta_ij/dx_i (loop over row(i)):                     pair (a, b) for e_ij, pair (a, t_k) for k's taper, centre a
//   3. pair part of j -> i at fixed b_ji (b_ji from row(j)):      pair (b, a)
//   4. P_ji dzeta_ji/dx_i, i the end of the bond j -> i:          pair (b, a) for the edge j -> i, pair (b, t_k) for k's taper,
//                                                                 centre b
//   5. P_jk dzeta_jk/dx_i, i the third atom of the bond j -> k:   pair (b, t_k) for the edge j -> k, pair (b, a) for the taper
//                                                                 of i, centre b
// 1 and 2 need r_ij inside the support of (a, b); 3, 4, 5 need it inside the support of (b, a), which is tested on its own: with
// R_ab + D_ab != R_ba + D_ba one of the two directed bonds can exist without the other.
// The support test 0 < r < R + D of an entry uses that entry's own pair constants, so the list may have been searched with
// any radius >= max_ab (R_ab + D_ab).  A slot that fails it gets (0, 0, 0, 0) in bond_work.
#pragma clang fp contract(off)
#include <type_traits>
#include "common.hpp"
#include "dual.hpp"

namespace {

constexpr int TERSM_LPA = 16;                 // lanes per atom, as in tersoff.hip
constexpr int TERSM_BLOCK = 256;
constexpr int TERSM_SMAX = 4;                 // species
constexpr int TERSM_TAB_MAX = 8 * TERSM_SMAX * (TERSM_SMAX + 1);
// pair entry
constexpr int PA_A = 0, PA_B = 1, PA_L1 = 2, PA_L2 = 3, PA_R = 4, PA_RIN = 5, PA_RC = 6, PA_PD = 7;
// centre entry
constexpr int CE_H = 0, CE_BETA = 1, CE_N = 2, CE_MH = 3, CE_D2 = 4, CE_GAMMA = 5, CE_GCD = 6, CE_GU2 = 7;

struct TersMArgs {
    const float* pos; int N; MdgCell cell;
    const int32_t* col; const int32_t* shift; const int32_t* cnt; int max_nbr;
    const int32_t* types; int S;
    const float* tables;                       // device, 8 S (S + 1) floats
    const float* w;
    float* work;                               // bond_work [N * max_nbr, 4]
    float* grad; float* hw; float* pth; float* pthw; float* partial;
    float oscale; int oacc;
};

template <class T> __device__ __forceinline__ T tm_mk(float v, float d);
template <> __device__ __forceinline__ float tm_mk<float>(float v, float) { return v; }
template <> __device__ __forceinline__ Dual tm_mk<Dual>(float v, float d) { return {v, d}; }
__device__ __forceinline__ float tm_dual(float) { return 0.f; }
__device__ __forceinline__ float tm_dual(Dual a) { return a.d; }

// the block's copy of the table in LDS; every thread of the block calls this (one barrier)
__device__ __forceinline__ void tm_stage(const TersMArgs& A, float* tab) {
    const int n = 8 * A.S * (A.S + 1);
    for (int k = threadIdx.x; k < n; k += TERSM_BLOCK) tab[k] = A.tables[k];
    __syncthreads();
}
__device__ __forceinline__ const float* tm_pair(const float* tab, int S, int a, int b) { return tab + 8 * (a * S + b); }
__device__ __forceinline__ const float* tm_centre(const float* tab, int S, int a) { return tab + 8 * (S * S + a); }
// a species read from `types`, kept inside the table whatever the buffer holds
__device__ __forceinline__ int tm_type(const TersMArgs& A, int i) { return min(max(A.types[i], 0), A.S - 1); }

// one list entry seen from its centre: unit vector centre -> end, r, 1/r, fc(r), fc'(r)
template <class T> struct TersMEdge { T ex, ey, ez, r, ir, fc, dfc; };

// fc and fc' of the edge under the pair entry pp, from e.r.  False outside the support of that entry.
template <class T>
__device__ __forceinline__ bool tm_taper(const float* pp, TersMEdge<T>& e) {
    const float rv = val(e.r);
    if (!(rv < pp[PA_RC])) return false;
    if (rv <= pp[PA_RIN]) {
        e.fc = tm_mk<T>(1.f, 0.f); e.dfc = tm_mk<T>(0.f, 0.f);
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
__device__ __forceinline__ bool tm_geom(float dx, float dy, float dz, float ax, float ay, float az, float rmax, TersMEdge<T>& e) {
    const T x = tm_mk<T>(dx, ax), y = tm_mk<T>(dy, ay), z = tm_mk<T>(dz, az);
    const T d2 = x * x + y * y + z * z;
    const float rv = sqrtf(val(d2));
    if (!(rv > 0.f && rv < rmax)) return false;              // the support test, on the r that fc is formed from
    e.r = fsqrt_(d2);
    e.ir = tm_mk<T>(1.f, 0.f) / e.r;
    e.ex = x * e.ir; e.ey = y * e.ir; e.ez = z * e.ir;
    return true;
}

// the entry in slot s of the row of a centre of species tc (position xc, seed wc) as an edge centre -> end under the pair
// entry (tc, t_end); returns the end atom, or -1 when there is nothing to add
template <class T, int LEVEL>
__device__ __forceinline__ int tm_entry(const TersMArgs& A, const float* tab, int tc, size_t row, int s, float xc, float yc,
                                        float zc, float wxc, float wyc, float wzc, TersMEdge<T>& e) {
    const int j = A.col[row + s];
    if ((unsigned)j >= (unsigned)A.N) return -1;
    float dx = xc - A.pos[3 * j], dy = yc - A.pos[3 * j + 1], dz = zc - A.pos[3 * j + 2];
    apply_shift(A.cell, A.shift[row + s], dx, dy, dz);                      // x_c - x_j - o.h
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (LEVEL >= 2) { ax = A.w[3 * j] - wxc; ay = A.w[3 * j + 1] - wyc; az = A.w[3 * j + 2] - wzc; }
    const float* pp = tm_pair(tab, A.S, tc, tm_type(A, j));
    if (!tm_geom<T>(-dx, -dy, -dz, ax, ay, az, pp[PA_RC], e)) return -1;
    return tm_taper<T>(pp, e) ? j : -1;
}

// One third atom k of the bond centre -> j:  t = fc(r_k) g(cos), th = dt/dh, and the derivatives with respect to the two
// vectors d_j, d_k (end - centre) as coefficients of the unit vectors:
//   dt/dd_j = cjj e_j + cjk e_k,   dt/dd_k = ckj e_j + ckk e_k
// cc: the centre entry of the centre's species; ek.fc: the taper of the pair entry (centre, k)
template <class T> struct TersMTerm { T t, th, cjj, cjk, ckj, ckk; };

template <class T>
__device__ __forceinline__ TersMTerm<T> tm_term(const float* cc, const TersMEdge<T>& ej, const TersMEdge<T>& ek) {
    TersMTerm<T> o;
    const T c = ej.ex * ek.ex + ej.ey * ek.ey + ej.ez * ek.ez;
    const T u = cc[CE_H] - c;
    const T u2 = u * u;
    const T iden = tm_mk<T>(1.f, 0.f) / (u2 + cc[CE_D2]);
    const T g = cc[CE_GCD] * (u2 * iden) + cc[CE_GAMMA];
    const T gu = cc[CE_GU2] * (u * (iden * iden));            // dg/du = dg/dh = -dg/dcos
    o.t = ek.fc * g;
    o.th = ek.fc * gu;
    // dcos/dd_j = (e_k - c e_j) / r_j, dcos/dd_k = (e_j - c e_k) / r_k, dr_k/dd_k = e_k
    const T pj = o.th * ej.ir, pk = o.th * ek.ir;
    o.cjj = pj * c;
    o.cjk = tm_mk<T>(0.f, 0.f) - pj;
    o.ckj = tm_mk<T>(0.f, 0.f) - pk;
    o.ckk = ek.dfc * g + pk * c;
    return o;
}

// b(zeta) = (1 + (beta zeta)^n)^(-1/(2n)) and b'(zeta) = -1/2 b (beta zeta)^n / ((1 + (beta zeta)^n) zeta);  zeta = 0: (1, 0)
template <class T>
__device__ __forceinline__ void tm_bond_order(const float* cc, T zeta, T& b, T& bp) {
    b = tm_mk<T>(1.f, 0.f); bp = tm_mk<T>(0.f, 0.f);
    if (!(val(zeta) > 0.f)) return;
    const T zn = fpow_(cc[CE_BETA] * zeta, cc[CE_N]);
    const T q = zn + 1.f;
    b = fexp_(cc[CE_MH] * flog_(q));
    bp = (-0.5f) * ((b * zn) / (q * zeta));
}

// ---- pass 1: the bonds i -> j of one atom.  e = u_i;  pa[b], pb[b] = d u_i / dA[a, b], dB[a, b];  ph = d u_i / dh[a]
template <class T, int LEVEL>
__device__ __forceinline__ void tm_bonds(const TersMArgs& A, const float* tab, int i, int ti, int sub, float& e,
                                         T (&pa)[TERSM_SMAX], T (&pb)[TERSM_SMAX], T& ph) {
    const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
    float wxi = 0.f, wyi = 0.f, wzi = 0.f;
    if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
    const T zero = tm_mk<T>(0.f, 0.f);
    const float* cc = tm_centre(tab, A.S, ti);
    const int n = min(A.cnt[i], A.max_nbr);
    const size_t row = (size_t)i * A.max_nbr;
    for (int s = sub; s < n; s += TERSM_LPA) {
        float* wk = (LEVEL >= 1 && A.work) ? A.work + 4 * (row + s) : nullptr;
        TersMEdge<T> ej;
        const int j = tm_entry<T, LEVEL>(A, tab, ti, row, s, xi, yi, zi, wxi, wyi, wzi, ej);
        if (j < 0) {
            if (wk) { wk[0] = 0.f; wk[1] = 0.f; wk[2] = 0.f; wk[3] = 0.f; }
            continue;
        }
        const int tj = tm_type(A, j);
        const float* pp = tm_pair(tab, A.S, ti, tj);
        T zeta = zero, zh = zero;
        for (int t = 0; t < n; ++t) {
            if (t == s) continue;
            TersMEdge<T> ek;
            if (tm_entry<T, LEVEL>(A, tab, ti, row, t, xi, yi, zi, wxi, wyi, wzi, ek) < 0) continue;
            const TersMTerm<T> tt = tm_term<T>(cc, ej, ek);
            zeta = zeta + tt.t;
            if (LEVEL >= 1) zh = zh + tt.th;
        }
        T b, bp;
        tm_bond_order<T>(cc, zeta, b, bp);
        const T hR = 0.5f * (ej.fc * fexp_((-pp[PA_L1]) * ej.r));           // 1/2 fc exp(-lam1 r)
        const T hA = 0.5f * (ej.fc * fexp_((-pp[PA_L2]) * ej.r));           // 1/2 fc exp(-lam2 r)
        const T bA = b * hA;
#pragma unroll
        for (int q = 0; q < TERSM_SMAX; ++q) {                              // (constant indices: the sums stay in registers)
            if (q == tj) { pa[q] = pa[q] + hR; pb[q] = pb[q] - bA; }
        }
        if (LEVEL >= 1) {
            const T P = (-pp[PA_B]) * (hA * bp);                            // dU/dzeta of this bond
            ph = ph + P * zh;
            if (wk) { wk[0] = val(P); wk[1] = tm_dual(P); wk[2] = val(b); wk[3] = tm_dual(b); }
        }
    }
    e = 0.f;
#pragma unroll
    for (int q = 0; q < TERSM_SMAX; ++q) {
        if (q < A.S) {
            const float* pp = tm_pair(tab, A.S, ti, q);
            e = e + (pp[PA_A] * val(pa[q]) + pp[PA_B] * val(pb[q]));
        }
    }
}

// row i of a per-atom parameter table [N, 2 S S + S]: zero but for A[a, :], B[a, :], h[a]
__device__ __forceinline__ void tm_store_theta(float* dst, int i, int S, int a, const float (&va)[TERSM_SMAX],
                                               const float (&vb)[TERSM_SMAX], float vh) {
    const int S2 = S * S, P = 2 * S2 + S;
    float* r = dst + (size_t)i * P;
    for (int k = 0; k < P; ++k) r[k] = 0.f;
#pragma unroll
    for (int q = 0; q < TERSM_SMAX; ++q) {
        if (q < S) { r[a * S + q] = va[q]; r[S2 + a * S + q] = vb[q]; }
    }
    r[2 * S2 + a] = vh;
}

// LEVEL 0: U        1: + pth, bond_work        2: + pthw, bond_work with dual parts
template <int LEVEL>
__global__ void __launch_bounds__(TERSM_BLOCK) tersoff_multi_bond_kernel(const TersMArgs A) {
    using T = typename std::conditional<LEVEL >= 2, Dual, float>::type;
    __shared__ float red[17];
    __shared__ float tab[TERSM_TAB_MAX];
    tm_stage(A, tab);
    constexpr int apb = TERSM_BLOCK / TERSM_LPA;
    const int i = blockIdx.x * apb + threadIdx.x / TERSM_LPA, sub = threadIdx.x % TERSM_LPA;
    float e = 0.f;
    if (i < A.N) {
        const int ti = tm_type(A, i);
        const T zero = tm_mk<T>(0.f, 0.f);
        T pa[TERSM_SMAX], pb[TERSM_SMAX], ph = zero;
#pragma unroll
        for (int q = 0; q < TERSM_SMAX; ++q) { pa[q] = zero; pb[q] = zero; }
        tm_bonds<T, LEVEL>(A, tab, i, ti, sub, e, pa, pb, ph);
        e = group_sum<TERSM_LPA>(e);
        if (LEVEL >= 1 && (A.pth || A.pthw)) {
            float va[TERSM_SMAX], vb[TERSM_SMAX], da[TERSM_SMAX], db[TERSM_SMAX];
#pragma unroll
            for (int q = 0; q < TERSM_SMAX; ++q) {
                va[q] = group_sum<TERSM_LPA>(val(pa[q])); vb[q] = group_sum<TERSM_LPA>(val(pb[q]));
                da[q] = LEVEL >= 2 ? group_sum<TERSM_LPA>(tm_dual(pa[q])) : 0.f;
                db[q] = LEVEL >= 2 ? group_sum<TERSM_LPA>(tm_dual(pb[q])) : 0.f;
            }
            const float vh = group_sum<TERSM_LPA>(val(ph));
            const float dh = LEVEL >= 2 ? group_sum<TERSM_LPA>(tm_dual(ph)) : 0.f;
            if (sub == 0) {
                if (A.pth) tm_store_theta(A.pth, i, A.S, ti, va, vb, vh);
                if (LEVEL >= 2 && A.pthw) tm_store_theta(A.pthw, i, A.S, ti, da, db, dh);
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
template <class T, int LEVEL>
__device__ __forceinline__ T tm_around_neighbour(const TersMArgs& A, const float* tab, int i, int j, int tj,
                                                 const TersMEdge<T>& eji, T& gx, T& gy, T& gz) {
    const T zero = tm_mk<T>(0.f, 0.f);
    const float* cc = tm_centre(tab, A.S, tj);
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
            Pji = tm_mk<T>(wk[0], wk[1]); bji = tm_mk<T>(wk[2], wk[3]);
            continue;
        }
        TersMEdge<T> ek;                                                    // centre j -> end k: pair (t_j, t_k), j's stored image
        if (tm_entry<T, LEVEL>(A, tab, tj, rowj, t, xj, yj, zj, wxj, wyj, wzj, ek) < 0) continue;
        // the bond j -> i with the third atom k: x_i moves d_ji
        const TersMTerm<T> a = tm_term<T>(cc, eji, ek);
        sj = sj + a.cjj;
        sx = sx + a.cjk * ek.ex; sy = sy + a.cjk * ek.ey; sz = sz + a.cjk * ek.ez;
        // the bond j -> k with the third atom i (taper of the pair (t_j, t_i)): x_i moves the second vector
        const TersMTerm<T> c = tm_term<T>(cc, ek, eji);
        const T Pjk = tm_mk<T>(wk[0], wk[1]);
        const T ca = Pjk * c.ckj, cb = Pjk * c.ckk;
        gx = gx + (ca * ek.ex + cb * eji.ex); gy = gy + (ca * ek.ey + cb * eji.ey); gz = gz + (ca * ek.ez + cb * eji.ez);
    }
    gx = gx + Pji * (sj * eji.ex + sx); gy = gy + Pji * (sj * eji.ey + sy); gz = gz + Pji * (sj * eji.ez + sz);
    return bji;
}

// d/dr of 1/2 fc(r) (A exp(-lam1 r) - b B exp(-lam2 r)) at fixed b, under the pair entry pp
template <class T>
__device__ __forceinline__ T tm_pair_slope(const float* pp, const TersMEdge<T>& e, T b) {
    const T eR = pp[PA_A] * fexp_((-pp[PA_L1]) * e.r), eA = pp[PA_B] * fexp_((-pp[PA_L2]) * e.r);
    const T bA = b * eA;
    return 0.5f * (e.dfc * (eR - bA) + e.fc * (pp[PA_L2] * bA - pp[PA_L1] * eR));
}

template <class T, int LEVEL>
__device__ __forceinline__ void tm_atom(const TersMArgs& A, const float* tab, int i, int sub, float (&out)[6]) {
    const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
    float wxi = 0.f, wyi = 0.f, wzi = 0.f;
    if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
    const T zero = tm_mk<T>(0.f, 0.f);
    const int ti = tm_type(A, i);
    const float* cc = tm_centre(tab, A.S, ti);
    T gx = zero, gy = zero, gz = zero;                       // dU/dx_i
    const int n = min(A.cnt[i], A.max_nbr);
    const size_t row = (size_t)i * A.max_nbr;
    for (int s = sub; s < n; s += TERSM_LPA) {
        const int j = A.col[row + s];
        if ((unsigned)j >= (unsigned)A.N) continue;
        const int tj = tm_type(A, j);
        const float* pij = tm_pair(tab, A.S, ti, tj);
        const float* pji = tm_pair(tab, A.S, tj, ti);
        float dx = xi - A.pos[3 * j], dy = yi - A.pos[3 * j + 1], dz = zi - A.pos[3 * j + 2];
        apply_shift(A.cell, A.shift[row + s], dx, dy, dz);
        float ax = 0.f, ay = 0.f, az = 0.f;
        if (LEVEL >= 2) { ax = A.w[3 * j] - wxi; ay = A.w[3 * j + 1] - wyi; az = A.w[3 * j + 2] - wzi; }
        TersMEdge<T> ej;                                                    // i -> j under (t_i, t_j)
        if (!tm_geom<T>(-dx, -dy, -dz, ax, ay, az, fmaxf(pij[PA_RC], pji[PA_RC]), ej)) continue;
        TersMEdge<T> eji = ej;                                              // j -> i under (t_j, t_i): the unit vector is -e
        eji.ex = (-1.f) * ej.ex; eji.ey = (-1.f) * ej.ey; eji.ez = (-1.f) * ej.ez;
        T dV = zero;                                                        // d/dr_ij of the pair parts of both bonds
        if (tm_taper<T>(pij, ej)) {
            const float* wk = A.work + 4 * (row + s);
            const T Pij = tm_mk<T>(wk[0], wk[1]), bij = tm_mk<T>(wk[2], wk[3]);
            // ---- P_ij dzeta_ij/dx_i = -P_ij sum_k (dt/dd_j + dt/dd_k)
            T sj = zero, sx = zero, sy = zero, sz = zero;
            for (int t = 0; t < n; ++t) {
                if (t == s) continue;
                TersMEdge<T> ek;
                if (tm_entry<T, LEVEL>(A, tab, ti, row, t, xi, yi, zi, wxi, wyi, wzi, ek) < 0) continue;
                const TersMTerm<T> a = tm_term<T>(cc, ej, ek);
                const T ck = a.cjk + a.ckk;
                sj = sj + (a.cjj + a.ckj);
                sx = sx + ck * ek.ex; sy = sy + ck * ek.ey; sz = sz + ck * ek.ez;
            }
            gx = gx - Pij * (sj * ej.ex + sx); gy = gy - Pij * (sj * ej.ey + sy); gz = gz - Pij * (sj * ej.ez + sz);
            dV = dV + tm_pair_slope<T>(pij, ej, bij);
        }
        if (tm_taper<T>(pji, eji)) {
            // ---- the bonds of j that x_i enters through zeta, then the pair part of j -> i
            const T bji = tm_around_neighbour<T, LEVEL>(A, tab, i, j, tj, eji, gx, gy, gz);
            dV = dV + tm_pair_slope<T>(pji, eji, bji);
        }
        gx = gx - dV * ej.ex; gy = gy - dV * ej.ey; gz = gz - dV * ej.ez;                      // d r / d x_i = -e
    }
    out[0] = val(gx); out[1] = val(gy); out[2] = val(gz);
    if (LEVEL >= 2) { out[3] = tm_dual(gx); out[4] = tm_dual(gy); out[5] = tm_dual(gz); }
}

__device__ __forceinline__ void tm_store3(float* dst, int i, float os, int oacc, float x, float y, float z) {
    if (oacc) { dst[3 * i] = fmaf(os, x, dst[3 * i]); dst[3 * i + 1] = fmaf(os, y, dst[3 * i + 1]); dst[3 * i + 2] = fmaf(os, z, dst[3 * i + 2]); }
    else { dst[3 * i] = os * x; dst[3 * i + 1] = os * y; dst[3 * i + 2] = os * z; }
}

// LEVEL 1: grad        2: + hw
template <int LEVEL>
__global__ void __launch_bounds__(TERSM_BLOCK) tersoff_multi_force_kernel(const TersMArgs A) {
    using T = typename std::conditional<LEVEL >= 2, Dual, float>::type;
    __shared__ float tab[TERSM_TAB_MAX];
    tm_stage(A, tab);
    const int i = blockIdx.x * (TERSM_BLOCK / TERSM_LPA) + threadIdx.x / TERSM_LPA, sub = threadIdx.x % TERSM_LPA;
    if (i >= A.N) return;
    float o[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = 0.f;
    tm_atom<T, LEVEL>(A, tab, i, sub, o);
    constexpr int NV = LEVEL >= 2 ? 6 : 3;
#pragma unroll
    for (int k = 0; k < NV; ++k) o[k] = group_sum<TERSM_LPA>(o[k]);
    if (sub != 0) return;
    if (A.grad) tm_store3(A.grad, i, A.oscale, A.oacc, o[0], o[1], o[2]);
    if (LEVEL >= 2 && A.hw) tm_store3(A.hw, i, A.oscale, A.oacc, o[3], o[4], o[5]);
}

// one wave, fixed summation order
__global__ void tersoff_multi_finish(const float* __restrict__ partial, int nblocks, float* energy) {
    const int lane = threadIdx.x;
    float s = 0.f;
    for (int b = lane; b < nblocks; b += 64) s += partial[b];
    s = wave_sum(s);
    if (lane == 0) energy[0] = s;
}

}  // namespace

extern "C" int64_t mdg_tersoff_multi_partial_size(int n_atoms) {
    if (n_atoms <= 0) return 0;
    const int apb = TERSM_BLOCK / TERSM_LPA;
    return (int64_t)((n_atoms + apb - 1) / apb);
}

extern "C" int64_t mdg_tersoff_multi_work_size(int n_atoms, int max_nbr) {
    if (n_atoms <= 0 || max_nbr <= 0) return 0;
    return 4 * (int64_t)n_atoms * (int64_t)max_nbr;
}

extern "C" int64_t mdg_tersoff_multi_table_size(int n_species) {
    if (n_species < 1 || n_species > TERSM_SMAX) return 0;
    return 8 * (int64_t)n_species * (n_species + 1);
}

extern "C" int mdg_tersoff_multi_eval(const float* pos, int n_atoms, const MdgCell* cell, const int32_t* col, const int32_t* shift,
                                      const int32_t* cnt, int max_nbr, const int32_t* types, int n_species, const float* tables,
                                      const float* w, float* energy, float* grad, float* hw, float* pth, float* pthw,
                                      float* partial, float* bond_work, float out_scale, int accumulate, void* stream) {
    MDG_CHECK_ARG(pos && cell && col && shift && cnt, "tersoff_multi_eval: null buffer (pos, cell or list)");
    MDG_CHECK_ARG(n_atoms > 0 && max_nbr > 0, "tersoff_multi_eval: bad sizes (n_atoms, max_nbr must be positive)");
    MDG_CHECK_ARG(n_species >= 1 && n_species <= TERSM_SMAX, "tersoff_multi_eval: n_species must lie in [1, %d] (got %d)",
                  TERSM_SMAX, n_species);
    MDG_CHECK_ARG(types, "tersoff_multi_eval: types is null (device int32 [n_atoms])");
    MDG_CHECK_ARG(tables, "tersoff_multi_eval: tables is null (device float [mdg_tersoff_multi_table_size(n_species)])");
    MDG_CHECK_ARG(w || !(hw || pthw), "tersoff_multi_eval: hw / pthw need w");
    MDG_CHECK_ARG(!w || hw || pthw, "tersoff_multi_eval: w given without hw or pthw output");
    MDG_CHECK_ARG(energy || grad || hw || pth || pthw, "tersoff_multi_eval: no output requested");
    MDG_CHECK_ARG(!energy || partial, "tersoff_multi_eval: energy needs the partial buffer");
    MDG_CHECK_ARG(bond_work || !(grad || hw),
                  "tersoff_multi_eval: grad / hw need bond_work (the scratch of the bond pass, mdg_tersoff_multi_work_size() floats)");
    const int level = w ? 2 : ((grad || pth) ? 1 : 0);
    // (accumulate bit 2, "the list was searched with a skin", needs nothing here: the support test is always applied)
    TersMArgs a{pos, n_atoms, *cell, col, shift, cnt, max_nbr, types, n_species, tables, w, bond_work, grad, hw, pth, pthw,
                energy ? partial : nullptr, out_scale, accumulate & 1};
    const int nblocks = (int)mdg_tersoff_multi_partial_size(n_atoms);
    dim3 grid(nblocks);
    hipStream_t st = (hipStream_t)stream;
    const bool forces = grad || hw;
    if (level == 2) {
        hipLaunchKernelGGL((tersoff_multi_bond_kernel<2>), grid, dim3(TERSM_BLOCK), 0, st, a);
        if (forces) hipLaunchKernelGGL((tersoff_multi_force_kernel<2>), grid, dim3(TERSM_BLOCK), 0, st, a);
    } else if (level == 1) {
        hipLaunchKernelGGL((tersoff_multi_bond_kernel<1>), grid, dim3(TERSM_BLOCK), 0, st, a);
        if (forces) hipLaunchKernelGGL((tersoff_multi_force_kernel<1>), grid, dim3(TERSM_BLOCK), 0, st, a);
    } else {
        hipLaunchKernelGGL((tersoff_multi_bond_kernel<0>), grid, dim3(TERSM_BLOCK), 0, st, a);
    }
    if (energy) hipLaunchKernelGGL(tersoff_multi_finish, dim3(1), dim3(64), 0, st, partial, nblocks, energy);
    MDG_CHECK_LAUNCH("tersoff_multi_kernel");
    return MDG_OK;
}
