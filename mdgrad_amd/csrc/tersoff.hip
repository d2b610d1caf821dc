// K25: Tersoff bond-order potential for one species over the per-atom (ELL) list
// (mdgrad_amd/interface.py Tersoff; Tersoff 1988 for silicon, 1989 for carbon; the LAMMPS convention).
//
//   U      = 1/2 sum_i sum_{j in row(i)} fc(r_ij) [ A exp(-lam1 r_ij) - b_ij B exp(-lam2 r_ij) ]
//   b_ij   = (1 + (beta zeta_ij)^n)^(-1/(2n))
//   zeta_ij = sum_{k in row(i), k != j} fc(r_ik) g(cos theta_jik) exp[(lam3 (r_ij - r_ik))^m]            m = 1 or 3
//   g(x)   = gamma (1 + c^2/d^2 - c^2/(d^2 + (h - x)^2))
//   fc(r)  = 1 for r <= R - D;  1/2 - 1/2 sin(pi (r - R) / (2 D)) inside the taper;  exactly 0 for r >= R + D
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
// Both are laid out like sw_ell_kernel (csrc/sw.hip): LPA lanes walk one atom's row, wave shuffles combine the per-atom sums,
// the energy goes through a fixed-order block partial and a finish kernel.  No float atomics => bitwise reproducible.  Rows
// are read from global memory where they are needed, nothing is staged, so there is no row cap; the cost is O(n^2) per atom.
// The support test 0 < r < R + D is applied on r = sqrtf(d2) for every entry; a list searched with a larger radius (a skin)
// is exact.  A slot inside cnt that fails the test gets (0, 0, 0, 0), so the force pass never reads an unwritten word.
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
#pragma clang fp contract(off)
#include <type_traits>
#include "common.hpp"
#include "dual.hpp"

namespace {

constexpr int TERS_LPA = 16;                  // lanes per atom: taken over from sw.hip (covalent rows hold 4 - 16 entries);
                                              // the choice has not been measured for this kernel
constexpr int TERS_BLOCK = 256;

struct TersArgs {
    const float* pos; int N; MdgCell cell;
    const int32_t* col; const int32_t* shift; const int32_t* cnt; int max_nbr;
    const float* theta;                        // device (A, B, h), or null: the three host values below
    const float* w;
    float A, B, h;
    float lam1, lam2, beta, n, c, d, R, D, rc, rin, lam3, gamma; int m;
    float* work;                               // bond_work [N * max_nbr, 4]
    float* grad; float* hw; float* pth; float* pthw; float* partial;
    float oscale; int oacc;
};

struct TersK {                                 // per-thread constants
    float A, B, h, lam1, lam2, beta, n, mh;    // mh = -1 / (2 n)
    float d2, gamma, gcd, gu2;                 // d^2, gamma, gamma (c/d)^2, 2 gamma (c/d)^2 d^2
    float R, rc, rin, pd;                      // pd = pi / (2 D)
    float lam3; int m;
};

template <class T> __device__ __forceinline__ T ters_mk(float v, float d);
template <> __device__ __forceinline__ float ters_mk<float>(float v, float) { return v; }
template <> __device__ __forceinline__ Dual ters_mk<Dual>(float v, float d) { return {v, d}; }
__device__ __forceinline__ float ters_dual(float) { return 0.f; }
__device__ __forceinline__ float ters_dual(Dual a) { return a.d; }

__device__ __forceinline__ TersK ters_constants(const TersArgs& A) {
    TersK K;
    K.A = A.theta ? A.theta[0] : A.A;
    K.B = A.theta ? A.theta[1] : A.B;
    K.h = A.theta ? A.theta[2] : A.h;
    K.lam1 = A.lam1; K.lam2 = A.lam2; K.beta = A.beta; K.n = A.n; K.mh = -0.5f / A.n;
    const float cd = A.c / A.d;
    K.d2 = A.d * A.d; K.gamma = A.gamma; K.gcd = A.gamma * (cd * cd); K.gu2 = 2.f * (K.gcd * K.d2);
    K.R = A.R; K.rc = A.rc; K.rin = A.rin; K.pd = 1.57079632679489662f / A.D;
    K.lam3 = A.lam3; K.m = A.m;
    return K;
}

// one list entry seen from its centre: unit vector centre -> end, r, 1/r, fc(r), fc'(r)
template <class T> struct TersEdge { T ex, ey, ez, r, ir, fc, dfc; };

// (dx, dy, dz) = end - centre with the stored image applied, (ax, ay, az) = w_end - w_centre.  False outside the support.
template <class T>
__device__ __forceinline__ bool ters_edge(const TersK& K, float dx, float dy, float dz, float ax, float ay, float az, TersEdge<T>& e) {
    const T x = ters_mk<T>(dx, ax), y = ters_mk<T>(dy, ay), z = ters_mk<T>(dz, az);
    const T d2 = x * x + y * y + z * z;
    const float rv = sqrtf(val(d2));
    if (!(rv > 0.f && rv < K.rc)) return false;              // the support test, on the r that fc is formed from
    e.r = fsqrt_(d2);
    e.ir = ters_mk<T>(1.f, 0.f) / e.r;
    e.ex = x * e.ir; e.ey = y * e.ir; e.ez = z * e.ir;
    if (rv <= K.rin) {
        e.fc = ters_mk<T>(1.f, 0.f); e.dfc = ters_mk<T>(0.f, 0.f);
    } else {
        const T arg = K.pd * (e.r - K.R);
        e.fc = 0.5f - 0.5f * fsin_(arg);
        e.dfc = (-0.5f * K.pd) * fcos_(arg);
    }
    return true;
}

// the entry in slot s of the row of a centre (position xc, seed wc) as an edge centre -> end; returns the end atom, or -1 when
// there is nothing to add
template <class T, int LEVEL>
__device__ __forceinline__ int ters_entry(const TersArgs& A, const TersK& K, size_t row, int s, float xc, float yc, float zc,
                                          float wxc, float wyc, float wzc, TersEdge<T>& e) {
    const int j = A.col[row + s];
    if ((unsigned)j >= (unsigned)A.N) return -1;
    float dx = xc - A.pos[3 * j], dy = yc - A.pos[3 * j + 1], dz = zc - A.pos[3 * j + 2];
    apply_shift(A.cell, A.shift[row + s], dx, dy, dz);                      // x_c - x_j - o.h
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (LEVEL >= 2) { ax = A.w[3 * j] - wxc; ay = A.w[3 * j + 1] - wyc; az = A.w[3 * j + 2] - wzc; }
    return ters_edge<T>(K, -dx, -dy, -dz, ax, ay, az, e) ? j : -1;
}

// One third atom k of the bond centre -> j:  t = fc(r_k) g(cos) E,  E = exp[(lam3 (r_j - r_k))^m],  th = dt/dh, and the
// derivatives with respect to the two vectors d_j, d_k (end - centre) as coefficients of the unit vectors:
//   dt/dd_j = cjj e_j + cjk e_k,   dt/dd_k = ckj e_j + ckk e_k
template <class T> struct TersTerm { T t, th, cjj, cjk, ckj, ckk; };

template <class T>
__device__ __forceinline__ TersTerm<T> ters_term(const TersK& K, const TersEdge<T>& ej, const TersEdge<T>& ek) {
    TersTerm<T> o;
    const T c = ej.ex * ek.ex + ej.ey * ek.ey + ej.ez * ek.ez;
    const T u = K.h - c;
    const T u2 = u * u;
    const T iden = ters_mk<T>(1.f, 0.f) / (u2 + K.d2);
    const T g = K.gcd * (u2 * iden) + K.gamma;
    const T gu = K.gu2 * (u * (iden * iden));                 // dg/du = dg/dh = -dg/dcos
    T gE = g, guE = gu, q = ters_mk<T>(0.f, 0.f);             // g E, dg/du E, fc(r_k) g dE/dr_j
    if (K.lam3 != 0.f) {
        const T a = K.lam3 * (ej.r - ek.r);
        T E, dE;
        if (K.m == 1) { E = fexp_(a); dE = K.lam3 * E; }
        else { const T a2 = a * a; E = fexp_(a2 * a); dE = (3.f * K.lam3) * (a2 * E); }
        gE = g * E; guE = gu * E;
        q = ek.fc * (g * dE);
    }
    o.t = ek.fc * gE;
    o.th = ek.fc * guE;
    // dcos/dd_j = (e_k - c e_j) / r_j, dcos/dd_k = (e_j - c e_k) / r_k, dr_j/dd_j = e_j, dr_k/dd_k = e_k
    const T pj = o.th * ej.ir, pk = o.th * ek.ir;
    o.cjj = pj * c + q;
    o.cjk = ters_mk<T>(0.f, 0.f) - pj;
    o.ckj = ters_mk<T>(0.f, 0.f) - pk;
    o.ckk = (ek.dfc * gE + pk * c) - q;
    return o;
}

// b(zeta) = (1 + (beta zeta)^n)^(-1/(2n)) and b'(zeta) = -1/2 b (beta zeta)^n / ((1 + (beta zeta)^n) zeta);  zeta = 0: (1, 0)
template <class T>
__device__ __forceinline__ void ters_bond_order(const TersK& K, T zeta, T& b, T& bp) {
    b = ters_mk<T>(1.f, 0.f); bp = ters_mk<T>(0.f, 0.f);
    if (!(val(zeta) > 0.f)) return;
    const T zn = fpow_(K.beta * zeta, K.n);
    const T q = zn + 1.f;
    b = fexp_(K.mh * flog_(q));
    bp = (-0.5f) * ((b * zn) / (q * zeta));
}

// ---- pass 1: the bonds i -> j of one atom.  out = (u_i; pA, pB, pH; their dual parts)
template <class T, int LEVEL>
__device__ __forceinline__ void ters_bonds(const TersArgs& A, const TersK& K, int i, int sub, float (&out)[7]) {
    const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
    float wxi = 0.f, wyi = 0.f, wzi = 0.f;
    if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
    const T zero = ters_mk<T>(0.f, 0.f);
    T pA = zero, pB = zero, pH = zero;        // d u_i / dA, d u_i / dB, d u_i / dh
    const int n = min(A.cnt[i], A.max_nbr);
    const size_t row = (size_t)i * A.max_nbr;
    for (int s = sub; s < n; s += TERS_LPA) {
        float* wk = (LEVEL >= 1 && A.work) ? A.work + 4 * (row + s) : nullptr;
        TersEdge<T> ej;
        if (ters_entry<T, LEVEL>(A, K, row, s, xi, yi, zi, wxi, wyi, wzi, ej) < 0) {
            if (wk) { wk[0] = 0.f; wk[1] = 0.f; wk[2] = 0.f; wk[3] = 0.f; }
            continue;
        }
        T zeta = zero, zh = zero;
        for (int t = 0; t < n; ++t) {
            if (t == s) continue;
            TersEdge<T> ek;
            if (ters_entry<T, LEVEL>(A, K, row, t, xi, yi, zi, wxi, wyi, wzi, ek) < 0) continue;
            const TersTerm<T> tt = ters_term<T>(K, ej, ek);
            zeta = zeta + tt.t;
            if (LEVEL >= 1) zh = zh + tt.th;
        }
        T b, bp;
        ters_bond_order<T>(K, zeta, b, bp);
        const T hR = 0.5f * (ej.fc * fexp_((-K.lam1) * ej.r));             // 1/2 fc exp(-lam1 r)
        const T hA = 0.5f * (ej.fc * fexp_((-K.lam2) * ej.r));             // 1/2 fc exp(-lam2 r)
        pA = pA + hR;
        pB = pB - b * hA;
        if (LEVEL >= 1) {
            const T P = (-K.B) * (hA * bp);                                // dU/dzeta of this bond
            pH = pH + P * zh;
            if (wk) { wk[0] = val(P); wk[1] = ters_dual(P); wk[2] = val(b); wk[3] = ters_dual(b); }
        }
    }
    out[0] = K.A * val(pA) + K.B * val(pB);
    if (LEVEL >= 1) {
        out[1] = val(pA); out[2] = val(pB); out[3] = val(pH);
        if (LEVEL >= 2) { out[4] = ters_dual(pA); out[5] = ters_dual(pB); out[6] = ters_dual(pH); }
    }
}

// LEVEL 0: U        1: + pth, bond_work        2: + pthw, bond_work with dual parts
template <int LEVEL>
__global__ void __launch_bounds__(TERS_BLOCK) tersoff_bond_kernel(const TersArgs A) {
    using T = typename std::conditional<LEVEL >= 2, Dual, float>::type;
    __shared__ float red[17];
    constexpr int apb = TERS_BLOCK / TERS_LPA;
    const int i = blockIdx.x * apb + threadIdx.x / TERS_LPA, sub = threadIdx.x % TERS_LPA;
    float e = 0.f;
    if (i < A.N) {
        const TersK K = ters_constants(A);
        float o[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) o[k] = 0.f;
        ters_bonds<T, LEVEL>(A, K, i, sub, o);
        constexpr int NV = LEVEL >= 2 ? 7 : (LEVEL >= 1 ? 4 : 1);
#pragma unroll
        for (int k = 0; k < NV; ++k) o[k] = group_sum<TERS_LPA>(o[k]);
        if (sub == 0) {
            e = o[0];
            if (LEVEL >= 1 && A.pth) { A.pth[3 * i] = o[1]; A.pth[3 * i + 1] = o[2]; A.pth[3 * i + 2] = o[3]; }
            if (LEVEL >= 2 && A.pthw) { A.pthw[3 * i] = o[4]; A.pthw[3 * i + 1] = o[5]; A.pthw[3 * i + 2] = o[6]; }
        }
    }
    if (A.partial) {                         // (block-uniform: a force-only evaluation has no scalar to reduce)
        e = block_sum(e, red);
        if (threadIdx.x == 0) A.partial[blockIdx.x] = e;
    }
}

// ---- pass 2
// the bonds j -> i and j -> k (k in row(j), k != i) seen from atom i, whose edge i -> j is ej: adds to (gx, gy, gz) what they
// contribute to dU/dx_i through zeta, and returns b_ji
template <class T, int LEVEL>
__device__ __forceinline__ T ters_around_neighbour(const TersArgs& A, const TersK& K, int i, int j, const TersEdge<T>& ej, T& gx,
                                                T& gy, T& gz) {
    const T zero = ters_mk<T>(0.f, 0.f);
    TersEdge<T> eji = ej;                                                   // the unit vector j -> i is -ej.e
    eji.ex = (-1.f) * ej.ex; eji.ey = (-1.f) * ej.ey; eji.ez = (-1.f) * ej.ez;
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
            Pji = ters_mk<T>(wk[0], wk[1]); bji = ters_mk<T>(wk[2], wk[3]);
            continue;
        }
        TersEdge<T> ek;                                                     // centre j -> end k, with j's own stored image
        if (ters_entry<T, LEVEL>(A, K, rowj, t, xj, yj, zj, wxj, wyj, wzj, ek) < 0) continue;
        // the bond j -> i with the third atom k: x_i moves d_ji
        const TersTerm<T> a = ters_term<T>(K, eji, ek);
        sj = sj + a.cjj;
        sx = sx + a.cjk * ek.ex; sy = sy + a.cjk * ek.ey; sz = sz + a.cjk * ek.ez;
        // the bond j -> k with the third atom i: x_i moves the second vector
        const TersTerm<T> c = ters_term<T>(K, ek, eji);
        const T Pjk = ters_mk<T>(wk[0], wk[1]);
        const T ca = Pjk * c.ckj, cb = Pjk * c.ckk;
        gx = gx + (ca * ek.ex + cb * eji.ex); gy = gy + (ca * ek.ey + cb * eji.ey); gz = gz + (ca * ek.ez + cb * eji.ez);
    }
    gx = gx + Pji * (sj * eji.ex + sx); gy = gy + Pji * (sj * eji.ey + sy); gz = gz + Pji * (sj * eji.ez + sz);
    return bji;
}

template <class T, int LEVEL>
__device__ __forceinline__ void ters_atom(const TersArgs& A, const TersK& K, int i, int sub, float (&out)[6]) {
    const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
    float wxi = 0.f, wyi = 0.f, wzi = 0.f;
    if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
    const T zero = ters_mk<T>(0.f, 0.f);
    T gx = zero, gy = zero, gz = zero;                       // dU/dx_i
    const int n = min(A.cnt[i], A.max_nbr);
    const size_t row = (size_t)i * A.max_nbr;
    for (int s = sub; s < n; s += TERS_LPA) {
        TersEdge<T> ej;
        const int j = ters_entry<T, LEVEL>(A, K, row, s, xi, yi, zi, wxi, wyi, wzi, ej);
        if (j < 0) continue;
        const float* wk = A.work + 4 * (row + s);
        const T Pij = ters_mk<T>(wk[0], wk[1]), bij = ters_mk<T>(wk[2], wk[3]);
        // ---- P_ij dzeta_ij/dx_i = -P_ij sum_k (dt/dd_j + dt/dd_k)
        T sj = zero, sx = zero, sy = zero, sz = zero;
        for (int t = 0; t < n; ++t) {
            if (t == s) continue;
            TersEdge<T> ek;
            if (ters_entry<T, LEVEL>(A, K, row, t, xi, yi, zi, wxi, wyi, wzi, ek) < 0) continue;
            const TersTerm<T> a = ters_term<T>(K, ej, ek);
            const T ck = a.cjk + a.ckk;
            sj = sj + (a.cjj + a.ckj);
            sx = sx + ck * ek.ex; sy = sy + ck * ek.ey; sz = sz + ck * ek.ez;
        }
        gx = gx - Pij * (sj * ej.ex + sx); gy = gy - Pij * (sj * ej.ey + sy); gz = gz - Pij * (sj * ej.ez + sz);
        // ---- the bonds of j that x_i enters through zeta
        const T bji = ters_around_neighbour<T, LEVEL>(A, K, i, j, ej, gx, gy, gz);
        // ---- the pair parts of i -> j and j -> i at fixed bond orders: d/dr of 1/2 fc (A exp(-lam1 r) - b B exp(-lam2 r)), twice
        const T eR = K.A * fexp_((-K.lam1) * ej.r), eA = K.B * fexp_((-K.lam2) * ej.r);
        const T bA = (0.5f * (bij + bji)) * eA;
        const T dV = ej.dfc * (eR - bA) + ej.fc * (K.lam2 * bA - K.lam1 * eR);
        gx = gx - dV * ej.ex; gy = gy - dV * ej.ey; gz = gz - dV * ej.ez;                      // d r / d x_i = -e
    }
    out[0] = val(gx); out[1] = val(gy); out[2] = val(gz);
    if (LEVEL >= 2) { out[3] = ters_dual(gx); out[4] = ters_dual(gy); out[5] = ters_dual(gz); }
}

__device__ __forceinline__ void ters_store3(float* dst, int i, float os, int oacc, float x, float y, float z) {
    if (oacc) { dst[3 * i] = fmaf(os, x, dst[3 * i]); dst[3 * i + 1] = fmaf(os, y, dst[3 * i + 1]); dst[3 * i + 2] = fmaf(os, z, dst[3 * i + 2]); }
    else { dst[3 * i] = os * x; dst[3 * i + 1] = os * y; dst[3 * i + 2] = os * z; }
}

// LEVEL 1: grad        2: + hw
template <int LEVEL>
__global__ void __launch_bounds__(TERS_BLOCK) tersoff_force_kernel(const TersArgs A) {
    using T = typename std::conditional<LEVEL >= 2, Dual, float>::type;
    const int i = blockIdx.x * (TERS_BLOCK / TERS_LPA) + threadIdx.x / TERS_LPA, sub = threadIdx.x % TERS_LPA;
    if (i >= A.N) return;
    const TersK K = ters_constants(A);
    float o[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = 0.f;
    ters_atom<T, LEVEL>(A, K, i, sub, o);
    constexpr int NV = LEVEL >= 2 ? 6 : 3;
#pragma unroll
    for (int k = 0; k < NV; ++k) o[k] = group_sum<TERS_LPA>(o[k]);
    if (sub != 0) return;
    if (A.grad) ters_store3(A.grad, i, A.oscale, A.oacc, o[0], o[1], o[2]);
    if (LEVEL >= 2 && A.hw) ters_store3(A.hw, i, A.oscale, A.oacc, o[3], o[4], o[5]);
}

// one wave, fixed summation order
__global__ void tersoff_finish(const float* __restrict__ partial, int nblocks, float* energy) {
    const int lane = threadIdx.x;
    float s = 0.f;
    for (int b = lane; b < nblocks; b += 64) s += partial[b];
    s = wave_sum(s);
    if (lane == 0) energy[0] = s;
}

}  // namespace

extern "C" int64_t mdg_tersoff_partial_size(int n_atoms) {
    if (n_atoms <= 0) return 0;
    const int apb = TERS_BLOCK / TERS_LPA;
    return (int64_t)((n_atoms + apb - 1) / apb);
}

extern "C" int64_t mdg_tersoff_work_size(int n_atoms, int max_nbr) {
    if (n_atoms <= 0 || max_nbr <= 0) return 0;
    return 4 * (int64_t)n_atoms * (int64_t)max_nbr;
}

extern "C" int mdg_tersoff_eval(const float* pos, int n_atoms, const MdgCell* cell, const int32_t* col, const int32_t* shift,
                                const int32_t* cnt, int max_nbr, const MdgTersoffConsts* k, const float* theta, const float* w,
                                float* energy, float* grad, float* hw, float* pth, float* pthw, float* partial, float* bond_work,
                                float out_scale, int accumulate, void* stream) {
    MDG_CHECK_ARG(pos && cell && col && shift && cnt, "tersoff_eval: null buffer (pos, cell or list)");
    MDG_CHECK_ARG(k, "tersoff_eval: consts is null");
    MDG_CHECK_ARG(n_atoms > 0 && max_nbr > 0, "tersoff_eval: bad sizes (n_atoms, max_nbr must be positive)");
    MDG_CHECK_ARG(theta || (k->A > 0.0 && k->B > 0.0), "tersoff_eval: consts need A > 0 and B > 0 (or a device theta)");
    MDG_CHECK_ARG(k->lam1 > 0.0 && k->lam2 > 0.0, "tersoff_eval: consts need lam1 > 0 and lam2 > 0");
    MDG_CHECK_ARG(k->D > 0.0 && k->R > k->D, "tersoff_eval: consts need D > 0 and R > D");
    MDG_CHECK_ARG(k->m == 1 || k->m == 3, "tersoff_eval: m must be 1 or 3");
    MDG_CHECK_ARG(k->n > 0.0 && k->beta >= 0.0, "tersoff_eval: consts need n > 0 and beta >= 0");
    MDG_CHECK_ARG(k->d != 0.0, "tersoff_eval: d must not be 0");
    MDG_CHECK_ARG(w || !(hw || pthw), "tersoff_eval: hw / pthw need w");
    MDG_CHECK_ARG(!w || hw || pthw, "tersoff_eval: w given without hw or pthw output");
    MDG_CHECK_ARG(energy || grad || hw || pth || pthw, "tersoff_eval: no output requested");
    MDG_CHECK_ARG(!energy || partial, "tersoff_eval: energy needs the partial buffer");
    MDG_CHECK_ARG(bond_work || !(grad || hw),
                  "tersoff_eval: grad / hw need bond_work (the scratch of the bond pass, mdg_tersoff_work_size() floats)");
    const int level = w ? 2 : ((grad || pth) ? 1 : 0);
    // (accumulate bit 2, "the list was searched with a skin", needs nothing here: the support test r < R + D is always applied)
    TersArgs a{pos, n_atoms, *cell, col, shift, cnt, max_nbr, theta, w,
               (float)k->A, (float)k->B, (float)k->h, (float)k->lam1, (float)k->lam2, (float)k->beta, (float)k->n, (float)k->c,
               (float)k->d, (float)k->R, (float)k->D, (float)(k->R + k->D), (float)(k->R - k->D), (float)k->lam3,
               (float)k->gamma, (int)k->m, bond_work, grad, hw, pth, pthw, energy ? partial : nullptr, out_scale, accumulate & 1};
    const int nblocks = (int)mdg_tersoff_partial_size(n_atoms);
    dim3 grid(nblocks);
    hipStream_t st = (hipStream_t)stream;
    const bool forces = grad || hw;
    if (level == 2) {
        hipLaunchKernelGGL((tersoff_bond_kernel<2>), grid, dim3(TERS_BLOCK), 0, st, a);
        if (forces) hipLaunchKernelGGL((tersoff_force_kernel<2>), grid, dim3(TERS_BLOCK), 0, st, a);
    } else if (level == 1) {
        hipLaunchKernelGGL((tersoff_bond_kernel<1>), grid, dim3(TERS_BLOCK), 0, st, a);
        if (forces) hipLaunchKernelGGL((tersoff_force_kernel<1>), grid, dim3(TERS_BLOCK), 0, st, a);
    } else {
        hipLaunchKernelGGL((tersoff_bond_kernel<0>), grid, dim3(TERS_BLOCK), 0, st, a);
    }
    if (energy) hipLaunchKernelGGL(tersoff_finish, dim3(1), dim3(64), 0, st, partial, nblocks, energy);
    MDG_CHECK_LAUNCH("tersoff_kernel");
    return MDG_OK;
}
