// K38: Tersoff energy of every frame of a trajectory, list-free -- thermo.TersoffEnergy, the energy side of trajectory
// reweighting (mdgrad_amd/reweight.py) for the bond-order models of csrc/tersoff.hip (K25) and csrc/tersoff_multi.hip (K26).
//
//   U[f]         = 1/2 sum_i sum_{j in row(i)} fc_ab(r_ij) [ A_ab exp(-lam1_ab r_ij) - b_ij B_ab exp(-lam2_ab r_ij) ]
//   dU_dtheta[f] = dU[f] / d(A, B, h)                                                from the same pass, when asked for
//
// with the definition, the formulas and the conventions of csrc/tersoff_core.hpp (read its header first): g in the
// cancellation-free form, b = 1 with zero derivatives where zeta = 0, the support test 0 < r < R_ab + D_ab on r = sqrtf(d2) with
// the entry of the directed pair (centre species, end species), exp[(lam3 (r_ij - r_ik))^m] for the one-species view.  The
// energy and dU/d(A, B, h) need the bond pass only: this file is ters_bonds without bond_work, over the neighbours an atom
// finds in its own frame -- D = x_j - x_i re-imaged with the strict minimum image on the diagonal cell
// (csrc/frame_pairs.hpp).  No list exists and nothing is searched or read on the host.
//
// Two parameter views (the protocol of tersoff_core.hpp):
//   TersFrameOneView     one species: the constants from the kernel arguments, (A, B, h) from the device theta[3]; P = 3
//   TersFrameTableView   1 <= S <= 4 species: the device table of K26 (8 S (S + 1) floats) and one frame's species (a byte per
//                        atom, clamped into the table), both staged into LDS once per workgroup; P = 2 S^2 + S in the order
//                        (A.flat, B.flat, h) of K26's pth
//
// Shape: the scaffold of csrc/frame_atoms.hpp.  Every thread, for each of its atoms,
//   1. builds the row of the atoms inside the support of (t_i, t_j) (build_row);
//   2. for every slot s forms zeta_is by a loop over the row, then b and b', the bond's half energy and
//      d u_i / d(A[a, .], B[a, .], h[a]);
//   3. adds them into per-thread sums (constant indices and predicated adds: nothing is indexed by a run-time species).
// The zeta loop rebuilds the edge of k for every j, as the list kernel does.
// Row cap: TF_ROW_CAP = 32 entries (16 KB of LDS for the 256 rows of a workgroup; silicon, carbon, germanium and their alloys
// hold 3 - 10 neighbours inside R + D); a frame in which any atom has more neighbours comes out NaN in U and dU_dtheta, alone.
//
// Every sum runs in a fixed order: per atom in slot order, per thread in atom order, then the shuffle / LDS trees of
// common.hpp.  No floating-point atomics; a frame's arithmetic does not depend on where it stands in the batch, and the value
// part does not depend on whether dU_dtheta is asked for (no fused multiply-add is formed in this file).
#pragma clang fp contract(off)
#include "tersoff_core.hpp"
#include "frame_atoms.hpp"

namespace {

using namespace frame_pairs;

constexpr int TF_ROW_CAP = 32;
constexpr int TF_SMAX = 4;                    // species of the table view

struct TfArgs {
    const float* pos;
    float* U; float* dU;
    int F, N;
    MdgCell cell;
};

// ---- one species: K25's view, fed from the kernel arguments and the device theta
struct TfOneArgs {
    const float* theta;                        // device (A, B, h)
    float lam1, lam2, beta, n, c, d, R, D, rc, rin, lam3, gamma; int m;
};

struct TersFrameOneView {
    using Args = TfOneArgs;
    static constexpr bool HAS_LAM3 = true;
    static constexpr int SMAX = 1;
    static constexpr int S = 1;
    static constexpr int LDS_FLOATS = 1, LDS_TYPES = 1;      // (nothing is staged)
    TersEntry pp, cc;
    float lam3; int m;

    __device__ __forceinline__ TersFrameOneView(const TfOneArgs& a, int, float*, uint8_t*) {
        const float A = a.theta[0], B = a.theta[1], h = a.theta[2];
        const float cd = a.c / a.d, d2 = a.d * a.d, gcd = a.gamma * (cd * cd);
        pp.v[PA_A] = A; pp.v[PA_B] = B; pp.v[PA_L1] = a.lam1; pp.v[PA_L2] = a.lam2;
        pp.v[PA_R] = a.R; pp.v[PA_RIN] = a.rin; pp.v[PA_RC] = a.rc; pp.v[PA_PD] = 1.57079632679489662f / a.D;
        cc.v[CE_H] = h; cc.v[CE_BETA] = a.beta; cc.v[CE_N] = a.n; cc.v[CE_MH] = -0.5f / a.n;
        cc.v[CE_D2] = d2; cc.v[CE_GAMMA] = a.gamma; cc.v[CE_GCD] = gcd; cc.v[CE_GU2] = 2.f * (gcd * d2);
        lam3 = a.lam3; m = a.m;
    }
    __device__ __forceinline__ int species(int) const { return 0; }
    __device__ __forceinline__ const TersEntry& pair(int, int) const { return pp; }
    __device__ __forceinline__ const TersEntry& centre(int) const { return cc; }
};

// ---- 1 <= S <= 4 species: K26's table and one frame's species in LDS
struct TfTableArgs {
    const int32_t* types; int S;
    const float* tables;                       // device, 8 S (S + 1) floats
};

struct TersFrameTableView {
    using Args = TfTableArgs;
    static constexpr bool HAS_LAM3 = false;
    static constexpr int SMAX = TF_SMAX;
    static constexpr int LDS_FLOATS = 8 * TF_SMAX * (TF_SMAX + 1), LDS_TYPES = FP_GROUP_ATOMS;
    int S;
    const TersEntry* tab;
    const uint8_t* ty;

    // every thread of the workgroup constructs the view (one barrier)
    __device__ __forceinline__ TersFrameTableView(const TfTableArgs& a, int N, float* flat, uint8_t* sty) : S(a.S) {
        const int n = 8 * S * (S + 1);
        for (int k = threadIdx.x; k < n; k += FP_BLOCK) flat[k] = a.tables[k];
        for (int i = threadIdx.x; i < N; i += FP_BLOCK) sty[i] = (uint8_t)min(max(a.types[i], 0), S - 1);
        __syncthreads();
        tab = reinterpret_cast<const TersEntry*>(flat);
        ty = sty;
    }
    __device__ __forceinline__ int species(int i) const { return ty[i]; }
    __device__ __forceinline__ const TersEntry& pair(int a, int b) const { return tab[a * S + b]; }
    __device__ __forceinline__ const TersEntry& centre(int a) const { return tab[S * S + a]; }
};

// the edge centre -> j of a staged frame under the pair entry pp; false outside its support
__device__ __forceinline__ bool tf_edge(const MdgCell& cell, const TersEntry& pp, const float* sx, const float* sy,
                                        const float* sz, int j, float xi, float yi, float zi, TersEdge<float>& e) {
    float dx = sx[j] - xi, dy = sy[j] - yi, dz = sz[j] - zi;
    min_image<true>(cell, dx, dy, dz);
    if (!ters_geom<float>(dx, dy, dz, 0.f, 0.f, 0.f, pp[PA_RC], e)) return false;
    return ters_taper<float>(pp, e);
}

template <class P, int TPF, bool DTH>
__global__ __launch_bounds__(FP_BLOCK) void tersoff_frames_kernel(const TfArgs A, const typename P::Args V) {
    using C = FrameCtx<TPF>;
    constexpr int SMAX = P::SMAX;
    // per-thread sums: U, overflowing rows, then dU/d(A[a, b], B[a, b], h[a]) at the register stride SMAX
    constexpr int NTH = DTH ? 2 * SMAX * SMAX + SMAX : 0, NV = 2 + NTH;
    constexpr int OA = 2, OB = 2 + SMAX * SMAX, OH = 2 + 2 * SMAX * SMAX;
    __shared__ float sp[C::FPB * 3 * C::CAP];
    __shared__ uint16_t rows[TF_ROW_CAP * FP_BLOCK];
    __shared__ float red[(FP_BLOCK / MDG_WAVE) * NV];
    __shared__ float stab[P::LDS_FLOATS];
    __shared__ uint8_t sty[P::LDS_TYPES];
    const P p(V, A.N, stab, sty);
    const C fr = open_frame<TPF>(sp, A.pos, A.F, A.N);
    const float *sx = fr.sx, *sy = fr.sy, *sz = fr.sz;
    uint16_t* row = rows + threadIdx.x;
    float v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.f;
    if (fr.live) {
        for (int i = fr.t; i < fr.N; i += TPF) {
            const float xi = sx[i], yi = sy[i], zi = sz[i];
            const int ti = p.species(i);
            // ---- 1. the row of atom i: the atoms inside the support of (t_i, t_j) (ters_geom's support test)
            int over;
            const int n = build_row<TF_ROW_CAP, C::CAP>(row, A.cell, fr.sf, fr.N, i, over, [&](int j, float rv) {
                return rv < p.pair(ti, p.species(j))[PA_RC];
            });
            if (over) { v[1] += 1.f; continue; }
            // ---- 2. the bonds i -> j of the row (ters_bonds without bond_work)
            const TersEntry& cc = p.centre(ti);
            float pa[SMAX], pb[SMAX], ph = 0.f;
#pragma unroll
            for (int q = 0; q < SMAX; ++q) { pa[q] = 0.f; pb[q] = 0.f; }
            for (int s = 0; s < n; ++s) {
                const int j = row_at(row, s);
                const int tj = p.species(j);
                const TersEntry& pp = p.pair(ti, tj);
                TersEdge<float> ej;
                if (!tf_edge(A.cell, pp, sx, sy, sz, j, xi, yi, zi, ej)) continue;
                float zeta = 0.f, zh = 0.f;
                for (int u = 0; u < n; ++u) {
                    if (u == s) continue;
                    const int k = row_at(row, u);
                    TersEdge<float> ek;
                    if (!tf_edge(A.cell, p.pair(ti, p.species(k)), sx, sy, sz, k, xi, yi, zi, ek)) continue;
                    const TersTerm<float> tt = ters_term<float>(p, cc, ej, ek);
                    zeta = zeta + tt.t;
                    if (DTH) zh = zh + tt.th;
                }
                float b, bp;
                ters_bond_order<float>(cc, zeta, b, bp);
                const float hR = 0.5f * (ej.fc * fexp_((-pp[PA_L1]) * ej.r));       // 1/2 fc exp(-lam1 r)
                const float hA = 0.5f * (ej.fc * fexp_((-pp[PA_L2]) * ej.r));       // 1/2 fc exp(-lam2 r)
                const float bA = b * hA;
#pragma unroll
                for (int q = 0; q < SMAX; ++q) {                                    // (constant indices: the sums stay in registers)
                    if (q == tj) { pa[q] = pa[q] + hR; pb[q] = pb[q] - bA; }
                }
                if (DTH) {
                    const float Pb = (-pp[PA_B]) * (hA * bp);                       // dU/dzeta of this bond
                    ph = ph + Pb * zh;
                }
            }
            // ---- 3. u_i and d u_i / d(A[a, .], B[a, .], h[a]) into the thread's sums
            float e = 0.f;
#pragma unroll
            for (int q = 0; q < SMAX; ++q) {
                if (q < p.S) {
                    const TersEntry& pq = p.pair(ti, q);
                    e = e + (pq[PA_A] * pa[q] + pq[PA_B] * pb[q]);
                }
            }
            v[0] += e;
            if constexpr (DTH) {
#pragma unroll
                for (int a = 0; a < SMAX; ++a) {
                    if (a == ti) {
#pragma unroll
                        for (int q = 0; q < SMAX; ++q) {
                            v[OA + a * SMAX + q] += pa[q];
                            v[OB + a * SMAX + q] += pb[q];
                        }
                        v[OH + a] += ph;
                    }
                }
            }
        }
    }
    if (frame_sums(fr, v, red)) {
        const bool bad = v[1] > 0.f;
        A.U[fr.f] = nan_if(bad, v[0]);
        if constexpr (DTH) {
            const int S = p.S, S2 = S * S;
            float* d = A.dU + (size_t)fr.f * (2 * S2 + S);
#pragma unroll
            for (int a = 0; a < SMAX; ++a) {
                if (a < S) {
#pragma unroll
                    for (int q = 0; q < SMAX; ++q) {
                        if (q < S) {
                            d[a * S + q] = nan_if(bad, v[OA + a * SMAX + q]);
                            d[S2 + a * S + q] = nan_if(bad, v[OB + a * SMAX + q]);
                        }
                    }
                    d[2 * S2 + a] = nan_if(bad, v[OH + a]);
                }
            }
        }
    }
}

template <class P>
inline void tersoff_frames_launch(const TfArgs& a, const typename P::Args& v, hipStream_t st) {
    launch_frames(a.F, a.N, a.dU != nullptr, [&](auto tpf, auto dth, dim3 grid) {
        hipLaunchKernelGGL((tersoff_frames_kernel<P, decltype(tpf)::value, decltype(dth)::value>), grid, dim3(FP_BLOCK), 0, st,
                           a, v);
    });
}

}  // namespace

extern "C" int mdg_tersoff_frames_row_cap(void) { return TF_ROW_CAP; }

extern "C" int mdg_tersoff_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const MdgTersoffConsts* k,
                                      const float* theta, float* U, float* dU_dtheta, void* stream) {
    const int rc = check_frames("tersoff_frames_fwd", pos, cell, k, n_frames, n_atoms, FP_GROUP_ATOMS);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(theta, "tersoff_frames_fwd: theta is null (the device buffer (A, B, h) is required)");
    MDG_CHECK_ARG(U, "tersoff_frames_fwd: null output U");
    MDG_CHECK_ARG(k->lam1 > 0.0 && k->lam2 > 0.0, "tersoff_frames_fwd: consts need lam1 > 0 and lam2 > 0");
    MDG_CHECK_ARG(k->D > 0.0 && k->R > k->D, "tersoff_frames_fwd: consts need D > 0 and R > D");
    MDG_CHECK_ARG(k->m == 1 || k->m == 3, "tersoff_frames_fwd: m must be 1 or 3");
    MDG_CHECK_ARG(k->n > 0.0 && k->beta >= 0.0, "tersoff_frames_fwd: consts need n > 0 and beta >= 0");
    MDG_CHECK_ARG(k->d != 0.0, "tersoff_frames_fwd: d must not be 0");
    const TfArgs a{pos, U, dU_dtheta, n_frames, n_atoms, *cell};
    const TfOneArgs v{theta, (float)k->lam1, (float)k->lam2, (float)k->beta, (float)k->n, (float)k->c, (float)k->d, (float)k->R,
                      (float)k->D, (float)(k->R + k->D), (float)(k->R - k->D), (float)k->lam3, (float)k->gamma, (int)k->m};
    tersoff_frames_launch<TersFrameOneView>(a, v, (hipStream_t)stream);
    MDG_CHECK_LAUNCH("tersoff_frames_kernel");
    return MDG_OK;
}

extern "C" int mdg_tersoff_multi_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const int32_t* types,
                                            int n_species, const float* tables, float* U, float* dU_dtheta, void* stream) {
    const int rc = check_frames("tersoff_multi_frames_fwd", pos, cell, tables, n_frames, n_atoms, FP_GROUP_ATOMS);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(n_species >= 1 && n_species <= TF_SMAX, "tersoff_multi_frames_fwd: n_species must lie in [1, %d] (got %d)",
                  TF_SMAX, n_species);
    MDG_CHECK_ARG(types, "tersoff_multi_frames_fwd: types is null (device int32 [n_atoms], one frame's species)");
    MDG_CHECK_ARG(U, "tersoff_multi_frames_fwd: null output U");
    const TfArgs a{pos, U, dU_dtheta, n_frames, n_atoms, *cell};
    const TfTableArgs v{types, n_species, tables};
    tersoff_frames_launch<TersFrameTableView>(a, v, (hipStream_t)stream);
    MDG_CHECK_LAUNCH("tersoff_multi_frames_kernel");
    return MDG_OK;
}
