// K36, K37: embedded-atom energy of every frame of a trajectory, list-free -- thermo.EAMEnergy, the energy side of trajectory
// reweighting (mdgrad_amd/reweight.py) for the tabulated term of csrc/eam_table.hip (K27) and the Sutton-Chen term of
// csrc/eam.hip (K24).
//
//   U[f] = sum_i [ 1/2 sum_j phi_ab(r_ij) + F_a(rho_i) ],   rho_i = sum_j f_b(r_ij)                 K27's / K24's definition
//
// over the atoms j of i's own frame: D = x_j - x_i re-imaged with the strict minimum image on the diagonal cell
// (csrc/frame_pairs.hpp), r = sqrtf(d2) with the un-contracted d2, 0 < r < rc.  Nothing is searched and no list exists; the
// value is the one the model gives for the frame.
//
// Shape: the scaffold of csrc/frame_atoms.hpp.  Every thread walks the whole frame once for each of its atoms: when the walk
// ends it holds both 1/2 sum phi and rho_i and applies F on the spot.  No rows, no row cap, no second pass.  K37 walks with
// walk_all; the two K36 kernels write the same loop out (ETF_WALK): through the callable their table offsets compile to other
// instructions, measured 1 - 2 % slower on an MI355X at 4 096 frames, with the same bits.
//
// K36 (tabulated): one bracket (g, t) per pair serves the phi_ab and the f_b lookup (csrc/eam_table_core.hpp).  The r-tables
// (pair and density) are read from a workgroup copy in LDS when they hold at most EF_LDS_TABLE_FLOATS floats and four frames
// share the copy (the wave-per-frame shape), from global memory through the caches otherwise: measured on an MI355X at 4 096
// frames and 1 024-node tables, the copy is 7 % faster at 108 atoms and 4 % slower at 256, where every frame pays for its own
// (docs/KERNELS.md K36); F, one lookup per atom, always from global memory.  K36b, the node gradient of sum_f gU_f U_f, is the same walk adding 1/2 gU_f basis(r_ij) to phi_ab,
// gU_f F_a'(rho_i) basis(r_ij) to f_b and, once per atom, gU_f basis(rho_i) to F_a: fx64 fixed point, integer atomics only
// (per workgroup in LDS first when the table set holds at most EF_LDS_WORDS words), at power-of-two scales taken on the device
// from bounds (max |gU|, max |F'| and max |basis(rho)| over the saved rho, the bound of basis(r) and the number of
// contributions), so that no sum can leave 2^62 and nothing is read on the host.
//
// K37 (Sutton-Chen): the closed-form S_n, S_m of csrc/eam_core.hpp with the live device (epsilon, a, c); the same pass emits
// dU[f]/d(epsilon, a, c) when asked (K24's pth formulas: S_k is homogeneous of degree k in a).
//
// Every floating-point sum runs in a fixed order: per atom in frame order, per thread in atom order, then the shuffle / LDS
// trees of common.hpp.  No floating-point atomics; a frame's arithmetic does not depend on where it stands in the batch, so
// permuting the frames permutes U bit for bit and leaves the node gradient (integer sums) unchanged bit for bit; the value part
// does not depend on whether rho or dU_dtheta is asked for (no fused multiply-add is formed in this file).
#include "eam_table_core.hpp"
#include "eam_core.hpp"
#include "frame_atoms.hpp"

namespace {

using namespace frame_pairs;

constexpr int EF_LDS_TABLE_FLOATS = 8192;     // forward: r-tables of at most 32 KiB get a workgroup copy in LDS
constexpr int EF_LDS_WORDS = 6144;            // node gradient: a table set of at most 48 KiB of int64 words is summed in LDS first
enum { EF_GU = 0, EF_FP, EF_EM, EF_NB };      // max |gU|, |F'(rho)|, |basis(rho)| as float bits in the first words of fx

// walk_all of csrc/frame_atoms.hpp written out for K36: atom i (at xi, yi, zi) of the frame `fr` against j = 0 .. N - 1 in
// index order, the body run with r = sqrtf(d2) for the atoms inside K27's support 0 < r < rc
#define ETF_WALK(fr, A, i, j, r)                                                                           \
    for (int j = 0; j < (fr).N; ++j)                                                                       \
        if (float dx_ = (fr).sx[j] - xi, dy_ = (fr).sy[j] - yi, dz_ = (fr).sz[j] - zi, d2_;                \
            j != i && pair_in((A).cell, __int_as_float(0x7f800000), dx_, dy_, dz_, d2_))                   \
            if (const float r = sqrtf(d2_); r > 0.f && r < (A).rc)

struct EtfArgs {
    const float* pos; const int32_t* types; const float* tab;
    float* U; float* rho;                      // forward
    const float* gU; const float* rho_in;      // node gradient
    unsigned long long* fx;                    // [ET_BOUNDS + table words]
    int F, N; MdgCell cell;
    int S, nr, nrho;
    float rmin, inv_hr, rhomin, inv_hrho, rc;
    int r_floats;                              // floats of the pair and density tables
    int lds_words;                             // > 0: the node gradient adds into a workgroup copy of the words in LDS first
    float lim_edge, lim_atom, bv;              // fx64_limit of a word fed by the pairs / by the atoms; the bound of |basis(r)|
};

__device__ __forceinline__ void etf_stage_types(uint8_t* sty, const EtfArgs& A) {
    for (int e = threadIdx.x; e < A.N; e += FP_BLOCK) sty[e] = (uint8_t)min(max(A.types[e], 0), A.S - 1);
}

// ---------------------------------------------------------------------------------- K36 forward
template <int TPF, bool LDS_TAB>
__global__ __launch_bounds__(FP_BLOCK) void etf_fwd_kernel(const EtfArgs A) {
    using C = FrameCtx<TPF>;
    __shared__ float sp[C::FPB * 3 * C::CAP];
    __shared__ uint8_t sty[C::CAP];
    __shared__ float red[17];
    extern __shared__ float etf_tab[];                        // LDS_TAB: [r_floats], the pair and density tables
    etf_stage_types(sty, A);
    if (LDS_TAB) {
        for (int e = threadIdx.x; e < A.r_floats; e += FP_BLOCK) etf_tab[e] = A.tab[e];
    }
    const C fr = open_frame<TPF>(sp, A.pos, A.F, A.N);
    const float* rt = LDS_TAB ? etf_tab : A.tab;
    float en = 0.f;
    if (fr.live) {
        for (int i = fr.t; i < fr.N; i += TPF) {
            const float xi = fr.sx[i], yi = fr.sy[i], zi = fr.sz[i];
            const int a = sty[i];
            float SP = 0.f, R = 0.f;
            ETF_WALK(fr, A, i, j, r) {
                const int b = sty[j];
                EtBasis<float> B;
                et_basis<float>(r, A.rmin, A.inv_hr, A.nr, B);
                SP = SP + et_dot<float>(B.b, rt + et_pair_off(et_pair(a, b), A.nr) + 2 * B.g);
                R = R + et_dot<float>(B.b, rt + et_dens_off(A.S, b, A.nr) + 2 * B.g);
            }
            EtBasis<float> B;
            et_basis<float>(R, A.rhomin, A.inv_hrho, A.nrho, B);
            const float Fe = et_dot<float>(B.b, A.tab + et_embed_off(A.S, a, A.nr, A.nrho) + 2 * B.g);
            en = en + (0.5f * SP + Fe);                       // u_i = 1/2 sum_j phi + F_a(rho_i)
            if (A.rho) A.rho[(size_t)fr.f * fr.N + i] = R;
        }
    }
    en = TPF == MDG_WAVE ? wave_sum(en) : block_sum(en, red);
    if (fr.live && fr.t == 0) A.U[fr.f] = en;
}

// ---------------------------------------------------------------------------------- K36b node gradient
__global__ void etf_zero_kernel(unsigned long long* fx, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) fx[k] = 0ull;
}

// F_a'(rho) and the weights of the four embedding entries at the saved rho of atom `idx` of the flat [F, N]
__device__ __forceinline__ float etf_embed(const EtfArgs& A, float rho, int a, EtBasis<float>& B, size_t& off) {
    et_basis<float>(rho, A.rhomin, A.inv_hrho, A.nrho, B);
    off = et_embed_off(A.S, a, A.nr, A.nrho) + 2 * B.g;
    return A.inv_hrho * et_dot<float>(B.d, A.tab + off);
}

// the bounds: one integer atomic maximum per bound and workgroup, and only where it raises the bound
__global__ __launch_bounds__(FP_BLOCK) void etf_bounds_kernel(const EtfArgs A) {
    __shared__ float mred[FP_BLOCK / MDG_WAVE][EF_NB];
    const long long idx = (long long)blockIdx.x * FP_BLOCK + threadIdx.x, total = (long long)A.F * A.N;
    float m[EF_NB] = {0.f, 0.f, 0.f};
    if (idx < A.F) m[EF_GU] = fabsf(A.gU[idx]);
    if (idx < total) {
        const int a = min(max(A.types[idx % A.N], 0), A.S - 1);
        EtBasis<float> B;
        size_t off;
        m[EF_FP] = fabsf(etf_embed(A, A.rho_in[idx], a, B, off));
#pragma unroll
        for (int k = 0; k < 4; ++k) m[EF_EM] = fmaxf(m[EF_EM], fabsf(B.b[k]));
    }
    unsigned* u = (unsigned*)A.fx;
#pragma unroll
    for (int k = 0; k < EF_NB; ++k) {
        const float v = wave_max(m[k]);
        if ((threadIdx.x & 63) == 0) mred[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < EF_NB) {
        float v = 0.f;
        for (int wv = 0; wv < FP_BLOCK / MDG_WAVE; ++wv) v = fmaxf(v, mred[wv][threadIdx.x]);
        // (non-negative floats order like their bits; an infinite bound ends in a scale of 1)
        if (v > 0.f) atomicMax(u + threadIdx.x, __float_as_uint(v));
    }
}

// the scales of the pair, density and embedding words from the bounds
__device__ __forceinline__ void etf_scales(const unsigned long long* fx, float bv, float lim_edge, float lim_atom, float (&s)[3]) {
    const unsigned* u = (const unsigned*)fx;
    const float gu = __uint_as_float(u[EF_GU]), fp = __uint_as_float(u[EF_FP]), em = __uint_as_float(u[EF_EM]);
    s[0] = et_pow2(0.5f * gu * bv, lim_edge);
    s[1] = et_pow2(gu * fp * bv, lim_edge);
    s[2] = et_pow2(gu * em, lim_atom);
}

template <int TPF>
__global__ __launch_bounds__(FP_BLOCK) void etf_nodes_kernel(const EtfArgs A) {
    using C = FrameCtx<TPF>;
    __shared__ float sp[C::FPB * 3 * C::CAP];
    __shared__ uint8_t sty[C::CAP];
    extern __shared__ unsigned long long etf_acc[];           // [lds_words]: this workgroup's share of the words
    unsigned long long* fxw = A.fx + ET_BOUNDS;
    const bool lds = A.lds_words > 0;                         // (grid-uniform)
    etf_stage_types(sty, A);
    if (lds) {
        for (int k = threadIdx.x; k < A.lds_words; k += FP_BLOCK) etf_acc[k] = 0ull;
    }
    const C fr = open_frame<TPF>(sp, A.pos, A.F, A.N);
    auto add = [&](size_t word, float v) {
        if (v == 0.f) return;
        if (lds) atomicAdd(etf_acc + word, fx64(v)); else atomicAdd(fxw + word, fx64(v));
    };
    const float gw = fr.live ? A.gU[fr.f] : 0.f;
    if (fr.live && gw != 0.f) {                                  // (a frame of weight zero adds nothing)
        float sc[3];
        etf_scales(A.fx, A.bv, A.lim_edge, A.lim_atom, sc);
        for (int i = fr.t; i < fr.N; i += TPF) {
            const float xi = fr.sx[i], yi = fr.sy[i], zi = fr.sz[i];
            const int a = sty[i];
            EtBasis<float> E;
            size_t eoff;
            const float FpI = etf_embed(A, A.rho_in[(size_t)fr.f * fr.N + i], a, E, eoff);
#pragma unroll
            for (int k = 0; k < 4; ++k) add(eoff + k, (gw * E.b[k]) * sc[2]);
            const float cp = 0.5f * gw, cd = gw * FpI;
            ETF_WALK(fr, A, i, j, r) {
                const int b = sty[j];
                EtBasis<float> B;
                et_basis<float>(r, A.rmin, A.inv_hr, A.nr, B);
                const size_t wp = et_pair_off(et_pair(a, b), A.nr) + 2 * B.g, wd = et_dens_off(A.S, b, A.nr) + 2 * B.g;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    add(wp + k, (cp * B.b[k]) * sc[0]);
                    add(wd + k, (cd * B.b[k]) * sc[1]);
                }
            }
        }
    }
    if (lds) {                               // the words this workgroup touched, one integer atomic each
        __syncthreads();
        for (int k = threadIdx.x; k < A.lds_words; k += FP_BLOCK) {
            const unsigned long long v = etf_acc[k];
            if (v != 0ull) atomicAdd(fxw + k, v);
        }
    }
}

// the fixed-point words as floats; pinned: the last node of every phi and f table is returned as exactly 0
__global__ void etf_finish_kernel(const unsigned long long* fx, int64_t n_words, float bv, float lim_edge, float lim_atom, int S,
                                  int nr, int pin, float* out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_words) return;
    float s[3];
    etf_scales(fx, bv, lim_edge, lim_atom, s);
    const int64_t r_words = 2 * (int64_t)(et_npair(S) + S) * nr;
    const int fam = k < 2 * (int64_t)et_npair(S) * nr ? 0 : (k < r_words ? 1 : 2);
    float v = (float)((double)(long long)fx[ET_BOUNDS + k] * (1.0 / (double)s[fam]));      // (s is a power of two: exact)
    if (pin && fam < 2 && (k / 2) % nr == nr - 1) v = 0.f;
    out[k] = v;
}

// ---------------------------------------------------------------------------------- K37 Sutton-Chen
struct EsfArgs {
    const float* pos; const float* theta;
    float* U; float* dU;
    int F, N; MdgCell cell;
    float rc; int n, m, shifted;
};

template <int TPF, bool DTH>
__global__ __launch_bounds__(FP_BLOCK) void eam_frames_kernel(const EsfArgs A) {
    using C = FrameCtx<TPF>;
    constexpr int NV = 4;                                     // U, dU/d(eps, a, c)
    __shared__ float sp[C::FPB * 3 * C::CAP];
    __shared__ float red[(FP_BLOCK / MDG_WAVE) * NV];
    const C fr = open_frame<TPF>(sp, A.pos, A.F, A.N);
    const EamK K = eam_constants(A.theta[0], A.theta[1], A.theta[2], A.rc, A.n, A.m, A.shifted);
    float v[NV] = {0.f, 0.f, 0.f, 0.f};
    if (fr.live) {
        for (int i = fr.t; i < fr.N; i += TPF) {
            float SP = 0.f, R = 0.f;
            walk_all<C::CAP>(A.cell, fr.sf, fr.N, i, [&](int, float dx, float dy, float dz, float) {
                EamEdge<float> e;
                if (!eam_edge<float>(K, dx, dy, dz, 0.f, 0.f, 0.f, e)) return;        // K24's support test
                const float sr = K.a * e.ir;
                float Sn, dSn, Sm, dSm;
                eam_shape<float>(e, sr, K.n, K.fn, K.qn, K.ln, K.rc, Sn, dSn);
                eam_shape<float>(e, sr, K.m, K.fm, K.qm, K.lm, K.rc, Sm, dSm);
                SP = SP + Sn;
                R = R + Sm;
            });
            // u_i = eps (1/2 sum_j S_n - c sqrt(rho_i)) and its parameter derivatives (eam_force_kernel's pe, pa, pc);
            // rho_i <= 0 (no neighbour): embedding energy and F' exactly 0
            const bool dense = R > 0.f;
            const float rho = dense ? R : 0.f;
            const float sq = dense ? sqrtf(rho) : 0.f;
            const float pe = 0.5f * SP - K.c * sq;
            v[0] += K.eps * pe;
            if (DTH) {
                const float Fp = dense ? (-0.5f * (K.eps * K.c)) / sqrtf(rho) : 0.f;
                v[1] += pe;
                v[2] += (1.f / K.a) * ((0.5f * K.fn * K.eps) * SP + K.fm * (rho * Fp));
                v[3] += (-K.eps) * sq;
            }
        }
    }
    if (frame_sums(fr, v, red)) {
        A.U[fr.f] = v[0];
        if (DTH) {
#pragma unroll
            for (int k = 0; k < 3; ++k) A.dU[3 * fr.f + k] = v[1 + k];
        }
    }
}

// the checks of the grids (those of mdg_eam_table_eval) and the argument block
int etf_make_args(const char* who, EtfArgs& a, const float* pos, int n_frames, int n_atoms, const MdgCell* cell,
                  const int32_t* types, const MdgEAMTableConsts* k, const float* tables) {
    int rc = check_frames(who, pos, cell, k, n_frames, n_atoms, FP_GROUP_ATOMS);
    if (rc == MDG_OK) rc = check_frame_count(who, n_frames);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(types && tables, "%s: null buffer (types or tables)", who);
    MDG_CHECK_ARG(k->n_species >= 1 && k->n_species <= 4, "%s: n_species must lie in [1, 4]", who);
    MDG_CHECK_ARG(k->n_r >= 4 && k->n_r <= 4096 && k->n_rho >= 4 && k->n_rho <= 4096,
                  "%s: the node counts n_r, n_rho must lie in [4, 4096]", who);
    MDG_CHECK_ARG(k->h_r > 0.0 && k->h_rho > 0.0, "%s: the grid spacings h_r, h_rho must be positive", who);
    MDG_CHECK_ARG(k->r_min >= 0.0 && k->rc > k->r_min, "%s: consts need 0 <= r_min < rc", who);
    MDG_CHECK_ARG(k->pin_cutoff == 0 || k->pin_cutoff == 1, "%s: pin_cutoff must be 0 or 1", who);
    a = EtfArgs{};
    a.pos = pos; a.types = types; a.tab = tables;
    a.F = n_frames; a.N = n_atoms; a.cell = *cell;
    a.S = (int)k->n_species; a.nr = (int)k->n_r; a.nrho = (int)k->n_rho;
    a.rmin = (float)k->r_min; a.inv_hr = (float)(1.0 / k->h_r); a.rhomin = (float)k->rho_min; a.inv_hrho = (float)(1.0 / k->h_rho);
    a.rc = (float)k->rc;
    a.r_floats = (int)et_dens_off(a.S, a.S, a.nr);
    return MDG_OK;
}

}  // namespace

extern "C" int mdg_eam_table_frames_lds_floats(void) { return EF_LDS_TABLE_FLOATS; }

extern "C" int mdg_eam_table_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const int32_t* types,
                                        const MdgEAMTableConsts* k, const float* tables, int table_mode, float* U, float* rho,
                                        void* stream) {
    EtfArgs a;
    const int rc = etf_make_args("eam_table_frames_fwd", a, pos, n_frames, n_atoms, cell, types, k, tables);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(U, "eam_table_frames_fwd: null output U");
    MDG_CHECK_ARG(table_mode >= -1 && table_mode <= 1, "eam_table_frames_fwd: table_mode is -1 (by size), 0 (global) or 1 (LDS)");
    MDG_CHECK_ARG(table_mode != 1 || a.r_floats <= EF_LDS_TABLE_FLOATS,
                  "eam_table_frames_fwd: table_mode 1 needs pair and density tables of at most %d floats, got %d",
                  EF_LDS_TABLE_FLOATS, a.r_floats);
    a.U = U; a.rho = rho;
    // by size: the copy pays where four frames share it (measured: docs/KERNELS.md K36); a workgroup per frame reads global memory
    const bool lds = table_mode == 1 || (table_mode == -1 && a.r_floats <= EF_LDS_TABLE_FLOATS && n_atoms <= FP_WAVE_ATOMS);
    const size_t dyn = lds ? (size_t)a.r_floats * sizeof(float) : 0;
    launch_frames(n_frames, n_atoms, lds, [&](auto tpf, auto tab, dim3 grid) {
        hipLaunchKernelGGL((etf_fwd_kernel<decltype(tpf)::value, decltype(tab)::value>), grid, dim3(FP_BLOCK), dyn,
                           (hipStream_t)stream, a);
    });
    MDG_CHECK_LAUNCH("etf_fwd_kernel");
    return MDG_OK;
}

extern "C" int mdg_eam_table_frames_nodes_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell,
                                              const int32_t* types, const MdgEAMTableConsts* k, const float* tables,
                                              const float* gU, const float* rho, float* g_tables, int64_t* fx, void* stream) {
    EtfArgs a;
    const int rc = etf_make_args("eam_table_frames_nodes_bwd", a, pos, n_frames, n_atoms, cell, types, k, tables);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(gU && rho, "eam_table_frames_nodes_bwd: null input (gU or the saved rho of the forward pass)");
    MDG_CHECK_ARG(g_tables && fx, "eam_table_frames_nodes_bwd: null output g_tables or fixed-point scratch fx");
    a.gU = gU; a.rho_in = rho; a.fx = (unsigned long long*)fx;
    const int64_t n_words = mdg_eam_table_size(a.S, a.nr, a.nrho);
    if (n_words <= EF_LDS_WORDS) a.lds_words = (int)n_words;
    const double per_frame = (double)n_atoms * (double)(n_atoms > 1 ? n_atoms - 1 : 1);
    a.lim_edge = fx64_limit((double)n_frames * per_frame);
    a.lim_atom = fx64_limit((double)n_frames * (double)n_atoms);
    // |basis(r)| <= 1 inside the grid; below it (0 < r < r_min) the slope entry weighs |t| < r_min / h_r
    a.bv = 1.0009765625f * fmaxf(1.f, a.rmin * a.inv_hr);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nz = n_words + ET_BOUNDS;
    hipLaunchKernelGGL(etf_zero_kernel, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, st, a.fx, nz);
    const long long total = (long long)n_frames * n_atoms;
    hipLaunchKernelGGL(etf_bounds_kernel, dim3((unsigned)((total + FP_BLOCK - 1) / FP_BLOCK)), dim3(FP_BLOCK), 0, st, a);
    const size_t dyn = (size_t)a.lds_words * sizeof(unsigned long long);
    launch_frames(n_frames, n_atoms, [&](auto tpf, dim3 grid) {
        hipLaunchKernelGGL((etf_nodes_kernel<decltype(tpf)::value>), grid, dim3(FP_BLOCK), dyn, st, a);
    });
    hipLaunchKernelGGL(etf_finish_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st, a.fx, n_words, a.bv,
                       a.lim_edge, a.lim_atom, a.S, a.nr, (int)k->pin_cutoff, g_tables);
    MDG_CHECK_LAUNCH("etf_nodes_kernel");
    return MDG_OK;
}

extern "C" int mdg_eam_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell, const MdgEAMConsts* k,
                                  const float* theta, float* U, float* dU_dtheta, void* stream) {
    const int rc = check_frames("eam_frames_fwd", pos, cell, k, n_frames, n_atoms, FP_GROUP_ATOMS);
    if (rc != MDG_OK) return rc;
    MDG_CHECK_ARG(theta, "eam_frames_fwd: theta is null (the device buffer (epsilon, a, c) is required)");
    MDG_CHECK_ARG(U, "eam_frames_fwd: null output U");
    MDG_CHECK_ARG(k->rc > 0.0, "eam_frames_fwd: consts need rc > 0");
    MDG_CHECK_ARG(k->m >= 1 && k->m < k->n && k->n <= 16, "eam_frames_fwd: exponents need 1 <= m < n <= 16");
    MDG_CHECK_ARG(k->shift == 0 || k->shift == 1, "eam_frames_fwd: shift must be 0 (as published) or 1 (shifted force)");
    EsfArgs A{pos, theta, U, dU_dtheta, n_frames, n_atoms, *cell, (float)k->rc, (int)k->n, (int)k->m, (int)k->shift};
    launch_frames(n_frames, n_atoms, dU_dtheta != nullptr, [&](auto tpf, auto dth, dim3 grid) {
        hipLaunchKernelGGL((eam_frames_kernel<decltype(tpf)::value, decltype(dth)::value>), grid, dim3(FP_BLOCK), 0,
                           (hipStream_t)stream, A);
    });
    MDG_CHECK_LAUNCH("eam_frames_kernel");
    return MDG_OK;
}
