// K27: tabulated embedded-atom potential ("eam/alloy") for 1 <= S <= 4 species over the per-atom (ELL) list
// (mdgrad_amd/interface.py EAM).  With a = types[i], b = types[j]:
//
//   U     = sum_i [ 1/2 sum_{j in row(i)} phi_ab(r_ij) + F_a(rho_i) ],   rho_i = sum_{j in row(i)} f_b(r_ij)
//
// Every function is a cubic-Hermite interpolant on a uniform grid with node entries (value, h * derivative), the convention of
// MDG_PAIR_TABLE: phi (S (S + 1) / 2 tables, pair (a, b) at hi (hi + 1) / 2 + lo) and f (S tables) on r_g = r_min + g h_r,
// g = 0 .. n_r - 1, r_{n_r - 1} = rc; F (S tables) on rho_g = rho_min + g h_rho.  Outside its grid a function continues linearly
// with the end node's value and slope, so every argument has a finite, C1 value.  An empty row has rho = 0 and gets F_a(0) from
// the table.  The nodes are the trainable parameters: `tables` is the flat image (pair, density, embed) and the table gradients
// gtab = dU/dnodes, gtabw = d(w.dU/dx)/dnodes have the same layout.
//
// Two passes, laid out like csrc/eam.hip (EAM_LPA lanes walk one atom's row, group shuffles combine):
//   1. density pass:  rho_i, F_a'(rho_i) and their dual parts -> atom_work[i] = (rho_i, d rho_i, F', F'' d rho_i)
//   2. force pass:    dU/dx_i = -sum_j [phi_ab'(r_ij) + F'_i f_b'(r_ij) + F'_j f_a'(r_ij)] e_ij  -- the density an atom receives
//                     comes from its NEIGHBOUR's table, so the i side carries f_b and the j side f_a.
// The tables are read from global memory: phi_ab, f_a and f_b of an edge share one bracketing cell (one grid in r), 4 floats each,
// and a 16-atom block makes ~10^3 lookups, fewer words than staging even one 1024-node table set into LDS would move (the full
// set, 18 tables of 4096 nodes, is 590 KB and cannot be staged at all).  docs/KERNELS.md K27.
//
// Table gradient.  The value is linear in the nodes, so an edge adds 1/2 basis(r_ij) to its pair table and F'_i basis(r_ij) to
// f_b, an atom adds basis(rho_i) to F_a; at LEVEL 2 the dual parts of the same products are d(w.dU/dx)/dnodes.  This is a
// scatter into a few thousand words: fx64 fixed point (common.hpp), one int64 word per node entry, integer atomics only, so the
// sums do not depend on the order of arrival.  A table set of at most 6144 words (48 KiB) is first summed per workgroup in LDS
// (LDS integer atomics), and a workgroup then adds the words it touched to the global ones; a larger set takes the global
// atomics directly.  The power-of-two scale of each table family is taken on the device from upper bounds that the density pass measures with integer atomic maxima (max |basis|, max |F'|, max |F'' d rho|: every contribution
// is a product of factors below them), so that the largest contribution times the number of contributions stays under 2^61:
// no flag, no host read, no re-run.  A finish kernel turns the words into floats.
//
// No fused multiply-adds are formed by the compiler in this file: the float and the Dual instantiation round the value parts
// identically, so dU/dx of a LEVEL 1 launch equals that of a LEVEL 2 launch bit for bit.  The layout of the flat image, the
// bracketing cell with its weights, the fixed-order dot product and the power-of-two scale live in csrc/eam_table_core.hpp,
// shared with the list-free frame energy (csrc/eam_frames.hip, K36).
#include "eam_table_core.hpp"
#include "manybody.hpp"

namespace {

constexpr int EAM_LPA = 16;                   // lanes per atom, as in csrc/eam.hip
constexpr int EAM_BLOCK = 256;
constexpr int ET_LDS_WORDS = 6144;            // 48 KiB of int64 words: the largest table set that gets a workgroup copy in LDS
enum { ET_BV = 0, ET_BD, ET_FP, ET_FPP, ET_EM };   // max |basis|, |d basis|, |F'|, |F'' d rho|, |embed weight| as float bits

struct EtArgs {
    const float* pos; int N; MdgCell cell;
    const int32_t* col; const int32_t* shift; const int32_t* cnt; int max_nbr;
    const int32_t* types; const float* tab; const float* w;
    int S, nr, nrho;
    float rmin, inv_hr, rhomin, inv_hrho, rc;
    float* work;                               // atom_work [N, 4]
    float* grad; float* hw; float* partial;
    unsigned long long* fx;                    // [ET_BOUNDS + table words]
    int lds_words;                             // > 0: the force pass adds into a workgroup copy of the words in LDS first
    float lim_edge, lim_atom;                  // fx64_limit of a word fed by the edges / by the atoms
    float oscale; int oacc;
};

__device__ __forceinline__ int et_type(const EtArgs& A, int i) { return min(max(A.types[i], 0), A.S - 1); }
__device__ __forceinline__ const float* et_pair_tab(const EtArgs& A, int p) { return A.tab + et_pair_off(p, A.nr); }
__device__ __forceinline__ const float* et_dens_tab(const EtArgs& A, int b) { return A.tab + et_dens_off(A.S, b, A.nr); }
__device__ __forceinline__ size_t et_embed_off(const EtArgs& A, int a) { return et_embed_off(A.S, a, A.nr, A.nrho); }

// one list entry seen from its centre: unit vector centre -> end, r
template <class T> struct EtEdge { T ex, ey, ez, r; };

// the entry in slot s of row(i) as an edge i -> j; returns j, or -1 when there is nothing to add (0 < r < rc fails)
template <class T, int LEVEL>
__device__ __forceinline__ int et_entry(const EtArgs& A, size_t row, int s, float xi, float yi, float zi,
                                        float wxi, float wyi, float wzi, EtEdge<T>& e) {
    const int j = A.col[row + s];
    if ((unsigned)j >= (unsigned)A.N) return -1;
    float dx = xi - A.pos[3 * j], dy = yi - A.pos[3 * j + 1], dz = zi - A.pos[3 * j + 2];
    apply_shift(A.cell, A.shift[row + s], dx, dy, dz);                      // x_i - x_j - o.h
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (LEVEL >= 2) { ax = A.w[3 * j] - wxi; ay = A.w[3 * j + 1] - wyi; az = A.w[3 * j + 2] - wzi; }
    const T x = mk<T>(-dx, ax), y = mk<T>(-dy, ay), z = mk<T>(-dz, az);
    const T d2 = x * x + y * y + z * z;
    const float rv = sqrtf(val(d2));
    if (!(rv > 0.f && rv < A.rc)) return -1;
    e.r = fsqrt_(d2);
    const T ir = mk<T>(1.f, 0.f) / e.r;
    e.ex = x * ir; e.ey = y * ir; e.ez = z * ir;
    return j;
}

template <class T> __device__ __forceinline__ float et_max_abs4(float m, const T (&c)[4], bool dual) {
#pragma unroll
    for (int k = 0; k < 4; ++k) m = fmaxf(m, fabsf(dual ? dual_part(c[k]) : val(c[k])));
    return m;
}

// the scales of the pair, density and embedding words of a launch at `level`, from the bounds of the density pass
__device__ __forceinline__ void et_scales(const unsigned long long* fx, int level, float lim_edge, float lim_atom, float (&s)[3]) {
    const unsigned* u = (const unsigned*)fx;
    const float bv = __uint_as_float(u[ET_BV]), bd = __uint_as_float(u[ET_BD]), fp = __uint_as_float(u[ET_FP]),
                fpp = __uint_as_float(u[ET_FPP]), em = __uint_as_float(u[ET_EM]);
    s[0] = et_pow2(0.5f * (level >= 2 ? bd : bv), lim_edge);
    s[1] = et_pow2(level >= 2 ? fpp * bv + fp * bd : fp * bv, lim_edge);
    s[2] = et_pow2(em, lim_atom);
}

__global__ void et_zero_kernel(unsigned long long* fx, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) fx[k] = 0ull;
}

// ---- pass 1: rho_i, F'(rho_i) and their dual parts; TG: the bounds of the table-gradient scatter
template <int LEVEL, bool TG>
__global__ void __launch_bounds__(EAM_BLOCK) et_density_kernel(const EtArgs A) {
    using T = typename std::conditional<LEVEL >= 2, Dual, float>::type;
    constexpr int apb = EAM_BLOCK / EAM_LPA;
    const int i = blockIdx.x * apb + threadIdx.x / EAM_LPA, sub = threadIdx.x % EAM_LPA;
    float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < A.N) {
        const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
        float wxi = 0.f, wyi = 0.f, wzi = 0.f;
        if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
        T part = mk<T>(0.f, 0.f);
        const int n = min(A.cnt[i], A.max_nbr);
        const size_t row = (size_t)i * A.max_nbr;
        for (int s = sub; s < n; s += EAM_LPA) {
            EtEdge<T> e;
            const int j = et_entry<T, LEVEL>(A, row, s, xi, yi, zi, wxi, wyi, wzi, e);
            if (j < 0) continue;
            EtBasis<T> B;
            et_basis<T>(e.r, A.rmin, A.inv_hr, A.nr, B);
            part = part + et_dot<T>(B.b, et_dens_tab(A, et_type(A, j)) + 2 * B.g);
            if (TG) {
                m[ET_BV] = et_max_abs4<T>(m[ET_BV], B.b, false);
                if (LEVEL >= 2) m[ET_BD] = et_max_abs4<T>(m[ET_BD], B.b, true);
            }
        }
        const float rho = group_sum<EAM_LPA>(val(part));
        float drho = 0.f;
        if (LEVEL >= 2) drho = group_sum<EAM_LPA>(dual_part(part));
        if (sub == 0) {
            EtBasis<T> B;
            et_basis<T>(mk<T>(rho, drho), A.rhomin, A.inv_hrho, A.nrho, B);
            const T Fp = A.inv_hrho * et_dot<T>(B.d, A.tab + et_embed_off(A, et_type(A, i)) + 2 * B.g);   // dual part: F'' d rho
            float* o = A.work + 4 * (size_t)i;
            o[0] = rho; o[1] = drho; o[2] = val(Fp); o[3] = dual_part(Fp);
            if (TG) {
                m[ET_FP] = fabsf(val(Fp)); m[ET_FPP] = fabsf(dual_part(Fp));
                m[ET_EM] = et_max_abs4<T>(0.f, B.b, LEVEL >= 2);
            }
        }
    }
    if (TG) {                                // one integer atomic maximum per bound and workgroup, and only where it raises the bound
        __shared__ float mred[EAM_BLOCK / 64][5];
        unsigned* u = (unsigned*)A.fx;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float v = wave_max(m[k]);
            if ((threadIdx.x & 63) == 0) mred[threadIdx.x >> 6][k] = v;
        }
        __syncthreads();
        if (threadIdx.x < 5) {
            float v = 0.f;
            for (int wv = 0; wv < EAM_BLOCK / 64; ++wv) v = fmaxf(v, mred[wv][threadIdx.x]);
            // (non-negative floats order like their bits; a stale read only costs an atomic that changes nothing)
            if (v > 0.f && __float_as_uint(v) > __hip_atomic_load(u + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(u + threadIdx.x, __float_as_uint(v));
        }
    }
}

// ---- pass 2.  LEVEL 0: U        1: + grad, TG: gtab words        2: + hw, TG: gtabw words
template <int LEVEL, bool TG>
__global__ void __launch_bounds__(EAM_BLOCK) et_force_kernel(const EtArgs A) {
    using T = typename std::conditional<LEVEL >= 2, Dual, float>::type;
    __shared__ float red[17];
    extern __shared__ unsigned long long et_acc[];            // [lds_words]: this workgroup's share of the table-gradient words
    constexpr int apb = EAM_BLOCK / EAM_LPA;
    const int i = blockIdx.x * apb + threadIdx.x / EAM_LPA, sub = threadIdx.x % EAM_LPA;
    float en = 0.f;
    unsigned long long* fxw = A.fx + ET_BOUNDS;
    const bool lds = TG && A.lds_words > 0;                   // (block-uniform)
    if (lds) {
        for (int k = threadIdx.x; k < A.lds_words; k += EAM_BLOCK) et_acc[k] = 0ull;
        __syncthreads();
    }
    auto add = [&](size_t word, unsigned long long v) {
        if (lds) atomicAdd(et_acc + word, v); else atomicAdd(fxw + word, v);
    };
    if (i < A.N) {
        float sc[3] = {1.f, 1.f, 1.f};
        if (TG) et_scales(A.fx, LEVEL, A.lim_edge, A.lim_atom, sc);
        const float* wi = A.work + 4 * (size_t)i;
        const T zero = mk<T>(0.f, 0.f);
        const T R = mk<T>(wi[0], wi[1]), FpI = mk<T>(wi[2], wi[3]);
        const int a = et_type(A, i);
        const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
        float wxi = 0.f, wyi = 0.f, wzi = 0.f;
        if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
        T SP = zero, gx = zero, gy = zero, gz = zero;
        const int n = min(A.cnt[i], A.max_nbr);
        const size_t row = (size_t)i * A.max_nbr;
        for (int s = sub; s < n; s += EAM_LPA) {
            EtEdge<T> e;
            const int j = et_entry<T, LEVEL>(A, row, s, xi, yi, zi, wxi, wyi, wzi, e);
            if (j < 0) continue;
            const int b = et_type(A, j), p = et_pair(a, b);
            EtBasis<T> B;
            et_basis<T>(e.r, A.rmin, A.inv_hr, A.nr, B);
            const float* np = et_pair_tab(A, p) + 2 * B.g;
            SP = SP + et_dot<T>(B.b, np);
            if (LEVEL >= 1) {
                const T dphi = et_dot<T>(B.d, np);
                const T dfb = et_dot<T>(B.d, et_dens_tab(A, b) + 2 * B.g);       // the density i receives from j: j's table
                const T dfa = et_dot<T>(B.d, et_dens_tab(A, a) + 2 * B.g);       // the density j receives from i: i's table
                const float* wj = A.work + 4 * (size_t)j;
                const T FpJ = mk<T>(wj[2], wj[3]);
                const T du = A.inv_hr * ((dphi + FpI * dfb) + FpJ * dfa);        // dU/dr_ij;  d r / d x_i = -e
                gx = gx - du * e.ex; gy = gy - du * e.ey; gz = gz - du * e.ez;
                if (TG) {
                    const size_t wp = 2 * ((size_t)p * A.nr + B.g), wd = 2 * ((size_t)(et_npair(A.S) + b) * A.nr + B.g);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const T c = FpI * B.b[k];
                        const float vp = 0.5f * (LEVEL >= 2 ? dual_part(B.b[k]) : val(B.b[k]));
                        const float vd = LEVEL >= 2 ? dual_part(c) : val(c);
                        if (vp != 0.f) add(wp + k, fx64(vp * sc[0]));
                        if (vd != 0.f) add(wd + k, fx64(vd * sc[1]));
                    }
                }
            }
        }
        float o[8];
        o[0] = val(SP); o[1] = val(gx); o[2] = val(gy); o[3] = val(gz);
        o[4] = dual_part(SP); o[5] = dual_part(gx); o[6] = dual_part(gy); o[7] = dual_part(gz);
        o[0] = group_sum<EAM_LPA>(o[0]);
        if (LEVEL >= 1) {
#pragma unroll
            for (int k = 1; k < 4; ++k) o[k] = group_sum<EAM_LPA>(o[k]);
        }
        if (LEVEL >= 2) {
#pragma unroll
            for (int k = 5; k < 8; ++k) o[k] = group_sum<EAM_LPA>(o[k]);
        }
        if (sub == 0) {
            EtBasis<T> B;
            et_basis<T>(R, A.rhomin, A.inv_hrho, A.nrho, B);
            const size_t off = et_embed_off(A, a) + 2 * B.g;
            en = 0.5f * o[0] + val(et_dot<T>(B.b, A.tab + off));          // u_i = 1/2 sum_j phi + F_a(rho_i)
            if (LEVEL >= 1) {
                if (A.grad) store3(A.grad, i, A.oscale, A.oacc, o[1], o[2], o[3]);
                if (LEVEL >= 2 && A.hw) store3(A.hw, i, A.oscale, A.oacc, o[5], o[6], o[7]);
                if (TG) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float ve = LEVEL >= 2 ? dual_part(B.b[k]) : val(B.b[k]);
                        if (ve != 0.f) add(off + k, fx64(ve * sc[2]));
                    }
                }
            }
        }
    }
    if (lds) {                               // the words this workgroup touched, one integer atomic each
        __syncthreads();
        for (int k = threadIdx.x; k < A.lds_words; k += EAM_BLOCK) {
            const unsigned long long v = et_acc[k];
            if (v != 0ull) atomicAdd(fxw + k, v);
        }
    }
    if (A.partial) {                         // (block-uniform: a force-only evaluation has no scalar to reduce)
        en = block_sum(en, red);
        if (threadIdx.x == 0) A.partial[blockIdx.x] = en;
    }
}

// the fixed-point words as floats; pinned: the last node of every phi and f table is returned as exactly 0
__global__ void et_finish_kernel(const unsigned long long* fx, int64_t n_words, int level, float lim_edge, float lim_atom,
                                 int S, int nr, int pin, float* out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_words) return;
    float s[3];
    et_scales(fx, level, lim_edge, lim_atom, s);
    const int64_t r_words = 2 * (int64_t)(et_npair(S) + S) * nr;
    const int fam = k < 2 * (int64_t)et_npair(S) * nr ? 0 : (k < r_words ? 1 : 2);
    float v = (float)((double)(long long)fx[ET_BOUNDS + k] * (1.0 / (double)s[fam]));      // (s is a power of two: exact)
    if (pin && fam < 2 && (k / 2) % nr == nr - 1) v = 0.f;
    out[k] = v;
}

}  // namespace

extern "C" int64_t mdg_eam_table_partial_size(int n_atoms) { return atom_blocks(n_atoms, EAM_LPA, EAM_BLOCK); }

extern "C" int64_t mdg_eam_table_size(int n_species, int n_r, int n_rho) {
    if (n_species < 1 || n_species > 4 || n_r < 4 || n_r > 4096 || n_rho < 4 || n_rho > 4096) return -1;
    return 2 * ((int64_t)(n_species * (n_species + 1) / 2 + n_species) * n_r + (int64_t)n_species * n_rho);
}

extern "C" int64_t mdg_eam_table_fx_size(int n_species, int n_r, int n_rho) {
    const int64_t n = mdg_eam_table_size(n_species, n_r, n_rho);
    return n < 0 ? -1 : n + ET_BOUNDS;
}

extern "C" int mdg_eam_table_eval(const float* pos, int n_atoms, const MdgCell* cell, const int32_t* col, const int32_t* shift,
                                  const int32_t* cnt, int max_nbr, const int32_t* types, const MdgEAMTableConsts* k,
                                  const float* tables, const float* w, float* energy, float* grad, float* hw, float* gtab,
                                  float* gtabw, float* partial, float* atom_work, int64_t* fx, float out_scale, int accumulate,
                                  void* stream) {
    MDG_CHECK_ARG(pos && cell && col && shift && cnt, "eam_table_eval: null buffer (pos, cell or list)");
    MDG_CHECK_ARG(types && tables, "eam_table_eval: null buffer (types or tables)");
    MDG_CHECK_ARG(k, "eam_table_eval: consts is null");
    MDG_CHECK_ARG(n_atoms > 0 && max_nbr > 0, "eam_table_eval: bad sizes (n_atoms, max_nbr must be positive)");
    MDG_CHECK_ARG(k->n_species >= 1 && k->n_species <= 4, "eam_table_eval: n_species must lie in [1, 4]");
    MDG_CHECK_ARG(k->n_r >= 4 && k->n_r <= 4096 && k->n_rho >= 4 && k->n_rho <= 4096,
                  "eam_table_eval: the node counts n_r, n_rho must lie in [4, 4096]");
    MDG_CHECK_ARG(k->h_r > 0.0 && k->h_rho > 0.0, "eam_table_eval: the grid spacings h_r, h_rho must be positive");
    MDG_CHECK_ARG(k->r_min >= 0.0 && k->rc > k->r_min, "eam_table_eval: consts need 0 <= r_min < rc");
    MDG_CHECK_ARG(k->pin_cutoff == 0 || k->pin_cutoff == 1, "eam_table_eval: pin_cutoff must be 0 or 1");
    MDG_CHECK_ARG(w || !(hw || gtabw), "eam_table_eval: hw / gtabw need w");
    MDG_CHECK_ARG(!w || hw || gtabw, "eam_table_eval: w given without hw or gtabw output");
    MDG_CHECK_ARG(!(gtab && w), "eam_table_eval: gtab is the output of a call without w (with w: gtabw)");
    MDG_CHECK_ARG(energy || grad || hw || gtab || gtabw, "eam_table_eval: no output requested");
    MDG_CHECK_ARG(!energy || partial, "eam_table_eval: energy needs the partial buffer");
    MDG_CHECK_ARG(atom_work, "eam_table_eval: atom_work is null (the scratch of the density pass, 4 floats per atom)");
    MDG_CHECK_ARG(!(gtab || gtabw) || fx, "eam_table_eval: gtab / gtabw need the fixed-point scratch fx");
    const int level = w ? 2 : ((grad || gtab) ? 1 : 0);
    float* tg_out = w ? gtabw : gtab;
    // (accumulate bit 2, "the list was searched with a skin", needs nothing here: the support test r < rc is always applied)
    EtArgs a{pos, n_atoms, *cell, col, shift, cnt, max_nbr, types, tables, w,
             (int)k->n_species, (int)k->n_r, (int)k->n_rho,
             (float)k->r_min, (float)(1.0 / k->h_r), (float)k->rho_min, (float)(1.0 / k->h_rho), (float)k->rc,
             atom_work, grad, hw, energy ? partial : nullptr, (unsigned long long*)fx, 0,
             fx64_limit((double)n_atoms * (double)max_nbr), fx64_limit((double)n_atoms), out_scale, accumulate & 1};
    const int nblocks = (int)mdg_eam_table_partial_size(n_atoms);
    const int64_t n_words = mdg_eam_table_size(a.S, a.nr, a.nrho);
    if (n_words <= ET_LDS_WORDS) a.lds_words = (int)n_words;
    dim3 grid(nblocks);
    hipStream_t st = (hipStream_t)stream;
    if (tg_out) {
        const int64_t nz = n_words + ET_BOUNDS;
        hipLaunchKernelGGL(et_zero_kernel, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, st, a.fx, nz);
    }
    with_level(level, [&](auto L) {
        constexpr int LV = decltype(L)::value;
        constexpr int DL = LV >= 2 ? 2 : 1;                                   // (0 and 1: the float pass)
        if (tg_out && LV >= 1) {
            hipLaunchKernelGGL((et_density_kernel<DL, true>), grid, dim3(EAM_BLOCK), 0, st, a);
            hipLaunchKernelGGL((et_force_kernel<(LV >= 1 ? LV : 1), true>), grid, dim3(EAM_BLOCK),
                               (size_t)a.lds_words * sizeof(unsigned long long), st, a);
        } else {
            hipLaunchKernelGGL((et_density_kernel<DL, false>), grid, dim3(EAM_BLOCK), 0, st, a);
            hipLaunchKernelGGL((et_force_kernel<LV, false>), grid, dim3(EAM_BLOCK), 0, st, a);
        }
    });
    if (tg_out)
        hipLaunchKernelGGL(et_finish_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st, a.fx, n_words, level,
                           a.lim_edge, a.lim_atom, a.S, a.nr, (int)k->pin_cutoff, tg_out);
    if (energy) hipLaunchKernelGGL(energy_finish, dim3(1), dim3(64), 0, st, partial, nblocks, energy);
    MDG_CHECK_LAUNCH("eam_table_eval");
    return MDG_OK;
}
