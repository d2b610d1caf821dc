// K20: damped shifted-force Coulomb sum with one charge per atom over the per-atom (ELL) list
// (mdgrad_amd/interface.py CoulombPotentials; the corrected form of torchmd/interface.py:303-361).
//
// Laid out like pair_ell_kernel (csrc/pair_ell.hip): LPA lanes walk one atom's row, the per-atom sums are combined with
// wave shuffles, the energy goes through a fixed-order block partial and a finish kernel.  A per-atom charge does not fit
// MdgPairTerm (one theta per term), hence its own kernel.  No float atomics anywhere => bitwise reproducible.
//
//   E = erfc(alpha r), G = g0 exp(-alpha^2 r^2):  psi = E/r - c0 + c1 (r - rc),  psi' = -E/r^2 - G/r + c1,
//   psi'' = 2E/r^3 + 2G/r^2 + 2 alpha^2 G   -- one erfcf and one expf per pair (the library functions, not the fast
//   intrinsics); alpha == 0 takes E = 1, G = 0 without calling either.
#include "manybody.hpp"

namespace {

struct CoulombArgs {
    const float* pos; int N; MdgCell cell;
    const int32_t* col; const int32_t* shift; const int32_t* cnt; int max_nbr;
    const float* q; const float* w;
    float alpha, rc, rc2, c0, c1, g0, alpha2, conv, self_s;
    float* grad; float* hw; float* pot; float* potw; float* partial;
    float oscale; int oacc;      // grad / hw outputs: out = (oacc ? out : 0) + oscale * value  (force sums of a Stack)
    int recheck;                 // the list was searched with a skin: re-apply the builders' exact cutoff test per pair
};

// LEVEL 0: U        1: + grad, pot        2: + hw, potw
template <int LPA, int LEVEL>
__global__ void coulomb_ell_kernel(const CoulombArgs A) {
    __shared__ float red[16];
    const int apb = blockDim.x / LPA;
    const int i = blockIdx.x * apb + threadIdx.x / LPA, sub = threadIdx.x % LPA;
    float e = 0.f;
    if (i < A.N) {
        const float xi = A.pos[3 * i], yi = A.pos[3 * i + 1], zi = A.pos[3 * i + 2];
        const float qi = A.q[i], qc = A.conv * qi;
        float wxi = 0.f, wyi = 0.f, wzi = 0.f;
        if (LEVEL >= 2) { wxi = A.w[3 * i]; wyi = A.w[3 * i + 1]; wzi = A.w[3 * i + 2]; }
        float gx = 0.f, gy = 0.f, gz = 0.f, hx = 0.f, hy = 0.f, hz = 0.f, pt = 0.f, pw = 0.f;
        const int n = A.cnt[i];
        const size_t row = (size_t)i * A.max_nbr;
        for (int k = sub; k < n; k += LPA) {
            const int j = A.col[row + k];
            float dx = xi - A.pos[3 * j], dy = yi - A.pos[3 * j + 1], dz = zi - A.pos[3 * j + 2];
            if (A.recheck) {
                // the test of the list builders at the current positions (csrc/nbr.hip pair_test; see pair_ell_kernel)
                float bx = -dx, by = -dy, bz = -dz;
                if (A.cell.diag) min_image<true>(A.cell, bx, by, bz); else min_image<false>(A.cell, bx, by, bz);
                const float b2 = norm2_ref(bx, by, bz);
                if (!((b2 < A.rc2) && (b2 != 0.f))) continue;
            }
            apply_shift(A.cell, A.shift[row + k], dx, dy, dz);      // d = x_i - x_j - o.h
            const float d2 = dx * dx + dy * dy + dz * dz;
            const float ir = __builtin_amdgcn_rsqf(d2), r = d2 * ir;
            const float qj = A.q[j];
            float E = 1.f, G = 0.f;
            if (A.alpha != 0.f) {
                E = erfcf(A.alpha * r);
                if (LEVEL >= 1) G = A.g0 * expf(-A.alpha2 * d2);
            }
            const float Er = E * ir;
            const float psi = fmaf(A.c1, r - A.rc, Er - A.c0);
            pt = fmaf(qj, psi, pt);
            if (LEVEL >= 1) {
                const float t = (Er + G) * ir;                       // E/r^2 + G/r
                const float dpsi = A.c1 - t;
                const float du = qc * qj * dpsi;
                const float rx = dx * ir, ry = dy * ir, rz = dz * ir;
                gx = fmaf(du, rx, gx); gy = fmaf(du, ry, gy); gz = fmaf(du, rz, gz);
                if (LEVEL >= 2) {
                    const float d2psi = 2.f * fmaf(t, ir, A.alpha2 * G);
                    const float ax = wxi - A.w[3 * j], ay = wyi - A.w[3 * j + 1], az = wzi - A.w[3 * j + 2];
                    const float a = rx * ax + ry * ay + rz * az;
                    const float c2 = qc * qj * d2psi * a, c3 = du * ir;
                    hx += c2 * rx + c3 * (ax - a * rx);
                    hy += c2 * ry + c3 * (ay - a * ry);
                    hz += c2 * rz + c3 * (az - a * rz);
                    pw = fmaf(qj * dpsi, a, pw);
                }
            }
        }
        pt = group_sum<LPA>(pt);
        if (LEVEL >= 1) {
            gx = group_sum<LPA>(gx); gy = group_sum<LPA>(gy); gz = group_sum<LPA>(gz);
            if (LEVEL >= 2) { hx = group_sum<LPA>(hx); hy = group_sum<LPA>(hy); hz = group_sum<LPA>(hz); pw = group_sum<LPA>(pw); }
        }
        if (sub == 0) {
            e = qc * (0.5f * pt - A.self_s * qi);
            const float os = A.oscale;
            if (LEVEL >= 1) {
                if (A.grad) store3(A.grad, i, os, A.oacc, gx, gy, gz);
                if (A.pot) A.pot[i] = pt;
            }
            if (LEVEL >= 2) {
                if (A.hw) store3(A.hw, i, os, A.oacc, hx, hy, hz);
                if (A.potw) A.potw[i] = pw;
            }
        }
    }
    if (A.partial) {                         // (block-uniform: a force-only evaluation has no scalar to reduce)
        e = block_sum(e, red);
        if (threadIdx.x == 0) A.partial[blockIdx.x] = e;
    }
}

// types == null: one wave per slot p = atom of a replica, lanes stride over the replicas.
// types != null: one 256-thread block per type, threads stride over all atoms.  Fixed order either way.
__global__ void coulomb_charge_reduce_kernel(const float* __restrict__ val, const int32_t* __restrict__ types, int N, int group,
                                             int n_slots, float* __restrict__ out) {
    __shared__ float red[17];
    if (types == nullptr) {
        const int p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (p >= n_slots) return;                                        // (wave-uniform; no barrier below)
        float s = 0.f;
        for (size_t i = (size_t)lane * group + p; i < (size_t)N; i += (size_t)64 * group) s += val[i];
        s = wave_sum(s);
        if (lane == 0) out[p] = s;
        return;
    }
    const int p = blockIdx.x;
    float s = 0.f;
    for (int i = threadIdx.x; i < N; i += blockDim.x)
        if (types[i % group] == p) s += val[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[p] = s;
}

int coulomb_lpa(int N) {                     // (pick_lpa of csrc/pair_ell.hip)
    int lpa = 64;
    while (lpa > 8 && (long long)N * lpa / 2 >= 131072) lpa /= 2;
    return lpa;
}

}  // namespace

extern "C" int64_t mdg_coulomb_partial_size(int n_atoms) { return atom_blocks(n_atoms, coulomb_lpa(n_atoms), 256); }

extern "C" int mdg_coulomb_eval(const float* pos, int n_atoms, const MdgCell* cell, const int32_t* col, const int32_t* shift,
                                const int32_t* cnt, int max_nbr, const float* q, const MdgCoulombConsts* k, const float* w,
                                float* energy, float* grad, float* hw, float* pot, float* potw, float* partial, float out_scale,
                                int accumulate, void* stream) {
    MDG_CHECK_ARG(pos && cell && col && shift && cnt, "coulomb_eval: null buffer (pos, cell or list)");
    MDG_CHECK_ARG(q, "coulomb_eval: q is null");
    MDG_CHECK_ARG(k, "coulomb_eval: consts is null");
    MDG_CHECK_ARG(n_atoms > 0 && max_nbr > 0, "coulomb_eval: bad sizes (n_atoms, max_nbr must be positive)");
    MDG_CHECK_ARG(k->alpha >= 0.0 && k->rc > 0.0, "coulomb_eval: consts need alpha >= 0 and rc > 0");
    MDG_CHECK_ARG(w || !(hw || potw), "coulomb_eval: hw / potw need w");
    MDG_CHECK_ARG(!w || hw || potw, "coulomb_eval: w given without hw or potw output");
    MDG_CHECK_ARG(energy || grad || hw || pot || potw, "coulomb_eval: no output requested");
    MDG_CHECK_ARG(!energy || partial, "coulomb_eval: energy needs the partial buffer");
    const int level = w ? 2 : ((grad || pot) ? 1 : 0);
    CoulombArgs a{pos, n_atoms, *cell, col, shift, cnt, max_nbr, q, w,
                  (float)k->alpha, (float)k->rc, (float)k->rc * (float)k->rc, (float)k->c0, (float)k->c1, (float)k->g0,
                  (float)k->alpha2, (float)k->conversion, (float)k->self_s,
                  grad, hw, pot, potw, energy ? partial : nullptr, out_scale, accumulate & 1, (accumulate >> 1) & 1};
    const int lpa = coulomb_lpa(n_atoms);
    const int nblocks = (int)atom_blocks(n_atoms, lpa, 256);
    dim3 grid(nblocks);
    hipStream_t st = (hipStream_t)stream;
    with_level(level, [&](auto L) {
        constexpr int LV = decltype(L)::value;
        switch (lpa) {
            case 8: hipLaunchKernelGGL((coulomb_ell_kernel<8, LV>), grid, dim3(256), 0, st, a); break;
            case 16: hipLaunchKernelGGL((coulomb_ell_kernel<16, LV>), grid, dim3(256), 0, st, a); break;
            case 32: hipLaunchKernelGGL((coulomb_ell_kernel<32, LV>), grid, dim3(256), 0, st, a); break;
            default: hipLaunchKernelGGL((coulomb_ell_kernel<64, LV>), grid, dim3(256), 0, st, a);
        }
    });
    if (energy) hipLaunchKernelGGL(energy_finish, dim3(1), dim3(64), 0, st, partial, nblocks, energy);
    MDG_CHECK_LAUNCH("coulomb_ell_kernel");
    return MDG_OK;
}

extern "C" int mdg_coulomb_charge_reduce(const float* val, const int32_t* types, int n_atoms, int group, int n_slots,
                                         float* out, void* stream) {
    MDG_CHECK_ARG(val, "coulomb_charge_reduce: val is null");
    MDG_CHECK_ARG(out, "coulomb_charge_reduce: out is null");
    MDG_CHECK_ARG(n_atoms > 0 && group > 0 && n_atoms % group == 0, "coulomb_charge_reduce: n_atoms must be a positive "
                  "multiple of group");
    MDG_CHECK_ARG(n_slots > 0 && (types || n_slots == group), "coulomb_charge_reduce: n_slots must be positive, and equal "
                  "group without types");
    hipStream_t st = (hipStream_t)stream;
    const int nblocks = types ? n_slots : (n_slots + 3) / 4;
    hipLaunchKernelGGL(coulomb_charge_reduce_kernel, dim3(nblocks), dim3(256), 0, st, val, types, n_atoms, group, n_slots, out);
    MDG_CHECK_LAUNCH("coulomb_charge_reduce_kernel");
    return MDG_OK;
}
