// torch.ops.mdgrad.* -- the TORCH_LIBRARY op layer of SURVEY 8b above the C ABI of libmdgrad_hip.so
// (include/mdgrad_hip.h).  Host-only C++: every op validates its tensors (TORCH_CHECK -> Python RuntimeError),
// allocates its outputs from the caching allocator, and enqueues the kernels of the C entry point on the current
// HIP stream of the tensors' device.  Stateless and re-entrant; no host synchronisation.  The differentiation
// contract stays in the Python autograd.Functions (mdgrad_amd/ops.py), which call these ops instead of the ctypes
// bindings when this library is present (≈ 3x less host time per launch).
//
//   nbr_build        K1   torchmd/topology.py:30-73        -> mdg_nbr_build_dense(_groups) / mdg_nbr_build_cell(_groups)
//   pair_force       K2/3 interface.py:298-300 + autograd  -> mdg_pair_eval_ell (energy, dU/dx, dU/dtheta)
//   pair_hvp         K4   sovlers.py:229-233 (double bwd)   -> mdg_pair_eval_ell (H w, d(w.dU/dx)/dtheta)
//   nhc_vv_forward   K5/6 sovlers.py:106-127 / :21-40       -> mdg_traj_fwd_small
//   nhc_vv_adjoint   K7   sovlers.py:211-293                -> mdg_traj_adj_small
//   rdf_fwd/rdf_bwd  K8   observable.py:62-76               -> mdg_rdf_fwd_uniform / mdg_rdf_bwd_uniform
//   adf_fwd/adf_bwd  K14  observable.py:120-151             -> mdg_adf_fwd / mdg_adf_bwd
//   virial_fwd/_bwd  K15  thermo.py Pressure (pair virial)   -> mdg_virial_fwd / mdg_virial_bwd
//   sk_fwd/sk_bwd    K16  observable.py structure_factor     -> mdg_sk_fwd / mdg_sk_bwd
//   msd_fwd/msd_bwd  K17  observable.py msd                  -> mdg_msd_fwd / mdg_msd_bwd
//   isf_fwd/isf_bwd  K18  observable.py intermediate_scattering -> mdg_isf_fwd / mdg_isf_bwd
//   dihedral_eval    K19  interface.py DihedralPotentials     -> mdg_dihedral_eval
//   coulomb_eval, coulomb_charge_reduce  K20  interface.py CoulombPotentials  -> mdg_coulomb_eval / mdg_coulomb_charge_reduce
//   ewald_eval       K21  interface.py EwaldReciprocal      -> mdg_ewald_eval
//   ewald_excl_eval  K22  interface.py EwaldExclusions      -> mdg_ewald_excl_eval
//   sw_eval          K23  interface.py StillingerWeber      -> mdg_sw_eval
//   eam_eval         K24  interface.py SuttonChen           -> mdg_eam_eval
//   tersoff_eval     K25  interface.py Tersoff              -> mdg_tersoff_eval
//   tersoff_multi_eval  K26  interface.py TersoffMulti      -> mdg_tersoff_multi_eval
//   sw_multi_eval    K28  interface.py StillingerWeberMulti -> mdg_sw_multi_eval
//   eam_table_eval   K27  interface.py EAM                  -> mdg_eam_table_eval
//   bond_order_fwd/_bwd  K29  observable.py bond_order      -> mdg_bond_order_fwd / mdg_bond_order_bwd
//   energy_frames_fwd/_bwd  K31  thermo.py PotentialEnergy  -> mdg_energy_frames_fwd / mdg_energy_frames_bwd
//   rdf_frames_fwd/_bwd  K32  observable.py rdf.per_frame   -> mdg_rdf_frames_fwd / mdg_rdf_frames_bwd
//   dihedral_phi_fwd/_bwd, dihedral_hist_fwd/_bwd  K19  observable.py Dihedrals / dihedral_distribution -> mdg_dihedral_phi_* / _hist_*
//   edge_geom(+_bwd) schnet.py:142                          -> mdg_edge_geom / mdg_edge_geom_bwd
//   cfconv_fwd/_bwd  K9+K10 modules.py:531-571              -> mdg_cfconv_fwd(_bf16) / mdg_cfconv_bwd(_bf16)
//   dense_ssp        K11/12 layers.py:86-134                -> mdg_dense
//   ssp_dual_bwd_t, atb                                     -> mdg_ssp_dual_bwd_t / mdg_atb
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <algorithm>
#include <tuple>
#include <vector>

#include "../../include/mdgrad_hip.h"

namespace {

using at::Tensor;
using OptTensor = c10::optional<Tensor>;

void* stream_of(const Tensor& t) { return (void*)c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

void check_f32(const Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), "mdgrad: ", name, " must live on a HIP device");
    TORCH_CHECK(t.scalar_type() == at::kFloat, "mdgrad: ", name, " must be float32");
    TORCH_CHECK(t.is_contiguous(), "mdgrad: ", name, " must be contiguous");
}
void check_i32(const Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kInt && t.is_contiguous(), "mdgrad: ", name,
                " must be a contiguous int32 tensor on a HIP device");
}
void same_device(const Tensor& a, const Tensor& b, const char* name) {
    TORCH_CHECK(a.device() == b.device(), "mdgrad: ", name, " is on a different device");
}
const float* fptr(const Tensor& t) { return t.data_ptr<float>(); }
const float* fptr(const OptTensor& t, const char* name) {
    if (!t.has_value() || !t->defined()) return nullptr;
    check_f32(*t, name);
    return t->data_ptr<float>();
}
float* mptr(Tensor& t) { return t.data_ptr<float>(); }
float* mptr(OptTensor& t) { return (t.has_value() && t->defined()) ? t->data_ptr<float>() : nullptr; }
void ok(int rc) { TORCH_CHECK(rc == 0, "mdgrad: ", mdg_last_error()); }
// bf16 mirrors of node matrices (the rows16 kernels, include/mdgrad_hip.h)
bool is_bf16(const Tensor& t) { return t.scalar_type() == at::kBFloat16; }
const uint16_t* hptr(const Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && is_bf16(t) && t.is_contiguous(), "mdgrad: ", name, " must be a contiguous bfloat16 tensor on a HIP device");
    return reinterpret_cast<const uint16_t*>(t.data_ptr());
}
const uint16_t* hptr(const OptTensor& t, const char* name) { return (t.has_value() && t->defined()) ? hptr(*t, name) : nullptr; }

// cell = the 9 row-major entries of h followed by the 9 of its inverse (the Python side computes the inverse the way
// the reference does, topology.py:59) and a diagonal flag
MdgCell make_cell(at::ArrayRef<double> c) {
    TORCH_CHECK(c.size() == 19, "mdgrad: cell descriptor = 9 (h) + 9 (inverse) + 1 (diag flag) numbers");
    MdgCell m;
    for (int k = 0; k < 9; ++k) { m.h[k] = (float)c[k]; m.inv[k] = (float)c[9 + k]; }
    m.diag = c[18] != 0.0;
    return m;
}

// one pair term = ints (kind, p, q, theta_off, n_theta) + floats (c, a, phi, cutoff) (+ optional [N,N] uint8 mask)
MdgPairTerm make_term(at::ArrayRef<int64_t> ti, at::ArrayRef<double> tf, const OptTensor& mask) {
    TORCH_CHECK(ti.size() == 5 && tf.size() == 4, "mdgrad: pair term = 5 ints (kind, p, q, theta_off, n_theta) + 4 floats "
                "(c, a, phi, cutoff)");
    MdgPairTerm t{};
    t.kind = (int32_t)ti[0]; t.p = (int32_t)ti[1]; t.q = (int32_t)ti[2]; t.theta_off = (int32_t)ti[3]; t.n_theta = (int32_t)ti[4];
    t.c = (float)tf[0]; t.a = (float)tf[1]; t.phi = (float)tf[2]; t.cutoff = (float)tf[3];
    t.mask = nullptr;
    if (mask.has_value() && mask->defined()) {
        TORCH_CHECK(mask->is_cuda() && mask->scalar_type() == at::kByte && mask->is_contiguous(), "mdgrad: mask must be a "
                    "contiguous uint8 tensor on the device");
        t.mask = mask->data_ptr<uint8_t>();
    }
    return t;
}

// ------------------------------------------------------------------------------------------------ K1
// (col, shift, cnt, overflow): the padded per-atom full list of include/mdgrad_hip.h; `overflow` stays on the device
std::tuple<Tensor, Tensor, Tensor, Tensor> nbr_build(const Tensor& pos, at::ArrayRef<double> cell, double cutoff,
                                                     const OptTensor& mask, int64_t max_nbr, int64_t group, bool cell_list) {
    check_f32(pos, "pos");
    TORCH_CHECK(pos.dim() == 2 && pos.size(1) == 3, "mdgrad: pos must be [N,3]");
    const MdgCell c = make_cell(cell);
    const int64_t n = pos.size(0);
    const auto io = pos.options().dtype(at::kInt);
    Tensor col = at::empty({n, max_nbr}, io), shift = at::empty({n, max_nbr}, io), cnt = at::empty({n}, io);
    Tensor overflow = at::zeros({1}, io);
    const uint8_t* mk = nullptr;
    if (mask.has_value() && mask->defined()) {
        TORCH_CHECK(mask->is_cuda() && mask->scalar_type() == at::kByte && mask->is_contiguous(), "mdgrad: mask must be uint8");
        mk = mask->data_ptr<uint8_t>();
    }
    const int g = (int)(group > 0 ? group : n);
    void* st = stream_of(pos);
    if (cell_list) {
        const int64_t words = mdg_nbr_cell_scratch_groups((int)n, g, &c, (float)cutoff);
        TORCH_CHECK(words > 0, "mdgrad: the cell list needs an orthorhombic cell with at least 3 bins per side");
        Tensor scratch = at::empty({words}, io);
        ok(mdg_nbr_build_cell_groups(fptr(pos), (int)n, g, &c, (float)cutoff, mk, col.data_ptr<int32_t>(),
                                     shift.data_ptr<int32_t>(), cnt.data_ptr<int32_t>(), (int)max_nbr,
                                     overflow.data_ptr<int32_t>(), scratch.data_ptr<int32_t>(), st));
    } else {
        ok(mdg_nbr_build_dense_groups(fptr(pos), (int)n, g, &c, (float)cutoff, mk, col.data_ptr<int32_t>(),
                                      shift.data_ptr<int32_t>(), cnt.data_ptr<int32_t>(), (int)max_nbr,
                                      overflow.data_ptr<int32_t>(), st));
    }
    return {col, shift, cnt, overflow};
}

// ------------------------------------------------------------------------------------------------ K2-K4
struct EllRef { const int32_t* col; const int32_t* shift; const int32_t* cnt; int max_nbr; };
EllRef ell_of(const Tensor& pos, const Tensor& col, const Tensor& shift, const Tensor& cnt) {
    check_i32(col, "col"); check_i32(shift, "shift"); check_i32(cnt, "cnt");
    same_device(pos, col, "col");
    TORCH_CHECK(col.dim() == 2 && col.size(0) == pos.size(0) && shift.sizes() == col.sizes() && cnt.numel() == pos.size(0),
                "mdgrad: neighbour list does not match pos");
    return EllRef{col.data_ptr<int32_t>(), shift.data_ptr<int32_t>(), cnt.data_ptr<int32_t>(), (int)col.size(1)};
}

// (U[1], dU/dx [N,3], dU/dtheta [K])
std::tuple<Tensor, Tensor, Tensor> pair_force(const Tensor& pos, at::ArrayRef<double> cell, const Tensor& col,
                                              const Tensor& shift, const Tensor& cnt, at::ArrayRef<int64_t> term_i,
                                              at::ArrayRef<double> term_f, const OptTensor& mask, const OptTensor& theta) {
    check_f32(pos, "pos");
    const MdgCell c = make_cell(cell);
    const MdgPairTerm t = make_term(term_i, term_f, mask);
    const EllRef e = ell_of(pos, col, shift, cnt);
    const int n = (int)pos.size(0);
    Tensor U = at::empty({1}, pos.options()), g = at::empty_like(pos);
    Tensor gth = at::zeros({std::max<int64_t>(1, theta.has_value() && theta->defined() ? theta->numel() : 0)}, pos.options());
    Tensor partial = at::empty({mdg_pair_partial_size(n)}, pos.options());
    ok(mdg_pair_eval_ell(fptr(pos), n, &c, e.col, e.shift, e.cnt, e.max_nbr, &t, fptr(theta, "theta"), nullptr, mptr(U), mptr(g),
                         t.n_theta ? mptr(gth) : nullptr, nullptr, nullptr, mptr(partial), stream_of(pos)));
    return {U, g, gth};
}

// (H w [N,3], d(w . dU/dx)/dtheta [K])
std::tuple<Tensor, Tensor> pair_hvp(const Tensor& pos, at::ArrayRef<double> cell, const Tensor& col, const Tensor& shift,
                                    const Tensor& cnt, at::ArrayRef<int64_t> term_i, at::ArrayRef<double> term_f,
                                    const OptTensor& mask, const OptTensor& theta, const Tensor& w) {
    check_f32(pos, "pos"); check_f32(w, "w");
    TORCH_CHECK(w.sizes() == pos.sizes(), "mdgrad: w must have the shape of pos");
    const MdgCell c = make_cell(cell);
    const MdgPairTerm t = make_term(term_i, term_f, mask);
    const EllRef e = ell_of(pos, col, shift, cnt);
    const int n = (int)pos.size(0);
    Tensor hw = at::empty_like(pos);
    Tensor gth = at::zeros({std::max<int64_t>(1, theta.has_value() && theta->defined() ? theta->numel() : 0)}, pos.options());
    Tensor partial = at::empty({mdg_pair_partial_size(n)}, pos.options());
    ok(mdg_pair_eval_ell(fptr(pos), n, &c, e.col, e.shift, e.cnt, e.max_nbr, &t, fptr(theta, "theta"), fptr(w), nullptr, nullptr,
                         nullptr, mptr(hw), t.n_theta ? mptr(gth) : nullptr, mptr(partial), stream_of(pos)));
    return {hw, gth};
}

// ------------------------------------------------------------------------------------------------ K5-K7
struct TrajDesc { MdgTrajParams prm; MdgCell cell; MdgTerms terms; };
// iprm = (n_rep, n_atoms, n_frames, n_chains, ensemble, block); fprm = (T, n_dof, Q[0..n_chains));
// terms_i / terms_f = the terms' 5 ints / 4 floats back to back (no masks: masked Stacks take the generic path)
TrajDesc traj_desc(at::ArrayRef<int64_t> iprm, at::ArrayRef<double> fprm, at::ArrayRef<double> cell,
                   at::ArrayRef<int64_t> terms_i, at::ArrayRef<double> terms_f, int64_t n_theta_total) {
    TORCH_CHECK(iprm.size() == 6, "mdgrad: iprm = (n_rep, n_atoms, n_frames, n_chains, ensemble, block)");
    TrajDesc d{};
    d.prm.n_rep = (int32_t)iprm[0]; d.prm.n_atoms = (int32_t)iprm[1]; d.prm.n_frames = (int32_t)iprm[2];
    d.prm.n_chains = (int32_t)iprm[3]; d.prm.ensemble = (int32_t)iprm[4]; d.prm.block = (int32_t)iprm[5];
    TORCH_CHECK(fprm.size() >= 2 && fprm.size() <= 2 + MDG_MAX_CHAINS, "mdgrad: fprm = (T, n_dof, Q...)");
    d.prm.T = (float)fprm[0]; d.prm.n_dof = (float)fprm[1];
    for (size_t k = 2; k < fprm.size(); ++k) d.prm.Q[k - 2] = (float)fprm[k];
    d.cell = make_cell(cell);
    const size_t nt = terms_i.size() / 5;
    TORCH_CHECK(nt >= 1 && nt <= MDG_MAX_TERMS && terms_i.size() == 5 * nt && terms_f.size() == 4 * nt,
                "mdgrad: 1..", MDG_MAX_TERMS, " pair terms of 5 ints + 4 floats");
    d.terms.n_terms = (int32_t)nt; d.terms.n_theta_total = (int32_t)n_theta_total;
    for (size_t m = 0; m < nt; ++m)
        d.terms.t[m] = make_term(terms_i.slice(5 * m, 5), terms_f.slice(4 * m, 4), OptTensor());
    return d;
}

// (v_t [R,T,N,3], q_t [R,T,N,3], pv_t [R,T,C] (empty for NVE), nonfinite int32[R])
std::tuple<Tensor, Tensor, Tensor, Tensor> nhc_vv_forward(const Tensor& v0, const Tensor& q0, const OptTensor& pv0,
                                                          const Tensor& mass, const Tensor& t, const OptTensor& theta,
                                                          at::ArrayRef<int64_t> iprm, at::ArrayRef<double> fprm,
                                                          at::ArrayRef<double> cell, at::ArrayRef<int64_t> terms_i,
                                                          at::ArrayRef<double> terms_f, int64_t n_theta_total) {
    check_f32(v0, "v0"); check_f32(q0, "q0"); check_f32(mass, "mass"); check_f32(t, "t");
    const TrajDesc d = traj_desc(iprm, fprm, cell, terms_i, terms_f, n_theta_total);
    const int64_t R = d.prm.n_rep, T = d.prm.n_frames, N = d.prm.n_atoms, C = d.prm.n_chains;
    TORCH_CHECK(v0.numel() == R * N * 3 && q0.numel() == R * N * 3 && t.numel() == T, "mdgrad: state / time grid do not match iprm");
    const bool nhc = d.prm.ensemble == 0;
    Tensor v_t = at::empty({R, T, N, 3}, v0.options()), q_t = at::empty({R, T, N, 3}, v0.options());
    Tensor pv_t = at::empty({nhc ? R : 0, nhc ? T : 0, nhc ? C : 0}, v0.options());
    Tensor bad = at::zeros({R}, v0.options().dtype(at::kInt));
    ok(mdg_traj_fwd_small(&d.prm, &d.cell, &d.terms, fptr(theta, "theta"), fptr(mass), fptr(t), fptr(v0), fptr(q0),
                          fptr(pv0, "pv0"), mptr(v_t), mptr(q_t), nhc ? mptr(pv_t) : nullptr, bad.data_ptr<int32_t>(),
                          stream_of(v0)));
    return {v_t, q_t, pv_t, bad};
}

// (adj_v0 [R,N,3], adj_q0 [R,N,3], adj_pv0 [R,C], adj_theta [R,K])
std::tuple<Tensor, Tensor, Tensor, Tensor> nhc_vv_adjoint(const Tensor& v_t, const Tensor& q_t, const OptTensor& pv_t,
                                                          const OptTensor& g_v, const OptTensor& g_q, const OptTensor& g_pv,
                                                          const Tensor& mass, const Tensor& t, const OptTensor& theta,
                                                          at::ArrayRef<int64_t> iprm, at::ArrayRef<double> fprm,
                                                          at::ArrayRef<double> cell, at::ArrayRef<int64_t> terms_i,
                                                          at::ArrayRef<double> terms_f, int64_t n_theta_total) {
    check_f32(v_t, "v_t"); check_f32(q_t, "q_t"); check_f32(mass, "mass"); check_f32(t, "t");
    const TrajDesc d = traj_desc(iprm, fprm, cell, terms_i, terms_f, n_theta_total);
    const int64_t R = d.prm.n_rep, T = d.prm.n_frames, N = d.prm.n_atoms, C = d.prm.n_chains;
    TORCH_CHECK(v_t.numel() == R * T * N * 3 && q_t.numel() == R * T * N * 3, "mdgrad: trajectories do not match iprm");
    const bool nhc = d.prm.ensemble == 0;
    Tensor av = at::empty({R, N, 3}, v_t.options()), aq = at::empty({R, N, 3}, v_t.options());
    Tensor ap = at::empty({nhc ? R : 0, nhc ? C : 0}, v_t.options());
    Tensor ath = at::zeros({R, std::max<int64_t>(1, n_theta_total)}, v_t.options());
    ok(mdg_traj_adj_small(&d.prm, &d.cell, &d.terms, fptr(theta, "theta"), fptr(mass), fptr(t), fptr(v_t), fptr(q_t),
                          fptr(pv_t, "pv_t"), fptr(g_v, "g_v"), fptr(g_q, "g_q"), fptr(g_pv, "g_pv"), mptr(av), mptr(aq),
                          nhc ? mptr(ap) : nullptr, n_theta_total ? mptr(ath) : nullptr, stream_of(v_t)));
    return {av, aq, ap, ath};
}

// ------------------------------------------------------------------------------------------------ K8
Tensor rdf_fwd(const Tensor& xyz, at::ArrayRef<double> cell, double cutoff, const OptTensor& mask, const Tensor& mu,
               double spacing, double coeff) {
    check_f32(xyz, "xyz"); check_f32(mu, "mu");
    TORCH_CHECK(xyz.dim() == 3 && xyz.size(2) == 3, "mdgrad: xyz must be [F,N,3]");
    const MdgCell c = make_cell(cell);
    const int F = (int)xyz.size(0), N = (int)xyz.size(1), B = (int)mu.numel();
    Tensor raw = at::empty({B}, xyz.options()), partial = at::empty({mdg_rdf_partial_size(F, N, B)}, xyz.options());
    const uint8_t* mk = (mask.has_value() && mask->defined()) ? mask->data_ptr<uint8_t>() : nullptr;
    ok(mdg_rdf_fwd_uniform(fptr(xyz), F, N, &c, (float)cutoff, mk, fptr(mu), (float)spacing, (float)coeff, B, mptr(raw),
                           mptr(partial), stream_of(xyz)));
    return raw;
}
Tensor rdf_bwd(const Tensor& xyz, at::ArrayRef<double> cell, double cutoff, const OptTensor& mask, const Tensor& mu,
               double spacing, double coeff, const Tensor& g_raw) {
    check_f32(xyz, "xyz"); check_f32(mu, "mu"); check_f32(g_raw, "g_raw");
    const MdgCell c = make_cell(cell);
    const int F = (int)xyz.size(0), N = (int)xyz.size(1), B = (int)mu.numel();
    TORCH_CHECK(g_raw.numel() == B, "mdgrad: g_raw must have one entry per centre");
    Tensor g = at::empty_like(xyz);
    const uint8_t* mk = (mask.has_value() && mask->defined()) ? mask->data_ptr<uint8_t>() : nullptr;
    ok(mdg_rdf_bwd_uniform(fptr(xyz), F, N, &c, (float)cutoff, mk, fptr(mu), (float)spacing, (float)coeff, B, fptr(g_raw),
                           mptr(g), stream_of(xyz)));
    return g;
}

// ------------------------------------------------------------------------------------------------ K14
void adf_check(const Tensor& pos, int64_t n_frames, int64_t n_atoms, const Tensor& col, const Tensor& cnt, const Tensor& mu) {
    check_f32(pos, "pos"); check_f32(mu, "mu"); check_i32(col, "col"); check_i32(cnt, "cnt");
    same_device(pos, col, "col"); same_device(pos, cnt, "cnt"); same_device(pos, mu, "mu");
    TORCH_CHECK(n_frames > 0 && n_atoms > 0 && n_frames * n_atoms < (int64_t(1) << 31),
                "mdgrad: n_frames and n_atoms must be positive with n_frames * n_atoms < 2^31 (chunk the frames)");
    TORCH_CHECK(pos.numel() == n_frames * n_atoms * 3, "mdgrad: pos must hold n_frames * n_atoms rows of 3");
    TORCH_CHECK(col.dim() == 2 && col.size(0) == n_frames * n_atoms && cnt.numel() == col.size(0),
                "mdgrad: col must be [n_frames * n_atoms, max_nbr] and cnt [n_frames * n_atoms]");
}
Tensor adf_fwd(const Tensor& pos, int64_t n_frames, int64_t n_atoms, at::ArrayRef<double> cell, double cutoff, const Tensor& col,
               const Tensor& cnt, const Tensor& mu, double spacing, double coeff) {
    adf_check(pos, n_frames, n_atoms, col, cnt, mu);
    const MdgCell c = make_cell(cell);
    const int B = (int)mu.numel(), M = (int)col.size(1);
    Tensor raw = at::empty({B}, pos.options());
    Tensor scratch = at::empty({mdg_adf_partial_size((int)n_frames, (int)n_atoms, M, B)}, pos.options().dtype(at::kLong));
    ok(mdg_adf_fwd(fptr(pos), (int)n_frames, (int)n_atoms, &c, (float)cutoff, col.data_ptr<int32_t>(), cnt.data_ptr<int32_t>(), M,
                   fptr(mu), (float)spacing, (float)coeff, B, mptr(raw), scratch.data_ptr<int64_t>(), stream_of(pos)));
    return raw;
}
Tensor adf_bwd(const Tensor& pos, int64_t n_frames, int64_t n_atoms, at::ArrayRef<double> cell, double cutoff, const Tensor& col,
               const Tensor& cnt, const Tensor& mu, double spacing, double coeff, const Tensor& g_raw) {
    adf_check(pos, n_frames, n_atoms, col, cnt, mu);
    check_f32(g_raw, "g_raw"); same_device(pos, g_raw, "g_raw");
    const MdgCell c = make_cell(cell);
    const int B = (int)mu.numel(), M = (int)col.size(1);
    TORCH_CHECK(g_raw.numel() == B, "mdgrad: g_raw must have one entry per centre");
    Tensor g = at::empty_like(pos);
    ok(mdg_adf_bwd(fptr(pos), (int)n_frames, (int)n_atoms, &c, (float)cutoff, col.data_ptr<int32_t>(), cnt.data_ptr<int32_t>(), M,
                   fptr(mu), (float)spacing, (float)coeff, B, fptr(g_raw), mptr(g), stream_of(pos)));
    return g;
}

// ------------------------------------------------------------------------------------------------ K29
// (A [K, rows] component-major, n [rows]) and g_xyz [rows, 3] from gA [rows, K] row-major, gn [rows]; rows = n_frames * n_atoms
std::vector<int32_t> bond_order_ls(at::ArrayRef<int64_t> ls) {
    std::vector<int32_t> v(ls.begin(), ls.end());
    TORCH_CHECK(mdg_bond_order_components(v.data(), (int)v.size()) > 0, "mdgrad: ", mdg_last_error());
    return v;
}
std::tuple<Tensor, Tensor> bond_order_fwd(const Tensor& pos, int64_t n_frames, int64_t n_atoms, at::ArrayRef<double> cell, double cutoff,
                                          double r_in, const Tensor& col, const Tensor& cnt, at::ArrayRef<int64_t> ls) {
    adf_check(pos, n_frames, n_atoms, col, cnt, pos);
    const std::vector<int32_t> v = bond_order_ls(ls);
    const MdgCell c = make_cell(cell);
    const int64_t K = mdg_bond_order_components(v.data(), (int)v.size()), rows = n_frames * n_atoms;
    Tensor A = at::empty({K, rows}, pos.options()), n = at::empty({rows}, pos.options());
    ok(mdg_bond_order_fwd(fptr(pos), (int)n_frames, (int)n_atoms, &c, (float)cutoff, (float)r_in, col.data_ptr<int32_t>(),
                          cnt.data_ptr<int32_t>(), (int)col.size(1), v.data(), (int)v.size(), mptr(A), mptr(n), stream_of(pos)));
    return std::make_tuple(A, n);
}
Tensor bond_order_bwd(const Tensor& pos, int64_t n_frames, int64_t n_atoms, at::ArrayRef<double> cell, double cutoff, double r_in,
                      const Tensor& col, const Tensor& cnt, at::ArrayRef<int64_t> ls, const Tensor& gA, const Tensor& gn) {
    adf_check(pos, n_frames, n_atoms, col, cnt, pos);
    check_f32(gA, "gA"); check_f32(gn, "gn"); same_device(pos, gA, "gA"); same_device(pos, gn, "gn");
    const std::vector<int32_t> v = bond_order_ls(ls);
    const MdgCell c = make_cell(cell);
    const int64_t K = mdg_bond_order_components(v.data(), (int)v.size()), rows = n_frames * n_atoms;
    TORCH_CHECK(gA.numel() == rows * K && gn.numel() == rows, "mdgrad: gA must be [n_frames * n_atoms, K] and gn [n_frames * n_atoms]");
    Tensor g = at::empty_like(pos);
    ok(mdg_bond_order_bwd(fptr(pos), (int)n_frames, (int)n_atoms, &c, (float)cutoff, (float)r_in, col.data_ptr<int32_t>(),
                          cnt.data_ptr<int32_t>(), (int)col.size(1), v.data(), (int)v.size(), fptr(gA), fptr(gn), mptr(g),
                          stream_of(pos)));
    return g;
}

// ------------------------------------------------------------------------------------------------ K15
// terms_i / terms_f = the terms' 5 ints / 4 floats back to back; masks = one optional [N,N] uint8 selection per term
MdgTerms virial_terms(const Tensor& pos, at::ArrayRef<int64_t> terms_i, at::ArrayRef<double> terms_f,
                      const c10::List<c10::optional<Tensor>>& masks, const OptTensor& theta) {
    check_f32(pos, "pos");
    TORCH_CHECK(pos.dim() == 3 && pos.size(2) == 3, "mdgrad: pos must be [F,N,3]");
    const size_t nt = terms_i.size() / 5;
    TORCH_CHECK(nt >= 1 && nt <= MDG_MAX_TERMS && terms_i.size() == 5 * nt && terms_f.size() == 4 * nt && masks.size() == nt,
                "mdgrad: 1..", MDG_MAX_TERMS, " pair terms of 5 ints + 4 floats + an optional mask");
    MdgTerms ts{};
    ts.n_terms = (int32_t)nt;
    for (size_t m = 0; m < nt; ++m) {
        const OptTensor mk = masks.get(m);
        if (mk.has_value() && mk->defined()) {
            same_device(pos, *mk, "mask");
            TORCH_CHECK(mk->numel() == pos.size(1) * pos.size(1), "mdgrad: a mask must be [N,N]");
        }
        ts.t[m] = make_term(terms_i.slice(5 * m, 5), terms_f.slice(4 * m, 4), mk);
        ts.n_theta_total += ts.t[m].n_theta;
    }
    const int64_t have = (theta.has_value() && theta->defined()) ? theta->numel() : 0;
    TORCH_CHECK(have == ts.n_theta_total, "mdgrad: theta must hold the terms' ", ts.n_theta_total, " parameters");
    if (have) same_device(pos, *theta, "theta");
    return ts;
}
Tensor virial_fwd(const Tensor& pos, at::ArrayRef<double> cell, at::ArrayRef<int64_t> terms_i, at::ArrayRef<double> terms_f,
                  const c10::List<c10::optional<Tensor>>& masks, const OptTensor& theta) {
    const MdgTerms ts = virial_terms(pos, terms_i, terms_f, masks, theta);
    const MdgCell c = make_cell(cell);
    const int F = (int)pos.size(0), N = (int)pos.size(1);
    Tensor W = at::empty({F}, pos.options()), ws = at::empty({mdg_virial_workspace(F, N, ts.n_theta_total)}, pos.options());
    ok(mdg_virial_fwd(fptr(pos), F, N, &c, &ts, fptr(theta, "theta"), mptr(W), mptr(ws), stream_of(pos)));
    return W;
}
// (g_pos [F,N,3], g_theta [K])
std::tuple<Tensor, Tensor> virial_bwd(const Tensor& pos, at::ArrayRef<double> cell, at::ArrayRef<int64_t> terms_i,
                                      at::ArrayRef<double> terms_f, const c10::List<c10::optional<Tensor>>& masks,
                                      const OptTensor& theta, const Tensor& gW) {
    const MdgTerms ts = virial_terms(pos, terms_i, terms_f, masks, theta);
    check_f32(gW, "gW"); same_device(pos, gW, "gW");
    TORCH_CHECK(gW.numel() == pos.size(0), "mdgrad: gW must have one entry per frame");
    const MdgCell c = make_cell(cell);
    const int F = (int)pos.size(0), N = (int)pos.size(1), K = ts.n_theta_total;
    Tensor g = at::empty_like(pos), gth = at::empty({K}, pos.options());
    Tensor ws = at::empty({mdg_virial_workspace(F, N, K)}, pos.options());
    ok(mdg_virial_bwd(fptr(pos), F, N, &c, &ts, fptr(theta, "theta"), fptr(gW), mptr(g), K ? mptr(gth) : nullptr, mptr(ws),
                      stream_of(pos)));
    return {g, gth};
}

// ------------------------------------------------------------------------------------------------ K31
// arguments as K15; U [F]
Tensor energy_frames_fwd(const Tensor& pos, at::ArrayRef<double> cell, at::ArrayRef<int64_t> terms_i, at::ArrayRef<double> terms_f,
                         const c10::List<c10::optional<Tensor>>& masks, const OptTensor& theta) {
    const MdgTerms ts = virial_terms(pos, terms_i, terms_f, masks, theta);
    const MdgCell c = make_cell(cell);
    const int F = (int)pos.size(0), N = (int)pos.size(1);
    Tensor U = at::empty({F}, pos.options()), ws = at::empty({mdg_energy_frames_workspace(F, N, ts.n_theta_total)}, pos.options());
    ok(mdg_energy_frames_fwd(fptr(pos), F, N, &c, &ts, fptr(theta, "theta"), mptr(U), mptr(ws), stream_of(pos)));
    return U;
}
// (g_pos [F,N,3], g_theta [K]); want_pos = false: the parameters-only sweep, g_pos comes back empty
std::tuple<Tensor, Tensor> energy_frames_bwd(const Tensor& pos, at::ArrayRef<double> cell, at::ArrayRef<int64_t> terms_i,
                                             at::ArrayRef<double> terms_f, const c10::List<c10::optional<Tensor>>& masks,
                                             const OptTensor& theta, const Tensor& gU, bool want_pos) {
    const MdgTerms ts = virial_terms(pos, terms_i, terms_f, masks, theta);
    check_f32(gU, "gU"); same_device(pos, gU, "gU");
    TORCH_CHECK(gU.numel() == pos.size(0), "mdgrad: gU must have one entry per frame");
    const MdgCell c = make_cell(cell);
    const int F = (int)pos.size(0), N = (int)pos.size(1), K = ts.n_theta_total;
    TORCH_CHECK(want_pos || K > 0, "mdgrad: nothing to compute (no position gradient wanted and the terms hold no parameters)");
    Tensor g = want_pos ? at::empty_like(pos) : at::empty({0}, pos.options()), gth = at::empty({K}, pos.options());
    Tensor ws = at::empty({mdg_energy_frames_workspace(F, N, K)}, pos.options());
    ok(mdg_energy_frames_bwd(fptr(pos), F, N, &c, &ts, fptr(theta, "theta"), fptr(gU), want_pos ? mptr(g) : nullptr,
                             K ? mptr(gth) : nullptr, mptr(ws), stream_of(pos)));
    return {g, gth};
}

// ------------------------------------------------------------------------------------------------ K32
const uint8_t* rdf_frames_check(const Tensor& xyz, const OptTensor& mask, const Tensor& mu) {
    check_f32(xyz, "xyz"); check_f32(mu, "mu"); same_device(xyz, mu, "mu");
    TORCH_CHECK(xyz.dim() == 3 && xyz.size(2) == 3, "mdgrad: xyz must be [F,N,3]");
    if (!(mask.has_value() && mask->defined())) return nullptr;
    same_device(xyz, *mask, "mask");
    TORCH_CHECK(mask->scalar_type() == at::kByte && mask->is_contiguous() && mask->numel() == xyz.size(1) * xyz.size(1),
                "mdgrad: mask must be a contiguous uint8 [N,N] tensor");
    return mask->data_ptr<uint8_t>();
}
Tensor rdf_frames_fwd(const Tensor& xyz, at::ArrayRef<double> cell, double cutoff, const OptTensor& mask, const Tensor& mu,
                      double spacing, double coeff) {
    const uint8_t* mk = rdf_frames_check(xyz, mask, mu);
    const MdgCell c = make_cell(cell);
    const int F = (int)xyz.size(0), N = (int)xyz.size(1), B = (int)mu.numel();
    Tensor raw = at::empty({F, B}, xyz.options());
    ok(mdg_rdf_frames_fwd(fptr(xyz), F, N, &c, (float)cutoff, mk, fptr(mu), (float)spacing, (float)coeff, B, mptr(raw),
                          stream_of(xyz)));
    return raw;
}
Tensor rdf_frames_bwd(const Tensor& xyz, at::ArrayRef<double> cell, double cutoff, const OptTensor& mask, const Tensor& mu,
                      double spacing, double coeff, const Tensor& g_raw) {
    const uint8_t* mk = rdf_frames_check(xyz, mask, mu);
    check_f32(g_raw, "g_raw"); same_device(xyz, g_raw, "g_raw");
    const MdgCell c = make_cell(cell);
    const int F = (int)xyz.size(0), N = (int)xyz.size(1), B = (int)mu.numel();
    TORCH_CHECK(g_raw.numel() == (int64_t)F * B, "mdgrad: g_raw must be [F, nbins]");
    Tensor g = at::empty_like(xyz);
    ok(mdg_rdf_frames_bwd(fptr(xyz), F, N, &c, (float)cutoff, mk, fptr(mu), (float)spacing, (float)coeff, B, fptr(g_raw), mptr(g),
                          stream_of(xyz)));
    return g;
}

// ------------------------------------------------------------------------------------------------ K16
// pos [F,N,3]; kvec int32 [M,3] sorted by bin, seg int32 [B+1] (its host copy seg_host gives the shapes a check without a
// device read); weights [N] or none, norm = sum of the squared weights
void sk_check(const Tensor& pos, const OptTensor& weights, const Tensor& kvec, const Tensor& seg, at::ArrayRef<int64_t> seg_host) {
    check_f32(pos, "pos");
    TORCH_CHECK(pos.dim() == 3 && pos.size(2) == 3, "mdgrad: pos must be [F,N,3]");
    check_i32(kvec, "kvec"); check_i32(seg, "seg");
    same_device(pos, kvec, "kvec"); same_device(pos, seg, "seg");
    TORCH_CHECK(kvec.dim() == 2 && kvec.size(1) == 3, "mdgrad: kvec must be [M,3]");
    TORCH_CHECK(seg_host.size() >= 2 && (int64_t)seg_host.size() == seg.numel(), "mdgrad: seg and seg_host must hold the same "
                "n_bins + 1 offsets");
    TORCH_CHECK(seg_host.front() == 0 && seg_host.back() == kvec.size(0), "mdgrad: the vector table kvec must hold seg[-1] = ",
                seg_host.back(), " rows, got ", kvec.size(0));
    for (size_t b = 1; b < seg_host.size(); ++b) TORCH_CHECK(seg_host[b] >= seg_host[b - 1], "mdgrad: seg must be ascending");
    if (weights.has_value() && weights->defined()) {
        TORCH_CHECK(weights->numel() == pos.size(1), "mdgrad: weights must hold one entry per atom");
        same_device(pos, *weights, "weights");
    }
}
Tensor sk_fwd(const Tensor& pos, at::ArrayRef<double> cell, const OptTensor& weights, double norm, const Tensor& kvec,
              const Tensor& seg, at::ArrayRef<int64_t> seg_host) {
    sk_check(pos, weights, kvec, seg, seg_host);
    const MdgCell c = make_cell(cell);
    const int F = (int)pos.size(0), N = (int)pos.size(1), M = (int)kvec.size(0), B = (int)seg.numel() - 1;
    Tensor S = at::empty({F, B}, pos.options()), ws = at::empty({mdg_sk_workspace(F, N, M)}, pos.options());
    ok(mdg_sk_fwd(fptr(pos), F, N, &c, fptr(weights, "weights"), (float)norm, kvec.data_ptr<int32_t>(), M, seg.data_ptr<int32_t>(),
                  B, mptr(S), mptr(ws), stream_of(pos)));
    return S;
}
Tensor sk_bwd(const Tensor& pos, at::ArrayRef<double> cell, const OptTensor& weights, double norm, const Tensor& kvec,
              const Tensor& seg, at::ArrayRef<int64_t> seg_host, const Tensor& gS) {
    sk_check(pos, weights, kvec, seg, seg_host);
    check_f32(gS, "gS"); same_device(pos, gS, "gS");
    const MdgCell c = make_cell(cell);
    const int F = (int)pos.size(0), N = (int)pos.size(1), M = (int)kvec.size(0), B = (int)seg.numel() - 1;
    TORCH_CHECK(gS.numel() == (int64_t)F * B, "mdgrad: gS must be [F,B]");
    Tensor g = at::empty_like(pos), ws = at::empty({mdg_sk_workspace(F, N, M)}, pos.options());
    ok(mdg_sk_bwd(fptr(pos), F, N, &c, fptr(weights, "weights"), (float)norm, kvec.data_ptr<int32_t>(), M, seg.data_ptr<int32_t>(),
                  B, fptr(gS), mptr(g), mptr(ws), stream_of(pos)));
    return g;
}

// ------------------------------------------------------------------------------------------------ K17
// x [n_batch,T,n_cols,3]; the columns are n_cols / group replicas of `group` atoms; weights [group] or none
void msd_check(const Tensor& x, int64_t group, const OptTensor& weights, int64_t n_lags, int64_t origin_stride) {
    check_f32(x, "x");
    TORCH_CHECK(x.dim() == 4 && x.size(3) == 3, "mdgrad: x must be [n_batch,T,n_cols,3]");
    TORCH_CHECK(group >= 1 && x.size(2) % group == 0, "mdgrad: the columns of x (", x.size(2), ") must be a multiple of group (",
                group, ")");
    TORCH_CHECK(n_lags >= 1 && n_lags <= x.size(1), "mdgrad: 1 <= n_lags <= T (got ", n_lags, ", ", x.size(1), ")");
    TORCH_CHECK(origin_stride >= 1 && origin_stride <= INT32_MAX, "mdgrad: origin_stride must be >= 1");
    TORCH_CHECK(x.size(0) <= INT32_MAX && x.size(1) <= INT32_MAX && x.size(2) <= INT32_MAX, "mdgrad: x is too large");
    if (weights.has_value() && weights->defined()) {
        TORCH_CHECK(weights->numel() == group, "mdgrad: weights must hold one entry per atom of a replica (", group, ")");
        same_device(x, *weights, "weights");
    }
}
std::tuple<Tensor, Tensor> msd_fwd(const Tensor& x, int64_t group, const OptTensor& weights, int64_t n_lags, int64_t origin_stride,
                                   bool fourth) {
    msd_check(x, group, weights, n_lags, origin_stride);
    const int nb = (int)x.size(0), T = (int)x.size(1), nc = (int)x.size(2);
    const int64_t rows = (int64_t)nb * (nc / group);
    Tensor m2 = at::empty({rows, n_lags}, x.options()), m4 = at::empty({fourth ? rows : 0, n_lags}, x.options());
    Tensor ws = at::empty({std::max<int64_t>(mdg_msd_workspace(nb, nc, (int)group, (int)n_lags, fourth), 2)}, x.options());
    ok(mdg_msd_fwd(fptr(x), nb, T, nc, (int)group, fptr(weights, "weights"), (int)n_lags, (int)origin_stride, mptr(m2),
                   fourth ? mptr(m4) : nullptr, mptr(ws), stream_of(x)));
    return {m2, m4};
}
Tensor msd_bwd(const Tensor& x, int64_t group, const OptTensor& weights, int64_t n_lags, int64_t origin_stride, const Tensor& g2,
               const OptTensor& g4) {
    msd_check(x, group, weights, n_lags, origin_stride);
    check_f32(g2, "g2"); same_device(x, g2, "g2");
    const int nb = (int)x.size(0), T = (int)x.size(1), nc = (int)x.size(2);
    const int64_t rows = (int64_t)nb * (nc / group);
    TORCH_CHECK(g2.numel() == rows * n_lags, "mdgrad: g2 must be [rows,n_lags]");
    const bool fourth = g4.has_value() && g4->defined();
    if (fourth) {
        TORCH_CHECK(g4->numel() == rows * n_lags, "mdgrad: g4 must be [rows,n_lags]");
        same_device(x, *g4, "g4");
    }
    Tensor gx = at::empty_like(x);
    Tensor ws = at::empty({std::max<int64_t>(mdg_msd_workspace(nb, nc, (int)group, (int)n_lags, fourth), 2)}, x.options());
    ok(mdg_msd_bwd(fptr(x), nb, T, nc, (int)group, fptr(weights, "weights"), (int)n_lags, (int)origin_stride, fptr(g2),
                   fptr(g4, "g4"), mptr(gx), mptr(ws), stream_of(x)));
    return gx;
}

// ------------------------------------------------------------------------------------------------ K18
// x [n_batch,T,n_cols,3]; the replicas rep0 .. rep0 + n_reps - 1 of every batch; kvec / seg / seg_host / weights / norm as K16
void isf_check(const Tensor& x, int64_t kind, int64_t group, int64_t rep0, int64_t n_reps, const OptTensor& weights,
               const Tensor& kvec, const Tensor& seg, at::ArrayRef<int64_t> seg_host, int64_t n_lags, int64_t origin_stride) {
    check_f32(x, "x");
    TORCH_CHECK(kind == 0 || kind == 1, "mdgrad: kind must be 0 (coherent) or 1 (self)");
    TORCH_CHECK(x.dim() == 4 && x.size(3) == 3, "mdgrad: x must be [n_batch,T,n_cols,3]");
    TORCH_CHECK(group >= 1 && x.size(2) % group == 0, "mdgrad: the columns of x (", x.size(2), ") must be a multiple of group (",
                group, ")");
    TORCH_CHECK(rep0 >= 0 && n_reps >= 1 && rep0 + n_reps <= x.size(2) / group, "mdgrad: replicas ", rep0, " .. +", n_reps,
                " are not among the ", x.size(2) / group, " of x");
    TORCH_CHECK(n_lags >= 1 && n_lags <= x.size(1), "mdgrad: 1 <= n_lags <= T (got ", n_lags, ", ", x.size(1), ")");
    TORCH_CHECK(origin_stride >= 1 && origin_stride <= INT32_MAX, "mdgrad: origin_stride must be >= 1");
    TORCH_CHECK(x.size(0) <= INT32_MAX && x.size(1) <= INT32_MAX && x.size(2) <= INT32_MAX, "mdgrad: x is too large");
    check_i32(kvec, "kvec"); check_i32(seg, "seg");
    same_device(x, kvec, "kvec"); same_device(x, seg, "seg");
    TORCH_CHECK(kvec.dim() == 2 && kvec.size(1) == 3, "mdgrad: kvec must be [M,3]");
    TORCH_CHECK(seg_host.size() >= 2 && (int64_t)seg_host.size() == seg.numel(), "mdgrad: seg and seg_host must hold the same "
                "n_bins + 1 offsets");
    TORCH_CHECK(seg_host.front() == 0 && seg_host.back() == kvec.size(0), "mdgrad: the vector table kvec must hold seg[-1] = ",
                seg_host.back(), " rows, got ", kvec.size(0));
    for (size_t b = 1; b < seg_host.size(); ++b) TORCH_CHECK(seg_host[b] >= seg_host[b - 1], "mdgrad: seg must be ascending");
    if (weights.has_value() && weights->defined()) {
        TORCH_CHECK(weights->numel() == group, "mdgrad: weights must hold one entry per atom of a replica (", group, ")");
        same_device(x, *weights, "weights");
    }
}
int64_t isf_ws(int64_t kind, int64_t rows, int T, int64_t group, int M, int64_t n_lags) {
    return std::max<int64_t>(mdg_isf_workspace((int)kind, rows, T, (int)group, M, (int)n_lags), 1);
}
Tensor isf_fwd(const Tensor& x, int64_t kind, int64_t group, int64_t rep0, int64_t n_reps, at::ArrayRef<double> cell,
               const OptTensor& weights, double norm, const Tensor& kvec, const Tensor& seg, at::ArrayRef<int64_t> seg_host,
               int64_t n_lags, int64_t origin_stride) {
    isf_check(x, kind, group, rep0, n_reps, weights, kvec, seg, seg_host, n_lags, origin_stride);
    const MdgCell c = make_cell(cell);
    const int nb = (int)x.size(0), T = (int)x.size(1), nc = (int)x.size(2), M = (int)kvec.size(0), B = (int)seg.numel() - 1;
    const int64_t rows = (int64_t)nb * n_reps;
    Tensor F = at::empty({rows, B, n_lags}, x.options()), ws = at::empty({isf_ws(kind, rows, T, group, M, n_lags)}, x.options());
    ok(mdg_isf_fwd((int)kind, fptr(x), nb, T, nc, (int)group, (int)rep0, (int)n_reps, &c, fptr(weights, "weights"), norm,
                   kvec.data_ptr<int32_t>(), M, seg.data_ptr<int32_t>(), B, (int)n_lags, (int)origin_stride, mptr(F), mptr(ws),
                   stream_of(x)));
    return F;
}
// writes the columns of the call's replicas in gx (the shape of x) and leaves the others alone
void isf_bwd(const Tensor& x, int64_t kind, int64_t group, int64_t rep0, int64_t n_reps, at::ArrayRef<double> cell,
             const OptTensor& weights, double norm, const Tensor& kvec, const Tensor& seg, at::ArrayRef<int64_t> seg_host,
             int64_t n_lags, int64_t origin_stride, const Tensor& gF, Tensor gx) {
    isf_check(x, kind, group, rep0, n_reps, weights, kvec, seg, seg_host, n_lags, origin_stride);
    check_f32(gF, "gF"); same_device(x, gF, "gF");
    check_f32(gx, "gx"); same_device(x, gx, "gx");
    TORCH_CHECK(gx.sizes() == x.sizes(), "mdgrad: gx must have the shape of x");
    const MdgCell c = make_cell(cell);
    const int nb = (int)x.size(0), T = (int)x.size(1), nc = (int)x.size(2), M = (int)kvec.size(0), B = (int)seg.numel() - 1;
    const int64_t rows = (int64_t)nb * n_reps;
    TORCH_CHECK(gF.numel() == rows * B * n_lags, "mdgrad: gF must be [rows,n_bins,n_lags]");
    Tensor ws = at::empty({isf_ws(kind, rows, T, group, M, n_lags)}, x.options());
    ok(mdg_isf_bwd((int)kind, fptr(x), nb, T, nc, (int)group, (int)rep0, (int)n_reps, &c, fptr(weights, "weights"), norm,
                   kvec.data_ptr<int32_t>(), M, seg.data_ptr<int32_t>(), B, (int)n_lags, (int)origin_stride, fptr(gF), mptr(gx),
                   mptr(ws), stream_of(x)));
}

// ------------------------------------------------------------------------------------------------ SchNet block
MdgFilterNet filter_net(const Tensor& mu, const Tensor& coef, const Tensor& W1, const Tensor& b1, const Tensor& W2,
                        const Tensor& b2) {
    check_f32(mu, "mu"); check_f32(coef, "coef"); check_f32(W1, "W1"); check_f32(b1, "b1"); check_f32(W2, "W2"); check_f32(b2, "b2");
    MdgFilterNet n{};
    n.mu = fptr(mu); n.coef = fptr(coef); n.W1 = fptr(W1); n.b1 = fptr(b1); n.W2 = fptr(W2); n.b2 = fptr(b2);
    n.n_gauss = (int32_t)mu.numel(); n.n_filters = (int32_t)W2.size(0);
    TORCH_CHECK(W1.dim() == 2 && W1.size(0) == n.n_gauss && W1.size(1) == n.n_gauss && W2.dim() == 2 && W2.size(1) == n.n_gauss,
                "mdgrad: filter network shapes (W1 [G,G], W2 [F,G])");
    TORCH_CHECK(mdg_cfconv_supported(n.n_gauss, n.n_filters), "mdgrad: fused cfconv needs G <= 64 and F a multiple of 4 up to 64, of 8 up to 128, or of 128 up to 512");
    return n;
}

// (d, uhat, dd, ddel): dd / ddel are empty without w
std::tuple<Tensor, Tensor, Tensor, Tensor> edge_geom(const Tensor& x, const OptTensor& w, const Tensor& nbr, const Tensor& offsets) {
    check_f32(x, "x"); check_f32(offsets, "offsets");
    TORCH_CHECK(nbr.is_cuda() && nbr.scalar_type() == at::kLong && nbr.is_contiguous() && nbr.dim() == 2 && nbr.size(1) == 2,
                "mdgrad: nbr must be a contiguous int64 [E,2] tensor on the device");
    const int64_t E = nbr.size(0);
    const bool tan = w.has_value() && w->defined();
    Tensor d = at::empty({E}, x.options()), u = at::empty({E, 3}, x.options());
    Tensor dd = at::empty({tan ? E : 0}, x.options()), ddel = at::empty({tan ? E : 0, 3}, x.options());
    ok(mdg_edge_geom(fptr(x), fptr(w, "w"), nbr.data_ptr<int64_t>(), fptr(offsets), E, mptr(d), mptr(u), tan ? mptr(dd) : nullptr,
                     tan ? mptr(ddel) : nullptr, stream_of(x)));
    return {d, u, dd, ddel};
}

// (force [N,3], dwf [N,3] (empty without d_b))
std::tuple<Tensor, Tensor> edge_geom_bwd(const OptTensor& d_b, const Tensor& dd_b, const OptTensor& d, const OptTensor& dd,
                                         const Tensor& uhat, const OptTensor& ddel, const Tensor& col, const Tensor& eid,
                                         const Tensor& cnt) {
    check_f32(dd_b, "dd_b"); check_f32(uhat, "uhat");
    check_i32(col, "col"); check_i32(eid, "eid"); check_i32(cnt, "cnt");
    const int64_t N = cnt.numel();
    const bool full = d_b.has_value() && d_b->defined();
    TORCH_CHECK(!full || (d.has_value() && d->defined()), "mdgrad: d(w.F)/dx needs the distances d");
    Tensor f = at::empty({N, 3}, uhat.options()), dwf = at::empty({full ? N : 0, 3}, uhat.options());
    ok(mdg_edge_geom_bwd(fptr(d_b, "d_b"), fptr(dd_b), fptr(d, "d"), fptr(dd, "dd"), fptr(uhat), fptr(ddel, "ddel"),
                         col.data_ptr<int32_t>(), eid.data_ptr<int32_t>(), cnt.data_ptr<int32_t>(), (int)N, (int)col.size(1), mptr(f),
                         full ? mptr(dwf) : nullptr, stream_of(uhat)));
    return {f, dwf};
}

// (m, md, hsum, hdsum); md / hsum / hdsum are empty when not requested
std::tuple<Tensor, Tensor, Tensor, Tensor> cfconv_fwd(const Tensor& mu, const Tensor& coef, const Tensor& W1, const Tensor& b1,
                                                      const Tensor& W2, const Tensor& b2, bool bf16, const Tensor& d,
                                                      const OptTensor& dd, const Tensor& h, const OptTensor& hd,
                                                      const Tensor& col, const Tensor& eid, const Tensor& cnt, bool want_sums) {
    const MdgFilterNet net = filter_net(mu, coef, W1, b1, W2, b2);
    const bool r16 = is_bf16(h);                 // bf16 mirrors of the node rows: mdg_cfconv_fwd_rows16
    check_f32(d, "d");
    if (!r16) check_f32(h, "h");
    check_i32(col, "col"); check_i32(eid, "eid"); check_i32(cnt, "cnt");
    const int64_t N = cnt.numel(), F = net.n_filters;
    TORCH_CHECK(h.dim() == 2 && h.size(0) == N && h.size(1) == F, "mdgrad: h must be [N,F]");
    const bool tan = dd.has_value() && dd->defined(), htan = hd.has_value() && hd->defined();
    const auto fo = h.options().dtype(at::kFloat);
    Tensor m = at::empty({N, F}, fo), md = at::empty({tan ? N : 0, F}, fo);
    Tensor hs = at::empty({want_sums ? N : 0, F}, fo), hds = at::empty({want_sums && htan ? N : 0, F}, fo);
    if (r16) {
        TORCH_CHECK(bf16, "mdgrad: bf16 node rows go with the bf16 filter kernels");
        ok(mdg_cfconv_fwd_rows16(&net, fptr(d), fptr(dd, "dd"), hptr(h, "h"), hptr(hd, "hd"), col.data_ptr<int32_t>(),
                                 eid.data_ptr<int32_t>(), cnt.data_ptr<int32_t>(), (int)N, (int)col.size(1), mptr(m),
                                 tan ? mptr(md) : nullptr, want_sums ? mptr(hs) : nullptr, want_sums && htan ? mptr(hds) : nullptr,
                                 stream_of(h)));
        return {m, md, hs, hds};
    }
    auto fn = bf16 ? mdg_cfconv_fwd_bf16 : mdg_cfconv_fwd;
    ok(fn(&net, fptr(d), fptr(dd, "dd"), fptr(h), fptr(hd, "hd"), col.data_ptr<int32_t>(), eid.data_ptr<int32_t>(),
          cnt.data_ptr<int32_t>(), (int)N, (int)col.size(1), mptr(m), tan ? mptr(md) : nullptr, want_sums ? mptr(hs) : nullptr,
          want_sums && htan ? mptr(hds) : nullptr, stream_of(h)));
    return {m, md, hs, hds};
}

// accumulates into d_b / dd_b in place; (gW1, gb1, gW2) are empty unless want_theta
std::tuple<Tensor, Tensor, Tensor> cfconv_bwd(const Tensor& mu, const Tensor& coef, const Tensor& W1, const Tensor& b1,
                                              const Tensor& W2, const Tensor& b2, const Tensor& d, const OptTensor& dd,
                                              const Tensor& nbr, int64_t n_edges, const Tensor& h, const OptTensor& hd,
                                              const OptTensor& mb, const Tensor& mdb, const OptTensor& d_b, Tensor& dd_b,
                                              const OptTensor& n_valid, bool want_theta, bool bf16) {
    const MdgFilterNet net = filter_net(mu, coef, W1, b1, W2, b2);
    const bool r16 = is_bf16(h);                 // bf16 mirrors of the four gathered matrices: mdg_cfconv_bwd_rows16
    check_f32(d, "d"); check_f32(dd_b, "dd_b");
    if (!r16) { check_f32(h, "h"); check_f32(mdb, "mdb"); }
    TORCH_CHECK(nbr.is_cuda() && nbr.scalar_type() == at::kLong && nbr.is_contiguous(), "mdgrad: nbr must be int64 on the device");
    const int64_t G = net.n_gauss, F = net.n_filters;
    const auto fo = h.options().dtype(at::kFloat);
    Tensor gW1 = at::empty({want_theta ? G : 0, G}, fo), gb1 = at::empty({want_theta ? G : 0}, fo);
    Tensor gW2 = at::empty({want_theta ? F : 0, G}, fo);
    Tensor ws = at::empty({want_theta ? std::max<int64_t>(1, mdg_cfconv_bwd_workspace((int)G, (int)F, n_edges)) : 0}, fo);
    const int32_t* nv = nullptr;
    if (n_valid.has_value() && n_valid->defined()) { check_i32(*n_valid, "n_valid"); nv = n_valid->data_ptr<int32_t>(); }
    if (r16) {
        TORCH_CHECK(bf16, "mdgrad: bf16 node rows go with the bf16 filter kernels");
        ok(mdg_cfconv_bwd_rows16(&net, fptr(d), fptr(dd, "dd"), nbr.data_ptr<int64_t>(), n_edges, (int)h.size(0), hptr(h, "h"),
                                 hptr(hd, "hd"), hptr(mb, "mb"), hptr(mdb, "mdb"), const_cast<float*>(fptr(d_b, "d_b")), mptr(dd_b),
                                 want_theta ? mptr(gW1) : nullptr, want_theta ? mptr(gb1) : nullptr, want_theta ? mptr(gW2) : nullptr,
                                 nullptr, nullptr, want_theta ? mptr(ws) : nullptr, nv, stream_of(h)));
        return {gW1, gb1, gW2};
    }
    auto fn = bf16 ? mdg_cfconv_bwd_bf16 : mdg_cfconv_bwd;
    ok(fn(&net, fptr(d), fptr(dd, "dd"), nbr.data_ptr<int64_t>(), n_edges, fptr(h), fptr(hd, "hd"), fptr(mb, "mb"),
          fptr(mdb), const_cast<float*>(fptr(d_b, "d_b")), mptr(dd_b), want_theta ? mptr(gW1) : nullptr, want_theta ? mptr(gb1) : nullptr,
          want_theta ? mptr(gW2) : nullptr, want_theta ? mptr(ws) : nullptr, nv, stream_of(h)));
    return {gW1, gb1, gW2};
}

// out0 = act(x0 B + bias) * mul + res ; out1 = act'(.) (x1 B) + res1 ; (out0, sig0, out1)
std::tuple<Tensor, Tensor, Tensor> dense_ssp(const Tensor& W, bool trans, bool act, const Tensor& x0, const OptTensor& bias,
                                             const OptTensor& mul, const OptTensor& res, const OptTensor& x1,
                                             const OptTensor& res1, bool want_sig) {
    check_f32(W, "W"); check_f32(x0, "x0");
    TORCH_CHECK(W.dim() == 2 && x0.dim() == 2, "mdgrad: dense takes matrices");
    const int64_t N = x0.size(0), K = x0.size(1), M = trans ? W.size(1) : W.size(0);
    TORCH_CHECK((trans ? W.size(0) : W.size(1)) == K, "mdgrad: dense: shape mismatch");
    const bool dual = x1.has_value() && x1->defined();
    Tensor out0 = at::empty({N, M}, x0.options()), sig = at::empty({act && want_sig ? N : 0, M}, x0.options());
    Tensor out1 = at::empty({dual ? N : 0, M}, x0.options());
    ok(mdg_dense(fptr(W), trans, act, (int)N, (int)K, (int)M, fptr(x0), fptr(bias, "bias"), fptr(mul, "mul"), fptr(res, "res"),
                 mptr(out0), act && want_sig ? mptr(sig) : nullptr, fptr(x1, "x1"), fptr(res1, "res1"), dual ? mptr(out1) : nullptr,
                 stream_of(x0)));
    return {out0, sig, out1};
}

std::tuple<Tensor, Tensor> ssp_dual_bwd_t(const Tensor& sa, const Tensor& td, const Tensor& sdb, const Tensor& sb) {
    check_f32(sa, "sa"); check_f32(td, "td"); check_f32(sdb, "sdb"); check_f32(sb, "sb");
    Tensor xdb = at::empty_like(sa), xb = at::empty_like(sa);
    ok(mdg_ssp_dual_bwd_t(fptr(sa), fptr(td), fptr(sdb), fptr(sb), sa.numel(), mptr(xdb), mptr(xb), stream_of(sa)));
    return {xdb, xb};
}

Tensor atb(const Tensor& A, const Tensor& B) {
    check_f32(A, "A"); check_f32(B, "B");
    TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(0) == B.size(0), "mdgrad: atb takes [E,M] and [E,N]");
    const int64_t E = A.size(0), M = A.size(1), N = B.size(1);
    Tensor Cm = at::empty({M, N}, A.options());
    Tensor ws = at::empty({std::max<int64_t>(1, mdg_atb_workspace(E, (int)M, (int)N))}, A.options());
    ok(mdg_atb(fptr(A), fptr(B), E, (int)M, (int)N, mptr(Cm), mptr(ws), stream_of(A)));
    return Cm;
}

// ------------------------------------------------------------------------------------------------ K19
// cell_len = the three diagonal lengths; top int32 [n_terms, 4]; inc_ptr / inc = the incidence list of ops.DihedralTable
struct DihedralGeom { float L[3]; int n_atoms, n_terms; };
DihedralGeom dihedral_geom(const Tensor& pos, at::ArrayRef<double> cell_len, const Tensor& top) {
    check_f32(pos, "pos"); check_i32(top, "top"); same_device(pos, top, "top");
    TORCH_CHECK(cell_len.size() == 3, "mdgrad: cell_len = the three diagonal lengths of the cell");
    TORCH_CHECK(pos.dim() >= 2 && pos.size(-1) == 3 && pos.size(-2) > 0, "mdgrad: pos must be [..., N, 3]");
    TORCH_CHECK(top.dim() == 2 && top.size(1) == 4, "mdgrad: top must be [n_terms, 4]");
    DihedralGeom g;
    for (int k = 0; k < 3; ++k) g.L[k] = (float)cell_len[k];
    g.n_atoms = (int)pos.size(-2);
    g.n_terms = (int)top.size(0);
    return g;
}
void dihedral_inc_check(const Tensor& pos, const DihedralGeom& g, const Tensor& inc_ptr, const Tensor& inc) {
    check_i32(inc_ptr, "inc_ptr"); check_i32(inc, "inc"); same_device(pos, inc_ptr, "inc_ptr"); same_device(pos, inc, "inc");
    TORCH_CHECK(inc_ptr.numel() == g.n_atoms + 1 && inc.numel() == 4 * (int64_t)g.n_terms,
                "mdgrad: inc_ptr must be [n_atoms + 1] and inc [4 n_terms]");
}
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> dihedral_eval(const Tensor& pos, at::ArrayRef<double> cell_len, const Tensor& top,
                                                                 const Tensor& coeff, const OptTensor& type, const Tensor& inc_ptr,
                                                                 const Tensor& inc, const OptTensor& w, bool want_energy,
                                                                 bool want_terms) {
    const DihedralGeom g = dihedral_geom(pos, cell_len, top);
    TORCH_CHECK(pos.dim() == 2, "mdgrad: pos must be [N, 3]");
    check_f32(coeff, "coeff"); same_device(pos, coeff, "coeff");
    TORCH_CHECK(coeff.numel() >= 5 && coeff.numel() % 5 == 0, "mdgrad: coeff must be [n_types, 5]");
    dihedral_inc_check(pos, g, inc_ptr, inc);
    const int32_t* ty = nullptr;
    if (type.has_value() && type->defined()) {
        check_i32(*type, "type"); same_device(pos, *type, "type");
        TORCH_CHECK(type->numel() == g.n_terms, "mdgrad: type must hold one entry per term");
        ty = type->data_ptr<int32_t>();
    }
    const float* wp = fptr(w, "w");
    if (wp) { same_device(pos, *w, "w"); TORCH_CHECK(w->sizes() == pos.sizes(), "mdgrad: w must have the shape of pos"); }
    const auto o = pos.options();
    Tensor e = at::empty({want_energy ? g.n_atoms : 0}, o), grad = at::empty_like(pos);
    Tensor hw = wp ? at::empty_like(pos) : at::empty({0}, o);
    Tensor ct = at::empty({want_terms ? g.n_terms : 0}, o), cd = at::empty({(want_terms && wp) ? g.n_terms : 0}, o);
    ok(mdg_dihedral_eval(fptr(pos), g.n_atoms, g.L, top.data_ptr<int32_t>(), g.n_terms, fptr(coeff), ty, (int)(coeff.numel() / 5),
                         inc_ptr.data_ptr<int32_t>(), inc.data_ptr<int32_t>(), wp, want_energy ? mptr(e) : nullptr, mptr(grad),
                         wp ? mptr(hw) : nullptr, want_terms ? mptr(ct) : nullptr, (want_terms && wp) ? mptr(cd) : nullptr, 1.f, 0,
                         stream_of(pos)));
    return {e, grad, hw, ct, cd};
}
std::tuple<Tensor, Tensor> dihedral_phi_fwd(const Tensor& pos, at::ArrayRef<double> cell_len, const Tensor& top) {
    const DihedralGeom g = dihedral_geom(pos, cell_len, top);
    TORCH_CHECK(pos.dim() == 3 && pos.size(0) > 0, "mdgrad: pos must be [F, N, 3] with F > 0");
    Tensor phi = at::empty({pos.size(0), g.n_terms}, pos.options()), cs = at::empty_like(phi);
    ok(mdg_dihedral_phi_fwd(fptr(pos), (int)pos.size(0), g.n_atoms, g.L, top.data_ptr<int32_t>(), g.n_terms, mptr(phi), mptr(cs),
                            stream_of(pos)));
    return {phi, cs};
}
Tensor dihedral_phi_bwd(const Tensor& pos, at::ArrayRef<double> cell_len, const Tensor& top, const Tensor& inc_ptr, const Tensor& inc,
                        const OptTensor& g_phi, const OptTensor& g_cos) {
    const DihedralGeom g = dihedral_geom(pos, cell_len, top);
    TORCH_CHECK(pos.dim() == 3 && pos.size(0) > 0, "mdgrad: pos must be [F, N, 3] with F > 0");
    dihedral_inc_check(pos, g, inc_ptr, inc);
    const float* gp = fptr(g_phi, "g_phi");
    const float* gc = fptr(g_cos, "g_cos");
    TORCH_CHECK(gp || gc, "mdgrad: g_phi or g_cos must be given");
    const int64_t want = pos.size(0) * (int64_t)g.n_terms;
    if (gp) { same_device(pos, *g_phi, "g_phi"); TORCH_CHECK(g_phi->numel() == want, "mdgrad: g_phi must be [F, n_terms]"); }
    if (gc) { same_device(pos, *g_cos, "g_cos"); TORCH_CHECK(g_cos->numel() == want, "mdgrad: g_cos must be [F, n_terms]"); }
    Tensor gx = at::empty_like(pos);
    ok(mdg_dihedral_phi_bwd(fptr(pos), (int)pos.size(0), g.n_atoms, g.L, top.data_ptr<int32_t>(), g.n_terms,
                            inc_ptr.data_ptr<int32_t>(), inc.data_ptr<int32_t>(), gp, gc, mptr(gx), stream_of(pos)));
    return gx;
}
const float* dihedral_hist_check(const Tensor& phi, const OptTensor& cosphi) {
    check_f32(phi, "phi");
    const float* cp = fptr(cosphi, "cosphi");
    if (cp) { same_device(phi, *cosphi, "cosphi"); TORCH_CHECK(cosphi->numel() == phi.numel(), "mdgrad: cosphi must have the shape of phi"); }
    return cp;
}
Tensor dihedral_hist_fwd(const Tensor& phi, const OptTensor& cosphi, int64_t nbins, double width) {
    const float* cp = dihedral_hist_check(phi, cosphi);
    TORCH_CHECK(nbins >= 1 && nbins <= 4096, "mdgrad: nbins must be in [1, 4096]");
    Tensor raw = at::empty({nbins}, phi.options());
    Tensor scratch = at::empty({mdg_dihedral_hist_scratch(phi.numel(), (int)nbins)}, phi.options().dtype(at::kLong));
    ok(mdg_dihedral_hist_fwd(fptr(phi), cp, phi.numel(), (int)nbins, (float)width, mptr(raw), scratch.data_ptr<int64_t>(),
                             stream_of(phi)));
    return raw;
}
Tensor dihedral_hist_bwd(const Tensor& phi, const OptTensor& cosphi, int64_t nbins, double width, const Tensor& g_raw) {
    const float* cp = dihedral_hist_check(phi, cosphi);
    check_f32(g_raw, "g_raw"); same_device(phi, g_raw, "g_raw");
    TORCH_CHECK(nbins >= 1 && nbins <= 4096 && g_raw.numel() == nbins, "mdgrad: g_raw must have one entry per bin (1 .. 4096)");
    Tensor g = at::empty_like(phi);
    ok(mdg_dihedral_hist_bwd(fptr(phi), cp, phi.numel(), (int)nbins, (float)width, fptr(g_raw), mptr(g), stream_of(phi)));
    return g;
}

// ------------------------------------------------------------------------------------------------ K20
// consts = (alpha, rc, c0, c1, g0, alpha2, conversion, self_s) of MdgCoulombConsts; q float [N].
// (U [1] or [0], dU/dx [N,3], H w [N,3] or [0], pot [N] or [0], potw [N] or [0]); want_pot: pot without w, potw with it
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> coulomb_eval(const Tensor& pos, at::ArrayRef<double> cell, const Tensor& col,
                                                                const Tensor& shift, const Tensor& cnt, const Tensor& q,
                                                                at::ArrayRef<double> consts, const OptTensor& w, bool want_energy,
                                                                bool want_pot) {
    check_f32(pos, "pos"); check_f32(q, "q"); same_device(pos, q, "q");
    TORCH_CHECK(pos.dim() == 2 && pos.size(1) == 3 && pos.size(0) > 0, "mdgrad: pos must be [N,3]");
    TORCH_CHECK(q.numel() == pos.size(0), "mdgrad: q must hold one charge per atom");
    TORCH_CHECK(consts.size() == 8, "mdgrad: consts = (alpha, rc, c0, c1, g0, alpha2, conversion, self_s)");
    const MdgCell c = make_cell(cell);
    const EllRef e = ell_of(pos, col, shift, cnt);
    const MdgCoulombConsts k{consts[0], consts[1], consts[2], consts[3], consts[4], consts[5], consts[6], consts[7]};
    const float* wp = fptr(w, "w");
    if (wp) { same_device(pos, *w, "w"); TORCH_CHECK(w->sizes() == pos.sizes(), "mdgrad: w must have the shape of pos"); }
    const int n = (int)pos.size(0);
    const auto o = pos.options();
    Tensor U = at::empty({want_energy ? 1 : 0}, o), g = at::empty_like(pos);
    Tensor hw = wp ? at::empty_like(pos) : at::empty({0}, o);
    Tensor pot = at::empty({(want_pot && !wp) ? n : 0}, o), potw = at::empty({(want_pot && wp) ? n : 0}, o);
    Tensor partial = at::empty({mdg_coulomb_partial_size(n)}, o);
    ok(mdg_coulomb_eval(fptr(pos), n, &c, e.col, e.shift, e.cnt, e.max_nbr, fptr(q), &k, wp, want_energy ? mptr(U) : nullptr,
                        mptr(g), wp ? mptr(hw) : nullptr, (want_pot && !wp) ? mptr(pot) : nullptr, (want_pot && wp) ? mptr(potw) : nullptr,
                        mptr(partial), 1.f, 0, stream_of(pos)));
    return {U, g, hw, pot, potw};
}
// out [n_slots] = per-slot sums of val [N]; types int32 [group] or none (slot = atom of a replica, n_slots = group)
Tensor coulomb_charge_reduce(const Tensor& val, const OptTensor& types, int64_t group, int64_t n_slots) {
    check_f32(val, "val");
    TORCH_CHECK(val.dim() == 1 && val.numel() > 0 && val.numel() <= INT32_MAX, "mdgrad: val must be [N]");
    TORCH_CHECK(group > 0 && val.numel() % group == 0, "mdgrad: N must be a multiple of group");
    const int32_t* ty = nullptr;
    if (types.has_value() && types->defined()) {
        check_i32(*types, "types"); same_device(val, *types, "types");
        TORCH_CHECK(types->numel() == group, "mdgrad: types must hold one entry per atom of a replica");
        ty = types->data_ptr<int32_t>();
    }
    TORCH_CHECK(n_slots > 0 && n_slots <= INT32_MAX && (ty || n_slots == group), "mdgrad: n_slots must be positive, and equal "
                "group without types");
    Tensor out = at::empty({n_slots}, val.options());
    ok(mdg_coulomb_charge_reduce(fptr(val), ty, (int)val.numel(), (int)group, (int)n_slots, mptr(out), stream_of(val)));
    return out;
}

// ------------------------------------------------------------------------------------------------ K21
// pos [R n, 3] (R = n_rep replicas of n atoms), q float [R n], kvec int32 [M,3] (|n_d| <= 1024: checked here with one device
// read), coef float [M].  (energy [1] or [0], dU/dx [R n,3], H w [R n,3] or [0], pot [R n] or [0], potw [R n] or [0]) of
// mdg_ewald_eval: no conversion, background or self term; want_pot: pot without w, potw with it
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> ewald_eval(const Tensor& pos, int64_t n_rep, at::ArrayRef<double> cell,
                                                              const Tensor& q, const Tensor& kvec, const Tensor& coef,
                                                              const OptTensor& w, bool want_energy, bool want_pot) {
    check_f32(pos, "pos"); check_f32(q, "q"); check_f32(coef, "coef"); check_i32(kvec, "kvec");
    same_device(pos, q, "q"); same_device(pos, kvec, "kvec"); same_device(pos, coef, "coef");
    TORCH_CHECK(pos.dim() == 2 && pos.size(1) == 3 && pos.size(0) > 0, "mdgrad: pos must be [N,3]");
    TORCH_CHECK(n_rep > 0 && pos.size(0) % n_rep == 0 && pos.size(0) <= INT32_MAX, "mdgrad: pos must hold n_rep replicas");
    TORCH_CHECK(q.numel() == pos.size(0), "mdgrad: q must hold one charge per atom");
    TORCH_CHECK(kvec.dim() == 2 && kvec.size(1) == 3 && kvec.size(0) >= 1 && kvec.size(0) <= 65536, "mdgrad: kvec must be [M,3], "
                "1 <= M <= 65536");
    TORCH_CHECK(coef.numel() == kvec.size(0), "mdgrad: coef must hold one entry per wave vector");
    TORCH_CHECK(kvec.abs().max().item<int64_t>() <= 1024, "mdgrad: wave-vector indices must lie in [-1024, 1024]");
    const MdgCell c = make_cell(cell);
    const float* wp = fptr(w, "w");
    if (wp) { same_device(pos, *w, "w"); TORCH_CHECK(w->sizes() == pos.sizes(), "mdgrad: w must have the shape of pos"); }
    const int R = (int)n_rep, n = (int)(pos.size(0) / n_rep), M = (int)kvec.size(0);
    const int64_t N = pos.size(0);
    const auto o = pos.options();
    Tensor U = at::empty({want_energy ? 1 : 0}, o), g = at::empty_like(pos);
    Tensor hw = wp ? at::empty_like(pos) : at::empty({0}, o);
    Tensor pot = at::empty({(want_pot && !wp) ? N : 0}, o), potw = at::empty({(want_pot && wp) ? N : 0}, o);
    Tensor ws = at::empty({mdg_ewald_workspace(R, n, M)}, o);
    ok(mdg_ewald_eval(fptr(pos), R, n, &c, fptr(q), kvec.data_ptr<int32_t>(), fptr(coef), M, wp, want_energy ? mptr(U) : nullptr,
                      mptr(g), wp ? mptr(hw) : nullptr, (want_pot && !wp) ? mptr(pot) : nullptr,
                      (want_pot && wp) ? mptr(potw) : nullptr, mptr(ws), 1.f, 0, stream_of(pos)));
    return {U, g, hw, pot, potw};
}

// ------------------------------------------------------------------------------------------------ K23
// consts = (epsilon, sigma, lam, a, gamma, cos0, A, B, p, q) of MdgSWConsts; theta: device (epsilon, sigma, lam) read by the
// kernel instead of the first three.  (U [1] or [0], dU/dx [N,3], H w [N,3] or [0], pth [N,3] or [0], pthw [N,3] or [0]);
// want_theta: pth without w, pthw with it
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> sw_eval(const Tensor& pos, at::ArrayRef<double> cell, const Tensor& col,
                                                           const Tensor& shift, const Tensor& cnt, at::ArrayRef<double> consts,
                                                           const OptTensor& theta, const OptTensor& w, bool want_energy,
                                                           bool want_theta) {
    check_f32(pos, "pos");
    TORCH_CHECK(pos.dim() == 2 && pos.size(1) == 3 && pos.size(0) > 0 && pos.size(0) <= INT32_MAX, "mdgrad: pos must be [N,3]");
    TORCH_CHECK(consts.size() == 10, "mdgrad: consts = (epsilon, sigma, lam, a, gamma, cos0, A, B, p, q)");
    const MdgCell c = make_cell(cell);
    const EllRef e = ell_of(pos, col, shift, cnt);
    const MdgSWConsts k{consts[0], consts[1], consts[2], consts[3], consts[4], consts[5], consts[6], consts[7],
                        (int32_t)consts[8], (int32_t)consts[9]};
    TORCH_CHECK((double)k.p == consts[8] && (double)k.q == consts[9], "mdgrad: the exponents p, q must be integers");
    const float* tp = fptr(theta, "theta");
    if (tp) { same_device(pos, *theta, "theta"); TORCH_CHECK(theta->numel() == 3, "mdgrad: theta must be (epsilon, sigma, lam)"); }
    const float* wp = fptr(w, "w");
    if (wp) { same_device(pos, *w, "w"); TORCH_CHECK(w->sizes() == pos.sizes(), "mdgrad: w must have the shape of pos"); }
    const int n = (int)pos.size(0);
    const auto o = pos.options();
    Tensor U = at::empty({want_energy ? 1 : 0}, o), g = at::empty_like(pos);
    Tensor hw = wp ? at::empty_like(pos) : at::empty({0}, o);
    Tensor pth = (want_theta && !wp) ? at::empty_like(pos) : at::empty({0}, o);
    Tensor pthw = (want_theta && wp) ? at::empty_like(pos) : at::empty({0}, o);
    Tensor partial = at::empty({mdg_sw_partial_size(n)}, o);
    ok(mdg_sw_eval(fptr(pos), n, &c, e.col, e.shift, e.cnt, e.max_nbr, &k, tp, wp, want_energy ? mptr(U) : nullptr, mptr(g),
                   wp ? mptr(hw) : nullptr, (want_theta && !wp) ? mptr(pth) : nullptr, (want_theta && wp) ? mptr(pthw) : nullptr,
                   mptr(partial), 1.f, 0, stream_of(pos)));
    return {U, g, hw, pth, pthw};
}

// ------------------------------------------------------------------------------------------------ K24
// consts = (epsilon, a, c, rc, n, m, shift) of MdgEAMConsts; theta: device (epsilon, a, c) read by the kernels instead of the
// first three.  (U [1] or [0], dU/dx [N,3], H w [N,3] or [0], pth [N,3] or [0], pthw [N,3] or [0]); want_theta: pth without w,
// pthw with it.  The scratch of the density pass is allocated here.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> eam_eval(const Tensor& pos, at::ArrayRef<double> cell, const Tensor& col,
                                                            const Tensor& shift, const Tensor& cnt, at::ArrayRef<double> consts,
                                                            const OptTensor& theta, const OptTensor& w, bool want_energy,
                                                            bool want_theta) {
    check_f32(pos, "pos");
    TORCH_CHECK(pos.dim() == 2 && pos.size(1) == 3 && pos.size(0) > 0 && pos.size(0) <= INT32_MAX, "mdgrad: pos must be [N,3]");
    TORCH_CHECK(consts.size() == 7, "mdgrad: consts = (epsilon, a, c, rc, n, m, shift)");
    const MdgCell c = make_cell(cell);
    const EllRef e = ell_of(pos, col, shift, cnt);
    const MdgEAMConsts k{consts[0], consts[1], consts[2], consts[3], (int32_t)consts[4], (int32_t)consts[5], (int32_t)consts[6], 0};
    TORCH_CHECK((double)k.n == consts[4] && (double)k.m == consts[5] && (double)k.shift == consts[6],
                "mdgrad: the exponents n, m and the shift flag must be integers");
    const float* tp = fptr(theta, "theta");
    if (tp) { same_device(pos, *theta, "theta"); TORCH_CHECK(theta->numel() == 3, "mdgrad: theta must be (epsilon, a, c)"); }
    const float* wp = fptr(w, "w");
    if (wp) { same_device(pos, *w, "w"); TORCH_CHECK(w->sizes() == pos.sizes(), "mdgrad: w must have the shape of pos"); }
    const int n = (int)pos.size(0);
    const auto o = pos.options();
    Tensor U = at::empty({want_energy ? 1 : 0}, o), g = at::empty_like(pos);
    Tensor hw = wp ? at::empty_like(pos) : at::empty({0}, o);
    Tensor pth = (want_theta && !wp) ? at::empty_like(pos) : at::empty({0}, o);
    Tensor pthw = (want_theta && wp) ? at::empty_like(pos) : at::empty({0}, o);
    Tensor partial = at::empty({mdg_eam_partial_size(n)}, o), work = at::empty({(int64_t)n, 4}, o);
    ok(mdg_eam_eval(fptr(pos), n, &c, e.col, e.shift, e.cnt, e.max_nbr, &k, tp, wp, want_energy ? mptr(U) : nullptr, mptr(g),
                    wp ? mptr(hw) : nullptr, (want_theta && !wp) ? mptr(pth) : nullptr, (want_theta && wp) ? mptr(pthw) : nullptr,
                    mptr(partial), mptr(work), 1.f, 0, stream_of(pos)));
    return {U, g, hw, pth, pthw};
}

// ------------------------------------------------------------------------------------------------ K25
// consts = (A, B, lam1, lam2, beta, n, c, d, h, R, D, lam3, gamma, m) of MdgTersoffConsts; theta: device (A, B, h) read by the
// kernels instead of the host copies.  (U [1] or [0], dU/dx [N,3], H w [N,3] or [0], pth [N,3] or [0], pthw [N,3] or [0]);
// want_theta: pth without w, pthw with it.  The scratch of the bond pass is allocated here.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> tersoff_eval(const Tensor& pos, at::ArrayRef<double> cell, const Tensor& col,
                                                                const Tensor& shift, const Tensor& cnt,
                                                                at::ArrayRef<double> consts, const OptTensor& theta,
                                                                const OptTensor& w, bool want_energy, bool want_theta) {
    check_f32(pos, "pos");
    TORCH_CHECK(pos.dim() == 2 && pos.size(1) == 3 && pos.size(0) > 0 && pos.size(0) <= INT32_MAX, "mdgrad: pos must be [N,3]");
    TORCH_CHECK(consts.size() == 14, "mdgrad: consts = (A, B, lam1, lam2, beta, n, c, d, h, R, D, lam3, gamma, m)");
    const MdgCell c = make_cell(cell);
    const EllRef e = ell_of(pos, col, shift, cnt);
    const MdgTersoffConsts k{consts[0], consts[1], consts[2], consts[3], consts[4], consts[5], consts[6], consts[7], consts[8],
                             consts[9], consts[10], consts[11], consts[12], (int32_t)consts[13], 0};
    TORCH_CHECK((double)k.m == consts[13], "mdgrad: the exponent m must be an integer");
    const float* tp = fptr(theta, "theta");
    if (tp) { same_device(pos, *theta, "theta"); TORCH_CHECK(theta->numel() == 3, "mdgrad: theta must be (A, B, h)"); }
    const float* wp = fptr(w, "w");
    if (wp) { same_device(pos, *w, "w"); TORCH_CHECK(w->sizes() == pos.sizes(), "mdgrad: w must have the shape of pos"); }
    const int n = (int)pos.size(0);
    const auto o = pos.options();
    Tensor U = at::empty({want_energy ? 1 : 0}, o), g = at::empty_like(pos);
    Tensor hw = wp ? at::empty_like(pos) : at::empty({0}, o);
    Tensor pth = (want_theta && !wp) ? at::empty_like(pos) : at::empty({0}, o);
    Tensor pthw = (want_theta && wp) ? at::empty_like(pos) : at::empty({0}, o);
    Tensor partial = at::empty({mdg_tersoff_partial_size(n)}, o), work = at::empty({mdg_tersoff_work_size(n, e.max_nbr)}, o);
    ok(mdg_tersoff_eval(fptr(pos), n, &c, e.col, e.shift, e.cnt, e.max_nbr, &k, tp, wp, want_energy ? mptr(U) : nullptr, mptr(g),
                        wp ? mptr(hw) : nullptr, (want_theta && !wp) ? mptr(pth) : nullptr,
                        (want_theta && wp) ? mptr(pthw) : nullptr, mptr(partial), mptr(work), 1.f, 0, stream_of(pos)));
    return {U, g, hw, pth, pthw};
}

// ------------------------------------------------------------------------------------------------ K26
// types: int32 [N] with values in [0, n_species) (read back once to check them); tables: the derived constants of
// mdg_tersoff_multi_table_size(n_species) floats (mdgrad_amd/ops.py tersoff_multi_tables).  (U [1] or [0], dU/dx [N,3], H w
// [N,3] or [0], pth [N, 2 S S + S] or [0], pthw likewise or [0]); want_theta: pth without w, pthw with it.  The scratch of the
// bond pass is allocated here.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> tersoff_multi_eval(const Tensor& pos, at::ArrayRef<double> cell,
                                                                      const Tensor& col, const Tensor& shift, const Tensor& cnt,
                                                                      const Tensor& types, int64_t n_species, const Tensor& tables,
                                                                      const OptTensor& w, bool want_energy, bool want_theta) {
    check_f32(pos, "pos");
    TORCH_CHECK(pos.dim() == 2 && pos.size(1) == 3 && pos.size(0) > 0 && pos.size(0) <= INT32_MAX, "mdgrad: pos must be [N,3]");
    TORCH_CHECK(n_species >= 1 && n_species <= 4, "mdgrad: n_species must lie in [1, 4] (got ", n_species, ")");
    const MdgCell c = make_cell(cell);
    const EllRef e = ell_of(pos, col, shift, cnt);
    check_i32(types, "types"); same_device(pos, types, "types");
    TORCH_CHECK(types.dim() == 1 && types.size(0) == pos.size(0), "mdgrad: types must hold one entry per atom");
    TORCH_CHECK(types.min().item<int32_t>() >= 0 && types.max().item<int32_t>() < n_species,
                "mdgrad: types must lie in [0, n_species)");
    check_f32(tables, "tables"); same_device(pos, tables, "tables");
    TORCH_CHECK(tables.numel() == mdg_tersoff_multi_table_size((int)n_species),
                "mdgrad: tables must hold 8 S (S + 1) floats for S = n_species");
    const float* wp = fptr(w, "w");
    if (wp) { same_device(pos, *w, "w"); TORCH_CHECK(w->sizes() == pos.sizes(), "mdgrad: w must have the shape of pos"); }
    const int n = (int)pos.size(0);
    const int64_t P = 2 * n_species * n_species + n_species;
    const auto o = pos.options();
    Tensor U = at::empty({want_energy ? 1 : 0}, o), g = at::empty_like(pos);
    Tensor hw = wp ? at::empty_like(pos) : at::empty({0}, o);
    Tensor pth = (want_theta && !wp) ? at::empty({(int64_t)n, P}, o) : at::empty({0}, o);
    Tensor pthw = (want_theta && wp) ? at::empty({(int64_t)n, P}, o) : at::empty({0}, o);
    Tensor partial = at::empty({mdg_tersoff_multi_partial_size(n)}, o);
    Tensor work = at::empty({mdg_tersoff_multi_work_size(n, e.max_nbr)}, o);
    ok(mdg_tersoff_multi_eval(fptr(pos), n, &c, e.col, e.shift, e.cnt, e.max_nbr, types.data_ptr<int32_t>(), (int)n_species,
                              fptr(tables), wp, want_energy ? mptr(U) : nullptr, mptr(g), wp ? mptr(hw) : nullptr,
                              (want_theta && !wp) ? mptr(pth) : nullptr, (want_theta && wp) ? mptr(pthw) : nullptr,
                              mptr(partial), mptr(work), 1.f, 0, stream_of(pos)));
    return {U, g, hw, pth, pthw};
}

// ------------------------------------------------------------------------------------------------ K28
// types: int32 [N] with values in [0, n_species) (read back once to check them); tables: the derived constants of
// mdg_sw_multi_table_size(n_species) floats (mdgrad_amd/ops.py sw_multi_tables).  (U [1] or [0], dU/dx [N,3], H w [N,3] or
// [0], pth [N, 2 S S + S S S] or [0], pthw likewise or [0]); want_theta: pth without w, pthw with it.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> sw_multi_eval(const Tensor& pos, at::ArrayRef<double> cell, const Tensor& col,
                                                                 const Tensor& shift, const Tensor& cnt, const Tensor& types,
                                                                 int64_t n_species, const Tensor& tables, const OptTensor& w,
                                                                 bool want_energy, bool want_theta) {
    check_f32(pos, "pos");
    TORCH_CHECK(pos.dim() == 2 && pos.size(1) == 3 && pos.size(0) > 0 && pos.size(0) <= INT32_MAX, "mdgrad: pos must be [N,3]");
    TORCH_CHECK(n_species >= 1 && n_species <= 4, "mdgrad: n_species must lie in [1, 4] (got ", n_species, ")");
    const MdgCell c = make_cell(cell);
    const EllRef e = ell_of(pos, col, shift, cnt);
    check_i32(types, "types"); same_device(pos, types, "types");
    TORCH_CHECK(types.dim() == 1 && types.size(0) == pos.size(0), "mdgrad: types must hold one entry per atom");
    TORCH_CHECK(types.min().item<int32_t>() >= 0 && types.max().item<int32_t>() < n_species,
                "mdgrad: types must lie in [0, n_species)");
    check_f32(tables, "tables"); same_device(pos, tables, "tables");
    TORCH_CHECK(tables.numel() == mdg_sw_multi_table_size((int)n_species),
                "mdgrad: tables must hold 12 S S + 4 S S S floats for S = n_species");
    const float* wp = fptr(w, "w");
    if (wp) { same_device(pos, *w, "w"); TORCH_CHECK(w->sizes() == pos.sizes(), "mdgrad: w must have the shape of pos"); }
    const int n = (int)pos.size(0);
    const int64_t P = 2 * n_species * n_species + n_species * n_species * n_species;
    const auto o = pos.options();
    Tensor U = at::empty({want_energy ? 1 : 0}, o), g = at::empty_like(pos);
    Tensor hw = wp ? at::empty_like(pos) : at::empty({0}, o);
    Tensor pth = (want_theta && !wp) ? at::empty({(int64_t)n, P}, o) : at::empty({0}, o);
    Tensor pthw = (want_theta && wp) ? at::empty({(int64_t)n, P}, o) : at::empty({0}, o);
    Tensor partial = at::empty({mdg_sw_multi_partial_size(n)}, o);
    ok(mdg_sw_multi_eval(fptr(pos), n, &c, e.col, e.shift, e.cnt, e.max_nbr, types.data_ptr<int32_t>(), (int)n_species,
                         fptr(tables), wp, want_energy ? mptr(U) : nullptr, mptr(g), wp ? mptr(hw) : nullptr,
                         (want_theta && !wp) ? mptr(pth) : nullptr, (want_theta && wp) ? mptr(pthw) : nullptr, mptr(partial),
                         1.f, 0, stream_of(pos)));
    return {U, g, hw, pth, pthw};
}

// ------------------------------------------------------------------------------------------------ K27
// types: int32 [N] with values in [0, n_species) (read back once to check them); consts = (n_species, n_r, n_rho, r_min, rc,
// rho_min, rho_max, pin_cutoff) of the grids; tables: the flat node image (pair, density, embed) of mdg_eam_table_size floats.
// (U [1] or [0], dU/dx [N,3], H w [N,3] or [0], gtab [table size] or [0], gtabw likewise or [0]); want_theta: gtab without w,
// gtabw with it.  The scratch of the density pass and of the fixed-point scatter is allocated here.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> eam_table_eval(const Tensor& pos, at::ArrayRef<double> cell, const Tensor& col,
                                                                  const Tensor& shift, const Tensor& cnt, const Tensor& types,
                                                                  at::ArrayRef<double> consts, const Tensor& tables,
                                                                  const OptTensor& w, bool want_energy, bool want_theta) {
    check_f32(pos, "pos");
    TORCH_CHECK(pos.dim() == 2 && pos.size(1) == 3 && pos.size(0) > 0 && pos.size(0) <= INT32_MAX, "mdgrad: pos must be [N,3]");
    TORCH_CHECK(consts.size() == 8, "mdgrad: consts = (n_species, n_r, n_rho, r_min, rc, rho_min, rho_max, pin_cutoff)");
    const MdgCell c = make_cell(cell);
    const EllRef e = ell_of(pos, col, shift, cnt);
    MdgEAMTableConsts k{};
    k.n_species = (int32_t)consts[0]; k.n_r = (int32_t)consts[1]; k.n_rho = (int32_t)consts[2]; k.pin_cutoff = (int32_t)consts[7];
    TORCH_CHECK((double)k.n_species == consts[0] && (double)k.n_r == consts[1] && (double)k.n_rho == consts[2] &&
                (double)k.pin_cutoff == consts[7], "mdgrad: n_species, n_r, n_rho and pin_cutoff must be integers");
    TORCH_CHECK(k.n_species >= 1 && k.n_species <= 4, "mdgrad: n_species must lie in [1, 4] (got ", k.n_species, ")");
    TORCH_CHECK(k.n_r >= 4 && k.n_r <= 4096 && k.n_rho >= 4 && k.n_rho <= 4096, "mdgrad: n_r and n_rho must lie in [4, 4096]");
    k.r_min = consts[3]; k.rc = consts[4]; k.rho_min = consts[5];
    k.h_r = (k.rc - k.r_min) / (k.n_r - 1); k.h_rho = (consts[6] - k.rho_min) / (k.n_rho - 1);
    check_i32(types, "types"); same_device(pos, types, "types");
    TORCH_CHECK(types.dim() == 1 && types.size(0) == pos.size(0), "mdgrad: types must hold one entry per atom");
    TORCH_CHECK(types.min().item<int32_t>() >= 0 && types.max().item<int32_t>() < k.n_species,
                "mdgrad: types must lie in [0, n_species)");
    check_f32(tables, "tables"); same_device(pos, tables, "tables");
    const int64_t P = mdg_eam_table_size(k.n_species, k.n_r, k.n_rho);
    TORCH_CHECK(tables.numel() == P, "mdgrad: tables must hold ", P, " floats (pair, density, embed)");
    const float* wp = fptr(w, "w");
    if (wp) { same_device(pos, *w, "w"); TORCH_CHECK(w->sizes() == pos.sizes(), "mdgrad: w must have the shape of pos"); }
    const int n = (int)pos.size(0);
    const auto o = pos.options();
    Tensor U = at::empty({want_energy ? 1 : 0}, o), g = at::empty_like(pos);
    Tensor hw = wp ? at::empty_like(pos) : at::empty({0}, o);
    Tensor gtab = (want_theta && !wp) ? at::empty({P}, o) : at::empty({0}, o);
    Tensor gtabw = (want_theta && wp) ? at::empty({P}, o) : at::empty({0}, o);
    Tensor partial = at::empty({mdg_eam_table_partial_size(n)}, o), work = at::empty({(int64_t)n, 4}, o);
    Tensor fx = at::empty({want_theta ? mdg_eam_table_fx_size(k.n_species, k.n_r, k.n_rho) : 0}, o.dtype(at::kLong));
    ok(mdg_eam_table_eval(fptr(pos), n, &c, e.col, e.shift, e.cnt, e.max_nbr, types.data_ptr<int32_t>(), &k, fptr(tables), wp,
                          want_energy ? mptr(U) : nullptr, mptr(g), wp ? mptr(hw) : nullptr,
                          (want_theta && !wp) ? mptr(gtab) : nullptr, (want_theta && wp) ? mptr(gtabw) : nullptr, mptr(partial),
                          mptr(work), want_theta ? fx.data_ptr<int64_t>() : nullptr, 1.f, 0, stream_of(pos)));
    return {U, g, hw, gtab, gtabw};
}

// ------------------------------------------------------------------------------------------------ K22
// pos [R n, 3], q float [R n], cell_len = the three diagonal lengths; row_ptr int32 [n + 1], col int32 [nnz], scale float [nnz]:
// the CSR incidence list of ops.EwaldExclTable (checked here with device reads: the kernel indexes pos with col).
// (energy [1] or [0], dU/dx [R n,3], H w [R n,3] or [0], pot [R n] or [0], potw [R n] or [0]) of mdg_ewald_excl_eval
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> ewald_excl_eval(const Tensor& pos, int64_t n_rep, at::ArrayRef<double> cell_len,
                                                                   const Tensor& row_ptr, const Tensor& col, const Tensor& scale,
                                                                   const Tensor& q, double alpha, double conversion,
                                                                   const OptTensor& w, bool want_energy, bool want_pot) {
    check_f32(pos, "pos"); check_f32(q, "q"); check_f32(scale, "scale"); check_i32(row_ptr, "row_ptr"); check_i32(col, "col");
    same_device(pos, q, "q"); same_device(pos, scale, "scale"); same_device(pos, row_ptr, "row_ptr"); same_device(pos, col, "col");
    TORCH_CHECK(pos.dim() == 2 && pos.size(1) == 3 && pos.size(0) > 0, "mdgrad: pos must be [N,3]");
    TORCH_CHECK(n_rep > 0 && pos.size(0) % n_rep == 0 && pos.size(0) < (1LL << 29), "mdgrad: pos must hold n_rep replicas");
    TORCH_CHECK(q.numel() == pos.size(0), "mdgrad: q must hold one charge per atom");
    TORCH_CHECK(cell_len.size() == 3 && cell_len[0] > 0 && cell_len[1] > 0 && cell_len[2] > 0,
                "mdgrad: cell_len = the three (positive) diagonal lengths of the cell");
    TORCH_CHECK(alpha > 0.0, "mdgrad: alpha must be positive");
    const int64_t N = pos.size(0), n = N / n_rep, nnz = col.numel();
    TORCH_CHECK(row_ptr.dim() == 1 && row_ptr.numel() == n + 1, "mdgrad: row_ptr must be [n_atoms + 1]");
    TORCH_CHECK(col.dim() == 1 && scale.dim() == 1 && scale.numel() == nnz, "mdgrad: col and scale must be [nnz]");
    const Tensor rp = row_ptr.cpu();
    const int32_t* r = rp.data_ptr<int32_t>();
    TORCH_CHECK(r[0] == 0 && r[n] == nnz, "mdgrad: row_ptr must run from 0 to nnz");
    for (int64_t a = 0; a < n; ++a) TORCH_CHECK(r[a] <= r[a + 1], "mdgrad: row_ptr must not decrease");
    if (nnz > 0) TORCH_CHECK(col.min().item<int64_t>() >= 0 && col.max().item<int64_t>() < n, "mdgrad: col must lie in [0, n_atoms)");
    const float* wp = fptr(w, "w");
    if (wp) { same_device(pos, *w, "w"); TORCH_CHECK(w->sizes() == pos.sizes(), "mdgrad: w must have the shape of pos"); }
    float L[3] = {(float)cell_len[0], (float)cell_len[1], (float)cell_len[2]};
    const auto o = pos.options();
    Tensor U = at::empty({want_energy ? 1 : 0}, o), g = at::empty_like(pos);
    Tensor hw = wp ? at::empty_like(pos) : at::empty({0}, o);
    Tensor pot = at::empty({(want_pot && !wp) ? N : 0}, o), potw = at::empty({(want_pot && wp) ? N : 0}, o);
    Tensor partial = at::empty({mdg_ewald_excl_partial_size((int)n_rep, (int)n)}, o.dtype(at::kDouble));
    ok(mdg_ewald_excl_eval(fptr(pos), (int)n_rep, (int)n, L, row_ptr.data_ptr<int32_t>(), col.data_ptr<int32_t>(), fptr(scale), fptr(q),
                           alpha, conversion, wp, want_energy ? mptr(U) : nullptr, mptr(g), wp ? mptr(hw) : nullptr,
                           (want_pot && !wp) ? mptr(pot) : nullptr, (want_pot && wp) ? mptr(potw) : nullptr,
                           partial.data_ptr<double>(), 1.f, 0, stream_of(pos)));
    return {U, g, hw, pot, potw};
}

}  // namespace

TORCH_LIBRARY(mdgrad, m) {
    m.def("nbr_build(Tensor pos, float[] cell, float cutoff, Tensor? mask, int max_nbr, int group, bool cell_list) -> "
          "(Tensor, Tensor, Tensor, Tensor)");
    m.def("pair_force(Tensor pos, float[] cell, Tensor col, Tensor shift, Tensor cnt, int[] term_i, float[] term_f, Tensor? mask, "
          "Tensor? theta) -> (Tensor, Tensor, Tensor)");
    m.def("pair_hvp(Tensor pos, float[] cell, Tensor col, Tensor shift, Tensor cnt, int[] term_i, float[] term_f, Tensor? mask, "
          "Tensor? theta, Tensor w) -> (Tensor, Tensor)");
    m.def("nhc_vv_forward(Tensor v0, Tensor q0, Tensor? pv0, Tensor mass, Tensor t, Tensor? theta, int[] iprm, float[] fprm, "
          "float[] cell, int[] terms_i, float[] terms_f, int n_theta_total) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("nhc_vv_adjoint(Tensor v_t, Tensor q_t, Tensor? pv_t, Tensor? g_v, Tensor? g_q, Tensor? g_pv, Tensor mass, Tensor t, "
          "Tensor? theta, int[] iprm, float[] fprm, float[] cell, int[] terms_i, float[] terms_f, int n_theta_total) -> "
          "(Tensor, Tensor, Tensor, Tensor)");
    m.def("rdf_fwd(Tensor xyz, float[] cell, float cutoff, Tensor? mask, Tensor mu, float spacing, float coeff) -> Tensor");
    m.def("rdf_bwd(Tensor xyz, float[] cell, float cutoff, Tensor? mask, Tensor mu, float spacing, float coeff, Tensor g_raw) -> Tensor");
    m.def("adf_fwd(Tensor pos, int n_frames, int n_atoms, float[] cell, float cutoff, Tensor col, Tensor cnt, Tensor mu, "
          "float spacing, float coeff) -> Tensor");
    m.def("adf_bwd(Tensor pos, int n_frames, int n_atoms, float[] cell, float cutoff, Tensor col, Tensor cnt, Tensor mu, "
          "float spacing, float coeff, Tensor g_raw) -> Tensor");
    m.def("bond_order_fwd(Tensor pos, int n_frames, int n_atoms, float[] cell, float cutoff, float r_in, Tensor col, Tensor cnt, "
          "int[] ls) -> (Tensor, Tensor)");
    m.def("bond_order_bwd(Tensor pos, int n_frames, int n_atoms, float[] cell, float cutoff, float r_in, Tensor col, Tensor cnt, "
          "int[] ls, Tensor gA, Tensor gn) -> Tensor");
    m.def("virial_fwd(Tensor pos, float[] cell, int[] terms_i, float[] terms_f, Tensor?[] masks, Tensor? theta) -> Tensor");
    m.def("virial_bwd(Tensor pos, float[] cell, int[] terms_i, float[] terms_f, Tensor?[] masks, Tensor? theta, Tensor gW) -> "
          "(Tensor, Tensor)");
    m.def("energy_frames_fwd(Tensor pos, float[] cell, int[] terms_i, float[] terms_f, Tensor?[] masks, Tensor? theta) -> Tensor");
    m.def("energy_frames_bwd(Tensor pos, float[] cell, int[] terms_i, float[] terms_f, Tensor?[] masks, Tensor? theta, Tensor gU, "
          "bool want_pos) -> (Tensor, Tensor)");
    m.def("rdf_frames_fwd(Tensor xyz, float[] cell, float cutoff, Tensor? mask, Tensor mu, float spacing, float coeff) -> Tensor");
    m.def("rdf_frames_bwd(Tensor xyz, float[] cell, float cutoff, Tensor? mask, Tensor mu, float spacing, float coeff, "
          "Tensor g_raw) -> Tensor");
    m.def("sk_fwd(Tensor pos, float[] cell, Tensor? weights, float norm, Tensor kvec, Tensor seg, int[] seg_host) -> Tensor");
    m.def("sk_bwd(Tensor pos, float[] cell, Tensor? weights, float norm, Tensor kvec, Tensor seg, int[] seg_host, Tensor gS) -> "
          "Tensor");
    m.def("msd_fwd(Tensor x, int group, Tensor? weights, int n_lags, int origin_stride, bool fourth) -> (Tensor, Tensor)");
    m.def("msd_bwd(Tensor x, int group, Tensor? weights, int n_lags, int origin_stride, Tensor g2, Tensor? g4) -> Tensor");
    m.def("isf_fwd(Tensor x, int kind, int group, int rep0, int n_reps, float[] cell, Tensor? weights, float norm, Tensor kvec, "
          "Tensor seg, int[] seg_host, int n_lags, int origin_stride) -> Tensor");
    m.def("isf_bwd(Tensor x, int kind, int group, int rep0, int n_reps, float[] cell, Tensor? weights, float norm, Tensor kvec, "
          "Tensor seg, int[] seg_host, int n_lags, int origin_stride, Tensor gF, Tensor(a!) gx) -> ()");
    m.def("dihedral_eval(Tensor pos, float[] cell_len, Tensor top, Tensor coeff, Tensor? type, Tensor inc_ptr, Tensor inc, Tensor? w, "
          "bool want_energy, bool want_terms) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("dihedral_phi_fwd(Tensor pos, float[] cell_len, Tensor top) -> (Tensor, Tensor)");
    m.def("dihedral_phi_bwd(Tensor pos, float[] cell_len, Tensor top, Tensor inc_ptr, Tensor inc, Tensor? g_phi, Tensor? g_cos) -> "
          "Tensor");
    m.def("dihedral_hist_fwd(Tensor phi, Tensor? cosphi, int nbins, float width) -> Tensor");
    m.def("dihedral_hist_bwd(Tensor phi, Tensor? cosphi, int nbins, float width, Tensor g_raw) -> Tensor");
    m.def("coulomb_eval(Tensor pos, float[] cell, Tensor col, Tensor shift, Tensor cnt, Tensor q, float[] consts, Tensor? w, "
          "bool want_energy, bool want_pot) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("coulomb_charge_reduce(Tensor val, Tensor? types, int group, int n_slots) -> Tensor");
    m.def("sw_eval(Tensor pos, float[] cell, Tensor col, Tensor shift, Tensor cnt, float[] consts, Tensor? theta, Tensor? w, "
          "bool want_energy, bool want_theta) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("eam_eval(Tensor pos, float[] cell, Tensor col, Tensor shift, Tensor cnt, float[] consts, Tensor? theta, Tensor? w, "
          "bool want_energy, bool want_theta) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("tersoff_eval(Tensor pos, float[] cell, Tensor col, Tensor shift, Tensor cnt, float[] consts, Tensor? theta, Tensor? w, "
          "bool want_energy, bool want_theta) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("tersoff_multi_eval(Tensor pos, float[] cell, Tensor col, Tensor shift, Tensor cnt, Tensor types, int n_species, "
          "Tensor tables, Tensor? w, bool want_energy, bool want_theta) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("sw_multi_eval(Tensor pos, float[] cell, Tensor col, Tensor shift, Tensor cnt, Tensor types, int n_species, "
          "Tensor tables, Tensor? w, bool want_energy, bool want_theta) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("eam_table_eval(Tensor pos, float[] cell, Tensor col, Tensor shift, Tensor cnt, Tensor types, float[] consts, "
          "Tensor tables, Tensor? w, bool want_energy, bool want_theta) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("ewald_eval(Tensor pos, int n_rep, float[] cell, Tensor q, Tensor kvec, Tensor coef, Tensor? w, bool want_energy, "
          "bool want_pot) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("ewald_excl_eval(Tensor pos, int n_rep, float[] cell_len, Tensor row_ptr, Tensor col, Tensor scale, Tensor q, float alpha, "
          "float conversion, Tensor? w, bool want_energy, bool want_pot) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("edge_geom(Tensor x, Tensor? w, Tensor nbr, Tensor offsets) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("edge_geom_bwd(Tensor? d_b, Tensor dd_b, Tensor? d, Tensor? dd, Tensor uhat, Tensor? ddel, Tensor col, Tensor eid, "
          "Tensor cnt) -> (Tensor, Tensor)");
    m.def("cfconv_fwd(Tensor mu, Tensor coef, Tensor W1, Tensor b1, Tensor W2, Tensor b2, bool bf16, Tensor d, Tensor? dd, Tensor h, "
          "Tensor? hd, Tensor col, Tensor eid, Tensor cnt, bool want_sums) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("cfconv_bwd(Tensor mu, Tensor coef, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor d, Tensor? dd, Tensor nbr, "
          "int n_edges, Tensor h, Tensor? hd, Tensor? mb, Tensor mdb, Tensor(a!)? d_b, Tensor(b!) dd_b, Tensor? n_valid, "
          "bool want_theta, bool bf16=False) -> (Tensor, Tensor, Tensor)");
    m.def("dense_ssp(Tensor W, bool trans, bool act, Tensor x0, Tensor? bias, Tensor? mul, Tensor? res, Tensor? x1, Tensor? res1, "
          "bool want_sig) -> (Tensor, Tensor, Tensor)");
    m.def("ssp_dual_bwd_t(Tensor sa, Tensor td, Tensor sdb, Tensor sb) -> (Tensor, Tensor)");
    m.def("atb(Tensor A, Tensor B) -> Tensor");
}

TORCH_LIBRARY_IMPL(mdgrad, CUDA, m) {      // (the HIP backend registers under the CUDA dispatch key in PyTorch-ROCm)
    m.impl("nbr_build", nbr_build);
    m.impl("pair_force", pair_force);
    m.impl("pair_hvp", pair_hvp);
    m.impl("nhc_vv_forward", nhc_vv_forward);
    m.impl("nhc_vv_adjoint", nhc_vv_adjoint);
    m.impl("rdf_fwd", rdf_fwd);
    m.impl("rdf_bwd", rdf_bwd);
    m.impl("adf_fwd", adf_fwd);
    m.impl("adf_bwd", adf_bwd);
    m.impl("bond_order_fwd", bond_order_fwd);
    m.impl("bond_order_bwd", bond_order_bwd);
    m.impl("virial_fwd", virial_fwd);
    m.impl("virial_bwd", virial_bwd);
    m.impl("energy_frames_fwd", energy_frames_fwd);
    m.impl("energy_frames_bwd", energy_frames_bwd);
    m.impl("rdf_frames_fwd", rdf_frames_fwd);
    m.impl("rdf_frames_bwd", rdf_frames_bwd);
    m.impl("sk_fwd", sk_fwd);
    m.impl("sk_bwd", sk_bwd);
    m.impl("msd_fwd", msd_fwd);
    m.impl("msd_bwd", msd_bwd);
    m.impl("isf_fwd", isf_fwd);
    m.impl("isf_bwd", isf_bwd);
    m.impl("dihedral_eval", dihedral_eval);
    m.impl("dihedral_phi_fwd", dihedral_phi_fwd);
    m.impl("dihedral_phi_bwd", dihedral_phi_bwd);
    m.impl("dihedral_hist_fwd", dihedral_hist_fwd);
    m.impl("dihedral_hist_bwd", dihedral_hist_bwd);
    m.impl("coulomb_eval", coulomb_eval);
    m.impl("coulomb_charge_reduce", coulomb_charge_reduce);
    m.impl("sw_eval", sw_eval);
    m.impl("eam_eval", eam_eval);
    m.impl("tersoff_eval", tersoff_eval);
    m.impl("tersoff_multi_eval", tersoff_multi_eval);
    m.impl("sw_multi_eval", sw_multi_eval);
    m.impl("eam_table_eval", eam_table_eval);
    m.impl("ewald_eval", ewald_eval);
    m.impl("ewald_excl_eval", ewald_excl_eval);
    m.impl("edge_geom", edge_geom);
    m.impl("edge_geom_bwd", edge_geom_bwd);
    m.impl("cfconv_fwd", cfconv_fwd);
    m.impl("cfconv_bwd", cfconv_bwd);
    m.impl("dense_ssp", dense_ssp);
    m.impl("ssp_dual_bwd_t", ssp_dual_bwd_t);
    m.impl("atb", atb);
}
