"""K21: the reciprocal-space part of the Ewald sum (EwaldReciprocal, ewald, mdg_ewald_eval, csrc/ewald.hip) against the
float64 definitions of tests/ewald_ref.py (checked against autograd and the Madelung constant by tests/test_ewald_host.py)
and, in a Stack with a pair term and the real-space sum, the CPU oracle's trajectory and adjoint.

Tolerance of every kernel-vs-float64 comparison: C * 2^-24 * A per component, A = the float64 sum of the absolute mode
contributions to that component with |rho|, |sigma| replaced by the absolute sums sum_j |q_j|, sum_j |q_j| |k.w_j|
(ewald_ref.evaluate): a float32 mode sum over N atoms errs in proportion to the absolute sum.  `within` prints the largest
observed err / (2^-24 A); C = 3.3 is four times the largest figure observed on an MI355X over all cases of this file
(OBSERVED below: 0.82, potw of the one-vector table), and C * 2^-24 = 2.0e-7 stays below 1e-5.  The figures are small because A
is a worst-case scale: the phases carry ~3e-8 turns and sine / cosine 1 ulp, and the signed terms of a mode sum cancel where
A adds their magnitudes."""
import copy
import math

import numpy as np
import pytest
import torch

import coulomb_ref as R
import ewald_ref as E
import oracle as O
from test_gpu_parity import T, close, mk_system, DEV, oracle_run

pytestmark = pytest.mark.gpu
F32 = np.float32
ULP = 2.0 ** -24
# largest err / (2^-24 A) per output over all cases of this file on an MI355X
OBSERVED = dict(U=0.03, grad=0.43, pot=0.53, hw=0.75, potw=0.82, dcharges=0.26)
C_TOL = 3.3                              # 4 * max(OBSERVED.values()), rounded up
TOL = C_TOL * ULP
TOL_REAL = 64 * ULP                      # the real-space kernel's (tests/test_gpu_coulomb.py)
assert TOL <= 1e-5


def within(got, want, A, what, extra=0.0):
    """|got - want| <= TOL * A (+ extra) per component; returns (and prints) the largest err / (2^-24 A)."""
    got = got.detach().cpu().double().reshape(-1)
    want, A = torch.as_tensor(want).detach().double().reshape(-1), torch.as_tensor(A).detach().double().reshape(-1)
    assert got.shape == want.shape == A.shape, "%s: shapes %s %s %s" % (what, got.shape, want.shape, A.shape)
    assert bool(torch.isfinite(got).all()), what + ": non-finite"
    err = (got - want).abs()
    ratio = float((err[A > 0] / (ULP * A[A > 0])).max()) if bool((A > 0).any()) else 0.0
    print("%-64s max err / (2^-24 A) = %6.2f  (allowed %g)" % (what, ratio, C_TOL))
    bad = err > TOL * A + extra
    assert not bool(bad.any()), "%s: err %.3e at A = %.3e, ratio %.1f > %g" % (what, float(err[bad].max()), float(A[bad].min()), ratio, C_TOL)
    return ratio


def _terms(x32, cell32, charges, rc, alpha, kc, n_rep=1, **kw):
    from mdgrad_amd.interface import CoulombPotentials, EwaldReciprocal
    system = mk_system(x32, cell32)
    if n_rep > 1:
        system = system.replicate(n_rep)
    real = CoulombPotentials(system, charges, rc, alpha=alpha, shift="none", **kw)
    return system, real, EwaldReciprocal(system, real, k_cutoff=kc)


def _cut(table, m):
    """The table with its first m vectors."""
    t = copy.copy(table)
    t.n_host, t.k2_host, t.coef_host = table.n_host[:m], table.k2_host[:m], table.coef_host[:m]
    t.kvec, t.coef, t.n_vecs = table.kvec[:m].contiguous(), table.coef[:m].contiguous(), m
    return t


def _check_all_outputs(table, x32, cell32, q32, tag, seed=0, x_ref=None):
    """energy, dU/dx, H w, pot and potw of the low-level op against the explicit float64 mode sums; every launch twice,
    bitwise equal.  x_ref: the positions the float64 sums are taken at (default: x32)."""
    from mdgrad_amd import ops
    lengths = cell32.astype(np.float64)
    w32 = np.random.default_rng(seed + 17).normal(0, 1, x32.shape).astype(F32)
    cv = table.conversion
    ref = E.evaluate(x32 if x_ref is None else x_ref, q32, table.n_host.numpy(), lengths, table.alpha, cv, w=w32, group=table.n_atoms)
    x, w, q = T(x32, DEV), T(w32, DEV), T(q32, DEV)
    o1 = ops.ewald_eval(table, x, q, energy=True, grad=True, want_pot=True)
    o2 = ops.ewald_eval(table, x, q, w=w, energy=False, grad=True, want_pot=True)
    Q = torch.tensor(q32).double().reshape(table.n_rep, table.n_atoms).sum(1)
    U = o1["energy"].cpu().double() - 0.5 * table.background * Q.pow(2).sum()
    rs = dict(U=within(U, ref["U"].reshape(1), ref["A_U"].reshape(1), tag + " U"),
              grad=within(o1["grad"], ref["grad"], ref["A_grad"], tag + " dU/dx"),
              pot=within(o1["pot"], cv * ref["pot"], cv * ref["A_pot"], tag + " pot"),
              hw=within(o2["hw"], ref["hw"], ref["A_hw"], tag + " H.w"),
              potw=within(o2["potw"], cv * ref["potw"], cv * ref["A_potw"], tag + " potw"))
    assert torch.equal(o1["grad"], o2["grad"]) and o2["pot"] is None and o1["potw"] is None
    e0 = ops.ewald_eval(table, x, q, energy=True, grad=False)
    assert torch.equal(e0["energy"], o1["energy"]) and e0["grad"] is None, "energy-only evaluation"
    p1 = ops.ewald_eval(table, x, q, energy=True, grad=True, want_pot=True)
    p2 = ops.ewald_eval(table, x, q, w=w, energy=False, grad=True, want_pot=True)
    for a, b in ((o1, p1), (o2, p2)):
        for key in a:
            assert (a[key] is None and b[key] is None) or torch.equal(a[key], b[key]), "two launches differ in " + key
    return ref, o1, o2, rs


# ------------------------------------------------------------------------------------------------ 1: all outputs vs float64
def test_outputs_vs_float64_jittered_nacl64():
    """64 jittered NaCl ions, alpha 0.6, k_cutoff 4.5: 1102 vectors -- a ragged last chunk of the atom phase (1102 = 1024 + 78:
    its second slice is partial, the other fourteen idle); N = 64 fills exactly one workgroup of the atom phase."""
    x32, cell32, q32 = E.jittered_nacl64()
    _, _, rec = _terms(x32, cell32, q32, 5.0, 0.6, 4.5)
    assert rec.n_vectors == 1102
    ref, o1, _, _ = _check_all_outputs(rec.table(), x32, cell32, q32, "nacl64")
    U = rec(T(x32, DEV))
    within(U.reshape(1), ref["U"].reshape(1), ref["A_U"].reshape(1), "nacl64 U through the class")


def test_outputs_vs_float64_charged_gas37_with_a_zero_charge():
    """37 seeded atoms in 7 x 8 x 9, net charge -1.17, one zero charge; 37 is no multiple of the wave.  The zero charge feels
    no force (exactly) but has a potential; the background term enters U through the class."""
    x32, box, q32 = E.gas37()
    _, _, rec = _terms(x32, box, q32, 3.4, 1.0, 7.5)
    ref, o1, o2, _ = _check_all_outputs(rec.table(), x32, box, q32, "gas37")
    assert float(o1["grad"][5].abs().max()) == 0.0 and float(o2["hw"][5].abs().max()) == 0.0 and float(o1["pot"][5].abs()) > 0.0
    bg = 0.5 * rec.table().background * float(q32.astype(np.float64).sum()) ** 2
    within(rec(T(x32, DEV)).reshape(1), ref["U"].reshape(1), ref["A_U"].reshape(1), "gas37 U through the class (with background)")
    assert bg > 4 * TOL * float(ref["A_U"]), "the background term is well above the tolerance here: leaving it out would fail"


@pytest.mark.parametrize("m", [1, 1024], ids=["one_vector", "one_full_chunk"])
def test_outputs_vs_float64_gas37_with_the_table_cut(m):
    """The low-level op with the table cut to one vector, and to 1024 vectors: exactly one chunk of the atom phase
    (no ragged chunk at all)."""
    x32, box, q32 = E.gas37()
    _, _, rec = _terms(x32, box, q32, 3.4, 1.0, 7.5)
    assert rec.n_vectors > 1024
    _check_all_outputs(_cut(rec.table(), m), x32, box, q32, "gas37 M=%d" % m)


def test_outputs_vs_float64_513_atoms():
    """513 seeded atoms in a 20^3 box: one above the 512-atom LDS block of the mode phase, and one above eight 64-atom
    workgroups of the atom phase; k_cutoff 1.14 for ~100 vectors."""
    box = np.array([20.0, 20.0, 20.0], dtype=F32)
    x32 = R.seeded_gas(513, box, 1.0, seed=513).astype(F32)
    q32 = np.random.default_rng(5130).normal(0, 1, 513).astype(F32)
    _, _, rec = _terms(x32, box, q32, 6.0, 0.4, 1.14)
    assert 80 <= rec.n_vectors <= 130
    _check_all_outputs(rec.table(), x32, box, q32, "gas513")


def test_positions_displaced_by_whole_boxes_vs_the_wrapped_result():
    """Every atom of NaCl-64 moved by up to +-50 box lengths per axis (float32 positions up to ~570): against the float64 sums
    at the same positions wrapped back (exactly, in float64), with the unchanged tolerance."""
    x32, cell32, q32 = E.jittered_nacl64(seed=65)
    _, _, rec = _terms(x32, cell32, q32, 5.0, 0.6, 4.5)
    k = np.random.default_rng(650).integers(-50, 51, x32.shape)
    xd32 = (x32.astype(np.float64) + k * cell32.astype(np.float64)).astype(F32)
    wrapped = xd32.astype(np.float64) - k * cell32.astype(np.float64)
    assert float(np.abs(xd32).max()) > 400 and float(np.abs(wrapped - x32).max()) < 1e-4
    _check_all_outputs(rec.table(), xd32, cell32, q32, "nacl64 +-50 boxes", x_ref=wrapped)


# ------------------------------------------------------------------------------------------------ 2: replicas, charge gradients
def _replicas24():
    box = np.array([8.0, 8.0, 8.0], dtype=F32)
    base = R.seeded_gas(24, box, 1.3, seed=24)
    rng = np.random.default_rng(240)
    x32 = np.concatenate([np.mod(base + rng.normal(0, 0.1, base.shape), box) for _ in range(3)]).astype(F32)
    return base, box, x32, (np.arange(24) % 2).astype(np.int64)


@pytest.mark.parametrize("per_type", [False, True], ids=["per_atom", "per_type"])
def test_three_replicas_and_charge_gradients_vs_float64_autograd(per_type):
    """System.replicate(3) of a 24-ion cell with different jitters, alpha 0.8, k_cutoff 5.0: every replica against its own
    float64 reference (no replica sees another's modes); dU/dcharges and d(w.dU/dx)/dcharges per atom (24 slots, each summed
    over the replicas) and per type (2 slots) against float64 autograd of ewald_ref.energy, allowed C 2^-24 times the slot's
    sum of A_dq, resp. conversion A_potw; force_vjp's charge part with and without `accum`."""
    from mdgrad_amd import ops
    base, box, x32, types = _replicas24()
    alpha, kc = 0.8, 5.0
    rng = np.random.default_rng(241)
    c32 = (np.array([0.9, -1.1]) if per_type else np.where(types == 0, 1.0, -1.0) * rng.uniform(0.5, 1.5, 24)).astype(F32)
    ty = types if per_type else None
    system, real, rec = _terms(base, box, c32, 3.5, alpha, kc, n_rep=3, types=ty, trainable=True)
    assert rec.charges is real.charges and rec.n_slots == (2 if per_type else 24) and rec._q_atom().shape == (72,)
    cv, lengths, n = rec.conversion, box.astype(np.float64), rec.table().n_host.numpy()
    w32 = rng.normal(0, 1, x32.shape).astype(F32)
    qa32 = R.expand(torch.tensor(c32), ty, 3).numpy()
    ref = E.evaluate(x32, qa32, n, lengths, alpha, cv, w=w32, group=24)
    for r in range(3):                                          # the float64 reference itself is per replica
        sl = slice(24 * r, 24 * r + 24)
        one = E.evaluate(x32[sl], qa32[sl], n, lengths, alpha, cv, w=w32[sl])
        assert float((one["grad"] - ref["grad"][sl]).abs().max()) <= 1e-12 * float(ref["A_grad"].max())
    c64 = torch.tensor(c32).double().requires_grad_(True)
    x64 = torch.tensor(x32).double().requires_grad_(True)
    U = E.energy(x64, R.expand(c64, ty, 3), n, lengths, alpha, cv, group=24)
    gx, gc = torch.autograd.grad(U, (x64, c64), create_graph=True)
    (hc,) = torch.autograd.grad((gx * torch.tensor(w32).double()).sum(), c64)
    slot = torch.as_tensor(types if per_type else np.arange(24)).repeat(3)

    def per_slot(v):
        return torch.zeros(rec.n_slots, dtype=torch.float64).index_add_(0, slot, v)
    A_u, A_w = per_slot(ref["A_dq"]), cv * per_slot(ref["A_potw"])
    x, w = T(x32, DEV).requires_grad_(True), T(w32, DEV)
    Ud = rec(x)
    within(Ud.reshape(1), ref["U"].reshape(1), ref["A_U"].reshape(1), "U on three replicas")
    g1x, g1c = torch.autograd.grad(Ud, (x, rec.charges), create_graph=True)
    (h1c,) = torch.autograd.grad((g1x * w).sum(), rec.charges)
    within(g1x, ref["grad"], ref["A_grad"], "dU/dx on three replicas, each against its own modes")
    within(g1c, gc.detach(), A_u, "dU/dcharges")
    within(h1c, hc, A_w, "d(w.dU/dx)/dcharges")
    F, dq, gth = rec.force_vjp(x.detach(), w)
    within(-dq, ref["hw"], ref["A_hw"], "H.w on three replicas")
    within(-gth[0], hc, A_w, "force_vjp charge part")
    acc = ops.ThetaAccum([rec.charges])
    acc.flat.fill_(0.25)
    F3, dq3, none = rec.force_vjp(x.detach(), w, accum=acc)
    assert none is None and torch.equal(F3, F) and torch.equal(dq3, dq)
    within(0.25 - acc.views()[0], hc, A_w, "force_vjp charge part through accum", extra=2 * ULP * 0.25)
    F2, dq2, gth2 = rec.force_vjp(x.detach(), w)
    g2x, g2c = torch.autograd.grad(rec(x), (x, rec.charges))
    assert torch.equal(F, F2) and torch.equal(dq, dq2) and torch.equal(gth[0], gth2[0])
    assert torch.equal(g1x.detach(), g2x) and torch.equal(g1c.detach(), g2c)
    # replicas (2, 0, 1): per-atom outputs move with their replica, bit for bit
    perm = torch.cat([torch.arange(24) + 24 * r for r in (2, 0, 1)]).to(DEV)
    xd = x.detach()
    op = ops.ewald_eval(rec.table(), xd[perm].contiguous(), rec._q_atom(), w=w[perm].contiguous(), energy=False, want_pot=True)
    oo = ops.ewald_eval(rec.table(), xd, rec._q_atom(), w=w, energy=False, want_pot=True)
    for key in ("grad", "hw", "potw"):
        assert torch.equal(op[key], oo[key][perm]), key


# ------------------------------------------------------------------------------------------------ 3: autograd
def test_autograd_backward_and_double_backward_equal_force_vjp():
    x32, cell32, q32 = E.jittered_nacl64(seed=70)
    types = (q32 < 0).astype(np.int64)
    _, real, rec = _terms(x32, cell32, np.array([1.0, -1.0], dtype=F32), 5.0, 0.6, 4.5, types=types, trainable=True)
    ref = E.evaluate(x32, q32, rec.table().n_host.numpy(), cell32.astype(np.float64), 0.6, rec.conversion)
    x = T(x32, DEV).requires_grad_(True)
    rec(x).backward()
    within(x.grad, ref["grad"], ref["A_grad"], "backward of model(xyz) in xyz")
    A_c = torch.zeros(2, dtype=torch.float64).index_add_(0, torch.as_tensor(types), ref["A_dq"])
    want_c = torch.zeros(2, dtype=torch.float64).index_add_(0, torch.as_tensor(types), ref["dq"])
    within(rec.charges.grad, want_c, A_c, "backward of model(xyz) in charges")
    w = torch.randn(64, 3, device=DEV)
    x2 = T(x32, DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(rec(x2), x2, create_graph=True)
    hw, hc = torch.autograd.grad((g * w).sum(), (x2, rec.charges))
    F, dq, gth = rec.force_vjp(x2.detach(), w)
    assert torch.equal(F, -g.detach()) and torch.equal(dq, -hw) and torch.equal(gth[0], -hc)
    assert torch.equal(rec.force(x2.detach()), F)
    _, _, frozen = _terms(x32, cell32, q32, 5.0, 0.6, 4.5)
    assert frozen.force_vjp(x2.detach(), w)[2] == [] and frozen.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    assert rec.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    x3 = T(x32, DEV).requires_grad_(True)
    gx, gq = torch.autograd.grad(rec(x3), (x3, rec.charges), create_graph=True)
    with pytest.raises(NotImplementedError, match="dU/dcharges"):
        torch.autograd.grad(gq.sum(), x3)


# ------------------------------------------------------------------------------------------------ 4: into / accum in a Stack
def test_stack_sums_equal_the_members_separate_results():
    """Stack({"lj", **ewald(...)}).force and .force_vjp (the Coulomb and Ewald launches add onto the pair term's buffers)
    against the sum of the members' separate results, to 2^-22 of the largest entry; the gradient of the shared charges is the
    sum of both terms'; the same for `accum` against the list return."""
    from mdgrad_amd import ops
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack, ewald
    x32, cell32, q32 = E.jittered_nacl64(seed=66)
    system = mk_system(x32, cell32)
    lj = PairPotentials(system, P.LJFamily(2.0, 0.1), cutoff=5.0)
    terms = ewald(system, q32, 5.0, accuracy=1e-4, trainable=True)
    real, rec = terms["coulomb_real"], terms["coulomb_recip"]
    stack = Stack({"lj": lj, **terms})
    assert stack.supports_force_vjp() and stack.supports_static_topology()
    x, w = T(x32, DEV), torch.randn(64, 3, device=DEV)
    stack._reset_topology(x)

    def same(a, b, what):
        assert float((a - b).abs().max()) <= 2.0 ** -22 * float(b.abs().max()), what
    same(stack.force(x), lj.force(x) + real.force(x) + rec.force(x), "force")
    F, dq, gth = stack.force_vjp(x, w)
    f1, d1, g1 = lj.force_vjp(x, w)
    f2, d2, g2 = real.force_vjp(x, w)
    f3, d3, g3 = rec.force_vjp(x, w)
    same(F, f1 + f2 + f3, "force (vjp)")
    same(dq, d1 + d2 + d3, "d(w.F)/dx")
    params = list(stack.parameters())
    assert len(gth) == len(params) == 3 and params[2] is real.charges and rec.charges is real.charges
    for v, want in zip(gth, g1 + [g2[0] + g3[0]]):
        same(v, want, "parameter part (the charges: both terms')")
    acc = ops.ThetaAccum(params)
    acc.flat.fill_(0.25)
    assert stack.force_vjp(x, w, accum=acc)[2] is None
    for v, want in zip(acc.views(), gth):
        assert float((v - 0.25 - want).abs().max()) <= 2.0 ** -22 * max(float(want.abs().max()), 0.25), "accum vs list"
    F0, D0 = torch.randn_like(x), torch.randn_like(x)
    F1, D1, _ = rec.force_vjp(x, w, into=(F0.clone(), D0.clone()))
    same(F1 - F0, f3, "force added onto a buffer")
    same(D1 - D0, d3, "d(w.F)/dx added onto a buffer")
    same(rec.force(x, into=F0.clone()) - F0, f3, "force() added onto a buffer")


# ------------------------------------------------------------------------------------------------ 5: trajectory + adjoint
_oracle_cache = {}
TRAJ = dict(sigma=2.0, eps=0.1, rc=5.0, accuracy=1e-4, T=0.3, Q=20.0, chains=3, dt=0.005, mass=10.0, nbins=32, r_range=(1.5, 5.0))


def traj_inputs():
    x32, cell32, q32 = E.jittered_nacl64(seed=71, sigma=0.15)
    vel = np.random.default_rng(680).normal(0, math.sqrt(TRAJ["T"] / TRAJ["mass"]), x32.shape).astype(F32)
    return x32, cell32, (q32 < 0).astype(np.int64), vel, np.full(64, TRAJ["mass"], dtype=F32)


def oracle_traj(t, alpha, kc):
    if "run" not in _oracle_cache:
        x32, cell32, types, vel, mass = traj_inputs()
        cell = T(cell32)
        terms = [O.PairTerm("lj", torch.tensor([TRAJ["sigma"], TRAJ["eps"]]), TRAJ["rc"], cell, p=12, q=6, c=1),
                 R.CoulombTerm(np.array([1.0, -1.0]), TRAJ["rc"], cell32, alpha=alpha, shift="none", types=types),
                 E.EwaldTerm(np.array([1.0, -1.0]), cell32, alpha, kc, types=types, conversion=R.KE)]

        def loss_fn(Ls):
            _, _, gr = O.rdf_oracle(Ls[1][::2], cell, TRAJ["nbins"], TRAJ["r_range"])
            return gr.pow(2).mean() + Ls[0][-1].pow(2).mean() + 0.0 * Ls[2][-1].sum()
        _oracle_cache["run"] = oracle_run(x32, cell32, vel, mass, terms, TRAJ["T"], TRAJ["Q"], TRAJ["chains"], t, loss_fn)
    return _oracle_cache["run"]


@pytest.mark.parametrize("graphs_on", [True, False], ids=["graph_replay", "eager"])
def test_ewald_terms_in_a_stack_trajectory_and_adjoint_vs_oracle(graphs_on):
    """Stack(LJFamily pair + **ewald(...) with per-type trainable charges) on 64 jittered NaCl ions: 10 NHC steps through
    odeint_adjoint, the loss on rdf of q_t[::2] plus v_t[-1]^2 -- trajectories, adjoint of y0, dL/d(sigma, epsilon) and
    dL/dcharges against the oracle with coulomb_ref.CoulombTerm (shift "none") and ewald_ref.EwaldTerm appended.  The stack stays
    on the analytic adjoint (force_vjp) and HIP-graph replay.  Setup and tolerances: those of
    test_gpu_coulomb.test_coulomb_term_in_a_stack_trajectory_and_adjoint_vs_oracle, with the damped shifted-force term replaced
    by ewald(cutoff = 5.0, accuracy = 1e-4)."""
    from mdgrad_amd import graphs, units
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack, ewald
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.sovlers import odeint_adjoint
    assert abs(units.ke - R.KE) <= 1e-12 * R.KE
    x32, cell32, types, vel, mass = traj_inputs()
    system = mk_system(x32, cell32, vel, mass)
    mdl = P.LJFamily(TRAJ["sigma"], TRAJ["eps"])
    terms = ewald(system, [1.0, -1.0], TRAJ["rc"], accuracy=TRAJ["accuracy"], types=types, trainable=True)
    real, rec = terms["coulomb_real"], terms["coulomb_recip"]
    stack = Stack({"pair": PairPotentials(system, mdl, cutoff=TRAJ["rc"]), **terms})
    integ = NoseHooverChain(stack, system, T=TRAJ["T"], num_chains=TRAJ["chains"], Q=TRAJ["Q"], adjoint=True).to(DEV)
    assert integ.fused_spec("NH_verlet") is None, "the Ewald members keep the stack off the fused trajectory kernels"
    assert integ.model.supports_force_vjp() and integ.supports_rhs_vjp(), "the terms must not push the stack onto the autograd branch"
    assert graphs.enabled(integ)
    integ.use_graphs = graphs_on
    calls = {"n": 0}
    orig = integ.model.force_vjp

    def counted(*a, **k):
        calls["n"] += 1
        return orig(*a, **k)
    integ.model.force_vjp = counted
    t = torch.Tensor([TRAJ["dt"] * i for i in range(11)])
    y0 = [s.clone().requires_grad_(True) for s in integ.get_inital_states(wrap=True)]
    v_t, q_t, pv_t = odeint_adjoint(integ, tuple(y0), t.to(DEV), method="NH_verlet")
    _, _, gr = rdf(system, nbins=TRAJ["nbins"], r_range=TRAJ["r_range"])(q_t[::2])
    loss = gr.pow(2).mean() + v_t[-1].pow(2).mean() + 0.0 * pv_t[-1].sum()
    loss.backward()
    assert calls["n"] > 0, "the adjoint did not go through force_vjp"
    traj, lam, gth = oracle_traj(t, real.alpha, rec.k_cutoff)
    close(q_t, traj[1], 0, 2e-5, "q_t")
    close(v_t, traj[0], 1e-3, 1e-4 * float(traj[0].abs().max()), "v_t")
    close(pv_t, traj[2], 2e-3, 1e-5, "pv_t")
    for x, l, nm in zip(y0, lam, ("adj v0", "adj q0", "adj pv0")):
        close(x.grad, l, 5e-3, 2e-3 * float(l.abs().max()) + 1e-9, nm)
    got = torch.stack([mdl.sigma.grad.reshape(()), mdl.epsilon.grad.reshape(())])
    close(got, gth[:2], 5e-3, 5e-4 * float(gth[:2].abs().max()), "dL/d(sigma, epsilon)")
    assert gth.numel() == 6 and real.charges.grad is not None and rec.charges is real.charges
    want = gth[2:4] + gth[4:6]                                  # the oracle's two terms each carry the charges
    close(real.charges.grad, want, 5e-3, 5e-4 * float(want.abs().max()), "dL/dcharges")


# ------------------------------------------------------------------------------------------------ 6: Madelung, alpha independence
def _total_vs_float64(x32, cell32, q32, rc, real, rec):
    """(U on the device, U in float64, allowed difference, forces on the device, float64 dU/dx, allowed per component)."""
    lst = R.half_list(x32, cell32, rc)
    assert lst[3] > 1e-4, "a pair sits within float32 rounding of the cutoff"
    r1 = R.evaluate(x32, q32, lst, cell32, R.consts(rc, real.alpha, "none", real.conversion))
    r2 = E.evaluate(x32, q32, rec.table().n_host.numpy(), cell32.astype(np.float64), rec.alpha, rec.conversion)
    x = T(x32, DEV)
    U = float(real(x)) + float(rec(x))
    F = (real.force(x) + rec.force(x)).cpu().double()
    return (U, float(r1["U"] + r2["U"]), TOL_REAL * float(r1["A_U"]) + TOL * float(r2["A_U"]), F, r1["grad"] + r2["grad"],
            TOL_REAL * r1["A_grad"] + TOL * r2["A_grad"])


def test_perfect_nacl64_madelung_and_zero_forces():
    """Perfect 64-ion rock salt through ewald(cutoff = 5.5, accuracy = 1e-5, conversion = 1): the Madelung constant within the
    two kernels' tolerances of the float64 value of the same finite sums (which is within 1e-5 of 1.747565), and forces that
    vanish within them."""
    from mdgrad_amd.interface import ewald
    pos, q, L = R.nacl(2)
    x32, cell32, q32 = pos.astype(F32), np.array([L, L, L], dtype=F32), q.astype(F32)
    terms = ewald(mk_system(x32, cell32), q32, 5.5, accuracy=1e-5, conversion=1.0)
    real, rec = terms["coulomb_real"], terms["coulomb_recip"]
    assert rec.n_vectors == 895
    U, U64, tolU, F, g64, tolF = _total_vs_float64(x32, cell32, q32, 5.5, real, rec)
    M, M64 = R.madelung(U, 64, 2.82, 1.0), R.madelung(U64, 64, 2.82, 1.0)
    print("Madelung: device %.7f  float64 %.7f  allowed difference %.2e" % (M, M64, 2 * 2.82 * tolU / 64))
    assert abs(M64 - R.MADELUNG_NACL) <= 1e-5
    assert abs(M - M64) <= 2 * 2.82 * tolU / 64
    assert bool(((F + g64).abs() <= tolF).all()) and float(g64.abs().max()) <= 1e-5 * float(tolF.max() / TOL_REAL)


def test_total_energy_is_independent_of_alpha_on_the_device():
    """Jittered NaCl-64, rc = 5.5, conversion = 1, at (alpha, k_cutoff) = (0.6, 4.5) and (0.7, 5.2): the device totals differ
    by no more than the float64 totals do (4.6e-6 here) plus both evaluations' kernel tolerances."""
    x32, cell32, q32 = E.jittered_nacl64()
    out = []
    for alpha, kc in ((0.6, 4.5), (0.7, 5.2)):
        _, real, rec = _terms(x32, cell32, q32, 5.5, alpha, kc, conversion=1.0)
        out.append(_total_vs_float64(x32, cell32, q32, 5.5, real, rec)[:3])
    (U1, V1, t1), (U2, V2, t2) = out
    print("device %.7f %.7f  float64 %.7f %.7f  tolerances %.2e %.2e" % (U1, U2, V1, V2, t1, t2))
    assert abs(V1 - V2) <= 1e-5, "the float64 sums themselves depend on alpha: cutoffs too short"
    assert abs(U1 - U2) <= abs(V1 - V2) + t1 + t2


# ------------------------------------------------------------------------------------------------ 7: torch ops
def test_torch_ops_equal_ctypes_path_and_reject_bad_input():
    from mdgrad_amd import _lib, _torch_ops, ops
    ns = _torch_ops.get()
    assert ns is not None
    base, box, x32, types = _replicas24()
    _, real, rec = _terms(base, box, np.where(types == 0, 1.0, -0.8).astype(F32), 3.5, 0.8, 5.0, n_rep=3)
    tb = rec.table()
    cell = _torch_ops.cell_args(tb.cell_struct)
    x, w, q = T(x32, DEV), torch.randn(72, 3, device=DEV), rec._q_atom()
    a = ops.ewald_eval(tb, x, q, energy=True, grad=True, want_pot=True)
    U, g, hw, pot, potw = ns.ewald_eval(x, 3, cell, q, tb.kvec, tb.coef, None, True, True)
    assert torch.equal(U, a["energy"]) and torch.equal(g, a["grad"]) and torch.equal(pot, a["pot"]) and hw.numel() == potw.numel() == 0
    b = ops.ewald_eval(tb, x, q, w=w, energy=False, grad=True, want_pot=True)
    U, g, hw, pot, potw = ns.ewald_eval(x, 3, cell, q, tb.kvec, tb.coef, w, False, True)
    assert torch.equal(g, b["grad"]) and torch.equal(hw, b["hw"]) and torch.equal(potw, b["potw"]) and U.numel() == pot.numel() == 0
    big = tb.kvec.clone()
    big[3, 1] = 1025
    tric = list(cell)
    tric[1], tric[18] = 0.5, 0.0
    bad = [lambda: ns.ewald_eval(x.double(), 3, cell, q, tb.kvec, tb.coef, None, True, False),
           lambda: ns.ewald_eval(x.cpu(), 3, cell, q, tb.kvec, tb.coef, None, True, False),
           lambda: ns.ewald_eval(x, 3, cell, q.cpu(), tb.kvec, tb.coef, None, True, False),
           lambda: ns.ewald_eval(x, 3, cell, q, tb.kvec.cpu(), tb.coef, None, True, False),
           lambda: ns.ewald_eval(x, 5, cell, q, tb.kvec, tb.coef, None, True, False),
           lambda: ns.ewald_eval(x, 0, cell, q, tb.kvec, tb.coef, None, True, False),
           lambda: ns.ewald_eval(x, 3, cell[:5], q, tb.kvec, tb.coef, None, True, False),
           lambda: ns.ewald_eval(x, 3, tric, q, tb.kvec, tb.coef, None, True, False),
           lambda: ns.ewald_eval(x, 3, cell, q[:5].contiguous(), tb.kvec, tb.coef, None, True, False),
           lambda: ns.ewald_eval(x, 3, cell, q.double(), tb.kvec, tb.coef, None, True, False),
           lambda: ns.ewald_eval(x, 3, cell, q, tb.kvec.long(), tb.coef, None, True, False),
           lambda: ns.ewald_eval(x, 3, cell, q, tb.kvec[:0].contiguous(), tb.coef[:0].contiguous(), None, True, False),
           lambda: ns.ewald_eval(x, 3, cell, q, tb.kvec.reshape(-1), tb.coef, None, True, False),
           lambda: ns.ewald_eval(x, 3, cell, q, tb.kvec, tb.coef[:5].contiguous(), None, True, False),
           lambda: ns.ewald_eval(x, 3, cell, q, big, tb.coef, None, True, False),
           lambda: ns.ewald_eval(x, 3, cell, q, tb.kvec, tb.coef, w[:5].contiguous(), True, False),
           lambda: ns.ewald_eval(x, 3, cell, q, tb.kvec, tb.coef, w.cpu(), True, False)]
    for n, fn in enumerate(bad):
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
            pytest.fail("bad input %d was accepted" % n)
    # the C entry point itself answers bad arguments with an error code
    lib = _lib.load()
    ws = torch.empty(int(lib.mdg_ewald_workspace(3, 24, tb.n_vecs)), device=DEV)
    e = torch.empty(1, device=DEV)
    p = _lib.ptr

    def call(n_rep=3, n_atoms=24, n_vecs=tb.n_vecs, cs=tb.cell_struct, wp=None, hw=None, energy=e, work=ws):
        import ctypes
        return lib.mdg_ewald_eval(p(x), n_rep, n_atoms, ctypes.byref(cs), p(q), p(tb.kvec), p(tb.coef), n_vecs, p(wp), p(energy),
                                  None, p(hw), None, None, p(work), 1.0, 0, _lib.stream_ptr(x.device))
    assert call() == 0
    assert call(n_vecs=0) == -1 and b"wave vectors" in lib.mdg_last_error()
    assert call(n_vecs=65537) == -1 and call(n_atoms=32769) == -1 and call(n_rep=0) == -1
    assert call(cs=_lib.make_cell(torch.tensor([[8.0, 0, 0], [1.0, 8.0, 0], [0, 0, 8.0]]))) == -1 and b"diagonal" in lib.mdg_last_error()
    assert call(hw=torch.empty(72, 3, device=DEV)) == -1 and call(wp=w) == -1 and call(energy=None) == -1 and call(work=None) == -1
    torch.cuda.synchronize()
