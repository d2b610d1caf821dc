"""K22: the erf correction of the Ewald sum for excluded and scaled pairs (EwaldExclusions, ewald(..., ex_pairs=),
mdg_ewald_excl_eval, csrc/ewald_excl.hip) against the float64 definitions of tests/ewald_excl_ref.py (checked against
autograd, the exclusion identity and alpha independence by tests/test_ewald_excl_host.py) and, in a Stack with a pair term,
bonds, angles and the two other members of the sum, the CPU oracle's trajectory and adjoint.

Tolerance of every kernel-vs-float64 comparison: 64 * 2^-24 * A per component, the project's figure for a pair kernel built on
erff / expf (tests/test_gpu_coulomb.py), A = the float64 sum of the absolute pair contributions to that component built from
|chi|, |chi'|, |chi''| (ewald_excl_ref.evaluate).  `within` prints the largest observed err / (2^-24 A);
the largest figure over all cases of this file on an MI355X is 28.92 (H w of the isolated dimers; OBSERVED below, per output)."""
import math

import numpy as np
import pytest
import torch

import coulomb_ref as R
import ewald_ref as E
import ewald_excl_ref as X
import oracle as O
from test_gpu_parity import T, close, mk_system, DEV, oracle_run
from test_gpu_ewald import TOL as TOL_RECIP                   # the reciprocal kernel's C * 2^-24

pytestmark = pytest.mark.gpu
F32 = np.float32
ULP = 2.0 ** -24
C_TOL = 64.0
TOL = C_TOL * ULP
# largest err / (2^-24 A) per output over all cases of this file on an MI355X
OBSERVED = dict(U=0.68, grad=14.82, pot=5.20, hw=28.92, potw=15.02, dcharges=0.85)


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


def _table(pairs, scale, n_atoms, lengths, alpha, conversion=1.0, n_rep=1):
    from mdgrad_amd import ops
    return ops.EwaldExclTable(pairs, scale, n_atoms, n_rep, np.asarray(lengths, dtype=np.float64), alpha, conversion, DEV)


def _check_all_outputs(table, x32, q32, tag, seed=0):
    """energy, dU/dx, H w, pot and potw of the low-level op against the explicit float64 pair sums; every launch twice,
    bitwise equal; the energy-only launch."""
    from mdgrad_amd import ops
    w32 = np.random.default_rng(seed + 17).normal(0, 1, x32.shape).astype(F32)
    ref = X.evaluate(x32, q32, table.pairs.numpy(), table.scale.numpy(), table.lengths, table.alpha, table.conversion, w=w32,
                     group=table.n_atoms)
    x, w, q = T(x32, DEV), T(w32, DEV), T(q32, DEV)
    o1 = ops.ewald_excl_eval(table, x, q, energy=True, grad=True, want_pot=True)
    o2 = ops.ewald_excl_eval(table, x, q, w=w, energy=False, grad=True, want_pot=True)
    rs = dict(U=within(o1["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + " U"),
              grad=within(o1["grad"], ref["grad"], ref["A_grad"], tag + " dU/dx"),
              pot=within(o1["pot"], ref["pot"], ref["A_pot"], tag + " pot"),
              hw=within(o2["hw"], ref["hw"], ref["A_hw"], tag + " H.w"),
              potw=within(o2["potw"], ref["potw"], ref["A_potw"], tag + " potw"))
    assert torch.equal(o1["grad"], o2["grad"]) and o2["pot"] is None and o1["potw"] is None
    e0 = ops.ewald_excl_eval(table, x, q, energy=True, grad=False)
    assert torch.equal(e0["energy"], o1["energy"]) and e0["grad"] is None, "energy-only evaluation"
    p1 = ops.ewald_excl_eval(table, x, q, energy=True, grad=True, want_pot=True)
    p2 = ops.ewald_excl_eval(table, x, q, w=w, energy=False, grad=True, want_pot=True)
    for a, b in ((o1, p1), (o2, p2)):
        for key in a:
            assert (a[key] is None and b[key] is None) or torch.equal(a[key], b[key]), "two launches differ in " + key
    return ref, o1, o2, w32


def _members(x32, cell32, charges, pairs, rc, alpha, kc=None, scale=None, n_rep=1, **kw):
    from mdgrad_amd.interface import CoulombPotentials, EwaldExclusions, EwaldReciprocal
    system = mk_system(x32, cell32)
    if n_rep > 1:
        system = system.replicate(n_rep)
    real = CoulombPotentials(system, charges, rc, alpha=alpha, shift="none", ex_pairs=pairs, **kw)
    excl = EwaldExclusions(system, real, scale=scale)
    rec = EwaldReciprocal(system, real, k_cutoff=kc, exclusions=excl) if kc is not None else None
    return system, real, rec, excl


# ------------------------------------------------------------------------------------------------ 1: all outputs on water27
def test_outputs_vs_float64_water27():
    """81 atoms (no multiple of the wave), 81 excluded pairs, alpha 0.754: through the low-level op and through the class."""
    x32, cell32, q32, _, pairs, _, _ = X.water27()
    _, real, _, excl = _members(x32, cell32, q32, pairs, 4.5, 0.754, conversion=2.5)
    ref, _, _, _ = _check_all_outputs(excl.table(), x32, q32, "water27")
    U = excl(T(x32, DEV))
    within(U.reshape(1), ref["U"].reshape(1), ref["A_U"].reshape(1), "water27 U through the class")
    F = excl.force(T(x32, DEV))
    within(-F, ref["grad"], ref["A_grad"], "water27 force through the class")


# ------------------------------------------------------------------------------------------------ 2: small alpha r
def _dimers():
    """129 atoms in a 40^3 box: 64 dimers (atoms 2k, 2k + 1) and one spare atom; 63 separations log-spaced from 1e-3 to 4.0
    along seeded random directions, dimer 63 exactly coincident.  No dimer crosses the boundary, so every float32 difference
    x_i - x_j is exact."""
    rng = np.random.default_rng(129)
    c = rng.uniform(5.0, 35.0, (65, 3)).astype(F32)
    u = rng.normal(0, 1, (64, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    sep = np.concatenate([np.geomspace(1e-3, 4.0, 63), [0.0]])
    x = np.empty((129, 3), dtype=F32)
    x[0:128:2] = c[:64]
    x[1:128:2] = (c[:64].astype(np.float64) + sep[:, None] * u).astype(F32)
    x[128] = c[64]
    assert np.array_equal(x[126], x[127])
    q = rng.normal(0, 1, 129).astype(F32)
    q[np.abs(q) < 0.2] = 0.5
    pairs = np.stack([np.arange(0, 128, 2), np.arange(1, 128, 2)], 1)
    return x, np.array([40.0, 40.0, 40.0], dtype=F32), q, pairs, sep


def test_small_alpha_r_and_a_coincident_pair():
    """alpha = 0.75, s = 0: alpha r from 7.5e-4 to 3.0 and exactly 0.  All outputs within the tolerance; the coincident pair
    gives the limits exactly (zero gradient and potw).  The closed form (G r - E1) / r^2 in float32 loses 2e-5 (340 * 2^-24) at
    alpha r = 0.1 and 3e-4 at 0.02, so it fails this test there: the kernel's power series does not."""
    x32, cell32, q32, pairs, sep = _dimers()
    alpha = 0.75
    tb = _table(pairs, None, 129, cell32, alpha)
    ref, o1, o2, w32 = _check_all_outputs(tb, x32, q32, "dimers")
    g0 = 2 * alpha / math.sqrt(math.pi)
    assert float(o1["grad"][126:128].abs().max()) == 0.0 and float(o2["potw"][126:128].abs().max()) == 0.0
    assert float(o1["grad"][128].abs().max()) == 0.0 and float(o1["pot"][128]) == 0.0 and float(o2["hw"][128].abs().max()) == 0.0
    assert abs(float(o1["pot"][126]) + float(q32[127]) * g0) <= 4 * ULP * abs(float(q32[127])) * g0
    lim = float(q32[126]) * float(q32[127]) * 4 * alpha ** 3 / (3 * math.sqrt(math.pi)) * (w32[126] - w32[127]).astype(np.float64)
    assert float((o2["hw"][126].cpu().double() - torch.tensor(lim)).abs().max()) <= 8 * ULP * float(np.abs(lim).max())
    # per dimer, so that the smallest separations are seen on their own
    for k in (0, 10, 20, 30):
        i = 2 * k
        within(o1["grad"][i], ref["grad"][i], ref["A_grad"][i], "dimer %d (alpha r = %.1e) dU/dx" % (k, alpha * sep[k]))
        within(o2["hw"][i], ref["hw"][i], ref["A_hw"][i], "dimer %d (alpha r = %.1e) H.w" % (k, alpha * sep[k]))


# ------------------------------------------------------------------------------------------------ 3: hub atom, empty rows
@pytest.mark.parametrize("hub_to", [33, 19], ids=["every_atom_paired", "rows_20_to_33_empty"])
def test_hub_atom_and_empty_rows(hub_to):
    """gas37 with atom 0 paired to atoms 1 .. hub_to and the pairs (34, 35), (35, 36): a row of 33 (19) entries beside rows of
    1 and 2 -- and, with hub_to = 19, fourteen empty rows.  Added onto `into` buffers of random numbers, atoms with empty rows
    keep their buffer bits; the zero-charge atom 5 has exactly zero gradient."""
    from mdgrad_amd import ops
    x32, box, q32 = E.gas37()
    pairs = np.array([[0, k] for k in range(1, hub_to + 1)] + [[34, 35], [35, 36]])
    tb = _table(pairs, None, 37, box, 1.0, conversion=1.7)
    assert np.diff(tb.row_ptr_host).max() == hub_to and sorted(set(np.diff(tb.row_ptr_host).tolist()))[:3] == ([1, 2, 33] if hub_to == 33 else [0, 1, 2])
    ref, o1, o2, w32 = _check_all_outputs(tb, x32, q32, "gas37 hub")
    assert float(o1["grad"][5].abs().max()) == 0.0 and float(o2["hw"][5].abs().max()) == 0.0
    empty = torch.tensor(np.diff(tb.row_ptr_host) == 0)
    x, w, q = T(x32, DEV), T(w32, DEV), T(q32, DEV)
    g0, h0 = torch.randn(37, 3, device=DEV), torch.randn(37, 3, device=DEV)
    g0[20], h0[21] = -0.0, float("nan")                          # bit patterns an added zero would not keep
    g, h = g0.clone(), h0.clone()
    o = ops.ewald_excl_eval(tb, x, q, w=w, energy=False, grad=True, into=(g, h), scale=-1.0)
    assert o["grad"] is g and o["hw"] is h
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(g)[empty.to(DEV)], bits(g0)[empty.to(DEV)]) and torch.equal(bits(h)[empty.to(DEV)], bits(h0)[empty.to(DEV)])
    # elsewhere the launch adds -1 times what the plain launch returns, rounded once: the same bits as torch's subtraction
    rows = (~empty).to(DEV)
    rows[21] = False                                             # (the NaN row)
    assert torch.equal(g[rows], (g0 - o1["grad"])[rows]) and torch.equal(h[rows], (h0 - o2["hw"])[rows])
    assert bool(torch.isnan(h[21]).all())
    g2 = g0.clone()
    ops.ewald_excl_eval(tb, x, q, energy=False, grad=True, into=(g2, None), scale=-1.0)
    assert torch.equal(bits(g2), bits(g)), "the force-only launch adds the same bits"


# ------------------------------------------------------------------------------------------------ 4: scales
def test_per_pair_and_scalar_scales_vs_float64():
    """water27 with per-pair s drawn from {0, 0.5, 1} and with the scalar s = 0.5; the s = 1 pairs alone agree with
    coulomb_ref.psi of shift "none" (the real-space kernel's formulas)."""
    x32, cell32, q32, _, pairs, _, _ = X.water27()
    s = np.random.default_rng(4).choice([0.0, 0.5, 1.0], len(pairs))
    assert all((s == v).sum() > 10 for v in (0.0, 0.5, 1.0))
    _check_all_outputs(_table(pairs, s, 81, cell32, 0.754, conversion=1.3), x32, q32, "water27 s in {0, .5, 1}")
    _check_all_outputs(_table(pairs, 0.5, 81, cell32, 0.754), x32, q32, "water27 s = 0.5")
    one = pairs[s == 1.0]
    tb = _table(one, 1.0, 81, cell32, 0.754)
    from mdgrad_amd import ops
    o = ops.ewald_excl_eval(tb, T(x32, DEV), T(q32, DEV), energy=True, grad=True, want_pot=True)
    x, q = torch.tensor(x32).double(), torch.tensor(q32).double()
    d = X.reimage(x[one[:, 0]] - x[one[:, 1]], cell32.astype(np.float64))
    r = d.pow(2).sum(-1).sqrt()
    p0, p1, _ = R.psi(r, R.consts(10.0, 0.754, "none"))
    qq = q[one[:, 0]] * q[one[:, 1]]
    within(o["energy"], (qq * p0).sum().reshape(1), (qq * p0).abs().sum().reshape(1), "s = 1 pairs: U vs coulomb_ref.psi")
    t = (qq * p1)[:, None] * d / r[:, None]
    g = torch.zeros(81, 3, dtype=torch.float64).index_add_(0, torch.tensor(one[:, 0]), t).index_add_(0, torch.tensor(one[:, 1]), -t)
    A = torch.zeros(81, 3, dtype=torch.float64).index_add_(0, torch.tensor(one[:, 0]), t.abs()).index_add_(0, torch.tensor(one[:, 1]), t.abs())
    within(o["grad"], g, A, "s = 1 pairs: dU/dx vs coulomb_ref.psi'")


# ------------------------------------------------------------------------------------------------ 5: replicas, charge gradients
def test_three_replicas_and_per_type_charge_gradients_vs_float64_autograd():
    """System.replicate(3) of water27 with different jitters, per-type trainable charges: every replica against the float64
    reference, dU/dcharges and d(w.dU/dx)/dcharges (2 slots, each summed over all atoms of the type) against float64 autograd,
    allowed 64 * 2^-24 times the slot's sum of conversion A_pot, resp. conversion A_potw; force_vjp's charge part with and
    without `accum`."""
    from mdgrad_amd import ops
    base, cell32, _, types, pairs, _, _ = X.water27()
    rng = np.random.default_rng(270)
    x32 = np.concatenate([base + rng.normal(0, 0.03, base.shape).astype(F32) for _ in range(3)]).astype(F32)
    c32 = np.array([-0.82, 0.41], dtype=F32)
    alpha, cv = 0.754, 2.5
    _, real, _, excl = _members(base, cell32, c32, pairs, 4.5, alpha, scale=0.5, n_rep=3, types=types, trainable=True, conversion=cv)
    assert excl.charges is real.charges and excl.n_slots == 2 and excl._q_atom().shape == (243,)
    w32 = rng.normal(0, 1, x32.shape).astype(F32)
    qa32 = R.expand(torch.tensor(c32), types, 3).numpy()
    L = cell32.astype(np.float64)
    ref = X.evaluate(x32, qa32, pairs, 0.5, L, alpha, cv, w=w32, group=81)
    c64 = torch.tensor(c32).double().requires_grad_(True)
    x64 = torch.tensor(x32).double().requires_grad_(True)
    U = X.energy(x64, R.expand(c64, types, 3), pairs, 0.5, L, alpha, cv, group=81)
    gx, gc = torch.autograd.grad(U, (x64, c64), create_graph=True)
    (hc,) = torch.autograd.grad((gx * torch.tensor(w32).double()).sum(), c64)
    slot = torch.as_tensor(types).repeat(3)

    def per_slot(v):
        return torch.zeros(2, dtype=torch.float64).index_add_(0, slot, v)
    A_u, A_w = cv * per_slot(ref["A_pot"]), cv * per_slot(ref["A_potw"])
    x, w = T(x32, DEV).requires_grad_(True), T(w32, DEV)
    Ud = excl(x)
    within(Ud.reshape(1), ref["U"].reshape(1), ref["A_U"].reshape(1), "U on three replicas")
    g1x, g1c = torch.autograd.grad(Ud, (x, excl.charges), create_graph=True)
    (h1c,) = torch.autograd.grad((g1x * w).sum(), excl.charges)
    within(g1x, ref["grad"], ref["A_grad"], "dU/dx on three replicas")
    within(g1c, gc.detach(), A_u, "dU/dcharges")
    within(h1c, hc, A_w, "d(w.dU/dx)/dcharges")
    F, dq, gth = excl.force_vjp(x.detach(), w)
    within(-dq, ref["hw"], ref["A_hw"], "H.w on three replicas")
    within(-gth[0], hc, A_w, "force_vjp charge part")
    acc = ops.ThetaAccum([excl.charges])
    acc.flat.fill_(0.25)
    F3, dq3, none = excl.force_vjp(x.detach(), w, accum=acc)
    assert none is None and torch.equal(F3, F) and torch.equal(dq3, dq)
    within(0.25 - acc.views()[0], hc, A_w, "force_vjp charge part through accum", extra=2 * ULP * 0.25)
    # replicas (2, 0, 1): per-atom outputs move with their replica, bit for bit
    perm = torch.cat([torch.arange(81) + 81 * r for r in (2, 0, 1)]).to(DEV)
    xd = x.detach()
    op = ops.ewald_excl_eval(excl.table(), xd[perm].contiguous(), excl._q_atom(), w=w[perm].contiguous(), energy=False, want_pot=True)
    oo = ops.ewald_excl_eval(excl.table(), xd, excl._q_atom(), w=w, energy=False, want_pot=True)
    for key in ("grad", "hw", "potw"):
        assert torch.equal(op[key], oo[key][perm]), key


# ------------------------------------------------------------------------------------------------ 6: autograd
def test_autograd_backward_and_double_backward_equal_force_vjp():
    x32, cell32, q32, types, pairs, _, _ = X.water27()
    _, real, _, excl = _members(x32, cell32, np.array([-0.82, 0.41], dtype=F32), pairs, 4.5, 0.754, types=types, trainable=True)
    ref = X.evaluate(x32, q32, pairs, None, cell32.astype(np.float64), 0.754, excl.conversion)
    x = T(x32, DEV).requires_grad_(True)
    excl(x).backward()
    within(x.grad, ref["grad"], ref["A_grad"], "backward of model(xyz) in xyz")
    ty = torch.as_tensor(types)
    A_c = excl.conversion * torch.zeros(2, dtype=torch.float64).index_add_(0, ty, ref["A_pot"])
    want_c = excl.conversion * torch.zeros(2, dtype=torch.float64).index_add_(0, ty, ref["pot"])
    within(excl.charges.grad, want_c, A_c, "backward of model(xyz) in charges")
    w = torch.randn(81, 3, device=DEV)
    x2 = T(x32, DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(excl(x2), x2, create_graph=True)
    hw, hc = torch.autograd.grad((g * w).sum(), (x2, excl.charges))
    F, dq, gth = excl.force_vjp(x2.detach(), w)
    assert torch.equal(F, -g.detach()) and torch.equal(dq, -hw) and torch.equal(gth[0], -hc)
    assert torch.equal(excl.force(x2.detach()), F)
    _, _, _, frozen = _members(x32, cell32, q32, pairs, 4.5, 0.754)
    assert frozen.force_vjp(x2.detach(), w)[2] == [] and frozen.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    assert excl.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    x3 = T(x32, DEV).requires_grad_(True)
    gx, gq = torch.autograd.grad(excl(x3), (x3, excl.charges), create_graph=True)
    with pytest.raises(NotImplementedError, match="dU/dcharges"):
        torch.autograd.grad(gq.sum(), x3)


# ------------------------------------------------------------------------------------------------ 7: into / accum in a Stack
def test_stack_sums_equal_the_members_separate_results():
    """Stack({"lj", **ewald(..., ex_pairs=)}).force and .force_vjp against the sum of the members' separate results, to 2^-22
    of the largest entry; the gradient of the shared charges is the sum of the three terms'; `accum` against the list return;
    `into` and force(into=)."""
    from mdgrad_amd import ops
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack, ewald
    x32, cell32, q32, types, pairs, _, _ = X.water27()
    system = mk_system(x32, cell32)
    ox = np.nonzero(types == 0)[0].tolist()
    lj = PairPotentials(system, P.LJFamily(2.0, 0.1), cutoff=4.5, index_tuple=(ox, ox))
    terms = ewald(system, q32, 4.5, accuracy=1e-4, trainable=True, ex_pairs=pairs, scale=0.5)
    real, rec, excl = terms["coulomb_real"], terms["coulomb_recip"], terms["coulomb_excl"]
    stack = Stack({"lj": lj, **terms})
    assert stack.supports_force_vjp() and stack.supports_static_topology()
    x, w = T(x32, DEV), torch.randn(81, 3, device=DEV)
    stack._reset_topology(x)

    def same(a, b, what):
        assert float((a - b).abs().max()) <= 2.0 ** -22 * float(b.abs().max()), what
    same(stack.force(x), lj.force(x) + real.force(x) + rec.force(x) + excl.force(x), "force")
    F, dq, gth = stack.force_vjp(x, w)
    f1, d1, g1 = lj.force_vjp(x, w)
    f2, d2, g2 = real.force_vjp(x, w)
    f3, d3, g3 = rec.force_vjp(x, w)
    f4, d4, g4 = excl.force_vjp(x, w)
    same(F, f1 + f2 + f3 + f4, "force (vjp)")
    same(dq, d1 + d2 + d3 + d4, "d(w.F)/dx")
    params = list(stack.parameters())
    assert len(gth) == len(params) == 3 and params[2] is real.charges and rec.charges is real.charges and excl.charges is real.charges
    for v, want in zip(gth, g1 + [g2[0] + g3[0] + g4[0]]):
        same(v, want, "parameter part (the charges: all three terms')")
    acc = ops.ThetaAccum(params)
    acc.flat.fill_(0.25)
    assert stack.force_vjp(x, w, accum=acc)[2] is None
    for v, want in zip(acc.views(), gth):
        assert float((v - 0.25 - want).abs().max()) <= 2.0 ** -22 * max(float(want.abs().max()), 0.25), "accum vs list"
    F0, D0 = torch.randn_like(x), torch.randn_like(x)
    F1, D1, _ = excl.force_vjp(x, w, into=(F0.clone(), D0.clone()))
    same(F1 - F0, f4, "force added onto a buffer")
    same(D1 - D0, d4, "d(w.F)/dx added onto a buffer")
    same(excl.force(x, into=F0.clone()) - F0, f4, "force() added onto a buffer")


# ------------------------------------------------------------------------------------------------ 8: trajectory + adjoint
_oracle_cache = {}
TRAJ = dict(sigma=2.0, eps=0.1, rc=4.5, accuracy=1e-4, T=0.3, Q=20.0, chains=3, dt=0.005, mass=10.0, nbins=32, r_range=(1.5, 5.0),
            k_bond=3.0, ro=1.0, k_angle=2.0, theta0=math.radians(109.47))


def traj_inputs():
    x32, cell32, q32, types, pairs, bonds, angles = X.water27()
    vel = np.random.default_rng(680).normal(0, math.sqrt(TRAJ["T"] / TRAJ["mass"]), x32.shape).astype(F32)
    return x32, cell32, types, pairs, bonds, angles, vel, np.full(81, TRAJ["mass"], dtype=F32)


def oracle_traj(t, alpha, kc):
    if "run" not in _oracle_cache:
        x32, cell32, types, pairs, bonds, angles, vel, mass = traj_inputs()
        cell = T(cell32)
        ox = np.nonzero(types == 0)[0].tolist()
        ch = np.array([-0.82, 0.41])
        terms = [O.PairTerm("lj", torch.tensor([TRAJ["sigma"], TRAJ["eps"]]), TRAJ["rc"], cell, index_tuple=(ox, ox), p=12, q=6, c=1),
                 O.BondTerm(bonds, TRAJ["k_bond"], TRAJ["ro"], cell), O.AngleTerm(angles, TRAJ["k_angle"], TRAJ["theta0"], cell),
                 R.CoulombTerm(ch, TRAJ["rc"], cell32, alpha=alpha, shift="none", types=types, ex_pairs=pairs),
                 E.EwaldTerm(ch, cell32, alpha, kc, types=types, conversion=R.KE),
                 X.ExclTerm(ch, cell32, alpha, pairs, types=types, conversion=R.KE)]

        def loss_fn(Ls):
            _, _, gr = O.rdf_oracle(Ls[1][::2], cell, TRAJ["nbins"], TRAJ["r_range"])
            return gr.pow(2).mean() + Ls[0][-1].pow(2).mean() + 0.0 * Ls[2][-1].sum()
        _oracle_cache["run"] = oracle_run(x32, cell32, vel, mass, terms, TRAJ["T"], TRAJ["Q"], TRAJ["chains"], t, loss_fn)
    return _oracle_cache["run"]


@pytest.mark.parametrize("graphs_on", [True, False], ids=["graph_replay", "eager"])
def test_water_stack_trajectory_and_adjoint_vs_oracle(graphs_on):
    """Stack(O-O LJFamily pair (index_tuple) + BondPotentials + AnglePotentials + **ewald(..., per-type trainable charges,
    ex_pairs = the 81 intramolecular pairs)) on water27: 10 NHC steps through odeint_adjoint, the loss on rdf of q_t[::2] plus
    v_t[-1]^2 -- trajectories, adjoint of y0, dL/d(sigma, epsilon) and dL/dcharges against the oracle with PairTerm, BondTerm,
    AngleTerm, CoulombTerm (with ex_pairs), EwaldTerm and ExclTerm.  The stack stays on the analytic adjoint (force_vjp) and
    HIP-graph replay.  Loss, masses, thermostat and tolerances: those of
    test_gpu_ewald.test_ewald_terms_in_a_stack_trajectory_and_adjoint_vs_oracle."""
    from mdgrad_amd import graphs, units
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import AnglePotentials, BondPotentials, PairPotentials, Stack, ewald
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.sovlers import odeint_adjoint
    assert abs(units.ke - R.KE) <= 1e-12 * R.KE
    x32, cell32, types, pairs, bonds, angles, vel, mass = traj_inputs()
    system = mk_system(x32, cell32, vel, mass)
    mdl = P.LJFamily(TRAJ["sigma"], TRAJ["eps"])
    ox = np.nonzero(types == 0)[0].tolist()
    terms = ewald(system, [-0.82, 0.41], TRAJ["rc"], accuracy=TRAJ["accuracy"], types=types, trainable=True, ex_pairs=pairs)
    real, rec, excl = terms["coulomb_real"], terms["coulomb_recip"], terms["coulomb_excl"]
    stack = Stack({"pair": PairPotentials(system, mdl, cutoff=TRAJ["rc"], index_tuple=(ox, ox)),
                   "bond": BondPotentials(system, torch.as_tensor(bonds), TRAJ["k_bond"], TRAJ["ro"]),
                   "angle": AnglePotentials(system, torch.as_tensor(angles), TRAJ["k_angle"], TRAJ["theta0"]), **terms})
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
    assert gth.numel() == 8 and real.charges.grad is not None and rec.charges is real.charges and excl.charges is real.charges
    want = gth[2:4] + gth[4:6] + gth[6:8]                       # the oracle's three terms each carry the charges
    close(real.charges.grad, want, 5e-3, 5e-4 * float(want.abs().max()), "dL/dcharges")


# ------------------------------------------------------------------------------------------------ 9: alpha independence, identity
def _total_vs_float64(x32, cell32, q32, pairs, rc, real, rec, excl):
    """(U on the device, U in float64, allowed difference): the three kernels' tolerances, 64 ulp * A for the two pair kernels
    and test_gpu_ewald's TOL * A for the reciprocal one."""
    lst = R.half_list(x32, cell32, rc, ex_pairs=pairs if real.ex_pairs is not None else None)
    assert lst[3] > 1e-4, "a pair sits within float32 rounding of the cutoff"
    r1 = R.evaluate(x32, q32, lst, cell32, R.consts(rc, real.alpha, "none", real.conversion))
    r2 = E.evaluate(x32, q32, rec.table().n_host.numpy(), cell32.astype(np.float64), rec.alpha, rec.conversion)
    x = T(x32, DEV)
    U, U64, tol = float(real(x)) + float(rec(x)), float(r1["U"] + r2["U"]), TOL * float(r1["A_U"]) + TOL_RECIP * float(r2["A_U"])
    if excl is not None:
        r3 = X.evaluate(x32, q32, pairs, None, cell32.astype(np.float64), excl.alpha, excl.conversion)
        U, U64, tol = U + float(excl(x)), U64 + float(r3["U"]), tol + TOL * float(r3["A_U"])
    return U, U64, tol


def test_alpha_independence_and_the_exclusion_identity_on_the_device():
    """water27, rc = 4.5, conversion = 1, at (alpha, k_cutoff) = (0.7540, 5.117) and (0.8445, 6.419): the device totals with
    exclusions differ by no more than the float64 totals do (2.6e-6) plus both evaluations' kernel tolerances; and the device
    total equals the float64 value of  U_real(unmasked) + U_rec - sum_P q_i q_j / r_ij  within them."""
    from mdgrad_amd.interface import CoulombPotentials, EwaldReciprocal
    x32, cell32, q32, _, pairs, _, _ = X.water27()
    out = []
    for alpha, kc in ((0.7540, 5.117), (0.8445, 6.419)):
        _, real, rec, excl = _members(x32, cell32, q32, pairs, 4.5, alpha, kc, conversion=1.0)
        out.append(_total_vs_float64(x32, cell32, q32, pairs, 4.5, real, rec, excl))
    (U1, V1, t1), (U2, V2, t2) = out
    print("device %.7f %.7f  float64 %.7f %.7f  tolerances %.2e %.2e" % (U1, U2, V1, V2, t1, t2))
    assert abs(V1 - V2) <= 1e-5, "the float64 sums themselves depend on alpha: cutoffs too short"
    assert abs(U1 - U2) <= abs(V1 - V2) + t1 + t2
    assert abs(U1 - V1) <= t1 and abs(U2 - V2) <= t2
    # the identity: the unmasked real-space sum and the reciprocal sum in float64, minus the bare Coulomb energy of the pairs
    x, q = torch.tensor(x32).double(), torch.tensor(q32).double()
    d = X.reimage(x[pairs[:, 0]] - x[pairs[:, 1]], cell32.astype(np.float64))
    bare = float((q[pairs[:, 0]] * q[pairs[:, 1]] / d.pow(2).sum(-1).sqrt()).sum())
    system = mk_system(x32, cell32)
    plain = CoulombPotentials(system, q32, 4.5, alpha=0.7540, shift="none", conversion=1.0)
    Up, Vp, tp = _total_vs_float64(x32, cell32, q32, pairs, 4.5, plain, EwaldReciprocal(system, plain, k_cutoff=5.117), None)
    print("identity: device with exclusions %.7f, float64 unmasked - bare %.7f, device unmasked - bare %.7f" % (U1, Vp - bare, Up - bare))
    assert abs(V1 - (Vp - bare)) <= 1e-10
    assert abs(U1 - (Vp - bare)) <= t1 + 1e-10
    assert abs(U1 - (Up - bare)) <= t1 + tp + 1e-10


# ------------------------------------------------------------------------------------------------ 10: torch op
def test_torch_op_equals_ctypes_path_and_rejects_bad_input():
    from mdgrad_amd import _lib, _torch_ops, ops
    ns = _torch_ops.get()
    assert ns is not None
    base, cell32, _, types, pairs, _, _ = X.water27()
    x32 = np.concatenate([base, base + F32(0.05), base - F32(0.07)]).astype(F32)
    _, real, _, excl = _members(base, cell32, np.array([-0.82, 0.41], dtype=F32), pairs, 4.5, 0.754, scale=0.5, n_rep=3, types=types,
                                conversion=1.9)
    tb = excl.table()
    L = [float(v) for v in tb.lengths]
    x, w, q = T(x32, DEV), torch.randn(243, 3, device=DEV), excl._q_atom()
    args = (tb.row_ptr, tb.col, tb.scl, q, tb.alpha, tb.conversion)
    a = ops.ewald_excl_eval(tb, x, q, energy=True, grad=True, want_pot=True)
    U, g, hw, pot, potw = ns.ewald_excl_eval(x, 3, L, *args, None, True, True)
    assert torch.equal(U, a["energy"]) and torch.equal(g, a["grad"]) and torch.equal(pot, a["pot"]) and hw.numel() == potw.numel() == 0
    b = ops.ewald_excl_eval(tb, x, q, w=w, energy=False, grad=True, want_pot=True)
    U, g, hw, pot, potw = ns.ewald_excl_eval(x, 3, L, *args, w, False, True)
    assert torch.equal(g, b["grad"]) and torch.equal(hw, b["hw"]) and torch.equal(potw, b["potw"]) and U.numel() == pot.numel() == 0
    big, neg, dec = tb.col.clone(), tb.col.clone(), tb.row_ptr.clone()
    big[3], neg[5], dec[4] = 81, -1, 0
    rp, col, scl = tb.row_ptr, tb.col, tb.scl

    def call(xx=x, n_rep=3, cl=L, r=rp, c=col, s=scl, qq=q, al=tb.alpha, ww=None):
        return ns.ewald_excl_eval(xx, n_rep, cl, r, c, s, qq, al, 1.0, ww, True, False)
    bad = [lambda: call(xx=x.double()), lambda: call(xx=x.cpu()), lambda: call(qq=q.cpu()), lambda: call(qq=q.double()),
           lambda: call(qq=q[:5].contiguous()), lambda: call(n_rep=5), lambda: call(n_rep=0), lambda: call(cl=L[:2]),
           lambda: call(cl=[9.3, 0.0, 9.3]), lambda: call(al=0.0), lambda: call(r=rp.cpu()), lambda: call(r=rp.long()),
           lambda: call(r=rp[:-1].contiguous()), lambda: call(r=dec), lambda: call(c=col.cpu()), lambda: call(c=col.long()),
           lambda: call(c=col[:-1].contiguous()), lambda: call(c=big), lambda: call(c=neg), lambda: call(s=scl.double()),
           lambda: call(s=scl[:-1].contiguous()), lambda: call(ww=w[:5].contiguous()), lambda: call(ww=w.cpu())]
    assert call()[0].numel() == 1
    for n, fn in enumerate(bad):
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
            pytest.fail("bad input %d was accepted" % n)
    # the C entry point itself answers bad arguments with an error code
    import ctypes
    lib = _lib.load()
    part = torch.empty(int(lib.mdg_ewald_excl_partial_size(3, 81)), device=DEV, dtype=torch.float64)
    e = torch.empty(1, device=DEV)
    p = _lib.ptr

    def ccall(n_rep=3, n_atoms=81, cl=tb.cell_len, alpha=tb.alpha, wp=None, hw=None, energy=e, partial=part, r=rp):
        return lib.mdg_ewald_excl_eval(p(x), n_rep, n_atoms, cl, p(r), p(col), p(scl), p(q), alpha, 1.0, p(wp), p(energy),
                                       None, p(hw), None, None, p(partial), 1.0, 0, _lib.stream_ptr(x.device))
    assert ccall() == 0
    assert ccall(n_rep=0) == -1 and ccall(n_atoms=0) == -1 and ccall(alpha=0.0) == -1 and b"alpha" in lib.mdg_last_error()
    assert ccall(cl=(ctypes.c_float * 3)(9.3, -1.0, 9.3)) == -1 and b"cell lengths" in lib.mdg_last_error()
    assert ccall(hw=torch.empty(243, 3, device=DEV)) == -1 and ccall(wp=w) == -1 and ccall(energy=None) == -1
    assert ccall(partial=None) == -1 and ccall(r=None) == -1
    torch.cuda.synchronize()
