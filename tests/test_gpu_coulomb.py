"""K20: the damped shifted-force Coulomb sum with per-atom charges (CoulombPotentials, mdg_coulomb_eval, csrc/coulomb.hip)
against the float64 definitions of tests/coulomb_ref.py (pinned to the reference's goldens E1 / E2 by
tests/test_coulomb_host.py), the goldens themselves and, in a Stack with a pair term, the CPU oracle's trajectory and adjoint.

Tolerance of every kernel-vs-float64 comparison: 64 * 2^-24 * A per component, A = the float64 sum of the absolute pair
contributions to that component (coulomb_ref.evaluate): a few ulp per pair from erfcf / expf / the reciprocal square root,
plus at most a few dozen sequential float32 additions per lane.  `within` prints the largest observed err / (2^-24 A); on an
MI355X the largest over all cases of this file were U 0.91, dU/dx 7.86, pot 12.84, H.w 13.07, potw 6.19."""
import math

import numpy as np
import pytest
import torch

import coulomb_ref as R
import oracle as O
from conftest import load_golden
from test_gpu_parity import T, close, mk_system, DEV, oracle_run

pytestmark = pytest.mark.gpu
F32 = np.float32
ULP = 2.0 ** -24
TOL = 64 * ULP
SHIFTS = ("none", "potential", "force")


def within(got, want, A, what, extra=0.0):
    """|got - want| <= TOL * A (+ extra * A) per component; returns (and prints) the largest err / (2^-24 A)."""
    got = got.detach().cpu().double().reshape(-1)
    want, A = torch.as_tensor(want).detach().double().reshape(-1), torch.as_tensor(A).detach().double().reshape(-1)
    assert got.shape == want.shape == A.shape, "%s: shapes %s %s %s" % (what, got.shape, want.shape, A.shape)
    assert bool(torch.isfinite(got).all()), what + ": non-finite"
    err = (got - want).abs()
    ratio = float((err[A > 0] / (ULP * A[A > 0])).max()) if bool((A > 0).any()) else 0.0
    print("%-60s max err / (2^-24 A) = %6.2f  (allowed 64)" % (what, ratio))
    bad = err > (TOL + extra) * A
    assert not bool(bad.any()), "%s: err %.3e at A = %.3e, ratio %.1f > 64" % (what, float(err[bad].max()), float(A[bad].min()), ratio)
    return ratio


def _module(x32, cell32, charges, rc, **kw):
    from mdgrad_amd.interface import CoulombPotentials
    return CoulombPotentials(mk_system(x32, cell32), charges, rc, **kw)


def _check_all_outputs(x32, cell32, q32, rc, alpha, shift, tag, index_tuple=None, ex_pairs=None, seed=0):
    """U, dU/dx, H w, pot and potw of one launch each against the explicit float64 pair sums."""
    from mdgrad_amd import ops
    mod = _module(x32, cell32, q32, rc, alpha=alpha, shift=shift, index_tuple=index_tuple, ex_pairs=ex_pairs)
    k = R.consts(rc, alpha, shift, mod.conversion)
    lst = R.half_list(x32, cell32, rc, index_tuple, ex_pairs)
    assert lst[3] > 1e-4, "a pair sits within float32 rounding of the cutoff: choose another seed"
    w32 = np.random.default_rng(seed + 17).normal(0, 1, x32.shape).astype(F32)
    ref = R.evaluate(x32, q32, lst, cell32, k, w=w32)
    x, w = T(x32, DEV), T(w32, DEV)
    o1 = ops.coulomb_eval(mod._ell, x, mod._q_atom(), mod._consts, energy=True, grad=True, want_pot=True)
    o2 = ops.coulomb_eval(mod._ell, x, mod._q_atom(), mod._consts, w=w, energy=False, grad=True, want_pot=True)
    tag = "%s %s alpha=%.1f " % (tag, shift, alpha)
    rs = [within(o1["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + "U"),
          within(o1["grad"], ref["grad"], ref["A_grad"], tag + "dU/dx"),
          within(o1["pot"], ref["pot"], ref["A_pot"], tag + "pot"),
          within(o2["hw"], ref["hw"], ref["A_hw"], tag + "H.w"),
          within(o2["potw"], ref["potw"], ref["A_potw"], tag + "potw")]
    assert torch.equal(o1["grad"], o2["grad"]) and o2["pot"] is None and o1["potw"] is None
    e0 = ops.coulomb_eval(mod._ell, x, mod._q_atom(), mod._consts, energy=True, grad=False)          # LEVEL 0
    within(e0["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + "U (energy-only launch)")
    return mod, ref, o1, o2, max(rs)


def _jittered_nacl64(seed=64, sigma=0.25):
    pos, q, L = R.nacl(2)
    rng = np.random.default_rng(seed)
    x32 = np.mod(pos + rng.normal(0, sigma, pos.shape), L).astype(F32)
    return x32, np.array([L, L, L], dtype=F32), q.astype(F32)


def _gas37():
    box = np.array([7.0, 8.0, 9.0], dtype=F32)
    x32 = R.seeded_gas(37, box, 0.8, seed=37).astype(F32)
    rng = np.random.default_rng(370)
    q32 = rng.normal(0, 1, 37).astype(F32)
    q32[5] = 0.0
    ex = np.array([[0, 1], [2, 9], [3, 4], [10, 30], [11, 12], [20, 35]])
    it = (list(range(0, 30)), list(range(10, 36)))            # atom 36 is in neither selection: an empty row
    return x32, box, q32, it, ex


# ------------------------------------------------------------------------------------------------ 1: all outputs vs float64
@pytest.mark.parametrize("alpha", [0.0, 0.4])
@pytest.mark.parametrize("shift", SHIFTS)
def test_outputs_vs_float64_jittered_nacl64(shift, alpha):
    """64 NaCl ions jittered by sigma = 0.25 in L = 11.28, rc = 5.0 (rows of ~45 neighbours, one lane group per atom)."""
    x32, cell32, q32 = _jittered_nacl64()
    _check_all_outputs(x32, cell32, q32, 5.0, alpha, shift, "nacl64")


@pytest.mark.parametrize("alpha", [0.0, 0.4])
@pytest.mark.parametrize("shift", SHIFTS)
def test_outputs_vs_float64_gas37_with_masks_a_zero_charge_and_an_empty_row(shift, alpha):
    """37 seeded atoms (minimum separation 0.8) in a 7 x 8 x 9 cell, signed charges and one zero charge, 6 ex_pairs and an
    index_tuple that leaves atom 36 without neighbours: its outputs are exactly zero; 37 is no multiple of the 4 atoms of a
    workgroup."""
    x32, box, q32, it, ex = _gas37()
    mod, ref, o1, o2, _ = _check_all_outputs(x32, box, q32, 3.2, alpha, shift, "gas37", index_tuple=it, ex_pairs=ex)
    assert float(ref["A_pot"][36]) == 0.0 and int(mod._ell.cnt[36]) == 0
    for o in (o1["grad"][36], o1["pot"][36], o2["hw"][36], o2["potw"][36]):
        assert float(o.abs().max()) == 0.0
    assert float(o1["grad"][5].abs().max()) == 0.0 and float(o1["pot"][5].abs()) > 0.0, "a zero charge feels no force but has a potential"


@pytest.mark.parametrize("alpha", [0.0, 0.4])
@pytest.mark.parametrize("shift", SHIFTS)
def test_outputs_vs_float64_triclinic64(shift, alpha):
    g = load_golden("nbr_tric64")
    q32 = np.random.default_rng(640).normal(0, 1, 64).astype(F32)
    _check_all_outputs(g["xyz"].astype(F32), g["cell"].astype(F32), q32, float(g["cutoff"]), alpha, shift, "tric64")


# ------------------------------------------------------------------------------------------------ 2: goldens E1 / E2
@pytest.mark.parametrize("name", ["coulomb_e1", "coulomb_e2"])
def test_goldens_through_the_kernel(name):
    """shift="none", alpha=0 against -U_ref and +dU_ref/dx (= the force) of the reference's Electrostatics.  The goldens are
    float32 runs of the reference, pinned to float64 within 1e-6 A by tests/test_coulomb_host.py: allowed 64 * 2^-24 A + 1e-6 A."""
    g = load_golden(name)
    it = (g["idx_a"].tolist(), g["idx_b"].tolist()) if "idx_a" in g else None
    ex = g["ex_pairs"].astype(np.int64) if "ex_pairs" in g else None
    n, rc = g["xyz"].shape[0], float(g["cutoff"])
    for tag, it_, ex_ in [("a", None if name == "coulomb_e1" else it, None), ("b", it, ex)]:
        qv = np.full(n, float(g["q_" + tag]), dtype=F32)
        mod = _module(g["xyz"], g["cell"], qv, rc, shift="none", index_tuple=it_, ex_pairs=ex_)
        lst = R.half_list(g["xyz"], g["cell"], rc, it_, ex_)
        assert lst[3] > 1e-4
        ref = R.evaluate(g["xyz"], qv, lst, g["cell"], R.consts(rc, 0.0, "none", mod.conversion))
        x = T(g["xyz"], DEV)
        within(mod(x).reshape(1), g["energy_" + tag], ref["A_U"].reshape(1), name + tag + " U vs golden", extra=1e-6)
        within(mod.force(x), g["grad_" + tag], ref["A_grad"], name + tag + " force vs golden", extra=1e-6)


# ------------------------------------------------------------------------------------------------ 3: perfect lattice
def test_perfect_nacl64_madelung_and_zero_forces():
    """Perfect 64-ion rock salt, "force", alpha = 0.4, rc = 5.0: the Madelung constant within 0.005 (float64 gives 1.74668)
    and forces that vanish within the tolerance."""
    pos, q, L = R.nacl(2)
    x32, cell32, q32 = pos.astype(F32), np.array([L, L, L], dtype=F32), q.astype(F32)
    mod, ref, o1, _, _ = _check_all_outputs(x32, cell32, q32, 5.0, 0.4, "force", "perfect nacl64")
    M64 = R.madelung(ref["U"], 64, 2.82, mod.conversion)
    M = R.madelung(o1["energy"][0], 64, 2.82, mod.conversion)
    assert abs(M64 - 1.74668) <= 2e-5 and abs(M - R.MADELUNG_NACL) <= 0.005, (M, M64)
    assert float(ref["grad"].abs().max()) <= 1e-5 * float(ref["A_grad"].max()), "float64 forces vanish (float32 box length)"
    assert bool((o1["grad"].cpu().double().abs() <= TOL * ref["A_grad"] + ref["grad"].abs()).all())


# ------------------------------------------------------------------------------------------------ 4: charge gradients
def _replicas24():
    box = np.array([8.0, 8.0, 8.0], dtype=F32)
    base = R.seeded_gas(24, box, 1.3, seed=24)
    rng = np.random.default_rng(240)
    x32 = np.concatenate([np.mod(base + rng.normal(0, 0.1, base.shape), box) for _ in range(3)]).astype(F32)
    types = (np.arange(24) % 2).astype(np.int64)
    return base, box, x32, types


@pytest.mark.parametrize("per_type", [False, True], ids=["per_atom", "per_type"])
def test_charge_gradients_on_three_replicas_vs_float64_autograd(per_type):
    """System.replicate(3) of a 24-ion cell with different jitters: dU/dcharges and d(w.dU/dx)/dcharges per atom (24 slots,
    each summed over the replicas) and per type (2 slots) against float64 autograd of coulomb_ref.energy.  Allowed per slot:
    64 * 2^-24 * conversion * sum over the slot's atoms of (A_pot + 2 s |q|), resp. A_potw.  Two calls are bitwise equal, and a
    permutation of the replicas permutes the per-atom outputs bitwise."""
    from mdgrad_amd import ops
    from mdgrad_amd.interface import CoulombPotentials
    base, box, x32, types = _replicas24()
    rc, alpha = 3.5, 0.3
    rng = np.random.default_rng(241)
    c32 = (np.array([0.9, -1.1]) if per_type else np.where(types == 0, 1.0, -1.0) * rng.uniform(0.5, 1.5, 24)).astype(F32)
    system = mk_system(base, box).replicate(3)
    mod = CoulombPotentials(system, c32, rc, alpha=alpha, types=types if per_type else None, trainable=True)
    assert mod.n_slots == (2 if per_type else 24) and mod._q_atom().shape == (72,)
    k = R.consts(rc, alpha, "force", mod.conversion)
    lst = R.half_list(x32, box, rc, group=24)
    assert lst[3] > 1e-4 and int((lst[0] // 24 != lst[1] // 24).sum()) == 0
    w32 = rng.normal(0, 1, x32.shape).astype(F32)
    ty = types if per_type else None
    c64 = torch.tensor(c32).double().requires_grad_(True)
    x64 = torch.tensor(x32).double().requires_grad_(True)
    U = R.energy(x64, R.expand(c64, ty, 3), lst, box, k)
    gx, gc = torch.autograd.grad(U, (x64, c64), create_graph=True)
    (hc,) = torch.autograd.grad((gx * torch.tensor(w32).double()).sum(), c64)
    ref = R.evaluate(x32, R.expand(torch.tensor(c32), ty, 3), lst, box, k, w=w32)
    slot = torch.as_tensor(types if per_type else np.arange(24)).repeat(3)
    qa = R.expand(torch.tensor(c32).double(), ty, 3)

    def per_slot(v):
        return torch.zeros(mod.n_slots, dtype=torch.float64).index_add_(0, slot, v)
    A_u = mod.conversion * per_slot(ref["A_pot"] + 2 * k["s"] * qa.abs())
    A_w = mod.conversion * per_slot(ref["A_potw"])
    x, w = T(x32, DEV).requires_grad_(True), T(w32, DEV)
    mod._reset_topology(x.detach())                              # (the module was built at the unjittered positions)
    g1x, g1c = torch.autograd.grad(mod(x), (x, mod.charges), create_graph=True)
    (h1c,) = torch.autograd.grad((g1x * w).sum(), mod.charges)
    within(g1c, gc.detach(), A_u, "dU/dcharges")
    within(h1c, hc, A_w, "d(w.dU/dx)/dcharges")
    within(g1x, gx.detach(), ref["A_grad"], "dU/dx on three replicas")
    F, dq, gth = mod.force_vjp(x.detach(), w)
    within(-gth[0], hc, A_w, "force_vjp charge part")
    # bitwise reproducible
    F2, dq2, gth2 = mod.force_vjp(x.detach(), w)
    g2x, g2c = torch.autograd.grad(mod(x), (x, mod.charges))
    assert torch.equal(F, F2) and torch.equal(dq, dq2) and torch.equal(gth[0], gth2[0])
    assert torch.equal(g1x.detach(), g2x) and torch.equal(g1c.detach(), g2c)
    # replicas (2, 0, 1): per-atom outputs move with their replica, bit for bit
    perm = torch.cat([torch.arange(24) + 24 * r for r in (2, 0, 1)]).to(DEV)
    xd = x.detach()
    mod._reset_topology(xd[perm].contiguous())
    op = ops.coulomb_eval(mod._ell, xd[perm].contiguous(), mod._q_atom(), mod._consts, w=w[perm].contiguous(), energy=False, want_pot=True)
    mod._reset_topology(xd)
    oo = ops.coulomb_eval(mod._ell, xd, mod._q_atom(), mod._consts, w=w, energy=False, want_pot=True)
    for key in ("grad", "hw", "potw"):
        assert torch.equal(op[key], oo[key][perm]), key


# ------------------------------------------------------------------------------------------------ 5: autograd
def test_autograd_backward_and_double_backward_equal_force_vjp():
    x32, cell32, q32 = _jittered_nacl64(seed=70)
    types = (q32 < 0).astype(np.int64)
    mod = _module(x32, cell32, np.array([1.0, -1.0], dtype=F32), 5.0, alpha=0.4, types=types, trainable=True)
    k = R.consts(5.0, 0.4, "force", mod.conversion)
    lst = R.half_list(x32, cell32, 5.0)
    assert lst[3] > 1e-4
    ref = R.evaluate(x32, q32, lst, cell32, k)
    x = T(x32, DEV).requires_grad_(True)
    U = mod(x)
    U.backward()
    within(x.grad, ref["grad"], ref["A_grad"], "backward of model(xyz) in xyz")
    c64 = torch.tensor([1.0, -1.0], dtype=torch.float64, requires_grad=True)
    (gc,) = torch.autograd.grad(R.energy(torch.tensor(x32).double(), R.expand(c64, types), lst, cell32, k), c64)
    A_c = mod.conversion * torch.zeros(2, dtype=torch.float64).index_add_(0, torch.as_tensor(types), ref["A_pot"] + 2 * k["s"])
    within(mod.charges.grad, gc, A_c, "backward of model(xyz) in charges")
    w = torch.randn(64, 3, device=DEV)
    x2 = T(x32, DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(mod(x2), x2, create_graph=True)
    hw, hc = torch.autograd.grad((g * w).sum(), (x2, mod.charges))
    F, dq, gth = mod.force_vjp(x2.detach(), w)
    assert torch.equal(F, -g.detach()) and torch.equal(dq, -hw) and torch.equal(gth[0], -hc)
    frozen = _module(x32, cell32, q32, 5.0, alpha=0.4)
    assert frozen.force_vjp(x2.detach(), w)[2] == [] and frozen.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    assert mod.force_vjp(x2.detach(), w, want_theta=False)[2] is None


# ------------------------------------------------------------------------------------------------ 6: into / scale / accum
def test_stack_sums_equal_the_members_separate_results():
    """Stack({"lj", "coul"}).force and .force_vjp (the Coulomb launch adds onto the pair term's buffers) against the sum of the
    members' separate results, to 2^-22 of the largest entry; the same for `accum` against the list return."""
    from mdgrad_amd import ops
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    x32, cell32, q32 = _jittered_nacl64(seed=66)
    system = mk_system(x32, cell32)
    from mdgrad_amd.interface import CoulombPotentials
    lj = PairPotentials(system, P.LJFamily(2.0, 0.1), cutoff=5.0)
    coul = CoulombPotentials(system, q32, 5.0, alpha=0.3, trainable=True)
    stack = Stack({"lj": lj, "coul": coul})
    assert stack.supports_force_vjp() and stack.supports_static_topology()
    x, w = T(x32, DEV), torch.randn(64, 3, device=DEV)
    stack._reset_topology(x)
    assert lj._ell is coul._ell, "one search for both members"

    def same(a, b, what):
        assert float((a - b).abs().max()) <= 2.0 ** -22 * float(b.abs().max()), what
    same(stack.force(x), lj.force(x) + coul.force(x), "force")
    F, dq, gth = stack.force_vjp(x, w)
    f1, d1, g1 = lj.force_vjp(x, w)
    f2, d2, g2 = coul.force_vjp(x, w)
    same(F, f1 + f2, "force (vjp)")
    same(dq, d1 + d2, "d(w.F)/dx")
    params = list(stack.parameters())
    assert len(gth) == len(params) == 3
    by_id = {id(p): v for p, v in zip(list(lj.parameters()) + list(coul.parameters()), g1 + g2)}
    for p, v in zip(params, gth):
        same(v, by_id[id(p)], "parameter part")
    acc = ops.ThetaAccum(params)
    acc.flat.fill_(0.25)
    assert stack.force_vjp(x, w, accum=acc)[2] is None
    for v, want in zip(acc.views(), gth):
        assert float((v - 0.25 - want).abs().max()) <= 2.0 ** -22 * max(float(want.abs().max()), 0.25), "accum vs list"
    F0, D0 = torch.randn_like(x), torch.randn_like(x)
    F1, D1, _ = coul.force_vjp(x, w, into=(F0.clone(), D0.clone()))
    same(F1 - F0, f2, "force added onto a buffer")
    same(D1 - D0, d2, "d(w.F)/dx added onto a buffer")


# ------------------------------------------------------------------------------------------------ 7: skin list
def test_evaluation_on_a_list_searched_with_a_skin_equals_a_fresh_exact_list():
    from mdgrad_amd import _lib, ops
    x32, cell32, q32 = _jittered_nacl64(seed=67)
    rc, skin = 5.0, 0.4
    mod = _module(x32, cell32, q32, rc, alpha=0.4)
    cs = _lib.make_cell(cell32)
    x0 = T(x32, DEV)
    longest = int(ops.build_ell(x0, cs, rc + skin).cnt.max())
    vl = ops.VerletList(64, 64, cs, rc, skin, None, min(63, (longest + 15) // 8 * 8), 4096, DEV)
    need = torch.zeros(2, dtype=torch.int32, device=DEV)
    vl.rebuild(x0, need)
    rng = np.random.default_rng(670)
    step = rng.normal(0, 1, (64, 3))
    step = 0.18 * step / np.linalg.norm(step, axis=1)[:, None] * rng.uniform(0.3, 1.0, (64, 1))      # |move| < skin / 2
    x1_32 = (x32 + step).astype(F32)
    x1 = T(x1_32, DEV)
    vl.rebuild(x1, need)
    assert vl.builds() == 1 and need.tolist()[0] <= vl.max_nbr
    exact = ops.build_ell(x1, cs, rc)
    assert int(vl.cnt.sum()) > int(exact.cnt.sum()), "the stored list carries the skin's extra candidates"
    lst = R.half_list(x1_32, cell32, rc)
    assert lst[3] > 1e-4 and 2 * lst[0].numel() == int(exact.cnt.sum())
    w32 = rng.normal(0, 1, (64, 3)).astype(F32)
    ref = R.evaluate(x1_32, q32, lst, cell32, R.consts(rc, 0.4, "force", mod.conversion), w=w32)
    w = T(w32, DEV)
    for kw, keys in ((dict(energy=True), ("energy", "grad", "pot")), (dict(w=w, energy=False), ("grad", "hw", "potw"))):
        a = ops.coulomb_eval(vl.ell, x1, mod._q_atom(), mod._consts, want_pot=True, **kw)
        b = ops.coulomb_eval(exact, x1, mod._q_atom(), mod._consts, want_pot=True, **kw)
        for key in keys:
            A = {"energy": ref["A_U"].reshape(1), "grad": ref["A_grad"], "pot": ref["A_pot"], "hw": ref["A_hw"], "potw": ref["A_potw"]}[key]
            within(a[key], b[key].cpu(), A, "skin list vs exact list: " + key)
    within(a["hw"], ref["hw"], ref["A_hw"], "skin list vs float64: H.w")


# ------------------------------------------------------------------------------------------------ 8: trajectory + adjoint
_oracle_cache = {}
TRAJ = dict(sigma=2.0, eps=0.1, rc=5.0, alpha=0.3, T=0.3, Q=20.0, chains=3, dt=0.005, mass=10.0, nbins=32, r_range=(1.5, 5.0))


def traj_inputs():
    x32, cell32, q32 = _jittered_nacl64(seed=71, sigma=0.15)
    vel = np.random.default_rng(680).normal(0, math.sqrt(TRAJ["T"] / TRAJ["mass"]), x32.shape).astype(F32)
    return x32, cell32, (q32 < 0).astype(np.int64), vel, np.full(64, TRAJ["mass"], dtype=F32)


def oracle_traj(t):
    if "run" not in _oracle_cache:
        x32, cell32, types, vel, mass = traj_inputs()
        cell = T(cell32)
        terms = [O.PairTerm("lj", torch.tensor([TRAJ["sigma"], TRAJ["eps"]]), TRAJ["rc"], cell, p=12, q=6, c=1),
                 R.CoulombTerm(np.array([1.0, -1.0]), TRAJ["rc"], cell32, alpha=TRAJ["alpha"], types=types)]

        def loss_fn(Ls):
            _, _, gr = O.rdf_oracle(Ls[1][::2], cell, TRAJ["nbins"], TRAJ["r_range"])
            return gr.pow(2).mean() + Ls[0][-1].pow(2).mean() + 0.0 * Ls[2][-1].sum()
        _oracle_cache["run"] = oracle_run(x32, cell32, vel, mass, terms, TRAJ["T"], TRAJ["Q"], TRAJ["chains"], t, loss_fn)
    return _oracle_cache["run"]


@pytest.mark.parametrize("graphs_on", [True, False], ids=["graph_replay", "eager"])
def test_coulomb_term_in_a_stack_trajectory_and_adjoint_vs_oracle(graphs_on):
    """Stack(LJFamily pair + CoulombPotentials with per-type trainable charges) on 64 jittered NaCl ions: 10 NHC steps through
    odeint_adjoint, the loss on rdf of q_t[::2] plus v_t[-1]^2 -- trajectories, adjoint of y0, dL/d(sigma, epsilon) and
    dL/dcharges against the oracle with coulomb_ref.CoulombTerm appended.  The stack stays on the analytic adjoint (force_vjp)
    and HIP-graph replay although the charges require grad.  Tolerances: those of
    test_dihedral_term_in_a_stack_trajectory_and_adjoint_vs_oracle (the project's for this oracle and horizon).
    Observed on an MI355X (MDG_TEST_REPORT; graph replay and eager alike), observed / allowed at the worst entry: q_t 9.3e-10 /
    2.0e-05, v_t 1.5e-08 / 2.2e-04, pv_t 2.1e-07 / 5.3e-04, adj v0 1.3e-09 / 1.6e-05, adj q0 5.4e-08 / 2.9e-04, adj pv0 8.0e-13 /
    2.7e-07, dL/d(sigma, epsilon) 1.5e-11 / 4.8e-07, dL/dcharges 1.8e-11 / 2.1e-07.  (On the CPU the oracle's float32 run is
    2.4e-06 / 8.3e-08 / 1.3e-07 off its float64 run in q_t / v_t / pv_t.)"""
    from mdgrad_amd import graphs
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import CoulombPotentials, PairPotentials, Stack
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.sovlers import odeint_adjoint
    x32, cell32, types, vel, mass = traj_inputs()
    system = mk_system(x32, cell32, vel, mass)
    mdl = P.LJFamily(TRAJ["sigma"], TRAJ["eps"])
    coul = CoulombPotentials(system, [1.0, -1.0], TRAJ["rc"], alpha=TRAJ["alpha"], types=types, trainable=True)
    stack = Stack({"pair": PairPotentials(system, mdl, cutoff=TRAJ["rc"]), "coul": coul})
    integ = NoseHooverChain(stack, system, T=TRAJ["T"], num_chains=TRAJ["chains"], Q=TRAJ["Q"], adjoint=True).to(DEV)
    assert integ.fused_spec("NH_verlet") is None, "a Coulomb member keeps the stack off the fused trajectory kernels"
    assert integ.model.supports_force_vjp() and integ.supports_rhs_vjp(), "the term must not push the stack onto the autograd branch"
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
    traj, lam, gth = oracle_traj(t)
    close(q_t, traj[1], 0, 2e-5, "q_t")
    close(v_t, traj[0], 1e-3, 1e-4 * float(traj[0].abs().max()), "v_t")
    close(pv_t, traj[2], 2e-3, 1e-5, "pv_t")
    for x, l, nm in zip(y0, lam, ("adj v0", "adj q0", "adj pv0")):
        close(x.grad, l, 5e-3, 2e-3 * float(l.abs().max()) + 1e-9, nm)
    got = torch.stack([mdl.sigma.grad.reshape(()), mdl.epsilon.grad.reshape(())])
    close(got, gth[:2], 5e-3, 5e-4 * float(gth[:2].abs().max()), "dL/d(sigma, epsilon)")
    assert gth.numel() == 4 and coul.charges.grad is not None
    close(coul.charges.grad, gth[2:], 5e-3, 5e-4 * float(gth[2:].abs().max()), "dL/dcharges")


# ------------------------------------------------------------------------------------------------ 9: torch ops
def test_torch_ops_equal_ctypes_path_and_reject_bad_input():
    from mdgrad_amd import _torch_ops, ops
    ns = _torch_ops.get()
    assert ns is not None
    x32, box, q32, it, ex = _gas37()
    mod = _module(x32, box, q32, 3.2, alpha=0.4, index_tuple=it, ex_pairs=ex)
    ell, k = mod._ell, mod._consts
    cell = _torch_ops.cell_args(ell.cell_struct)
    kk = [k.alpha, k.rc, k.c0, k.c1, k.g0, k.alpha2, k.conversion, k.self_s]
    x, w, q = T(x32, DEV), torch.randn(37, 3, device=DEV), mod._q_atom()
    a = ops.coulomb_eval(ell, x, q, k, energy=True, grad=True, want_pot=True)
    U, g, hw, pot, potw = ns.coulomb_eval(x, cell, ell.col, ell.shift, ell.cnt, q, kk, None, True, True)
    assert torch.equal(U, a["energy"]) and torch.equal(g, a["grad"]) and torch.equal(pot, a["pot"]) and hw.numel() == potw.numel() == 0
    b = ops.coulomb_eval(ell, x, q, k, w=w, energy=False, grad=True, want_pot=True)
    U, g, hw, pot, potw = ns.coulomb_eval(x, cell, ell.col, ell.shift, ell.cnt, q, kk, w, False, True)
    assert torch.equal(g, b["grad"]) and torch.equal(hw, b["hw"]) and torch.equal(potw, b["potw"]) and U.numel() == pot.numel() == 0
    types = torch.as_tensor(np.arange(37) % 3, dtype=torch.int32, device=DEV)
    assert torch.equal(ns.coulomb_charge_reduce(a["pot"], types, 37, 3), ops.coulomb_charge_grad(a["pot"], types, 3))
    assert torch.equal(ns.coulomb_charge_reduce(a["pot"], None, 37, 37), a["pot"]), "one replica: the per-atom reduction is the identity"
    want = torch.zeros(3, dtype=torch.float64).index_add_(0, types.cpu().long(), a["pot"].cpu().double())
    close(ops.coulomb_charge_grad(a["pot"], types, 3), want, 0, 64 * ULP * float(a["pot"].abs().sum()), "per-type sums")
    bad = [lambda: ns.coulomb_eval(x.double(), cell, ell.col, ell.shift, ell.cnt, q, kk, None, True, False),
           lambda: ns.coulomb_eval(x.cpu(), cell, ell.col, ell.shift, ell.cnt, q, kk, None, True, False),
           lambda: ns.coulomb_eval(x, cell[:5], ell.col, ell.shift, ell.cnt, q, kk, None, True, False),
           lambda: ns.coulomb_eval(x, cell, ell.col.long(), ell.shift, ell.cnt, q, kk, None, True, False),
           lambda: ns.coulomb_eval(x, cell, ell.col, ell.shift, ell.cnt[:5].contiguous(), q, kk, None, True, False),
           lambda: ns.coulomb_eval(x, cell, ell.col, ell.shift, ell.cnt, q[:5].contiguous(), kk, None, True, False),
           lambda: ns.coulomb_eval(x, cell, ell.col, ell.shift, ell.cnt, q.double(), kk, None, True, False),
           lambda: ns.coulomb_eval(x, cell, ell.col, ell.shift, ell.cnt, q, kk[:7], None, True, False),
           lambda: ns.coulomb_eval(x, cell, ell.col, ell.shift, ell.cnt, q, kk, w[:5].contiguous(), True, False),
           lambda: ns.coulomb_eval(x, cell, ell.col, ell.shift, ell.cnt, q, [-1.0] + kk[1:], None, True, False),
           lambda: ns.coulomb_charge_reduce(a["pot"].double(), types, 37, 3),
           lambda: ns.coulomb_charge_reduce(a["pot"].cpu(), None, 37, 37),
           lambda: ns.coulomb_charge_reduce(a["pot"], types[:5].contiguous(), 37, 3),
           lambda: ns.coulomb_charge_reduce(a["pot"], types.long(), 37, 3),
           lambda: ns.coulomb_charge_reduce(a["pot"], None, 37, 3),
           lambda: ns.coulomb_charge_reduce(a["pot"], types, 5, 3),
           lambda: ns.coulomb_charge_reduce(a["pot"], types, 37, 0)]
    for n, fn in enumerate(bad):
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
            pytest.fail("bad input %d was accepted" % n)
