"""K24: the Sutton-Chen embedded-atom term (SuttonChen, mdg_eam_eval, csrc/eam.hip) against the float64 definition of
tests/eam_ref.py (pinned to an independent loop and to the fcc lattice sums by tests/test_eam_host.py) and, in a trajectory,
against the CPU oracle's adjoint.

Tolerance of every kernel-vs-float64 comparison: K * 2^-24 * A per component with K = 64 (the KTOL of tests/test_gpu_sw.py),
A = the float64 sum of the absolute values of what the kernel adds up (eam_ref.evaluate: the pieces of S_k and S_k' one by one,
the embedding contributions times kappa of the atom whose F' they carry).  `within` prints the largest observed
err / (2^-24 A); on an MI355X the largest over all cases of this file were U 4.28, dU/dx 25.05, H.w 24.75, dU/dtheta 7.05,
d(w.dU/dx)/dtheta 3.80, the sum of the forces 2.00 -- all on the triclinic 64-atom set; Cu-108 alone (both shifts): 0.33, 6.52,
8.56, 2.27, 1.08, 0.04; the 37-atom set 0.57, 5.73, 4.35, 2.46, 0.51; the perfect lattice 0.31 (U), 1.77 (dU/dx).

Why the triclinic set reaches 25, and why K stays 64: it is a random gas whose closest pair sits at r = 0.159 = 0.14 a, so the
sums of those atoms are a single term (a/r)^9 ~ 4e7, and its derivative carries (a/r)^10 / a: the one or two ulp that sqrtf
and the division leave in r and 1/r come back nine- and tenfold.  That is the conditioning of a power law at float32 inputs,
not a cancellation in the kernel, and A (which counts the term once) need not know about it.  K is not raised."""
import math

import numpy as np
import pytest
import torch

import coulomb_ref as CR
import eam_ref as R
import oracle as O
from conftest import load_golden
from test_gpu_parity import T, close, mk_system, DEV, oracle_run
from test_gpu_sw import _gas37 as _sw_gas37

pytestmark = pytest.mark.gpu
F32 = np.float32
ULP = 2.0 ** -24
KTOL = 64
TOL = KTOL * ULP
CU = R.PUBLISHED["copper"]
RC = 5.2
MARGIN = 1e-5            # no candidate pair closer than this to rc: float32 r = sqrtf(d2) selects the pairs of the float64 list


def within(got, want, A, what):
    """|got - want| <= TOL * A per component; returns (and prints) the largest err / (2^-24 A)."""
    got = got.detach().cpu().double().reshape(-1)
    want, A = torch.as_tensor(want).detach().double().reshape(-1), torch.as_tensor(A).detach().double().reshape(-1)
    assert got.shape == want.shape == A.shape, "%s: shapes %s %s %s" % (what, got.shape, want.shape, A.shape)
    assert bool(torch.isfinite(got).all()), what + ": non-finite"
    err = (got - want).abs()
    ratio = float((err[A > 0] / (ULP * A[A > 0])).max()) if bool((A > 0).any()) else 0.0
    print("%-64s max err / (2^-24 A) = %6.2f  (allowed %d)" % (what, ratio, KTOL))
    bad = err > TOL * A
    assert not bool(bad.any()), "%s: err %.3e at A = %.3e, ratio %.1f > %d" % (what, float(err[bad].max()), float(A[bad].min()), ratio, KTOL)
    return ratio


def _module(x32, cell32, theta=CU, rc=RC, shift="force", system=None, **kw):
    from mdgrad_amd.interface import SuttonChen
    eps, a, c, n, m = theta
    return SuttonChen(mk_system(x32, cell32) if system is None else system, eps, a, c, n, m, rc, shift=shift, **kw)


def _theta64(mod):
    """The module's float32 parameters, as the float64 reference sees them."""
    return [float(p.detach()) for p in (mod.epsilon, mod.a, mod.c)]


def _reference(mod, x32, cell32, w32=None, group=None):
    k = R.consts(mod.n, mod.m, mod.cutoff, mod.shift)
    lst = R.pairs(x32, cell32, mod.cutoff, group=group)
    assert lst["margin"] >= MARGIN, "a pair sits on the cutoff: choose another seed"
    return lst, R.evaluate(x32, _theta64(mod), lst, cell32, k, w=w32)


def _eval(mod, x, **kw):
    from mdgrad_amd import ops
    return ops.eam_eval(mod._ell, x, mod._consts, mod._theta(), work=mod._work, **kw)


def _check_all_outputs(x32, cell32, tag, theta=CU, rc=RC, shift="force", group=None, system=None, seed=0):
    """U, dU/dx, H w, dU/dtheta and d(w.dU/dx)/dtheta of one call each against float64; the energy-only call; the sum of the
    forces; LEVEL 1 and LEVEL 2 forces bit for bit."""
    from mdgrad_amd import ops
    mod = _module(x32, cell32, theta, rc, shift, system=system)
    w32 = np.random.default_rng(seed + 17).normal(0, 1, x32.shape).astype(F32)
    lst, ref = _reference(mod, x32, cell32, w32, group)
    x, w = T(x32, DEV), T(w32, DEV)
    mod._reset_topology(x)
    o1 = _eval(mod, x, energy=True, grad=True, want_theta=True)
    o2 = _eval(mod, x, w=w, energy=False, grad=True, want_theta=True)
    o1["dth"], o2["dthw"] = ops.eam_theta_sum(o1["pth"]), ops.eam_theta_sum(o2["pthw"])
    tag += " " + shift + " "
    rs = [within(o1["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + "U"),
          within(o1["grad"], ref["grad"], ref["A_grad"], tag + "dU/dx"),
          within(o2["hw"], ref["hw"], ref["A_hw"], tag + "H.w"),
          within(o1["dth"], ref["dth"], ref["A_dth"], tag + "dU/dtheta"),
          within(o2["dthw"], ref["dthw"], ref["A_dthw"], tag + "d(w.dU/dx)/dtheta")]
    assert torch.equal(o1["grad"], o2["grad"]) and o2["pth"] is None and o1["pthw"] is None
    e0 = _eval(mod, x, energy=True, grad=False)                                                      # LEVEL 0
    within(e0["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + "U (energy-only call)")
    within(o1["grad"].sum(0), torch.zeros(3), ref["A_grad"].sum(0), tag + "sum_i dU/dx_i")
    return mod, lst, ref, o1, o2, max(rs)


def _gas37(rc=RC):
    """test_gpu_sw._gas37 at metal distances (every length times 1.4: a 19.6 x 21 x 22.4 box, minimum separation 2.8): 34 atoms
    in a corner, one atom far from everything (index 33), and two atoms that only see each other (34, 35), put at r = 0.6 rc."""
    x, box = _sw_gas37()
    x, box = x.astype(np.float64) * 1.4, box.astype(np.float64) * 1.4
    x[35] = x[34] + np.array([0.0, 0.0, 0.6 * rc])
    return x.astype(F32), box.astype(F32)


# ------------------------------------------------------------------------------------------------ 1 - 4: outputs vs float64
@pytest.mark.parametrize("shift", ["force", "none"])
def test_outputs_vs_float64_jittered_cu108(shift):
    """3 x 3 x 3 fcc cells of copper (a0 = 3.61) jittered by 0.15 A: rows near 54, the fourth shell straddles rc = 5.2."""
    x32, cell32 = R.jittered_fcc(3, 3.61, 0.15, 108)
    mod, lst, ref, o1, o2, _ = _check_all_outputs(x32, cell32, "cu108", shift=shift)
    rows = lst["rows"]
    assert int(rows.min()) >= 40 and int(rows.max()) >= 54 and abs(float(rows.double().mean()) - 54) < 5


@pytest.mark.parametrize("shift", ["force", "none"])
def test_outputs_vs_float64_gas37_with_an_empty_row_and_an_isolated_pair(shift):
    x32, box = _gas37()
    mod, lst, ref, o1, o2, _ = _check_all_outputs(x32, box, "gas37", shift=shift)
    rows = lst["rows"].tolist()
    assert rows[33] == 0 and rows[34] == rows[35] == 1 and max(rows) >= 8 and 37 % 16 != 0
    assert int(mod._ell.cnt[33]) == 0 and int(mod._ell.cnt[34]) == 1
    for o in (o1["grad"][33], o1["pth"][33], o2["hw"][33], o2["pthw"][33], mod._work[33]):
        assert bool(torch.isfinite(o).all()) and float(o.abs().max()) == 0.0, "the atom with the empty row (rho = 0)"
    assert float(o1["grad"][34].abs().max()) > 0.0 and float(o1["pth"][34, 2]) < 0.0, "one neighbour: a pair and its density"


def test_outputs_vs_float64_triclinic64():
    g = load_golden("nbr_tric64")
    rc = float(g["cutoff"])
    theta = (1.0, rc / 2, CU[2], 9, 6)
    for shift in ("force", "none"):
        mod, lst, ref, o1, o2, _ = _check_all_outputs(g["xyz"].astype(F32), g["cell"].astype(F32), "tric64", theta=theta, rc=rc,
                                                      shift=shift)
    assert int(lst["rows"].max()) > 16, "rows longer than the lanes of an atom"


def test_perfect_fcc_through_the_kernel():
    """Perfect 3 x 3 x 3 fcc copper (float32 positions), as published: U / N against the truncated lattice sums, and forces
    that vanish: the 54 per-neighbour terms of an atom cancel by symmetry, so the force scale is the sum of their absolute
    values -- which is what eam_ref's A_grad holds."""
    x32, cell32 = R.jittered_fcc(3, 3.61, 0.0)
    mod = _module(x32, cell32, shift="none")
    lst, ref = _reference(mod, x32, cell32)
    assert lst["rows"].tolist() == [54] * 108
    x = T(x32, DEV)
    o = _eval(mod, x, energy=True, grad=True)
    eps, a, c = _theta64(mod)
    within(o["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), "perfect cu108 U")
    Sn, Sm, sites = R.fcc_sums(9, 6, a0=float(cell32[0]) / 3, a=a, rc=RC)
    want = eps * (0.5 * Sn - c * math.sqrt(Sm))
    assert sites == 54 and abs(want + 3.38955) <= 1e-4
    assert abs(float(o["energy"]) / 108 - want) <= TOL * float(ref["A_U"]) / 108 + 1e-6 * abs(want)    # (float32 coordinates)
    within(o["grad"], ref["grad"], ref["A_grad"], "perfect cu108 dU/dx")
    assert float(ref["grad"].abs().max()) <= 1e-4 * float(ref["A_grad"].max()), "float64 forces vanish (float32 positions)"
    assert float(o["grad"].abs().max()) <= TOL * float(ref["A_grad"].max()) + float(ref["grad"].abs().max())


# ------------------------------------------------------------------------------------------------ 5: replicas
def _replicas24():
    box = np.array([11.2, 11.2, 11.9], dtype=F32)
    base = CR.seeded_gas(24, box, 2.8, seed=24)
    rng = np.random.default_rng(240)
    x32 = np.concatenate([np.mod(base + rng.normal(0, 0.14, base.shape), box) for _ in range(3)]).astype(F32)
    return base, box, x32


def test_parameter_gradients_on_three_replicas_bitwise_repeatable_and_permutable():
    base, box, x32 = _replicas24()
    system = mk_system(base, box).replicate(3)
    mod, lst, ref, o1, o2, _ = _check_all_outputs(x32, box, "3 x gas24", group=24, system=system, seed=5)
    assert int((lst["i"] // 24 != lst["j"] // 24).sum()) == 0
    col, cnt = mod._ell.col.cpu(), mod._ell.cnt.cpu()
    for i in range(72):
        assert bool((col[i, :int(cnt[i])] // 24 == i // 24).all()), "a neighbour in another replica"
    x = T(x32, DEV).requires_grad_(True)
    w = T(np.random.default_rng(22).normal(0, 1, x32.shape).astype(F32), DEV)
    params = (mod.epsilon, mod.a, mod.c)
    g = torch.autograd.grad(mod(x), (x,) + params, create_graph=True)
    h = torch.autograd.grad((g[0] * w).sum(), params)
    within(torch.cat([t.reshape(1) for t in g[1:]]), ref["dth"], ref["A_dth"], "autograd dU/dtheta on three replicas")
    k = R.consts(mod.n, mod.m, mod.cutoff, mod.shift)
    ref_w = R.evaluate(x32, _theta64(mod), lst, box, k, w=w.cpu().numpy())
    within(torch.cat([t.reshape(1) for t in h]), ref_w["dthw"], ref_w["A_dthw"], "autograd d(w.dU/dx)/dtheta on three replicas")
    F, dq, gth = mod.force_vjp(x.detach(), w)
    within(-torch.cat([t.reshape(1) for t in gth]), ref_w["dthw"], ref_w["A_dthw"], "force_vjp parameter part")
    F2, dq2, gth2 = mod.force_vjp(x.detach(), w)
    assert torch.equal(F, F2) and torch.equal(dq, dq2) and all(torch.equal(a, b) for a, b in zip(gth, gth2))
    g2 = torch.autograd.grad(mod(x), (x,) + params)
    assert all(torch.equal(a.detach(), b) for a, b in zip(g, g2))
    # replicas (2, 0, 1): per-atom outputs move with their replica, bit for bit
    perm = torch.cat([torch.arange(24) + 24 * r for r in (2, 0, 1)]).to(DEV)
    xd = x.detach()
    mod._reset_topology(xd[perm].contiguous())
    op = _eval(mod, xd[perm].contiguous(), w=w[perm].contiguous(), energy=False, want_theta=True)
    mod._reset_topology(xd)
    oo = _eval(mod, xd, w=w, energy=False, want_theta=True)
    for key in ("grad", "hw", "pthw"):
        assert torch.equal(op[key], oo[key][perm]), key


# ------------------------------------------------------------------------------------------------ 6: autograd
def test_autograd_backward_and_double_backward_equal_force_vjp():
    x32, cell32 = R.jittered_fcc(3, 3.61, 0.15, 70)
    mod = _module(x32, cell32)
    lst, ref = _reference(mod, x32, cell32)
    x = T(x32, DEV).requires_grad_(True)
    mod(x).backward()
    within(x.grad, ref["grad"], ref["A_grad"], "backward of model(xyz) in xyz")
    got = torch.cat([p.grad.reshape(1) for p in (mod.epsilon, mod.a, mod.c)])
    within(got, ref["dth"], ref["A_dth"], "backward of model(xyz) in (epsilon, a, c)")
    w = torch.randn(108, 3, device=DEV)
    x2 = T(x32, DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(mod(x2), x2, create_graph=True)
    hw, he, ha, hc = torch.autograd.grad((g * w).sum(), (x2, mod.epsilon, mod.a, mod.c))
    F, dq, gth = mod.force_vjp(x2.detach(), w)
    assert torch.equal(F, -g.detach()) and torch.equal(dq, -hw)
    assert [t.shape for t in gth] == [p.shape for p in mod.parameters()]
    assert torch.equal(gth[0], -he) and torch.equal(gth[1], -ha) and torch.equal(gth[2], -hc)
    assert torch.equal(mod.force(x2.detach()), F)
    frozen = _module(x32, cell32, trainable=False)
    assert list(frozen.parameters()) == []
    assert frozen.force_vjp(x2.detach(), w)[2] == [] and frozen.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    assert torch.equal(frozen.force_vjp(x2.detach(), w)[1], dq)
    assert mod.force_vjp(x2.detach(), w, want_theta=False)[2] is None


# ------------------------------------------------------------------------------------------------ 7: into / scale / accum
def test_stack_sums_equal_the_members_separate_results():
    """Stack({"lj", "sc"}).force and .force_vjp (the force pass adds onto the pair term's buffers) against the sum of the
    members' separate results, to 2^-22 of the largest entry; the same for `accum` against the list return."""
    from mdgrad_amd import ops
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    x32, cell32 = R.jittered_fcc(3, 3.61, 0.15, 66)
    system = mk_system(x32, cell32)
    sc = _module(x32, cell32, system=system)
    lj = PairPotentials(system, P.LJFamily(2.3, 0.1), cutoff=RC)
    stack = Stack({"lj": lj, "sc": sc})
    assert stack.supports_force_vjp() and stack.supports_static_topology()
    x, w = T(x32, DEV), torch.randn(108, 3, device=DEV)
    stack._reset_topology(x)
    assert lj._ell is sc._ell, "one search for both members"

    def same(a, b, what):
        assert float((a - b).abs().max()) <= 2.0 ** -22 * float(b.abs().max()), what
    same(stack.force(x), lj.force(x) + sc.force(x), "force")
    F, dq, gth = stack.force_vjp(x, w)
    f1, d1, g1 = lj.force_vjp(x, w)
    f2, d2, g2 = sc.force_vjp(x, w)
    same(F, f1 + f2, "force (vjp)")
    same(dq, d1 + d2, "d(w.F)/dx")
    params = list(stack.parameters())
    assert len(gth) == len(params) == 5
    by_id = {id(p): v for p, v in zip(list(lj.parameters()) + list(sc.parameters()), g1 + g2)}
    for p, v in zip(params, gth):
        same(v, by_id[id(p)], "parameter part")
    acc = ops.ThetaAccum(params)
    acc.flat.fill_(0.25)
    assert stack.force_vjp(x, w, accum=acc)[2] is None
    for v, want in zip(acc.views(), gth):
        assert float((v - 0.25 - want).abs().max()) <= 2.0 ** -22 * max(float(want.abs().max()), 0.25), "accum vs list"
    # a flat buffer in which the three parameters are not adjacent
    acc2 = ops.ThetaAccum([sc.c, lj.model.sigma, sc.epsilon, sc.a])
    assert sc.force_vjp(x, w, accum=acc2)[2] is None
    for v, want in zip(acc2.views(), [g2[2], torch.zeros(1, device=DEV), g2[0], g2[1]]):
        assert float((v - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max()), "accum, scattered offsets"
    F0, D0 = torch.randn_like(x), torch.randn_like(x)
    F1, D1, _ = sc.force_vjp(x, w, into=(F0.clone(), D0.clone()))
    same(F1 - F0, f2, "force added onto a buffer")
    same(D1 - D0, d2, "d(w.F)/dx added onto a buffer")


# ------------------------------------------------------------------------------------------------ 8: skin list
def test_evaluation_on_a_list_searched_with_a_skin_equals_a_fresh_exact_list():
    """rc = 5.0 here: rc + skin = 5.4 has to stay below half the 10.83 A cell."""
    from mdgrad_amd import _lib, ops
    x32, cell32 = R.jittered_fcc(3, 3.61, 0.15, 67)
    rc, skin = 5.0, 0.4
    mod = _module(x32, cell32, rc=rc)
    cs = _lib.make_cell(cell32)
    x0 = T(x32, DEV)
    longest = int(ops.build_ell(x0, cs, rc + skin).cnt.max())
    vl = ops.VerletList(108, 108, cs, rc, skin, None, min(107, (longest + 15) // 8 * 8), 8192, DEV)
    need = torch.zeros(2, dtype=torch.int32, device=DEV)
    vl.rebuild(x0, need)
    rng = np.random.default_rng(670)
    step = rng.normal(0, 1, (108, 3))
    step = 0.18 * step / np.linalg.norm(step, axis=1)[:, None] * rng.uniform(0.3, 1.0, (108, 1))      # |move| < skin / 2
    x1_32 = (x32 + step).astype(F32)
    x1 = T(x1_32, DEV)
    vl.rebuild(x1, need)
    assert vl.builds() == 1 and need.tolist()[0] <= vl.max_nbr
    exact = ops.build_ell(x1, cs, rc)
    assert int(vl.cnt.sum()) > int(exact.cnt.sum()), "the stored list carries the skin's extra candidates"
    w32 = rng.normal(0, 1, (108, 3)).astype(F32)
    lst, ref = _reference(mod, x1_32, cell32, w32)
    w = T(w32, DEV)
    A = {"energy": ref["A_U"].reshape(1), "grad": ref["A_grad"], "hw": ref["A_hw"]}
    for kw, keys in ((dict(energy=True), ("energy", "grad", "pth")), (dict(w=w, energy=False), ("grad", "hw", "pthw"))):
        a = ops.eam_eval(vl.ell, x1, mod._consts, mod._theta(), want_theta=True, **kw)
        b = ops.eam_eval(exact, x1, mod._consts, mod._theta(), want_theta=True, **kw)
        for key in keys:
            if key in A:
                within(a[key], b[key].cpu(), A[key], "skin list vs exact list: " + key)
            else:
                within(ops.eam_theta_sum(a[key]), ops.eam_theta_sum(b[key]).cpu(), ref["A_dth" if key == "pth" else "A_dthw"],
                       "skin list vs exact list: sum of " + key)
    within(a["hw"], ref["hw"], ref["A_hw"], "skin list vs float64: H.w")
    within(a["grad"], ref["grad"], ref["A_grad"], "skin list vs float64: dU/dx")


# ------------------------------------------------------------------------------------------------ 9: trajectory + adjoint
_oracle_cache = {}
TRAJ = dict(T=0.05, Q=20.0, chains=3, dt=0.01, mass=2.0, nbins=32, r_range=(2.0, 5.0))


def traj_inputs():
    x32, cell32 = R.jittered_fcc(3, 3.61, 0.1, 71)
    vel = np.random.default_rng(710).normal(0, math.sqrt(TRAJ["T"] / TRAJ["mass"]), x32.shape).astype(F32)
    return x32, cell32, vel, np.full(108, TRAJ["mass"], dtype=F32)


def oracle_traj(t):
    if "run" not in _oracle_cache:
        x32, cell32, vel, mass = traj_inputs()
        cell = T(cell32)
        terms = [R.SCTerm(CU[0], CU[1], CU[2], CU[3], CU[4], RC, cell32)]

        def loss_fn(Ls):
            _, _, gr = O.rdf_oracle(Ls[1][::2], cell, TRAJ["nbins"], TRAJ["r_range"])
            return gr.pow(2).mean() + Ls[0][-1].pow(2).mean() + 0.0 * Ls[2][-1].sum()
        _oracle_cache["run"] = oracle_run(x32, cell32, vel, mass, terms, TRAJ["T"], TRAJ["Q"], TRAJ["chains"], t, loss_fn)
    return _oracle_cache["run"]


@pytest.mark.parametrize("graphs_on", [True, False], ids=["graph_replay", "eager"])
def test_sc_term_in_a_stack_trajectory_and_adjoint_vs_oracle(graphs_on):
    """Stack(SuttonChen, trainable) on 108 jittered copper atoms: 10 NHC steps through odeint_adjoint, the loss on rdf of
    q_t[::2] plus v_t[-1]^2 -- trajectories, adjoint of y0 and dL/d(epsilon, a, c) against the oracle with eam_ref.SCTerm.
    The stack stays on the analytic adjoint (force_vjp) and HIP-graph replay although the parameters require grad.
    Tolerances: those of test_sw_term_in_a_stack_trajectory_and_adjoint_vs_oracle (the project's for this oracle and horizon).
    Observed on an MI355X (MDG_TEST_REPORT; graph replay and eager alike), observed / allowed at the worst entry: q_t 1.2e-07 /
    2.0e-05, v_t 6.7e-08 / 1.4e-04, pv_t 2.9e-08 / 1.3e-05, adj v0 5.1e-09 / 4.4e-05, adj q0 9.7e-08 / 7.0e-04, adj pv0 1.1e-12 /
    4.2e-07, dL/d(epsilon, a, c) 2.4e-07 / 5.6e-03."""
    from mdgrad_amd import graphs
    from mdgrad_amd.interface import Stack
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.sovlers import odeint_adjoint
    x32, cell32, vel, mass = traj_inputs()
    system = mk_system(x32, cell32, vel, mass)
    sc = _module(x32, cell32, system=system)
    stack = Stack({"sc": sc})
    integ = NoseHooverChain(stack, system, T=TRAJ["T"], num_chains=TRAJ["chains"], Q=TRAJ["Q"], adjoint=True).to(DEV)
    assert integ.fused_spec("NH_verlet") is None, "a Sutton-Chen member keeps the stack off the fused trajectory kernels"
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
    assert gth.numel() == 3 and all(p.grad is not None for p in (sc.epsilon, sc.a, sc.c))
    got = torch.cat([p.grad.reshape(1) for p in (sc.epsilon, sc.a, sc.c)])
    close(got, gth, 5e-3, 5e-4 * float(gth.abs().max()), "dL/d(epsilon, a, c)")


# ------------------------------------------------------------------------------------------------ 10: torch ops
def test_torch_ops_equal_ctypes_path_and_reject_bad_input():
    from mdgrad_amd import _torch_ops, ops
    ns = _torch_ops.get()
    assert ns is not None
    x32, box = _gas37()
    mod = _module(x32, box)
    ell, k = mod._ell, mod._consts
    cell = _torch_ops.cell_args(ell.cell_struct)
    kk = [k.epsilon, k.a, k.c, k.rc, float(k.n), float(k.m), float(k.shift)]
    x, w, th = T(x32, DEV), torch.randn(37, 3, device=DEV), mod._theta()
    a = ops.eam_eval(ell, x, k, th, energy=True, grad=True, want_theta=True)
    U, g, hw, pth, pthw = ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th, None, True, True)
    assert torch.equal(U, a["energy"]) and torch.equal(g, a["grad"]) and torch.equal(pth, a["pth"]) and hw.numel() == pthw.numel() == 0
    b = ops.eam_eval(ell, x, k, th, w=w, energy=False, grad=True, want_theta=True)
    U, g, hw, pth, pthw = ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th, w, False, True)
    assert torch.equal(g, b["grad"]) and torch.equal(hw, b["hw"]) and torch.equal(pthw, b["pthw"]) and U.numel() == pth.numel() == 0
    # without the device theta the kernels take the host copies: the same numbers (float32 of the same doubles)
    c = ops.eam_eval(ell, x, k, None, energy=True, grad=True)
    U, g, _, _, _ = ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, None, None, True, False)
    assert torch.equal(U, c["energy"]) and torch.equal(g, c["grad"]) and torch.equal(g, a["grad"])
    with pytest.raises(ValueError):
        ops.eam_eval(ell, x, k, th, work=torch.empty(36, 4, device=DEV))
    bad = [lambda: ns.eam_eval(x.double(), cell, ell.col, ell.shift, ell.cnt, kk, th, None, True, False),
           lambda: ns.eam_eval(x.cpu(), cell, ell.col, ell.shift, ell.cnt, kk, th, None, True, False),
           lambda: ns.eam_eval(x, cell[:5], ell.col, ell.shift, ell.cnt, kk, th, None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col.long(), ell.shift, ell.cnt, kk, th, None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt[:5].contiguous(), kk, th, None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk[:6], th, None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th[:2].contiguous(), None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th.double(), None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th.cpu(), None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th, w[:5].contiguous(), True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th, w.double(), True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, [kk[0], 0.0] + kk[2:], None, None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, [kk[0], -2.0] + kk[2:], None, None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, [0.0] + kk[1:], None, None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk[:2] + [-1.0] + kk[3:], None, None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk[:3] + [0.0] + kk[4:], th, None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk[:4] + [6.0, 6.0, 1.0], th, None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk[:4] + [17.0, 6.0, 1.0], th, None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk[:4] + [9.5, 6.0, 1.0], th, None, True, False),
           lambda: ns.eam_eval(x, cell, ell.col, ell.shift, ell.cnt, kk[:6] + [2.0], th, None, True, False)]
    for n, fn in enumerate(bad):
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
            pytest.fail("bad input %d was accepted" % n)
