"""K25: the Tersoff bond-order term (Tersoff, mdg_tersoff_eval, csrc/tersoff.hip) against the float64 definition of
tests/tersoff_ref.py (pinned to an independent loop and to the diamond lattice in closed form by tests/test_tersoff_host.py,
which also checks the input conditions of every configuration used here) and, in a trajectory, against the CPU oracle's adjoint.

Tolerance of every kernel-vs-float64 comparison: K * 2^-24 * A per component with K = 64, the project's bound for the term
kernels, A = the float64 sum of the absolute contributions of the bond halves and the triplet terms to that component
(tersoff_ref.evaluate).  The reference keeps the published g = gamma (1 + c^2/d^2 - c^2/(d^2 + (h - cos)^2)); the kernel
evaluates gamma (1 + (c/d)^2 u^2 / (d^2 + u^2)), so their agreement is part of every comparison.  `within` prints the largest
observed err / (2^-24 A).

On an MI355X the largest observed ratios over all cases of this file were U 3.32 (gas37), dU/dx 23.35 (three replicas of the
16-atom gas), H.w 51.98 (c64), dU/dtheta 4.23 (replicas), d(w.dU/dx)/dtheta 3.59 (tric64), the sum of the forces 0.05; si64
alone: 2.67, 6.29, 22.92, 2.55, 1.55, 0.03; the perfect lattice: U 2.32, the forces against zero 2.30.  No case exceeds 64, so
no bound is taken from a float32 evaluation of the reference.  H.w is the largest throughout; the likely reason is that it
carries the second derivatives of g, whose argument u = h - cos theta is a difference of two numbers of order one half (a few
2^-24 of cos theta are 2^-22 of u at the tetrahedral angle), once more than dU/dx does."""
import math

import numpy as np
import pytest
import torch

import oracle as O
import tersoff_ref as R
from test_gpu_parity import T, close, mk_system, DEV, oracle_run
from test_gpu_sw import within

pytestmark = pytest.mark.gpu
F32 = np.float32
ULP = 2.0 ** -24
KTOL = 64
TOL = KTOL * ULP
CASES = {}
_refs = {}


def case(name):
    if "si64" not in CASES:
        CASES.update(R.gpu_cases())
    return CASES[name]


def _module(x32, cell32, params=R.SILICON, system=None, **kw):
    from mdgrad_amd.interface import Tersoff
    return Tersoff(mk_system(x32, cell32) if system is None else system, **dict(params, **kw))


def _theta64(mod):
    """The module's float32 parameters, as the float64 reference sees them."""
    return [float(p.detach()) for p in (mod.A, mod.B, mod.h)]


def _w(name, shape):
    return np.random.default_rng(sum(map(ord, name))).normal(0, 1, shape).astype(F32)


def _reference(name, mod):
    """(list, float64 evaluation with the w of the case) -- computed once per case and shared."""
    if name not in _refs:
        x32, cell32, params, group = case(name)
        k = R.consts(**params)
        lst = R.bonds_and_triplets(x32, cell32, k["rc"], group=group)
        _refs[name] = (lst, R.evaluate(x32, _theta64(mod), lst, cell32, k, w=_w(name, x32.shape)))
    return _refs[name]


def _eval(mod, x, **kw):
    from mdgrad_amd import ops
    return ops.tersoff_eval(mod._ell, x, mod._consts, mod._theta(), work=mod._scratch(), **kw)


def _check_all_outputs(name, system=None, **kw):
    """U, dU/dx, H w, dU/dtheta and d(w.dU/dx)/dtheta of one call each against float64; the energy-only call; the sum of the
    forces."""
    from mdgrad_amd import ops
    x32, cell32, params, group = case(name)
    mod = _module(x32, cell32, params, system=system, **kw)
    lst, ref = _reference(name, mod)
    x, w = T(x32, DEV), T(_w(name, x32.shape), DEV)
    mod._reset_topology(x)
    o1 = _eval(mod, x, energy=True, grad=True, want_theta=True)
    o2 = _eval(mod, x, w=w, energy=False, grad=True, want_theta=True)
    o1["dth"], o2["dthw"] = ops.sw_theta_sum(o1["pth"]), ops.sw_theta_sum(o2["pthw"])
    tag = name + " "
    within(o1["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + "U")
    within(o1["grad"], ref["grad"], ref["A_grad"], tag + "dU/dx")
    within(o2["hw"], ref["hw"], ref["A_hw"], tag + "H.w")
    within(o1["dth"], ref["dth"], ref["A_dth"], tag + "dU/dtheta")
    within(o2["dthw"], ref["dthw"], ref["A_dthw"], tag + "d(w.dU/dx)/dtheta")
    assert torch.equal(o1["grad"], o2["grad"]) and o2["pth"] is None and o1["pthw"] is None
    e0 = _eval(mod, x, energy=True, grad=False)                                                    # the bond pass alone
    within(e0["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + "U (energy-only call)")
    assert torch.equal(e0["energy"], o1["energy"])
    # translation invariance: what an atom receives as end and as third atom must balance its centre part
    within(o1["grad"].sum(0), torch.zeros(3), ref["A_grad"].sum(0), tag + "sum_i dU/dx_i")
    return mod, lst, ref, o1, o2


# ------------------------------------------------------------------------------------------------ 1, 2: outputs vs float64
def test_outputs_vs_float64_jittered_si64():
    """2 x 2 x 2 diamond cells (a = 5.432) with every coordinate jittered by 0.3 A: bonds enter the taper."""
    mod, lst, ref, o1, o2 = _check_all_outputs("si64")
    assert int(lst["rows"].max()) >= 5 and lst["tb"].numel() > 400


def test_outputs_vs_float64_jittered_c64():
    mod, lst, ref, o1, o2 = _check_all_outputs("c64")
    assert float(mod.A.detach()) == F32(1393.6) and abs(mod.cutoff - 2.1) < 1e-12


def test_outputs_vs_float64_gas37_isolated_atom_dimer_trimer_and_a_long_row():
    mod, lst, ref, o1, o2 = _check_all_outputs("gas37")
    rows = lst["rows"].tolist()
    assert rows[31] == 0 and rows[32] == rows[33] == 1 and rows[34:37] == [2, 1, 1] and rows[0] > 16 and 37 % 16 != 0
    assert int(mod._ell.cnt[31]) == 0 and int(mod._ell.cnt[32]) == 1 and int(mod._ell.cnt[0]) > 16
    for o in (o1["grad"][31], o1["pth"][31], o2["hw"][31], o2["pthw"][31]):
        assert float(o.abs().max()) == 0.0, "the atom with the empty row"
    # the dimer: zeta = 0, b = 1, nothing depends on h, and every output is finite (`within` checks that)
    dimer = (lst["bc"] == 32) | (lst["bc"] == 33)
    assert int(dimer.sum()) == 2 and float(ref["zeta"][dimer].abs().max()) == 0.0
    assert float(o1["pth"][32, 2].abs()) == 0.0 and float(o2["pthw"][32, 2].abs()) == 0.0
    assert float(o1["grad"][32].abs().max()) > 0.0
    # the trimer: the two bonds of the centre have different third atoms, b_ij != b_ji
    assert float(o1["pth"][34, 2].abs()) > 0.0


def test_outputs_vs_float64_triclinic64():
    mod, lst, ref, o1, o2 = _check_all_outputs("tric64")
    assert case("tric64")[1].shape == (3, 3) and float(np.abs(case("tric64")[1][1, 0])) > 1.0


@pytest.mark.parametrize("m", [3, 1])
def test_outputs_vs_float64_with_lam3(m):
    """lam3 = 1.3258: the exponential exp[(lam3 (r_ij - r_ik))^m] and its derivatives, for both exponents."""
    name = "lam3_m%d" % m
    if name not in CASES:
        x32, cell32, params, group = case("lam3")
        CASES[name] = (x32, cell32, dict(params, m=m), group)
    _check_all_outputs(name)


# ------------------------------------------------------------------------------------------------ 3: perfect diamond
def test_perfect_diamond_silicon_through_the_kernel():
    """Perfect 2 x 2 x 2 diamond at a = 5.432 (float32 positions): U / N against the closed form with zeta = 3 g(-1/3), and
    forces that vanish on the scale of the per-atom absolute sum of the bond halves and triplet terms (the repulsive and the
    attractive half of a bond nearly cancel at the equilibrium length; A_grad counts both)."""
    x32, cell32 = R.jittered_diamond(2, 5.432, 0.0)
    CASES.setdefault("perfect", (x32, cell32, R.SILICON, None))
    mod = _module(x32, cell32)
    lst, ref = _reference("perfect", mod)
    assert lst["rows"].tolist() == [4] * 64
    o = _eval(mod, T(x32, DEV), energy=True, grad=True)
    within(o["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), "perfect si64 U")
    p = dict(R.SILICON, **dict(zip("ABh", _theta64(mod))))
    u_n, zeta, b = R.diamond_closed_form(p, 5.432)
    # (float32 positions move r0 by 2^-24 * 10.9 A; dU/dr summed over the halves is below 10 eV/A per bond)
    assert abs(float(o["energy"]) / 64 - u_n) <= TOL * float(ref["A_U"]) / 64 + 1e-5
    assert abs(u_n + 4.62960) <= 2e-5 and abs(zeta - 30673.6) <= 0.1 and abs(b - 0.958303) <= 1e-6
    within(o["grad"], torch.zeros(64, 3), ref["A_grad"], "perfect si64 dU/dx against zero")
    assert float(ref["grad"].abs().max()) <= 1e-5 * float(ref["A_grad"].min()), "float64 forces vanish (float32 positions)"


# ------------------------------------------------------------------------------------------------ 4: orders, repeats, replicas
def test_first_and_second_order_calls_repeats_and_three_replicas():
    from mdgrad_amd import ops
    base, box, x32 = R.replicas16(R.SEEDS["replicas"])
    assert np.array_equal(x32, case("replicas")[0])
    system = mk_system(base, box).replicate(3)
    mod, lst, ref, o1, o2 = _check_all_outputs("replicas", system=system)
    assert torch.equal(o1["grad"], o2["grad"]), "dU/dx of the float and the Dual instantiation, bit for bit"
    assert int((lst["bc"] // 16 != lst["be"] // 16).sum()) == 0 and int((lst["bc"][lst["tb"]] // 16 != lst["tk"] // 16).sum()) == 0
    x, w = T(x32, DEV), T(_w("replicas", x32.shape), DEV)
    F, dq, gth = mod.force_vjp(x, w)
    within(-torch.cat([t.reshape(1) for t in gth]), ref["dthw"], ref["A_dthw"], "force_vjp parameter part on three replicas")
    F2, dq2, gth2 = mod.force_vjp(x, w)
    assert torch.equal(F, F2) and torch.equal(dq, dq2) and all(torch.equal(a, b) for a, b in zip(gth, gth2))
    assert torch.equal(F, -o2["grad"]) and torch.equal(dq, -o2["hw"])
    # every replica alone: the same per-atom parameter terms, so the sums of the three are those of the batch
    k = R.consts(**R.SILICON)
    alone, alone_w = torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    for r in range(3):
        sl = slice(16 * r, 16 * r + 16)
        one = _module(x32[sl], box)
        xr = T(x32[sl], DEV)
        one._reset_topology(xr)
        a = _eval(one, xr, energy=False, grad=True, want_theta=True)
        b = _eval(one, xr, w=w[sl].contiguous(), energy=False, grad=True, want_theta=True)
        within(a["grad"], o1["grad"][sl].cpu(), ref["A_grad"][sl], "replica %d alone: dU/dx" % r)
        within(b["hw"], o2["hw"][sl].cpu(), ref["A_hw"][sl], "replica %d alone: H.w" % r)
        alone += ops.sw_theta_sum(a["pth"]).cpu().double()
        alone_w += ops.sw_theta_sum(b["pthw"]).cpu().double()
    within(o1["dth"], alone, ref["A_dth"], "dU/dtheta: three replicas vs each alone")
    within(o2["dthw"], alone_w, ref["A_dthw"], "d(w.dU/dx)/dtheta: three replicas vs each alone")
    # replicas (2, 0, 1): per-atom outputs move with their replica, bit for bit
    perm = torch.cat([torch.arange(16) + 16 * r for r in (2, 0, 1)]).to(DEV)
    mod._reset_topology(x[perm].contiguous())
    op = _eval(mod, x[perm].contiguous(), w=w[perm].contiguous(), energy=False, want_theta=True)
    mod._reset_topology(x)
    oo = _eval(mod, x, w=w, energy=False, want_theta=True)
    for key in ("grad", "hw", "pthw"):
        assert torch.equal(op[key], oo[key][perm]), key


# ------------------------------------------------------------------------------------------------ 5: autograd
def test_autograd_backward_and_double_backward_equal_force_vjp():
    x32, cell32, params, _ = case("si64")
    mod = _module(x32, cell32)
    lst, ref = _reference("si64", mod)
    x = T(x32, DEV).requires_grad_(True)
    mod(x).backward()
    within(x.grad, ref["grad"], ref["A_grad"], "backward of model(xyz) in xyz")
    got = torch.cat([p.grad.reshape(1) for p in (mod.A, mod.B, mod.h)])
    within(got, ref["dth"], ref["A_dth"], "backward of model(xyz) in (A, B, h)")
    w = T(_w("si64", x32.shape), DEV)
    x2 = T(x32, DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(mod(x2), x2, create_graph=True)
    hw, hA, hB, hh = torch.autograd.grad((g * w).sum(), (x2, mod.A, mod.B, mod.h))
    within(hw, ref["hw"], ref["A_hw"], "double backward of model(xyz) in xyz")
    F, dq, gth = mod.force_vjp(x2.detach(), w)
    assert torch.equal(F, -g.detach()) and torch.equal(dq, -hw)
    assert [t.shape for t in gth] == [p.shape for p in mod.parameters()]
    assert torch.equal(gth[0], -hA) and torch.equal(gth[1], -hB) and torch.equal(gth[2], -hh)
    assert torch.equal(mod.force(x2.detach()), F)
    frozen = _module(x32, cell32, trainable=False)
    assert list(frozen.parameters()) == []
    assert frozen.force_vjp(x2.detach(), w)[2] == [] and frozen.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    assert torch.equal(frozen.force_vjp(x2.detach(), w)[1], dq)
    assert mod.force_vjp(x2.detach(), w, want_theta=False)[2] is None


# ------------------------------------------------------------------------------------------------ 6: into / scale / accum
def test_stack_sums_equal_the_members_separate_results():
    """Stack({"lj", "tersoff"}).force and .force_vjp (the Tersoff force pass adds onto the pair term's buffers) against the sum
    of the members' separate results, to 2^-22 of the largest entry; the same for `accum` against the list return."""
    from mdgrad_amd import ops
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    x32, cell32, params, _ = case("si64")
    system = mk_system(x32, cell32)
    ts = _module(x32, cell32, system=system)
    lj = PairPotentials(system, P.LJFamily(2.0, 0.1), cutoff=ts.cutoff)
    stack = Stack({"lj": lj, "tersoff": ts})
    assert stack.supports_force_vjp() and stack.supports_static_topology()
    x, w = T(x32, DEV), T(_w("si64", x32.shape), DEV)
    stack._reset_topology(x)
    assert lj._ell is ts._ell, "one search for both members"

    def same(a, b, what):
        assert float((a - b).abs().max()) <= 2.0 ** -22 * float(b.abs().max()), what
    same(stack.force(x), lj.force(x) + ts.force(x), "force")
    F, dq, gth = stack.force_vjp(x, w)
    f1, d1, g1 = lj.force_vjp(x, w)
    f2, d2, g2 = ts.force_vjp(x, w)
    same(F, f1 + f2, "force (vjp)")
    same(dq, d1 + d2, "d(w.F)/dx")
    params = list(stack.parameters())
    assert len(gth) == len(params) == 5
    by_id = {id(p): v for p, v in zip(list(lj.parameters()) + list(ts.parameters()), g1 + g2)}
    for p, v in zip(params, gth):
        same(v, by_id[id(p)], "parameter part")
    acc = ops.ThetaAccum(params)
    acc.flat.fill_(0.25)
    assert stack.force_vjp(x, w, accum=acc)[2] is None
    for v, want in zip(acc.views(), gth):
        assert float((v - 0.25 - want).abs().max()) <= 2.0 ** -22 * max(float(want.abs().max()), 0.25), "accum vs list"
    F0, D0 = torch.randn_like(x), torch.randn_like(x)
    F1, D1, _ = ts.force_vjp(x, w, into=(F0.clone(), D0.clone()))
    same(F1 - F0, f2, "force added onto a buffer")
    same(D1 - D0, d2, "d(w.F)/dx added onto a buffer")


# ------------------------------------------------------------------------------------------------ 7: skin list
def test_evaluation_on_a_list_searched_with_a_skin_equals_a_fresh_exact_list():
    from mdgrad_amd import _lib, ops
    x32, cell32, params, _ = case("si64")
    x1_32 = case("skin")[0]
    assert np.array_equal(x1_32, R.skin_step(x32, R.SEEDS["skin"])) and float(np.abs(x1_32 - x32).max()) < 0.2
    mod = _module(x32, cell32)
    rc, skin = mod.cutoff, 0.4
    cs = _lib.make_cell(cell32)
    x0, x1 = T(x32, DEV), T(x1_32, DEV)
    longest = int(ops.build_ell(x0, cs, rc + skin).cnt.max())
    vl = ops.VerletList(64, 64, cs, rc, skin, None, min(63, (longest + 15) // 8 * 8), 4096, DEV)
    need = torch.zeros(2, dtype=torch.int32, device=DEV)
    vl.rebuild(x0, need)
    vl.rebuild(x1, need)
    assert vl.builds() == 1 and need.tolist()[0] <= vl.max_nbr
    exact = ops.build_ell(x1, cs, rc)
    assert int(vl.cnt.sum()) > int(exact.cnt.sum()), "the stored list carries the skin's extra candidates"
    lst, ref = _reference("skin", mod)
    w = T(_w("skin", x32.shape), DEV)
    A = {"energy": ref["A_U"].reshape(1), "grad": ref["A_grad"], "hw": ref["A_hw"]}
    for kw, keys in ((dict(energy=True), ("energy", "grad", "pth")), (dict(w=w, energy=False), ("grad", "hw", "pthw"))):
        a = ops.tersoff_eval(vl.ell, x1, mod._consts, mod._theta(), want_theta=True, **kw)
        b = ops.tersoff_eval(exact, x1, mod._consts, mod._theta(), want_theta=True, **kw)
        for key in keys:
            if key in A:
                within(a[key], b[key].cpu(), A[key], "skin list vs exact list: " + key)
            else:
                within(ops.sw_theta_sum(a[key]), ops.sw_theta_sum(b[key]).cpu(), ref["A_dth" if key == "pth" else "A_dthw"],
                       "skin list vs exact list: sum of " + key)
    within(a["hw"], ref["hw"], ref["A_hw"], "skin list vs float64: H.w")
    within(a["grad"], ref["grad"], ref["A_grad"], "skin list vs float64: dU/dx")


# ------------------------------------------------------------------------------------------------ 8: trajectory + adjoint
_oracle_cache = {}
TRAJ = dict(T=0.05, Q=20.0, chains=3, dt=0.01, mass=2.0, nbins=32, r_range=(1.5, 5.0))


def traj_inputs():
    x32, cell32, _, _ = case("traj")
    vel = np.random.default_rng(710).normal(0, math.sqrt(TRAJ["T"] / TRAJ["mass"]), x32.shape).astype(F32)
    return x32, cell32, vel, np.full(64, TRAJ["mass"], dtype=F32)


def oracle_traj(t):
    if "run" not in _oracle_cache:
        x32, cell32, vel, mass = traj_inputs()
        cell = T(cell32)
        terms = [R.TersoffTerm(R.SILICON, cell32)]

        def loss_fn(Ls):
            _, _, gr = O.rdf_oracle(Ls[1][::2], cell, TRAJ["nbins"], TRAJ["r_range"])
            return gr.pow(2).mean() + Ls[0][-1].pow(2).mean() + 0.0 * Ls[2][-1].sum()
        _oracle_cache["run"] = oracle_run(x32, cell32, vel, mass, terms, TRAJ["T"], TRAJ["Q"], TRAJ["chains"], t, loss_fn)
    return _oracle_cache["run"]


@pytest.mark.parametrize("graphs_on", [True, False], ids=["graph_replay", "eager"])
def test_tersoff_term_in_a_stack_trajectory_and_adjoint_vs_oracle(graphs_on):
    """Stack(Tersoff.silicon, trainable) on 64 jittered silicon atoms: 10 NHC steps through odeint_adjoint, the loss on rdf of
    q_t[::2] plus v_t[-1]^2 -- trajectories, adjoint of y0 and dL/d(A, B, h) against the oracle with tersoff_ref.TersoffTerm.
    The stack stays on the analytic adjoint (force_vjp) and HIP-graph replay although the parameters require grad.
    Tolerances: those of test_sw_term_in_a_stack_trajectory_and_adjoint_vs_oracle.
    Observed on an MI355X (graph replay and eager alike), observed / allowed at the entry closest to its bound: q_t 9.5e-07 /
    2.0e-05, v_t 1.2e-06 / 1.1e-04, pv_t 0.0e+00 / 1.0e-05, adj v0 5.0e-09 / 1.8e-05, adj q0 1.6e-08 / 1.2e-04, adj pv0
    8.9e-16 / 1.3e-06, dL/d(A, B, h) 1.9e-10 / 2.2e-05."""
    from mdgrad_amd import graphs
    from mdgrad_amd.interface import Stack, Tersoff
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.sovlers import odeint_adjoint
    x32, cell32, vel, mass = traj_inputs()
    system = mk_system(x32, cell32, vel, mass)
    ts = Tersoff.silicon(system)
    stack = Stack({"tersoff": ts})
    integ = NoseHooverChain(stack, system, T=TRAJ["T"], num_chains=TRAJ["chains"], Q=TRAJ["Q"], adjoint=True).to(DEV)
    assert integ.fused_spec("NH_verlet") is None, "a Tersoff member keeps the stack off the fused trajectory kernels"
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

    def report(got, want, rtol, atol, what):
        err = (got.detach().cpu().double() - want.detach().double()).abs()
        allowed = atol + rtol * want.detach().double().abs()
        worst = int((err - allowed).argmax())
        print("%-28s observed %.1e / allowed %.1e" % (what, float(err.reshape(-1)[worst]), float(allowed.reshape(-1)[worst])))
        close(got, want, rtol, atol, what)
    report(q_t, traj[1], 0, 2e-5, "q_t")
    report(v_t, traj[0], 1e-3, 1e-4 * float(traj[0].abs().max()), "v_t")
    report(pv_t, traj[2], 2e-3, 1e-5, "pv_t")
    for x, l, nm in zip(y0, lam, ("adj v0", "adj q0", "adj pv0")):
        report(x.grad, l, 5e-3, 2e-3 * float(l.abs().max()) + 1e-9, nm)
    assert gth.numel() == 3 and all(p.grad is not None for p in (ts.A, ts.B, ts.h))
    got = torch.cat([p.grad.reshape(1) for p in (ts.A, ts.B, ts.h)])
    report(got, gth, 5e-3, 5e-4 * float(gth.abs().max()), "dL/d(A, B, h)")


# ------------------------------------------------------------------------------------------------ 9: torch ops
def test_torch_ops_equal_ctypes_path_and_reject_bad_input():
    from mdgrad_amd import _torch_ops, ops
    ns = _torch_ops.get()
    assert ns is not None
    x32, box, params, _ = case("gas37")
    mod = _module(x32, box)
    ell, k = mod._ell, mod._consts
    cell = _torch_ops.cell_args(ell.cell_struct)
    kk = [k.A, k.B, k.lam1, k.lam2, k.beta, k.n, k.c, k.d, k.h, k.R, k.D, k.lam3, k.gamma, float(k.m)]
    x, w, th = T(x32, DEV), T(_w("gas37", x32.shape), DEV), mod._theta()
    a = ops.tersoff_eval(ell, x, k, th, energy=True, grad=True, want_theta=True)
    U, g, hw, pth, pthw = ns.tersoff_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th, None, True, True)
    assert torch.equal(U, a["energy"]) and torch.equal(g, a["grad"]) and torch.equal(pth, a["pth"]) and hw.numel() == pthw.numel() == 0
    b = ops.tersoff_eval(ell, x, k, th, w=w, energy=False, grad=True, want_theta=True)
    U, g, hw, pth, pthw = ns.tersoff_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th, w, False, True)
    assert torch.equal(g, b["grad"]) and torch.equal(hw, b["hw"]) and torch.equal(pthw, b["pthw"]) and U.numel() == pth.numel() == 0
    # without the device theta the kernels take the host copies: the same numbers (float32 of the same doubles)
    c = ops.tersoff_eval(ell, x, k, None, energy=True, grad=True)
    U, g, _, _, _ = ns.tersoff_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, None, None, True, False)
    assert torch.equal(U, c["energy"]) and torch.equal(g, c["grad"]) and torch.equal(g, a["grad"])

    def swap(i, v):
        return kk[:i] + [v] + kk[i + 1:]
    args = (x, cell, ell.col, ell.shift, ell.cnt)
    bad = [lambda: ns.tersoff_eval(x.double(), cell, ell.col, ell.shift, ell.cnt, kk, th, None, True, False),
           lambda: ns.tersoff_eval(x.cpu(), cell, ell.col, ell.shift, ell.cnt, kk, th, None, True, False),
           lambda: ns.tersoff_eval(x, cell[:5], ell.col, ell.shift, ell.cnt, kk, th, None, True, False),
           lambda: ns.tersoff_eval(x, cell, ell.col.long(), ell.shift, ell.cnt, kk, th, None, True, False),
           lambda: ns.tersoff_eval(x, cell, ell.col, ell.shift, ell.cnt[:5].contiguous(), kk, th, None, True, False),
           lambda: ns.tersoff_eval(*args, kk[:13], th, None, True, False),
           lambda: ns.tersoff_eval(*args, kk, th[:2].contiguous(), None, True, False),
           lambda: ns.tersoff_eval(*args, kk, th.double(), None, True, False),
           lambda: ns.tersoff_eval(*args, kk, th.cpu(), None, True, False),
           lambda: ns.tersoff_eval(*args, kk, th, w[:5].contiguous(), True, False),
           lambda: ns.tersoff_eval(*args, kk, th, w.double(), True, False),
           lambda: ns.tersoff_eval(*args, swap(0, 0.0), None, None, True, False),          # A
           lambda: ns.tersoff_eval(*args, swap(1, -1.0), None, None, True, False),         # B
           lambda: ns.tersoff_eval(*args, swap(2, 0.0), th, None, True, False),            # lam1
           lambda: ns.tersoff_eval(*args, swap(5, 0.0), th, None, True, False),            # n
           lambda: ns.tersoff_eval(*args, swap(7, 0.0), th, None, True, False),            # d
           lambda: ns.tersoff_eval(*args, swap(10, 0.0), th, None, True, False),           # D
           lambda: ns.tersoff_eval(*args, swap(9, 0.1), th, None, True, False),            # R <= D
           lambda: ns.tersoff_eval(*args, swap(13, 2.0), th, None, True, False),           # m
           lambda: ns.tersoff_eval(*args, swap(13, 1.5), th, None, True, False)]
    for n, fn in enumerate(bad):
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
            pytest.fail("bad input %d was accepted" % n)
