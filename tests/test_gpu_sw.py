"""K23: the Stillinger-Weber term (StillingerWeber, mdg_sw_eval, csrc/sw.hip on csrc/sw_core.hpp) against the float64 definition of tests/sw_ref.py
(pinned to an independent loop and to the diamond ground state by tests/test_sw_host.py) and, in a trajectory, against the CPU
oracle's adjoint.

Tolerance of every kernel-vs-float64 comparison: K * 2^-24 * A per component with K = 64, A = the float64 sum of the absolute
pair and triplet contributions to that component (sw_ref.evaluate): a few ulp per term from sqrtf / expf / the divisions, the
conditioning of gamma sigma / (r - a sigma) near the cutoff, plus a few dozen sequential float32 additions per lane.  `within`
prints the largest observed err / (2^-24 A); on an MI355X the largest over all cases of this file were U 5.51 (perfect lattice),
dU/dx 40.53, H.w 40.27 (both on the isolated dimer of the 37-atom set), dU/dtheta 21.80 (Si-64), d(w.dU/dx)/dtheta 4.34, the
sum of the forces 2.10; Si-64 alone: 1.99, 12.20, 12.68, 21.80, 1.51, 0.30.  With the gather of csrc/sw_core.hpp (the same terms,
the additions in the order of the multi-species kernel) the maxima are the same five figures and the sum of the forces 0.56;
Si-64 alone: 1.99, 13.19, 11.58, 21.80, 1.63, 0.30.

Why some exceed 16, and why K stays 64: phi2' = eps A E [-(p B s^p - q s^q) / r - (B s^p - s^q) sigma / (r - a sigma)^2] is the
sum of two product-rule terms of opposite sign that cancel at the minimum of phi2 (r = 2.35 A for silicon).  A counts the net
contribution of a pair, but each term carries the rounding of r = sqrtf(d2) on its own: on the dimer of the 37-atom set
(r = 2.30 A) the terms are 4.74 eV/A in absolute sum against a net 0.57 eV/A, 8.3 times A, so 40.5 there is 4.9 on the scale of
what is actually added, and float32 autograd of sw_ref.energy itself is off by 26.5 * 2^-24 A at that atom.  dU/dsigma has the
same root (sigma dphi2/dsigma = -r phi2').  This is the conditioning of the function at float32 inputs, not a cancelling
formula in the kernel, and it is not the cutoff: pairs near a sigma contribute exp(-large).  K is not raised."""
import math

import numpy as np
import pytest
import torch

import coulomb_ref as CR
import oracle as O
import sw_ref as R
from conftest import load_golden
from test_gpu_parity import T, close, mk_system, DEV, oracle_run

pytestmark = pytest.mark.gpu
F32 = np.float32
ULP = 2.0 ** -24
KTOL = 64
TOL = KTOL * ULP
K = R.consts()
SI = (R.SILICON["epsilon"], R.SILICON["sigma"], R.SILICON["lam"])


def within(got, want, A, what):
    """|got - want| <= TOL * A per component; returns (and prints) the largest err / (2^-24 A)."""
    got = got.detach().cpu().double().reshape(-1)
    want, A = torch.as_tensor(want).detach().double().reshape(-1), torch.as_tensor(A).detach().double().reshape(-1)
    assert got.shape == want.shape == A.shape, "%s: shapes %s %s %s" % (what, got.shape, want.shape, A.shape)
    assert bool(torch.isfinite(got).all()), what + ": non-finite"
    err = (got - want).abs()
    ratio = float((err[A > 0] / (ULP * A[A > 0])).max()) if bool((A > 0).any()) else 0.0
    print("%-60s max err / (2^-24 A) = %6.2f  (allowed %d)" % (what, ratio, KTOL))
    bad = err > TOL * A
    assert not bool(bad.any()), "%s: err %.3e at A = %.3e, ratio %.1f > %d" % (what, float(err[bad].max()), float(A[bad].min()), ratio, KTOL)
    return ratio


def _module(x32, cell32, theta=SI, system=None, **kw):
    from mdgrad_amd.interface import StillingerWeber
    return StillingerWeber(mk_system(x32, cell32) if system is None else system, theta[0], theta[1], lam=theta[2], **kw)


def _theta64(mod):
    """The module's float32 parameters, as the float64 reference sees them."""
    return [float(p.detach()) for p in (mod.epsilon, mod.sigma, mod.lam)]


def _reference(mod, x32, cell32, w32=None, group=None):
    th = _theta64(mod)
    lst = R.pairs_and_triplets(x32, cell32, K["a"] * th[1], group=group)
    return lst, R.evaluate(x32, th, lst, cell32, K, w=w32)


def _check_all_outputs(x32, cell32, tag, theta=SI, group=None, system=None, seed=0):
    """U, dU/dx, H w, dU/dtheta and d(w.dU/dx)/dtheta of one launch each against float64; the energy-only launch; the sum of
    the forces."""
    from mdgrad_amd import ops
    mod = _module(x32, cell32, theta, system=system)
    w32 = np.random.default_rng(seed + 17).normal(0, 1, x32.shape).astype(F32)
    lst, ref = _reference(mod, x32, cell32, w32, group)
    x, w = T(x32, DEV), T(w32, DEV)
    mod._reset_topology(x)
    o1 = ops.sw_eval(mod._ell, x, mod._consts, mod._theta(), energy=True, grad=True, want_theta=True)
    o2 = ops.sw_eval(mod._ell, x, mod._consts, mod._theta(), w=w, energy=False, grad=True, want_theta=True)
    o1["dth"], o2["dthw"] = ops.sw_theta_sum(o1["pth"]), ops.sw_theta_sum(o2["pthw"])
    tag += " "
    rs = [within(o1["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + "U"),
          within(o1["grad"], ref["grad"], ref["A_grad"], tag + "dU/dx"),
          within(o2["hw"], ref["hw"], ref["A_hw"], tag + "H.w"),
          within(o1["dth"], ref["dth"], ref["A_dth"], tag + "dU/dtheta"),
          within(o2["dthw"], ref["dthw"], ref["A_dthw"], tag + "d(w.dU/dx)/dtheta")]
    assert torch.equal(o1["grad"], o2["grad"]) and o2["pth"] is None and o1["pthw"] is None
    e0 = ops.sw_eval(mod._ell, x, mod._consts, mod._theta(), energy=True, grad=False)               # LEVEL 0
    within(e0["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + "U (energy-only launch)")
    # translation invariance: the end-atom part of every triplet must balance its centre part
    within(o1["grad"].sum(0), torch.zeros(3), ref["A_grad"].sum(0), tag + "sum_i dU/dx_i")
    return mod, lst, ref, o1, o2, max(rs)


def _gas37():
    """33 + 1 atoms drawn in a 7.5 A corner (minimum separation 2.0) of a 14 x 15 x 16 box, one atom far from everything
    (index 33), and two atoms that only see each other (34, 35)."""
    rng = np.random.default_rng(37)
    pts = []
    while len(pts) < 34:
        p = rng.uniform(0, 7.5, 3)
        if all(np.linalg.norm(p - q) >= 2.0 for q in pts):
            pts.append(p)
    x = np.array(pts[:33] + [[11.0, 11.5, 12.0], [11.0, 4.0, 11.0], [11.0, 4.0, 13.3]] + pts[33:])
    return x.astype(F32), np.array([14.0, 15.0, 16.0], dtype=F32)


# ------------------------------------------------------------------------------------------------ 1 - 4: outputs vs float64
def test_outputs_vs_float64_jittered_si64():
    """2 x 2 x 2 diamond cells (a0 = 5.431) jittered by 0.3 A, seed 64: rows of 6 to 13 neighbours inside a sigma, 2 366
    triplets, many pairs close to the cutoff."""
    x32, cell32 = R.jittered_diamond(2, 5.431, 0.3, 64)
    mod, lst, ref, o1, o2, _ = _check_all_outputs(x32, cell32, "si64")
    assert lst["tc"].numel() > 2000 and int(lst["rows"].max()) >= 12


def test_outputs_vs_float64_gas37_with_an_empty_row_and_a_row_of_one():
    x32, box = _gas37()
    mod, lst, ref, o1, o2, _ = _check_all_outputs(x32, box, "gas37")
    rows = lst["rows"].tolist()
    assert rows[33] == 0 and rows[34] == rows[35] == 1 and max(rows) >= 8 and 37 % 16 != 0
    assert int(mod._ell.cnt[33]) == 0 and int(mod._ell.cnt[34]) == 1
    for o in (o1["grad"][33], o1["pth"][33], o2["hw"][33], o2["pthw"][33]):
        assert float(o.abs().max()) == 0.0, "the atom with the empty row"
    assert float(o1["pth"][34, 2].abs()) == 0.0 and float(o1["grad"][34].abs().max()) > 0.0, "one neighbour: a pair, no triplet"


def test_outputs_vs_float64_triclinic64():
    g = load_golden("nbr_tric64")
    sigma = float(g["cutoff"]) / K["a"]
    mod, lst, ref, o1, o2, _ = _check_all_outputs(g["xyz"].astype(F32), g["cell"].astype(F32), "tric64", theta=(1.0, sigma, 21.0))
    assert int(lst["rows"].max()) > 16, "rows longer than the lanes of an atom"


def test_perfect_diamond_through_the_kernel():
    """Perfect 2 x 2 x 2 diamond at a0 = 5.431 (float32 positions): U / N = -2 epsilon and forces that vanish.
    At the minimum of phi2 the two product-rule terms of phi2' = eps A E [-(p B s^p - q s^q) / r - (B s^p - s^q) sigma /
    (r - a sigma)^2] cancel (2.18 epsilon / sigma each against a net 5e-4 epsilon / sigma), so the net contribution of a pair
    does not scale the rounding of either: the force scale here is the sum over the four bonds of both terms' absolute values."""
    from mdgrad_amd import ops
    x32, cell32 = R.jittered_diamond(2, 5.431, 0.0)
    mod = _module(x32, cell32)
    lst, ref = _reference(mod, x32, cell32)
    assert lst["rows"].tolist() == [4] * 64
    x = T(x32, DEV)
    o = ops.sw_eval(mod._ell, x, mod._consts, mod._theta(), energy=True, grad=True)
    eps, sig, _ = _theta64(mod)
    within(o["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), "perfect si64 U")
    assert abs(float(o["energy"]) / 64 + 2 * eps) <= TOL * float(ref["A_U"]) / 64 + 1e-8 * 2 * eps
    r = 5.431 * math.sqrt(3) / 4
    s, E, inv2 = sig / r, math.exp(sig / (r - K["a"] * sig)), 1.0 / (r - K["a"] * sig) ** 2
    t1 = eps * K["A"] * E * (K["p"] * K["B"] * s ** K["p"] - K["q"] * s ** K["q"]) / r
    t2 = eps * K["A"] * E * (K["B"] * s ** K["p"] - s ** K["q"]) * sig * inv2
    assert abs(t1 + t2) <= 1e-3 * abs(t1), "the bond sits in the minimum of phi2"
    A_force = ref["A_grad"] + 4 * (abs(t1) + abs(t2)) / math.sqrt(3)
    ratio = float(((o["grad"].cpu().double() - ref["grad"]).abs() / (ULP * A_force)).max())
    print("perfect si64 dU/dx: max err / (2^-24 A) = %.2f (allowed %d)" % (ratio, KTOL))
    assert ratio <= KTOL
    assert float(ref["grad"].abs().max()) <= 1e-4 * abs(t1), "float64 forces vanish (float32 positions)"


# ------------------------------------------------------------------------------------------------ 5: replicas
def _replicas24():
    box = np.array([8.0, 8.0, 8.5], dtype=F32)
    base = CR.seeded_gas(24, box, 2.0, seed=24)
    rng = np.random.default_rng(240)
    x32 = np.concatenate([np.mod(base + rng.normal(0, 0.1, base.shape), box) for _ in range(3)]).astype(F32)
    return base, box, x32


def test_parameter_gradients_on_three_replicas_bitwise_repeatable_and_permutable():
    from mdgrad_amd import ops
    base, box, x32 = _replicas24()
    system = mk_system(base, box).replicate(3)
    mod, lst, ref, o1, o2, _ = _check_all_outputs(x32, box, "3 x gas24", group=24, system=system, seed=5)
    assert int((lst["i"] // 24 != lst["j"] // 24).sum()) == 0 and int((lst["tc"] // 24 != lst["tb"] // 24).sum()) == 0
    x = T(x32, DEV).requires_grad_(True)
    w = T(np.random.default_rng(22).normal(0, 1, x32.shape).astype(F32), DEV)
    params = (mod.epsilon, mod.sigma, mod.lam)
    g = torch.autograd.grad(mod(x), (x,) + params, create_graph=True)
    h = torch.autograd.grad((g[0] * w).sum(), params)
    within(torch.cat([t.reshape(1) for t in g[1:]]), ref["dth"], ref["A_dth"], "autograd dU/dtheta on three replicas")
    ref_w = R.evaluate(x32, _theta64(mod), lst, box, K, w=w.cpu().numpy())
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
    op = ops.sw_eval(mod._ell, xd[perm].contiguous(), mod._consts, mod._theta(), w=w[perm].contiguous(), energy=False, want_theta=True)
    mod._reset_topology(xd)
    oo = ops.sw_eval(mod._ell, xd, mod._consts, mod._theta(), w=w, energy=False, want_theta=True)
    for key in ("grad", "hw", "pthw"):
        assert torch.equal(op[key], oo[key][perm]), key


# ------------------------------------------------------------------------------------------------ 6: autograd
def test_autograd_backward_and_double_backward_equal_force_vjp():
    x32, cell32 = R.jittered_diamond(2, 5.431, 0.3, 70)
    mod = _module(x32, cell32)
    lst, ref = _reference(mod, x32, cell32)
    x = T(x32, DEV).requires_grad_(True)
    mod(x).backward()
    within(x.grad, ref["grad"], ref["A_grad"], "backward of model(xyz) in xyz")
    got = torch.cat([p.grad.reshape(1) for p in (mod.epsilon, mod.sigma, mod.lam)])
    within(got, ref["dth"], ref["A_dth"], "backward of model(xyz) in (epsilon, sigma, lam)")
    w = torch.randn(64, 3, device=DEV)
    x2 = T(x32, DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(mod(x2), x2, create_graph=True)
    hw, he, hs, hl = torch.autograd.grad((g * w).sum(), (x2, mod.epsilon, mod.sigma, mod.lam))
    F, dq, gth = mod.force_vjp(x2.detach(), w)
    assert torch.equal(F, -g.detach()) and torch.equal(dq, -hw)
    assert [t.shape for t in gth] == [p.shape for p in mod.parameters()]
    assert torch.equal(gth[0], -he) and torch.equal(gth[1], -hs) and torch.equal(gth[2], -hl)
    assert torch.equal(mod.force(x2.detach()), F)
    frozen = _module(x32, cell32, trainable=False)
    assert list(frozen.parameters()) == []
    assert frozen.force_vjp(x2.detach(), w)[2] == [] and frozen.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    assert torch.equal(frozen.force_vjp(x2.detach(), w)[1], dq)
    assert mod.force_vjp(x2.detach(), w, want_theta=False)[2] is None


# ------------------------------------------------------------------------------------------------ 7: into / scale / accum
def test_stack_sums_equal_the_members_separate_results():
    """Stack({"lj", "sw"}).force and .force_vjp (the SW launch adds onto the pair term's buffers) against the sum of the members'
    separate results, to 2^-22 of the largest entry; the same for `accum` against the list return."""
    from mdgrad_amd import ops
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    x32, cell32 = R.jittered_diamond(2, 5.431, 0.3, 66)
    system = mk_system(x32, cell32)
    sw = _module(x32, cell32, system=system)
    lj = PairPotentials(system, P.LJFamily(2.0, 0.1), cutoff=sw.cutoff)
    stack = Stack({"lj": lj, "sw": sw})
    assert stack.supports_force_vjp() and stack.supports_static_topology()
    x, w = T(x32, DEV), torch.randn(64, 3, device=DEV)
    stack._reset_topology(x)
    assert lj._ell is sw._ell, "one search for both members"

    def same(a, b, what):
        assert float((a - b).abs().max()) <= 2.0 ** -22 * float(b.abs().max()), what
    same(stack.force(x), lj.force(x) + sw.force(x), "force")
    F, dq, gth = stack.force_vjp(x, w)
    f1, d1, g1 = lj.force_vjp(x, w)
    f2, d2, g2 = sw.force_vjp(x, w)
    same(F, f1 + f2, "force (vjp)")
    same(dq, d1 + d2, "d(w.F)/dx")
    params = list(stack.parameters())
    assert len(gth) == len(params) == 5
    by_id = {id(p): v for p, v in zip(list(lj.parameters()) + list(sw.parameters()), g1 + g2)}
    for p, v in zip(params, gth):
        same(v, by_id[id(p)], "parameter part")
    acc = ops.ThetaAccum(params)
    acc.flat.fill_(0.25)
    assert stack.force_vjp(x, w, accum=acc)[2] is None
    for v, want in zip(acc.views(), gth):
        assert float((v - 0.25 - want).abs().max()) <= 2.0 ** -22 * max(float(want.abs().max()), 0.25), "accum vs list"
    # a flat buffer in which the three parameters are not adjacent
    acc2 = ops.ThetaAccum([sw.lam, lj.model.sigma, sw.epsilon, sw.sigma])
    assert sw.force_vjp(x, w, accum=acc2)[2] is None
    for v, want in zip(acc2.views(), [g2[2], torch.zeros(1, device=DEV), g2[0], g2[1]]):
        assert float((v - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max()), "accum, scattered offsets"
    F0, D0 = torch.randn_like(x), torch.randn_like(x)
    F1, D1, _ = sw.force_vjp(x, w, into=(F0.clone(), D0.clone()))
    same(F1 - F0, f2, "force added onto a buffer")
    same(D1 - D0, d2, "d(w.F)/dx added onto a buffer")


# ------------------------------------------------------------------------------------------------ 8: skin list
def test_evaluation_on_a_list_searched_with_a_skin_equals_a_fresh_exact_list():
    from mdgrad_amd import _lib, ops
    x32, cell32 = R.jittered_diamond(2, 5.431, 0.3, 67)
    mod = _module(x32, cell32)
    rc, skin = mod.cutoff, 0.4
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
    w32 = rng.normal(0, 1, (64, 3)).astype(F32)
    lst, ref = _reference(mod, x1_32, cell32, w32)
    w = T(w32, DEV)
    A = {"energy": ref["A_U"].reshape(1), "grad": ref["A_grad"], "hw": ref["A_hw"]}
    for kw, keys in ((dict(energy=True), ("energy", "grad", "pth")), (dict(w=w, energy=False), ("grad", "hw", "pthw"))):
        a = ops.sw_eval(vl.ell, x1, mod._consts, mod._theta(), want_theta=True, **kw)
        b = ops.sw_eval(exact, x1, mod._consts, mod._theta(), want_theta=True, **kw)
        for key in keys:
            if key in A:
                within(a[key], b[key].cpu(), A[key], "skin list vs exact list: " + key)
            else:
                within(ops.sw_theta_sum(a[key]), ops.sw_theta_sum(b[key]).cpu(), ref["A_dth" if key == "pth" else "A_dthw"],
                       "skin list vs exact list: sum of " + key)
    within(a["hw"], ref["hw"], ref["A_hw"], "skin list vs float64: H.w")
    within(a["grad"], ref["grad"], ref["A_grad"], "skin list vs float64: dU/dx")


# ------------------------------------------------------------------------------------------------ 9: trainable sigma
def test_a_changed_sigma_moves_the_cutoff_and_keeps_a_sufficient_list():
    x32, cell32 = R.jittered_diamond(2, 5.431, 0.3, 69)
    mod = _module(x32, cell32, theta=(SI[0], 1.9, SI[2]))
    x, w = T(x32, DEV), T(np.random.default_rng(690).normal(0, 1, x32.shape).astype(F32), DEV)
    mod.force_vjp(x, w)
    v0, ell0 = mod.static_version(), mod._ell
    with torch.no_grad():
        mod.sigma.mul_(1.1)
    F, dq, gth = mod.force_vjp(x, w)
    assert mod.static_version() != v0 and mod._ell is not ell0, "the list was searched again with the larger cutoff"
    assert abs(mod.cutoff - 1.02 * K["a"] * float(mod.sigma.detach())) <= 1e-5
    sig1 = float(mod.sigma.detach())
    fresh = _module(x32, cell32, theta=(SI[0], sig1, SI[2]))
    assert float(fresh.sigma.detach()) == sig1
    lst, ref = _reference(fresh, x32, cell32, w.cpu().numpy())
    F1, dq1, gth1 = fresh.force_vjp(x, w)
    for got, name in ((F, "module"), (F1, "fresh module")):
        within(-got, ref["grad"], ref["A_grad"], "sigma * 1.1, %s: force" % name)
    within(F, F1.cpu(), ref["A_grad"], "sigma * 1.1: force vs a fresh module")
    within(dq, dq1.cpu(), ref["A_hw"], "sigma * 1.1: d(w.F)/dx vs a fresh module")
    within(torch.cat(gth), torch.cat(gth1).cpu(), ref["A_dthw"], "sigma * 1.1: parameter part vs a fresh module")
    within(-dq, ref["hw"], ref["A_hw"], "sigma * 1.1: d(w.F)/dx vs float64")
    # a small step keeps the list and the graphs
    v1, ell1 = mod.static_version(), mod._ell
    with torch.no_grad():
        mod.sigma.mul_(1.01)
    F, dq, gth = mod.force_vjp(x, w)
    assert mod.static_version() == v1 and mod._ell is ell1
    lst, ref = _reference(mod, x32, cell32, w.cpu().numpy())
    within(-F, ref["grad"], ref["A_grad"], "sigma * 1.01 on the kept list: force")
    within(-dq, ref["hw"], ref["A_hw"], "sigma * 1.01 on the kept list: d(w.F)/dx")
    within(-torch.cat(gth), ref["dthw"], ref["A_dthw"], "sigma * 1.01 on the kept list: parameter part")


# ------------------------------------------------------------------------------------------------ 10: trajectory + adjoint
_oracle_cache = {}
TRAJ = dict(T=0.05, Q=20.0, chains=3, dt=0.01, mass=2.0, nbins=32, r_range=(1.5, 5.0))


def traj_inputs():
    x32, cell32 = R.jittered_diamond(2, 5.431, 0.15, 71)
    vel = np.random.default_rng(710).normal(0, math.sqrt(TRAJ["T"] / TRAJ["mass"]), x32.shape).astype(F32)
    return x32, cell32, vel, np.full(64, TRAJ["mass"], dtype=F32)


def oracle_traj(t):
    if "run" not in _oracle_cache:
        x32, cell32, vel, mass = traj_inputs()
        cell = T(cell32)
        terms = [R.SWTerm(SI[0], SI[1], SI[2], cell32)]

        def loss_fn(Ls):
            _, _, gr = O.rdf_oracle(Ls[1][::2], cell, TRAJ["nbins"], TRAJ["r_range"])
            return gr.pow(2).mean() + Ls[0][-1].pow(2).mean() + 0.0 * Ls[2][-1].sum()
        _oracle_cache["run"] = oracle_run(x32, cell32, vel, mass, terms, TRAJ["T"], TRAJ["Q"], TRAJ["chains"], t, loss_fn)
    return _oracle_cache["run"]


@pytest.mark.parametrize("graphs_on", [True, False], ids=["graph_replay", "eager"])
def test_sw_term_in_a_stack_trajectory_and_adjoint_vs_oracle(graphs_on):
    """Stack(StillingerWeber, trainable) on 64 jittered silicon atoms: 10 NHC steps through odeint_adjoint, the loss on rdf of
    q_t[::2] plus v_t[-1]^2 -- trajectories, adjoint of y0 and dL/d(epsilon, sigma, lam) against the oracle with
    sw_ref.SWTerm.  The stack stays on the analytic adjoint (force_vjp) and HIP-graph replay although the parameters require
    grad.  Tolerances: those of test_coulomb_term_in_a_stack_trajectory_and_adjoint_vs_oracle (the project's for this oracle
    and horizon).
    Observed on an MI355X (MDG_TEST_REPORT; graph replay and eager alike), observed / allowed at the worst entry: q_t 2.4e-07 /
    2.0e-05, v_t 8.9e-08 / 4.3e-04, pv_t 3.0e-08 / 4.7e-04, adj v0 3.3e-09 / 4.7e-05, adj q0 4.4e-08 / 2.1e-04, adj pv0 2.9e-11 /
    2.6e-06, dL/d(epsilon, sigma, lam) 1.9e-09 / 1.5e-04."""
    from mdgrad_amd import graphs
    from mdgrad_amd.interface import Stack
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.sovlers import odeint_adjoint
    x32, cell32, vel, mass = traj_inputs()
    system = mk_system(x32, cell32, vel, mass)
    sw = _module(x32, cell32, system=system)
    stack = Stack({"sw": sw})
    integ = NoseHooverChain(stack, system, T=TRAJ["T"], num_chains=TRAJ["chains"], Q=TRAJ["Q"], adjoint=True).to(DEV)
    assert integ.fused_spec("NH_verlet") is None, "an SW member keeps the stack off the fused trajectory kernels"
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
    assert gth.numel() == 3 and all(p.grad is not None for p in (sw.epsilon, sw.sigma, sw.lam))
    got = torch.cat([p.grad.reshape(1) for p in (sw.epsilon, sw.sigma, sw.lam)])
    close(got, gth, 5e-3, 5e-4 * float(gth.abs().max()), "dL/d(epsilon, sigma, lam)")


# ------------------------------------------------------------------------------------------------ 11: torch ops
def test_torch_ops_equal_ctypes_path_and_reject_bad_input():
    from mdgrad_amd import _torch_ops, ops
    ns = _torch_ops.get()
    assert ns is not None
    x32, box = _gas37()
    mod = _module(x32, box)
    ell, k = mod._ell, mod._consts
    cell = _torch_ops.cell_args(ell.cell_struct)
    kk = [k.epsilon, k.sigma, k.lam, k.a, k.gamma, k.cos0, k.A, k.B, float(k.p), float(k.q)]
    x, w, th = T(x32, DEV), torch.randn(37, 3, device=DEV), mod._theta()
    a = ops.sw_eval(ell, x, k, th, energy=True, grad=True, want_theta=True)
    U, g, hw, pth, pthw = ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th, None, True, True)
    assert torch.equal(U, a["energy"]) and torch.equal(g, a["grad"]) and torch.equal(pth, a["pth"]) and hw.numel() == pthw.numel() == 0
    b = ops.sw_eval(ell, x, k, th, w=w, energy=False, grad=True, want_theta=True)
    U, g, hw, pth, pthw = ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th, w, False, True)
    assert torch.equal(g, b["grad"]) and torch.equal(hw, b["hw"]) and torch.equal(pthw, b["pthw"]) and U.numel() == pth.numel() == 0
    # without the device theta the kernel takes the host copies: the same numbers (float32 of the same doubles)
    c = ops.sw_eval(ell, x, k, None, energy=True, grad=True)
    U, g, _, _, _ = ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, None, None, True, False)
    assert torch.equal(U, c["energy"]) and torch.equal(g, c["grad"]) and torch.equal(g, a["grad"])
    bad = [lambda: ns.sw_eval(x.double(), cell, ell.col, ell.shift, ell.cnt, kk, th, None, True, False),
           lambda: ns.sw_eval(x.cpu(), cell, ell.col, ell.shift, ell.cnt, kk, th, None, True, False),
           lambda: ns.sw_eval(x, cell[:5], ell.col, ell.shift, ell.cnt, kk, th, None, True, False),
           lambda: ns.sw_eval(x, cell, ell.col.long(), ell.shift, ell.cnt, kk, th, None, True, False),
           lambda: ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt[:5].contiguous(), kk, th, None, True, False),
           lambda: ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, kk[:9], th, None, True, False),
           lambda: ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th[:2].contiguous(), None, True, False),
           lambda: ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th.double(), None, True, False),
           lambda: ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th.cpu(), None, True, False),
           lambda: ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th, w[:5].contiguous(), True, False),
           lambda: ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, kk, th, w.double(), True, False),
           lambda: ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, [kk[0], 0.0] + kk[2:], None, None, True, False),
           lambda: ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, [kk[0], -2.0] + kk[2:], None, None, True, False),
           lambda: ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, [0.0] + kk[1:], None, None, True, False),
           lambda: ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, kk[:8] + [4.0, 4.0], th, None, True, False),
           lambda: ns.sw_eval(x, cell, ell.col, ell.shift, ell.cnt, kk[:8] + [4.5, 0.0], th, None, True, False)]
    for n, fn in enumerate(bad):
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
            pytest.fail("bad input %d was accepted" % n)
