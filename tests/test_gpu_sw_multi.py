"""K28: the multi-species Stillinger-Weber term (StillingerWeberMulti, mdg_sw_multi_eval, csrc/sw_multi.hip) against the float64
definition of tests/sw_multi_ref.py (pinned to an independent loop, to the one-species definition and to the zincblende ground
state by tests/test_sw_multi_host.py, which also checks the input conditions of every case used here) and, in a trajectory,
against the CPU oracle's adjoint.

Tolerance of every kernel-vs-float64 comparison: the project's bound for the term kernels, 64 * 2^-24 * A per component, A =
the float64 sum of the absolute pair-half and triplet contributions to that component (sw_multi_ref.evaluate); `within` is
that of tests/test_gpu_sw.py and prints the largest observed err / (2^-24 A).

Observed on an MI355X, the largest err / (2^-24 A) over all cases of this file: U 4.35 (gas37), dU/dx 40.53 and H.w 46.49 (both
gas37, which holds an isolated dimer at 2.30 A like the gas case of tests/test_gpu_sw.py; the one-species kernel has 40.53 and
40.27 there, from the cancellation inside phi2' that its docstring describes), dU/dtheta 23.57 (tric64), d(w.dU/dx)/dtheta 20.42 (three replicas),
the sum of the forces 0.30; ab64 alone: 0.25, 20.67, 14.81, 20.91, 12.00, 0.30; asym64: 1.04, 20.58, 14.56, 20.91, 10.59, 0.25;
s3_64: 2.92, 14.90, 13.77, 20.96, 17.89, 0.22; the perfect zincblende lattice: U 1.84, dU/dx 5.70 on its own scale; the list
searched with a skin against float64: dU/dx 16.50, H.w 14.17.  No case exceeds 64.  S = 1 and S = 2 identical silicon sets against
the one-species float64 reference: U 1.99, dU/dx 13.19, H.w 11.80, folded dU/dtheta 22.96, folded d(w.dU/dx)/dtheta 7.28; on
the same list the energy, dU/dx and H.w equal those of ops.sw_eval bit for bit, which is asserted (one kernel text, csrc/sw_core.hpp).

Every configuration meets the input conditions of tests/test_sw_multi_host.py; one of them (sw_multi_ref.cutoff_rounding) keeps
out atoms whose only terms lie a few tenths of an Angstrom inside a cutoff: there the rounding of the cutoff to float32 alone
moves the float64 result by more than the terms' own scale allows (the first gas37 seed: 18 * 2^-24 A from that rounding, and
the kernel at 95.6 on that atom's one pair at 3.352 A under a cutoff of 3.56 A)."""
import math

import numpy as np
import pytest
import torch

import oracle as O
import sw_multi_ref as R
import sw_ref as R1
from test_gpu_parity import T, close, mk_system, DEV, oracle_run
from test_gpu_sw import within, TOL, ULP, KTOL

pytestmark = pytest.mark.gpu
F32 = np.float32
_cases = {}


def case(name):
    if not _cases:
        _cases.update(R.gpu_cases())
    return _cases[name]


def _module(x32, cell32, types, tab, system=None, **kw):
    from mdgrad_amd.interface import StillingerWeberMulti
    pair, triplet = R.pair_triplet(tab)
    return StillingerWeberMulti.from_tables(mk_system(x32, cell32) if system is None else system, types, pair, triplet, **kw)


def _thetas(mod):
    return (mod.epsilon, mod.sigma, mod.lam)


def _tab64(mod, tab):
    """The table set with the module's float32 parameters, as the float64 reference sees them."""
    return R.with_theta(tab, torch.cat([p.detach().reshape(-1) for p in _thetas(mod)]).double().cpu().numpy())


def _reference(mod, x32, cell32, types, tab, w32=None, group=None):
    tab = _tab64(mod, tab)
    ty = np.tile(np.asarray(types), x32.shape[0] // len(types))
    lst = R.pairs_and_triplets(x32, cell32, tab, group=group)
    return lst, R.evaluate(x32, ty, tab, lst, cell32, w=w32)


def _eval(mod, x, ell=None, **kw):
    from mdgrad_amd import ops
    return ops.sw_multi_eval(mod._ell if ell is None else ell, x, mod.types, mod.n_species, mod._tables(), **kw)


def _check_all_outputs(name, tag=None, system=None, seed=0):
    """U, dU/dx, H w, dU/dtheta and d(w.dU/dx)/dtheta of one launch each against float64; the energy-only launch; the sum of
    the forces; LEVEL 1 against LEVEL 2; the zeros of the pth rows."""
    from mdgrad_amd import ops
    x32, cell32, types, tab, group = case(name)
    mod = _module(x32, cell32, types, tab, system=system)
    w32 = np.random.default_rng(seed + 17).normal(0, 1, x32.shape).astype(F32)
    lst, ref = _reference(mod, x32, cell32, types, tab, w32, group)
    x, w = T(x32, DEV), T(w32, DEV)
    mod._reset_topology(x)
    o1 = _eval(mod, x, energy=True, grad=True, want_theta=True)
    o2 = _eval(mod, x, w=w, energy=False, grad=True, want_theta=True)
    o1["dth"], o2["dthw"] = ops.theta_sum(o1["pth"]), ops.theta_sum(o2["pthw"])
    tag = (tag or name) + " "
    rs = [within(o1["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + "U"),
          within(o1["grad"], ref["grad"], ref["A_grad"], tag + "dU/dx"),
          within(o2["hw"], ref["hw"], ref["A_hw"], tag + "H.w"),
          within(o1["dth"], ref["dth"], ref["A_dth"], tag + "dU/dtheta"),
          within(o2["dthw"], ref["dthw"], ref["A_dthw"], tag + "d(w.dU/dx)/dtheta")]
    assert torch.equal(o1["grad"], o2["grad"]) and o2["pth"] is None and o1["pthw"] is None, "LEVEL 1 and LEVEL 2 agree bit for bit"
    e0 = _eval(mod, x, energy=True, grad=False)                                                 # LEVEL 0
    within(e0["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + "U (energy-only launch)")
    within(o1["grad"].sum(0), torch.zeros(3), ref["A_grad"].sum(0), tag + "sum_i dU/dx_i")
    # a pth row is exactly zero outside its atom's species blocks
    S = mod.n_species
    own = torch.zeros(x.shape[0], 2 * S * S + S ** 3, dtype=torch.bool, device=DEV)
    ty = mod.types.long()
    for a in range(S):
        rows = (ty == a).nonzero().reshape(-1)
        for lo, n in ((a * S, S), (S * S + a * S, S), (2 * S * S + a * S * S, S * S)):
            own[rows[:, None], torch.arange(lo, lo + n, device=DEV)[None, :]] = True
    for key, o in (("pth", o1), ("pthw", o2)):
        assert float(o[key][~own].abs().max()) == 0.0, key + " outside the atom's species blocks"
        assert float(o[key][own].abs().max()) > 0.0
    return mod, lst, ref, o1, o2, max(rs)


# ------------------------------------------------------------------------------------------------ 1: outputs vs float64
@pytest.mark.parametrize("name", ["ab64", "asym64", "tric64", "s3_64"])
def test_outputs_vs_float64(name):
    _check_all_outputs(name)


def test_outputs_vs_float64_gas37_isolated_atom_dimer_and_a_long_row():
    mod, lst, ref, o1, o2, _ = _check_all_outputs("gas37")
    rows = lst["rows"].tolist()
    assert rows[31] == 0 and rows[32] == rows[33] == 1 and rows[0] > 16 and 37 % 16 != 0
    for o in (o1["grad"][31], o1["pth"][31], o2["hw"][31], o2["pthw"][31]):
        assert float(o.abs().max()) == 0.0, "the isolated atom"
    S = mod.n_species
    assert float(o1["pth"][32, 2 * S * S:].abs().max()) == 0.0 and float(o2["pthw"][32, 2 * S * S:].abs().max()) == 0.0, "the dimer has no lam dependence"
    assert float(o1["grad"][32].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ 2: perfect zincblende
def test_perfect_zincblende_through_the_kernel():
    """Perfect zincblende AB with Stillinger and Weber's A, B, p = 4, q = 0, a = 1.8, the nearest-neighbour distance
    2^(1/6) sigma_01 and cos0 = -1/3: U / N = -2 epsilon_01 and forces that vanish.  As in tests/test_gpu_sw.py the force scale
    is the sum over the four bonds of both product-rule terms of phi2', which cancel at the minimum."""
    tab, a0 = zincblende_tables()
    x32, cell32, types = R.zincblende(a0)
    mod = _module(x32, cell32, types, tab)
    lst, ref = _reference(mod, x32, cell32, types, tab)
    x = T(x32, DEV)
    o = _eval(mod, x, energy=True, grad=True)
    t64 = _tab64(mod, tab)
    eps, sig = t64["epsilon"][0, 1], t64["sigma"][0, 1]
    within(o["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), "perfect zincblende U")
    assert abs(float(o["energy"]) / 64 + 2 * eps) <= TOL * float(ref["A_U"]) / 64 + 1e-8 * 2 * eps
    r = a0 * math.sqrt(3) / 4
    k = R.DEFAULTS
    s, E, inv2 = sig / r, math.exp(sig / (r - k["a"] * sig)), 1.0 / (r - k["a"] * sig) ** 2
    t1 = eps * k["A"] * E * (k["p"] * k["B"] * s ** k["p"]) / r
    t2 = eps * k["A"] * E * (k["B"] * s ** k["p"] - 1.0) * sig * inv2
    A_force = ref["A_grad"] + 4 * (abs(t1) + abs(t2)) / math.sqrt(3)
    ratio = float(((o["grad"].cpu().double() - ref["grad"]).abs() / (ULP * A_force)).max())
    print("perfect zincblende dU/dx: max err / (2^-24 A) = %.2f (allowed %d)" % (ratio, KTOL))
    assert ratio <= KTOL
    assert float(ref["grad"].abs().max()) <= 1e-4 * abs(t1), "float64 forces vanish (float32 positions)"


def zincblende_tables():
    """(table set, cubic constant): sigma_01 = 2.0951 with the bond length 2^(1/6) sigma_01; sigma_00 = sigma_11 = 1.9, so that
    the second shell (like atoms, a0 / sqrt(2)) lies beyond a sigma of the like pairs."""
    si = dict(R.SILICON)
    tab = R.mixed([si, si])
    tab["sigma"][0, 0] = tab["sigma"][1, 1] = 1.9
    a0 = 2.0 ** (1.0 / 6.0) * tab["sigma"][0, 1] * 4.0 / math.sqrt(3.0)
    assert a0 / math.sqrt(2.0) > 1.8 * 1.9 * 1.02 and a0 * math.sqrt(3) / 4 < 1.8 * tab["sigma"][0, 1]
    return tab, a0


# ------------------------------------------------------------------------------------------------ 3: S = 1, S = 2 identical
@pytest.mark.parametrize("S", [1, 2])
def test_identical_silicon_sets_equal_the_one_species_reference(S):
    from mdgrad_amd import ops
    from mdgrad_amd.interface import StillingerWeber, StillingerWeberMulti
    x32, cell32 = R1.jittered_diamond(2, 5.431, 0.3, 64)
    types = R.species_split(64, S, 3)
    system = mk_system(x32, cell32)
    mod = StillingerWeberMulti(system, types, [StillingerWeberMulti.PUBLISHED["silicon"]] * S)
    one = StillingerWeber.silicon(system)
    th = [float(p.detach()) for p in (one.epsilon, one.sigma, one.lam)]
    # the precondition of the bit comparison below: both modules hold the same float32 parameters
    for name, got, want in (("epsilon", mod.epsilon, one.epsilon), ("sigma", mod.sigma, one.sigma), ("lam", mod.lam, one.lam),
                            ("lam epsilon3", mod.lam * mod._e3, one.lam * one.epsilon)):
        got, want = got.detach().cpu().reshape(-1), want.detach().cpu().reshape(-1)
        assert got.dtype == torch.float32 and torch.equal(got, want.expand_as(got)), "float32 %s of the table module" % name
    ell = one._ell                                                          # (both kernels on the same list)
    w32 = np.random.default_rng(5).normal(0, 1, x32.shape).astype(F32)
    k = R1.consts()
    lst = R1.pairs_and_triplets(x32, cell32, k["a"] * th[1])
    ref = R1.evaluate(x32, th, lst, cell32, k, w=w32)
    x, w = T(x32, DEV), T(w32, DEV)
    o1 = _eval(mod, x, ell=ell, energy=True, grad=True, want_theta=True)
    o2 = _eval(mod, x, ell=ell, w=w, energy=False, grad=True, want_theta=True)
    within(o1["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), "S = %d identical sets: U" % S)
    within(o1["grad"], ref["grad"], ref["A_grad"], "S = %d identical sets: dU/dx" % S)
    within(o2["hw"], ref["hw"], ref["A_hw"], "S = %d identical sets: H.w" % S)
    # the fold of tests/test_sw_multi_host.py: dU/deps_one = sum dU/deps + (sum lam dU/dlam) / eps, and so on
    eps, lam = th[0], th[2]
    for key, o, rk in (("pth", o1, "dth"), ("pthw", o2, "dthw")):
        g = ops.theta_sum(o[key]).double().cpu()
        ge, gs, gl = g[:S * S].sum(), g[S * S:2 * S * S].sum(), g[2 * S * S:].sum()
        fold = torch.stack([ge + lam * gl / eps, gs, gl])
        within(fold, ref[rk], ref["A_" + rk], "S = %d identical sets: folded %s" % (S, rk))
    # one text (csrc/sw_core.hpp): on the same list the table kernel and the one-species kernel run the same operations in the
    # same order on the same float32 constants, so the energy, dU/dx and H.w agree bit for bit.  (The parameter rows keep the
    # tolerance comparison above: their epsilon column means something else in the two classes.)
    b1 = ops.sw_eval(ell, x, one._consts, one._theta(), energy=True, grad=True)
    b2 = ops.sw_eval(ell, x, one._consts, one._theta(), w=w, energy=False, grad=True)
    assert torch.equal(b1["energy"], o1["energy"]) and torch.equal(b1["grad"], o1["grad"]), "LEVEL 1: U and dU/dx of ops.sw_eval"
    assert torch.equal(b2["grad"], o2["grad"]) and torch.equal(b2["hw"], o2["hw"]), "LEVEL 2: dU/dx and H.w of ops.sw_eval"


# ------------------------------------------------------------------------------------------------ 4: relabelling
def test_relabelling_the_species_permutes_the_tables_and_nothing_else():
    """Species a renamed perm[a], tables relabelled alike: U (both the energy-only and the LEVEL 1 launch), dU/dx and H.w equal
    bit for bit; the per-atom parameter rows pth (LEVEL 1) and pthw (LEVEL 2) and their column sums are the same numbers at the
    permuted places of (epsilon, sigma, lam), bit for bit."""
    from mdgrad_amd import ops
    x32, cell32, types, tab, _ = case("s3_64")
    perm = np.array([2, 0, 1])
    a = _module(x32, cell32, types, tab)
    b = _module(x32, cell32, perm[types], R.relabelled(tab, perm))
    x, w = T(x32, DEV), T(np.random.default_rng(4).normal(0, 1, x32.shape).astype(F32), DEV)
    S = 3
    # column of entry (a, b) resp. (a, b, c) of the first module's row -> its column in the relabelled module's row
    idx2 = (perm[:, None] * S + perm[None, :]).reshape(-1)
    idx3 = ((perm[:, None, None] * S + perm[None, :, None]) * S + perm[None, None, :]).reshape(-1)
    cols = torch.as_tensor(np.concatenate([idx2, S * S + idx2, 2 * S * S + idx3]), device=DEV)
    assert sorted(cols.tolist()) == list(range(2 * S * S + S ** 3))
    for kw, keys, rows in ((dict(energy=True, grad=True), ("energy", "grad"), "pth"),
                           (dict(w=w, energy=False, grad=True), ("grad", "hw"), "pthw")):
        oa, ob = _eval(a, x, want_theta=True, **kw), _eval(b, x, want_theta=True, **kw)
        for key in keys:
            assert torch.equal(oa[key], ob[key]), key
        assert float(oa[rows].abs().max()) > 0.0
        assert torch.equal(oa[rows], ob[rows][:, cols]), "the per-atom rows of %s are permuted" % rows
        assert torch.equal(ops.theta_sum(oa[rows]), ops.theta_sum(ob[rows])[cols]), "the column sums of %s are permuted" % rows
    ea, eb = _eval(a, x, energy=True, grad=False), _eval(b, x, energy=True, grad=False)
    assert torch.equal(ea["energy"], eb["energy"]), "the energy-only launch"


# ------------------------------------------------------------------------------------------------ 5: replicas
def test_three_replicas_against_each_alone_permutable_and_bitwise_repeatable():
    base, box, x3, ty16 = R.replicas16(R.SEEDS["replicas"])
    tab = R.unlike2()
    system = mk_system(base, box).replicate(3)
    mod, lst, ref, o1, o2, _ = _check_all_outputs("replicas", system=system, seed=5)
    assert int((lst["i"] // 16 != lst["j"] // 16).sum()) == 0 and int((lst["tc"] // 16 != lst["tb"] // 16).sum()) == 0
    x = T(x3, DEV)
    w = T(np.random.default_rng(22).normal(0, 1, x3.shape).astype(F32), DEV)
    F, dq, gth = mod.force_vjp(x, w)
    F2, dq2, gth2 = mod.force_vjp(x, w)
    assert torch.equal(F, F2) and torch.equal(dq, dq2) and all(torch.equal(a, b) for a, b in zip(gth, gth2))
    assert [t.shape for t in gth] == [p.shape for p in _thetas(mod)]
    ref_w = R.evaluate(x3, np.tile(ty16, 3), _tab64(mod, tab), lst, box, w=w.cpu().numpy())
    within(-torch.cat([t.reshape(-1) for t in gth]), ref_w["dthw"], ref_w["A_dthw"], "force_vjp parameter part")
    alone_w = torch.zeros(R.n_theta(tab), dtype=torch.float64)
    for r in range(3):
        sl = slice(16 * r, 16 * r + 16)
        alone = _module(x3[sl], box, ty16, tab)
        Fr, dqr, gr = alone.force_vjp(x[sl].contiguous(), w[sl].contiguous())
        within(Fr, F[sl].cpu(), ref_w["A_grad"][sl], "replica %d alone: force" % r)
        within(dqr, dq[sl].cpu(), ref_w["A_hw"][sl], "replica %d alone: d(w.F)/dx" % r)
        alone_w += torch.cat([t.reshape(-1) for t in gr]).cpu().double()
    within(torch.cat([t.reshape(-1) for t in gth]), alone_w, ref_w["A_dthw"], "parameter part: three replicas vs each alone")
    perm = torch.cat([torch.arange(16) + 16 * r for r in (2, 0, 1)]).to(DEV)
    mod._reset_topology(x[perm].contiguous())
    op = _eval(mod, x[perm].contiguous(), w=w[perm].contiguous(), energy=False, want_theta=True)
    mod._reset_topology(x)
    oo = _eval(mod, x, w=w, energy=False, want_theta=True)
    for key in ("grad", "hw", "pthw"):
        assert torch.equal(op[key], oo[key][perm]), key


# ------------------------------------------------------------------------------------------------ 6: autograd
def test_autograd_backward_and_double_backward_equal_force_vjp():
    x32, cell32, types, tab, _ = case("ab64")
    mod = _module(x32, cell32, types, tab)
    lst, ref = _reference(mod, x32, cell32, types, tab)
    x = T(x32, DEV).requires_grad_(True)
    mod(x).backward()
    within(x.grad, ref["grad"], ref["A_grad"], "backward of model(xyz) in xyz")
    got = torch.cat([p.grad.reshape(-1) for p in _thetas(mod)])
    within(got, ref["dth"], ref["A_dth"], "backward of model(xyz) in (epsilon, sigma, lam)")
    w = torch.randn(64, 3, device=DEV)
    x2 = T(x32, DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(mod(x2), x2, create_graph=True)
    hw, he, hs, hl = torch.autograd.grad((g * w).sum(), (x2,) + _thetas(mod))
    F, dq, gth = mod.force_vjp(x2.detach(), w)
    assert torch.equal(F, -g.detach()) and torch.equal(dq, -hw)
    assert [t.shape for t in gth] == [p.shape for p in mod.parameters()]
    assert torch.equal(gth[0], -he) and torch.equal(gth[1], -hs) and torch.equal(gth[2], -hl)
    assert torch.equal(mod.force(x2.detach()), F)
    frozen = _module(x32, cell32, types, tab, trainable=False)
    assert list(frozen.parameters()) == []
    assert frozen.force_vjp(x2.detach(), w)[2] == [] and frozen.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    assert torch.equal(frozen.force_vjp(x2.detach(), w)[1], dq)
    assert mod.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    # the device table follows an in-place parameter change
    xd = x2.detach()
    U0 = float(mod(xd).detach())
    dlam = float(mod.lam.grad[0, 1, 1])
    with torch.no_grad():
        mod.lam[0, 1, 1] += 0.5
    U1 = float(mod(xd).detach())
    assert U1 != U0 and abs((U1 - U0) - 0.5 * dlam) <= 2 * TOL * float(ref["A_U"]), (U1 - U0, 0.5 * dlam)


# ------------------------------------------------------------------------------------------------ 7: into / scale / accum
def test_stack_sums_equal_the_members_separate_results():
    from mdgrad_amd import ops
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    x32, cell32, types, tab, _ = case("ab64")
    system = mk_system(x32, cell32)
    sw = _module(x32, cell32, types, tab, system=system)
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
    x32, cell32, types, tab, _ = case("ab64")
    x1_32 = case("skin")[0]
    mod = _module(x32, cell32, types, tab)
    rc, skin = mod.cutoff, 0.4
    cs = _lib.make_cell(cell32)
    x0 = T(x32, DEV)
    longest = int(ops.build_ell(x0, cs, rc + skin).cnt.max())
    vl = ops.VerletList(64, 64, cs, rc, skin, None, min(63, (longest + 15) // 8 * 8), 4096, DEV)
    need = torch.zeros(2, dtype=torch.int32, device=DEV)
    vl.rebuild(x0, need)
    x1 = T(x1_32, DEV)
    vl.rebuild(x1, need)
    assert vl.builds() == 1 and need.tolist()[0] <= vl.max_nbr
    exact = ops.build_ell(x1, cs, rc)
    assert int(vl.cnt.sum()) > int(exact.cnt.sum()), "the stored list carries the skin's extra candidates"
    w32 = np.random.default_rng(8).normal(0, 1, (64, 3)).astype(F32)
    lst, ref = _reference(mod, x1_32, cell32, types, tab, w32)
    w = T(w32, DEV)
    A = {"energy": ref["A_U"].reshape(1), "grad": ref["A_grad"], "hw": ref["A_hw"]}
    for kw, keys in ((dict(energy=True), ("energy", "grad", "pth")), (dict(w=w, energy=False), ("grad", "hw", "pthw"))):
        a = _eval(mod, x1, ell=vl.ell, want_theta=True, **kw)
        b = _eval(mod, x1, ell=exact, want_theta=True, **kw)
        for key in keys:
            if key in A:
                within(a[key], b[key].cpu(), A[key], "skin list vs exact list: " + key)
            else:
                within(ops.theta_sum(a[key]), ops.theta_sum(b[key]).cpu(), ref["A_dth" if key == "pth" else "A_dthw"],
                       "skin list vs exact list: sum of " + key)
    within(a["hw"], ref["hw"], ref["A_hw"], "skin list vs float64: H.w")
    within(a["grad"], ref["grad"], ref["A_grad"], "skin list vs float64: dU/dx")
    within(ops.theta_sum(a["pthw"]), ref["dthw"], ref["A_dthw"], "skin list vs float64: d(w.dU/dx)/dtheta")


# ------------------------------------------------------------------------------------------------ 9: trainable sigma
def test_a_changed_sigma_moves_the_cutoff_and_keeps_a_sufficient_list():
    """sigma[0, 0] carries the largest a sigma of the `ab64` tables; sigma[0, 1] = sigma[1, 0] is raised until it does."""
    x32, cell32, types, tab, _ = case("ab64")
    mod = _module(x32, cell32, types, tab)
    x, w = T(x32, DEV), T(np.random.default_rng(690).normal(0, 1, x32.shape).astype(F32), DEV)
    mod.force_vjp(x, w)
    v0, ell0, c0 = mod.static_version(), mod._ell, mod.cutoff
    with torch.no_grad():
        mod.sigma[0, 1] = 2.30
        mod.sigma[1, 0] = 2.30
    F, dq, gth = mod.force_vjp(x, w)
    assert mod.static_version() != v0 and mod._ell is not ell0, "the list was searched again with the larger cutoff"
    assert abs(mod.cutoff - 1.02 * 1.78 * float(mod.sigma[0, 1].detach())) <= 1e-5 and mod.cutoff > c0
    tab1 = _tab64(mod, tab)
    fresh = _module(x32, cell32, types, tab1)
    lst, ref = _reference(fresh, x32, cell32, types, tab1, w.cpu().numpy())
    F1, dq1, gth1 = fresh.force_vjp(x, w)
    cat = lambda g: torch.cat([t.reshape(-1) for t in g])
    for got, name in ((F, "module"), (F1, "fresh module")):
        within(-got, ref["grad"], ref["A_grad"], "sigma[0,1] = 2.3, %s: force" % name)
    within(F, F1.cpu(), ref["A_grad"], "sigma[0,1] = 2.3: force vs a fresh module")
    within(dq, dq1.cpu(), ref["A_hw"], "sigma[0,1] = 2.3: d(w.F)/dx vs a fresh module")
    within(cat(gth), cat(gth1).cpu(), ref["A_dthw"], "sigma[0,1] = 2.3: parameter part vs a fresh module")
    within(-dq, ref["hw"], ref["A_hw"], "sigma[0,1] = 2.3: d(w.F)/dx vs float64")
    # a small step keeps the list and the graphs
    v1, ell1 = mod.static_version(), mod._ell
    with torch.no_grad():
        mod.sigma[0, 1] *= 1.01
        mod.sigma[1, 0] *= 1.01
    F, dq, gth = mod.force_vjp(x, w)
    assert mod.static_version() == v1 and mod._ell is ell1
    lst, ref = _reference(mod, x32, cell32, types, tab, w.cpu().numpy())
    within(-F, ref["grad"], ref["A_grad"], "sigma * 1.01 on the kept list: force")
    within(-dq, ref["hw"], ref["A_hw"], "sigma * 1.01 on the kept list: d(w.F)/dx")
    within(-cat(gth), ref["dthw"], ref["A_dthw"], "sigma * 1.01 on the kept list: parameter part")


# ------------------------------------------------------------------------------------------------ 10: trajectory + adjoint
_oracle_cache = {}
TRAJ = dict(T=0.05, Q=20.0, chains=3, dt=0.01, mass=2.0, nbins=32, r_range=(1.5, 5.0))


def traj_inputs():
    x32, cell32, types, tab, _ = case("traj")
    vel = np.random.default_rng(710).normal(0, math.sqrt(TRAJ["T"] / TRAJ["mass"]), x32.shape).astype(F32)
    return x32, cell32, types, tab, vel, np.full(64, TRAJ["mass"], dtype=F32)


def oracle_traj(t, tab):
    if "run" not in _oracle_cache:
        x32, cell32, types, _, vel, mass = traj_inputs()
        cell = T(cell32)
        terms = [R.SWMultiTerm(tab, types, cell32)]

        def loss_fn(Ls):
            _, _, gr = O.rdf_oracle(Ls[1][::2], cell, TRAJ["nbins"], TRAJ["r_range"])
            return gr.pow(2).mean() + Ls[0][-1].pow(2).mean() + 0.0 * Ls[2][-1].sum()
        _oracle_cache["run"] = oracle_run(x32, cell32, vel, mass, terms, TRAJ["T"], TRAJ["Q"], TRAJ["chains"], t, loss_fn)
    return _oracle_cache["run"]


@pytest.mark.parametrize("graphs_on", [True, False], ids=["graph_replay", "eager"])
def test_sw_multi_term_in_a_stack_trajectory_and_adjoint_vs_oracle(graphs_on):
    """Stack(StillingerWeberMulti, trainable) on 64 jittered zincblende atoms: 10 NHC steps through odeint_adjoint, the loss on
    rdf of q_t[::2] plus v_t[-1]^2 -- trajectories, adjoint of y0 and dL/d(epsilon, sigma, lam) against the oracle with
    sw_multi_ref.SWMultiTerm.  Tolerances: those of test_sw_term_in_a_stack_trajectory_and_adjoint_vs_oracle."""
    from mdgrad_amd import graphs
    from mdgrad_amd.interface import Stack
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.sovlers import odeint_adjoint
    x32, cell32, types, tab, vel, mass = traj_inputs()
    system = mk_system(x32, cell32, vel, mass)
    sw = _module(x32, cell32, types, tab, system=system)
    stack = Stack({"sw": sw})
    integ = NoseHooverChain(stack, system, T=TRAJ["T"], num_chains=TRAJ["chains"], Q=TRAJ["Q"], adjoint=True).to(DEV)
    assert integ.fused_spec("NH_verlet") is None, "the term keeps the stack off the fused trajectory kernels"
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
    traj, lam, gth = oracle_traj(t, _tab64(sw, tab))

    def report(got, want, rtol, atol, name):
        err = (got.detach().cpu().double() - want.double()).abs()
        allowed = atol + rtol * want.double().abs()
        k = int((err / allowed).argmax())
        print("%-28s observed / allowed at the worst entry: %.1e / %.1e" % (name, float(err.reshape(-1)[k]), float(allowed.reshape(-1)[k])))
        close(got, want, rtol, atol, name)
    report(q_t, traj[1], 0, 2e-5, "q_t")
    report(v_t, traj[0], 1e-3, 1e-4 * float(traj[0].abs().max()), "v_t")
    report(pv_t, traj[2], 2e-3, 1e-5, "pv_t")
    for x, l, nm in zip(y0, lam, ("adj v0", "adj q0", "adj pv0")):
        report(x.grad, l, 5e-3, 2e-3 * float(l.abs().max()) + 1e-9, nm)
    assert gth.numel() == R.n_theta(tab) and all(p.grad is not None for p in _thetas(sw))
    got = torch.cat([p.grad.reshape(-1) for p in _thetas(sw)])
    report(got, gth, 5e-3, 5e-4 * float(gth.abs().max()), "dL/d(epsilon, sigma, lam)")


# ------------------------------------------------------------------------------------------------ 11: torch ops
def test_torch_ops_equal_ctypes_path_and_reject_bad_input():
    from mdgrad_amd import _torch_ops
    ns = _torch_ops.get()
    assert ns is not None
    x32, box, types, tab, _ = case("gas37")
    mod = _module(x32, box, types, tab)
    ell, S = mod._ell, mod.n_species
    cell = _torch_ops.cell_args(ell.cell_struct)
    x, w, ty, tb = T(x32, DEV), torch.randn(37, 3, device=DEV), mod.types, mod._tables()
    a = _eval(mod, x, energy=True, grad=True, want_theta=True)
    U, g, hw, pth, pthw = ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, ty, S, tb, None, True, True)
    assert torch.equal(U, a["energy"]) and torch.equal(g, a["grad"]) and torch.equal(pth, a["pth"]) and hw.numel() == pthw.numel() == 0
    b = _eval(mod, x, w=w, energy=False, grad=True, want_theta=True)
    U, g, hw, pth, pthw = ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, ty, S, tb, w, False, True)
    assert torch.equal(g, b["grad"]) and torch.equal(hw, b["hw"]) and torch.equal(pthw, b["pthw"]) and U.numel() == pth.numel() == 0
    three = torch.zeros(12 * 9 + 4 * 27, device=DEV)
    over = ty.clone()
    over[3] = S
    bad = [lambda: ns.sw_multi_eval(x.double(), cell, ell.col, ell.shift, ell.cnt, ty, S, tb, None, True, False),
           lambda: ns.sw_multi_eval(x.cpu(), cell, ell.col, ell.shift, ell.cnt, ty, S, tb, None, True, False),
           lambda: ns.sw_multi_eval(x, cell[:5], ell.col, ell.shift, ell.cnt, ty, S, tb, None, True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col.long(), ell.shift, ell.cnt, ty, S, tb, None, True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt[:5].contiguous(), ty, S, tb, None, True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, ty.long(), S, tb, None, True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, ty[:5].contiguous(), S, tb, None, True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, ty.cpu(), S, tb, None, True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, over, S, tb, None, True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, -ty - 1, S, tb, None, True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, ty, 0, tb, None, True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, ty, 5, tb, None, True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, ty, S, three, None, True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, ty, S, tb.double(), None, True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, ty, S, tb.cpu(), None, True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, ty, S, tb, w[:5].contiguous(), True, False),
           lambda: ns.sw_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, ty, S, tb, w.double(), True, False)]
    for n, fn in enumerate(bad):
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
            pytest.fail("bad input %d was accepted" % n)
