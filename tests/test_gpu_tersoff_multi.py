"""K26: the multi-species Tersoff term (TersoffMulti, mdg_tersoff_multi_eval, csrc/tersoff_multi.hip) against the float64
definition of tests/tersoff_multi_ref.py (pinned to an independent loop, to zincblende SiC and diamond Ge in closed form and to
the one-species definition by tests/test_tersoff_multi_host.py, which also checks the input conditions of every configuration
used here) and, in a trajectory, against the CPU oracle's adjoint.

Tolerance of every kernel-vs-float64 comparison: K * 2^-24 * A per component with K = 64, the project's bound for the term
kernels (tests/test_gpu_tersoff.py), A = the float64 sum of the absolute contributions of the bond halves and the triplet terms
to that component (tersoff_multi_ref.evaluate).  `within` (tests/test_gpu_sw.py) prints the largest observed err / (2^-24 A).

On an MI355X the largest observed ratios over all cases of this file were U 3.45 (the perfect lattice), dU/dx 15.49 (three
replicas of the 16-atom gas), H.w 54.26 (s3_64), dU/dtheta 23.22 (s3_64), d(w.dU/dx)/dtheta 8.37 (gas37), the sum of the forces
0.09; sic_alloy64 alone: 0.11, 9.18, 21.56, 4.43, 2.62, 0.02; tric64: 0.36, 6.93, 40.53, 3.68, 5.80; on the list searched with a
skin, against float64: dU/dx 5.04, H.w 19.39.  No case exceeds 64.  H.w is the largest throughout, as for the one-species kernel.
The single-species limits (S = 1 and S = 2 with identical silicon sets on si64) against the one-species float64 reference: U
2.40, dU/dx 6.54, H.w 22.80, dU/d(A, B, h) 4.90, d(w.dU/dx)/d(A, B, h) 1.43.  They are NOT bit-identical to the outputs of the
one-species kernel (U, dU/dx and H.w all differ in the last bits), although both run the same code (csrc/tersoff_core.hpp):
the table holds constants derived in float64 on the host (pi / (2 D), -1/(2n), gamma (c/d)^2 ...), the one-species kernel
derives them in float32 from its arguments, and the two do not round alike."""
import numpy as np
import pytest
import torch

import oracle as O
import tersoff_multi_ref as M
import tersoff_ref as R1
from test_gpu_parity import T, close, mk_system, DEV, oracle_run
from test_gpu_sw import within

pytestmark = pytest.mark.gpu
F32 = np.float32
ULP = 2.0 ** -24
TOL = 64 * ULP
CASES = {}
_refs = {}


def case(name):
    if not CASES:
        CASES.update(M.gpu_cases())
    return CASES[name]


def _module(x32, cell32, ty, tab, system=None, **kw):
    from mdgrad_amd.interface import TersoffMulti
    return TersoffMulti.from_tables(mk_system(x32, cell32) if system is None else system, ty, *M.pair_centre(tab), **kw)


def _tab32(mod, tab):
    """The table set with the module's float32 parameters, as the float64 reference sees them."""
    return dict(tab, **{k: getattr(mod, k).detach().cpu().double().numpy() for k in ("A", "B", "h")})


def _w(name, shape):
    return np.random.default_rng(sum(map(ord, name))).normal(0, 1, shape).astype(F32)


def _all_types(ty, x32, group):
    return np.tile(ty, len(x32) // (group or len(x32)))


def _reference(name, mod):
    """(list, float64 evaluation with the w of the case) -- computed once per case and shared."""
    if name not in _refs:
        x32, cell32, ty, tab, group = case(name)
        lst = M.bonds_and_triplets(x32, cell32, tab, group=group)
        _refs[name] = (lst, M.evaluate(x32, _all_types(ty, x32, group), _tab32(mod, tab), lst, cell32, w=_w(name, x32.shape)))
    return _refs[name]


def _eval(mod, x, ell=None, **kw):
    from mdgrad_amd import ops
    return ops.tersoff_multi_eval(mod._ell if ell is None else ell, x, mod.types, mod.n_species, mod._tables(),
                                  work=None if ell is not None else mod._scratch(), **kw)


def _flat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def _check_all_outputs(name, system=None):
    """U, dU/dx, H w, dU/dtheta and d(w.dU/dx)/dtheta of one call each against float64; the energy-only call; the sum of the
    forces; dU/dx of the LEVEL 1 and the LEVEL 2 launch bit for bit."""
    from mdgrad_amd import ops
    x32, cell32, ty, tab, group = case(name)
    mod = _module(x32, cell32, ty, tab, system=system)
    lst, ref = _reference(name, mod)
    x, w = T(x32, DEV), T(_w(name, x32.shape), DEV)
    mod._reset_topology(x)
    o1 = _eval(mod, x, energy=True, grad=True, want_theta=True)
    o2 = _eval(mod, x, w=w, energy=False, grad=True, want_theta=True)
    P = M.n_theta(tab)
    assert o1["pth"].shape == (len(x32), P) and o2["pthw"].shape == (len(x32), P)
    o1["dth"], o2["dthw"] = ops.tersoff_multi_theta_sum(o1["pth"]), ops.tersoff_multi_theta_sum(o2["pthw"])
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
    within(o1["grad"].sum(0), torch.zeros(3), ref["A_grad"].sum(0), tag + "sum_i dU/dx_i")
    # a row of the per-atom parameter table is zero outside the blocks of its atom's species
    S = tab["S"]
    t_all = torch.as_tensor(_all_types(ty, x32, group)).long()
    owner = torch.cat([torch.arange(S).repeat_interleave(S), torch.arange(S).repeat_interleave(S), torch.arange(S)])
    foreign = owner[None, :] != t_all[:, None]
    assert float(o1["pth"].cpu()[foreign].abs().max()) == 0.0 and float(o2["pthw"].cpu()[foreign].abs().max()) == 0.0
    return mod, lst, ref, o1, o2


# ------------------------------------------------------------------------------------------------ 1, 2: outputs vs float64
def test_outputs_vs_float64_random_sic_alloy64():
    """2 x 2 x 2 diamond cells (a = 4.6), 32 Si + 32 C in random order, every coordinate jittered by 0.25 A: bonds inside the
    taper of each of the four ordered species pairs, each of the 8 (centre, end, third) classes."""
    mod, lst, ref, o1, o2 = _check_all_outputs("sic_alloy64")
    assert int(lst["rows"].max()) >= 8 and lst["tb"].numel() > 400
    assert float(ref["dth"][1]) != float(ref["dth"][2]), "dU/dA[0, 1] and dU/dA[1, 0] are different numbers"


def test_outputs_vs_float64_triclinic64():
    mod, lst, ref, o1, o2 = _check_all_outputs("tric64")
    assert case("tric64")[1].shape == (3, 3) and float(np.abs(case("tric64")[1][1, 0])) > 0.5


def test_outputs_vs_float64_gas37_isolated_atom_dimer_trimer_and_a_long_row():
    mod, lst, ref, o1, o2 = _check_all_outputs("gas37")
    rows = lst["rows"].tolist()
    assert rows[31] == 0 and rows[32] == rows[33] == 1 and rows[34:37] == [2, 1, 1] and rows[0] > 16 and 37 % 16 != 0
    assert int(mod._ell.cnt[31]) == 0 and int(mod._ell.cnt[32]) == 1 and int(mod._ell.cnt[0]) > 16
    for o in (o1["grad"][31], o1["pth"][31], o2["hw"][31], o2["pthw"][31]):
        assert float(o.abs().max()) == 0.0, "the atom with the empty row"
    dimer = (lst["bc"] == 32) | (lst["bc"] == 33)
    assert int(dimer.sum()) == 2 and float(ref["zeta"][dimer].abs().max()) == 0.0
    assert float(o1["pth"][32, 8].abs()) == 0.0 and float(o2["pthw"][32, 8].abs()) == 0.0, "nothing depends on h[0] in the dimer"
    assert float(o1["grad"][32].abs().max()) > 0.0
    assert float(o1["pth"][34, 8].abs()) > 0.0, "the trimer's centre"


def test_outputs_vs_float64_three_species_s3_64():
    mod, lst, ref, o1, o2 = _check_all_outputs("s3_64")
    assert mod.n_species == 3 and o1["dth"].numel() == 21 and abs(mod.cutoff - 3.1) < 1e-12


# ------------------------------------------------------------------------------------------------ 3: perfect zincblende
def test_perfect_zincblende_sic_through_the_kernel():
    """Perfect 2 x 2 x 2 zincblende SiC at a = 4.36 (float32 positions; the second shell at 3.083 A is beyond the Si-Si cutoff):
    U / N against the closed form with zeta = 3 g(-1/3) of either centre, and forces that vanish on the scale A_grad."""
    x32, cell32, ty, tab, _ = case("zb_perfect")
    mod = _module(x32, cell32, ty, tab)
    lst, ref = _reference("zb_perfect", mod)
    assert lst["rows"].tolist() == [4] * 64
    o = _eval(mod, T(x32, DEV), energy=True, grad=True)
    within(o["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), "perfect zincblende U")
    u_n, b0, b1 = M.zincblende_closed_form(_tab32(mod, tab), 4.36)
    assert abs(float(o["energy"]) / 64 - u_n) <= TOL * float(ref["A_U"]) / 64 + 1e-5
    assert abs(b0 - 0.958303) <= 1e-6 and abs(b1 - 0.883754) <= 1e-6
    within(o["grad"], torch.zeros(64, 3), ref["A_grad"], "perfect zincblende dU/dx against zero")
    assert float(ref["grad"].abs().max()) <= 1e-5 * float(ref["A_grad"].min()), "float64 forces vanish (float32 positions)"


# ------------------------------------------------------------------------------------------------ 4: single-species limits
@pytest.mark.parametrize("S", [2, 1])
def test_identical_silicon_sets_equal_the_one_species_reference(S):
    """S identical silicon sets with random types on tersoff_ref's si64 against the ONE-species float64 reference, every output
    within its bound; the parameter gradients summed over the entries of A, of B and of h.  Whether the outputs equal those of
    the one-species kernel (Tersoff.silicon) bit for bit is printed, not asserted: see the module docstring."""
    from mdgrad_amd import ops
    from mdgrad_amd.interface import Tersoff
    x32, cell32, p, _ = R1.gpu_cases()["si64"]
    ty = np.random.default_rng(5).integers(0, S, 64)
    tab = M.mixed([p] * S)
    mod = _module(x32, cell32, ty, tab)
    k = R1.consts(**p)
    lst = R1.bonds_and_triplets(x32, cell32, k["rc"])
    w32 = _w("si64", x32.shape)
    th = [float(p.detach().reshape(-1)[0]) for p in (mod.A, mod.B, mod.h)]
    key = ("one-species", tuple(th))
    if key not in _refs:
        _refs[key] = R1.evaluate(x32, th, lst, cell32, k, w=w32)
    ref = _refs[key]
    x, w = T(x32, DEV), T(w32, DEV)
    o1 = _eval(mod, x, energy=True, grad=True, want_theta=True)
    o2 = _eval(mod, x, w=w, energy=False, grad=True, want_theta=True)
    fold = lambda v: torch.stack([v[:S * S].sum(), v[S * S:2 * S * S].sum(), v[2 * S * S:].sum()])
    tag = "S = %d identical sets: " % S
    within(o1["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + "U")
    within(o1["grad"], ref["grad"], ref["A_grad"], tag + "dU/dx")
    within(o2["hw"], ref["hw"], ref["A_hw"], tag + "H.w")
    within(fold(ops.tersoff_multi_theta_sum(o1["pth"]).cpu().double()), ref["dth"], ref["A_dth"], tag + "dU/d(A, B, h)")
    within(fold(ops.tersoff_multi_theta_sum(o2["pthw"]).cpu().double()), ref["dthw"], ref["A_dthw"], tag + "d(w.dU/dx)/d(A, B, h)")
    one = Tersoff.silicon(mk_system(x32, cell32))
    a = ops.tersoff_eval(one._ell, x, one._consts, one._theta(), energy=True, grad=True, work=one._scratch())
    b = ops.tersoff_eval(one._ell, x, one._consts, one._theta(), w=w, energy=False, grad=True, work=one._scratch())
    print(tag + "bit-identical to the one-species kernel: U %s, dU/dx %s, H.w %s" % (
        torch.equal(a["energy"], o1["energy"]), torch.equal(a["grad"], o1["grad"]), torch.equal(b["hw"], o2["hw"])))


# ------------------------------------------------------------------------------------------------ 5: relabelling
def test_swapping_the_species_labels_permutes_the_tables_and_nothing_else():
    from mdgrad_amd import ops
    x32, cell32, ty, tab, _ = case("sic_alloy64")
    a_mod = _module(x32, cell32, ty, tab)
    b_mod = _module(x32, cell32, 1 - ty, M.relabelled(tab, [1, 0]))
    x, w = T(x32, DEV), T(_w("sic_alloy64", x32.shape), DEV)
    perm = torch.tensor([3, 2, 1, 0, 7, 6, 5, 4, 9, 8], device=DEV)
    for kw, keys in ((dict(energy=True), ("energy", "grad", "pth")), (dict(w=w, energy=False), ("grad", "hw", "pthw"))):
        a = _eval(a_mod, x, want_theta=True, **kw)
        b = _eval(b_mod, x, want_theta=True, **kw)
        for key in keys:
            if key.startswith("pth"):
                assert torch.equal(a[key][:, perm], b[key]), key
                sa, sb = ops.tersoff_multi_theta_sum(a[key]), ops.tersoff_multi_theta_sum(b[key])
                assert torch.equal(sa[perm], sb) and float(sa[1]) != float(sa[2]), "sum of " + key
            else:
                assert torch.equal(a[key], b[key]), key


# ------------------------------------------------------------------------------------------------ 6: replicas
def test_three_replicas_vs_each_alone_permutation_and_repeats():
    from mdgrad_amd import ops
    base, box, x32, ty = M.replicas16(M.SEEDS["replicas"])
    assert np.array_equal(x32, case("replicas")[0])
    tab = case("replicas")[3]
    system = mk_system(base, box).replicate(3)
    mod, lst, ref, o1, o2 = _check_all_outputs("replicas", system=system)
    assert mod.types.tolist() == np.tile(ty, 3).tolist()
    assert int((lst["bc"] // 16 != lst["be"] // 16).sum()) == 0 and int((lst["bc"][lst["tb"]] // 16 != lst["tk"] // 16).sum()) == 0
    x, w = T(x32, DEV), T(_w("replicas", x32.shape), DEV)
    F, dq, gth = mod.force_vjp(x, w)
    within(-_flat(gth), ref["dthw"], ref["A_dthw"], "force_vjp parameter part on three replicas")
    F2, dq2, gth2 = mod.force_vjp(x, w)
    assert torch.equal(F, F2) and torch.equal(dq, dq2) and all(torch.equal(a, b) for a, b in zip(gth, gth2))
    assert torch.equal(F, -o2["grad"]) and torch.equal(dq, -o2["hw"])
    P = M.n_theta(tab)
    alone, alone_w = torch.zeros(P, dtype=torch.float64), torch.zeros(P, dtype=torch.float64)
    for r in range(3):
        sl = slice(16 * r, 16 * r + 16)
        one = _module(x32[sl], box, ty, tab)
        xr = T(x32[sl], DEV)
        one._reset_topology(xr)
        a = _eval(one, xr, energy=False, grad=True, want_theta=True)
        b = _eval(one, xr, w=w[sl].contiguous(), energy=False, grad=True, want_theta=True)
        within(a["grad"], o1["grad"][sl].cpu(), ref["A_grad"][sl], "replica %d alone: dU/dx" % r)
        within(b["hw"], o2["hw"][sl].cpu(), ref["A_hw"][sl], "replica %d alone: H.w" % r)
        alone += ops.tersoff_multi_theta_sum(a["pth"]).cpu().double()
        alone_w += ops.tersoff_multi_theta_sum(b["pthw"]).cpu().double()
    within(o1["dth"], alone, ref["A_dth"], "dU/dtheta: three replicas vs each alone")
    within(o2["dthw"], alone_w, ref["A_dthw"], "d(w.dU/dx)/dtheta: three replicas vs each alone")
    perm = torch.cat([torch.arange(16) + 16 * r for r in (2, 0, 1)]).to(DEV)
    mod._reset_topology(x[perm].contiguous())
    op = _eval(mod, x[perm].contiguous(), w=w[perm].contiguous(), energy=False, want_theta=True)
    mod._reset_topology(x)
    oo = _eval(mod, x, w=w, energy=False, want_theta=True)
    for key in ("grad", "hw", "pthw"):
        assert torch.equal(op[key], oo[key][perm]), key


# ------------------------------------------------------------------------------------------------ 7: autograd
def test_autograd_backward_and_double_backward_equal_force_vjp():
    x32, cell32, ty, tab, _ = case("sic_alloy64")
    mod = _module(x32, cell32, ty, tab)
    lst, ref = _reference("sic_alloy64", mod)
    x = T(x32, DEV).requires_grad_(True)
    mod(x).backward()
    within(x.grad, ref["grad"], ref["A_grad"], "backward of model(xyz) in xyz")
    assert [tuple(p.grad.shape) for p in (mod.A, mod.B, mod.h)] == [(2, 2), (2, 2), (2,)]
    within(_flat([p.grad for p in (mod.A, mod.B, mod.h)]), ref["dth"], ref["A_dth"], "backward of model(xyz) in (A, B, h)")
    w = T(_w("sic_alloy64", x32.shape), DEV)
    x2 = T(x32, DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(mod(x2), x2, create_graph=True)
    hw, hA, hB, hh = torch.autograd.grad((g * w).sum(), (x2, mod.A, mod.B, mod.h))
    within(hw, ref["hw"], ref["A_hw"], "double backward of model(xyz) in xyz")
    within(_flat([hA, hB, hh]), ref["dthw"], ref["A_dthw"], "double backward of model(xyz) in (A, B, h)")
    F, dq, gth = mod.force_vjp(x2.detach(), w)
    assert torch.equal(F, -g.detach()) and torch.equal(dq, -hw)
    assert [t.shape for t in gth] == [p.shape for p in mod.parameters()]
    assert torch.equal(gth[0], -hA) and torch.equal(gth[1], -hB) and torch.equal(gth[2], -hh)
    assert torch.equal(mod.force(x2.detach()), F)
    frozen = _module(x32, cell32, ty, tab, trainable=False)
    assert list(frozen.parameters()) == []
    assert frozen.force_vjp(x2.detach(), w)[2] == [] and frozen.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    assert torch.equal(frozen.force_vjp(x2.detach(), w)[1], dq)
    assert mod.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    # the device table follows the parameters: B[0, 1] moved, the energy moves with dU/dB[0, 1]
    u0 = float(mod(T(x32, DEV)).detach())
    with torch.no_grad():
        mod.B[0, 1] += 1.0
    u1 = float(mod(T(x32, DEV)).detach())
    assert abs((u1 - u0) - float(ref["dth"][5])) <= 2 * TOL * float(ref["A_U"]), (u1 - u0, float(ref["dth"][5]))


# ------------------------------------------------------------------------------------------------ 8: into / scale / accum
def test_stack_sums_equal_the_members_separate_results():
    from mdgrad_amd import ops
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    x32, cell32, ty, tab, _ = case("sic_alloy64")
    system = mk_system(x32, cell32)
    ts = _module(x32, cell32, ty, tab, system=system)
    lj = PairPotentials(system, P.LJFamily(2.0, 0.1), cutoff=ts.cutoff)
    stack = Stack({"lj": lj, "tersoff": ts})
    assert stack.supports_force_vjp() and stack.supports_static_topology()
    x, w = T(x32, DEV), T(_w("sic_alloy64", x32.shape), DEV)
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
        assert v.shape == p.shape
        same(v, by_id[id(p)], "parameter part")
    acc = ops.ThetaAccum(params)
    acc.flat.fill_(0.25)
    assert stack.force_vjp(x, w, accum=acc)[2] is None
    for v, want in zip(acc.views(), gth):
        assert float((v - 0.25 - want).abs().max()) <= 2.0 ** -22 * max(float(want.abs().max()), 0.25), "accum vs list"
    # parameters that are not adjacent in the flat buffer: each block goes to its own offset
    acc2 = ops.ThetaAccum([ts.h] + list(lj.parameters()) + [ts.A, ts.B])
    assert ts.force_vjp(x, w, accum=acc2)[2] is None
    for p, want in zip((ts.A, ts.B, ts.h), g2):
        got = acc2.flat[acc2.off[id(p)]:acc2.off[id(p)] + p.numel()].view(p.shape)
        same(got, want, "accum at scattered offsets")
    F0, D0 = torch.randn_like(x), torch.randn_like(x)
    F1, D1, _ = ts.force_vjp(x, w, into=(F0.clone(), D0.clone()))
    same(F1 - F0, f2, "force added onto a buffer")
    same(D1 - D0, d2, "d(w.F)/dx added onto a buffer")


# ------------------------------------------------------------------------------------------------ 9: skin list
def test_evaluation_on_a_list_searched_with_a_skin_equals_a_fresh_exact_list():
    """The stored list was searched at max (R + D) + 0.4 A; the Si-C and C-C entries have cutoffs 0.49 and 0.9 A below the
    list's own, so this is the test of the per-entry support as well."""
    from mdgrad_amd import _lib, ops
    x32, cell32, ty, tab, _ = case("sic_alloy64")
    x1_32 = case("skin")[0]
    assert np.array_equal(x1_32, R1.skin_step(x32, M.SEEDS["skin"])) and float(np.abs(x1_32 - x32).max()) < 0.2
    mod = _module(x32, cell32, ty, tab)
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
        a = _eval(mod, x1, ell=vl.ell, want_theta=True, **kw)
        b = _eval(mod, x1, ell=exact, want_theta=True, **kw)
        for key in keys:
            if key in A:
                within(a[key], b[key].cpu(), A[key], "skin list vs exact list: " + key)
            else:
                within(ops.tersoff_multi_theta_sum(a[key]), ops.tersoff_multi_theta_sum(b[key]).cpu(),
                       ref["A_dth" if key == "pth" else "A_dthw"], "skin list vs exact list: sum of " + key)
    within(a["hw"], ref["hw"], ref["A_hw"], "skin list vs float64: H.w")
    within(a["grad"], ref["grad"], ref["A_grad"], "skin list vs float64: dU/dx")
    within(ops.tersoff_multi_theta_sum(a["pthw"]), ref["dthw"], ref["A_dthw"], "skin list vs float64: d(w.dU/dx)/dtheta")


# ------------------------------------------------------------------------------------------------ 10: trajectory + adjoint
_oracle_cache = {}
TRAJ = dict(T=0.05, Q=20.0, chains=3, dt=0.01, mass=(2.8, 1.2), nbins=32, r_range=(1.2, 4.3))


def traj_inputs():
    x32, cell32, ty, tab, _ = case("traj")
    mass = np.where(ty == 0, TRAJ["mass"][0], TRAJ["mass"][1]).astype(F32)
    vel = (np.random.default_rng(711).normal(0, 1, x32.shape) * np.sqrt(TRAJ["T"] / mass)[:, None]).astype(F32)
    return x32, cell32, ty, tab, vel, mass


def oracle_traj(t):
    if "run" not in _oracle_cache:
        x32, cell32, ty, tab, vel, mass = traj_inputs()
        cell = T(cell32)
        terms = [M.TersoffMultiTerm(tab, ty, cell32)]

        def loss_fn(Ls):
            _, _, gr = O.rdf_oracle(Ls[1][::2], cell, TRAJ["nbins"], TRAJ["r_range"])
            return gr.pow(2).mean() + Ls[0][-1].pow(2).mean() + 0.0 * Ls[2][-1].sum()
        _oracle_cache["run"] = oracle_run(x32, cell32, vel, mass, terms, TRAJ["T"], TRAJ["Q"], TRAJ["chains"], t, loss_fn)
    return _oracle_cache["run"]


@pytest.mark.parametrize("graphs_on", [True, False], ids=["graph_replay", "eager"])
def test_sic_term_in_a_stack_trajectory_and_adjoint_vs_oracle(graphs_on):
    """Stack(TersoffMulti.silicon_carbide, trainable) on 64 zincblende SiC atoms (a = 4.36, jittered by 0.1 A, masses 2.8 and
    1.2): 10 NHC steps through odeint_adjoint, the loss on rdf of q_t[::2] plus v_t[-1]^2 -- trajectories, adjoint of y0 and
    dL/d(A, B, h) against the oracle with tersoff_multi_ref.TersoffMultiTerm.  The stack stays on the analytic adjoint
    (force_vjp) and HIP-graph replay although the parameters require grad.  Tolerances: those of
    test_tersoff_term_in_a_stack_trajectory_and_adjoint_vs_oracle.
    Observed on an MI355X (graph replay and eager alike), observed / allowed at the entry closest to its bound: q_t 4.8e-07 /
    2.0e-05, v_t 5.1e-07 / 8.6e-05, pv_t 0.0e+00 / 1.0e-05, adj v0 4.0e-09 / 2.3e-05, adj q0 9.3e-08 / 2.2e-04, adj pv0
    8.0e-15 / 1.5e-06, dL/d(A, B, h) 0.0e+00 / 4.0e-05 (an entry that is exactly zero on both sides: no C-C pair is inside
    its cutoff)."""
    from mdgrad_amd import graphs
    from mdgrad_amd.interface import Stack, TersoffMulti
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.sovlers import odeint_adjoint
    x32, cell32, ty, tab, vel, mass = traj_inputs()
    system = mk_system(x32, cell32, vel, mass)
    ts = TersoffMulti.silicon_carbide(system, ty)
    stack = Stack({"tersoff": ts})
    integ = NoseHooverChain(stack, system, T=TRAJ["T"], num_chains=TRAJ["chains"], Q=TRAJ["Q"], adjoint=True).to(DEV)
    assert integ.fused_spec("NH_verlet") is None, "a TersoffMulti member keeps the stack off the fused trajectory kernels"
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
    assert gth.numel() == 10 and all(p.grad is not None for p in (ts.A, ts.B, ts.h))
    report(_flat([p.grad for p in (ts.A, ts.B, ts.h)]), gth, 5e-3, 5e-4 * float(gth.abs().max()), "dL/d(A, B, h)")


# ------------------------------------------------------------------------------------------------ 11: torch ops
def test_torch_ops_equal_ctypes_path_and_reject_bad_input():
    from mdgrad_amd import _torch_ops
    ns = _torch_ops.get()
    assert ns is not None
    x32, box, ty, tab, _ = case("gas37")
    mod = _module(x32, box, ty, tab)
    ell = mod._ell
    cell = _torch_ops.cell_args(ell.cell_struct)
    x, w, tb, tys = T(x32, DEV), T(_w("gas37", x32.shape), DEV), mod._tables(), mod.types
    a = _eval(mod, x, energy=True, grad=True, want_theta=True)
    U, g, hw, pth, pthw = ns.tersoff_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, tys, 2, tb, None, True, True)
    assert torch.equal(U, a["energy"]) and torch.equal(g, a["grad"]) and torch.equal(pth, a["pth"]) and hw.numel() == pthw.numel() == 0
    b = _eval(mod, x, w=w, energy=False, grad=True, want_theta=True)
    U, g, hw, pth, pthw = ns.tersoff_multi_eval(x, cell, ell.col, ell.shift, ell.cnt, tys, 2, tb, w, False, True)
    assert torch.equal(g, b["grad"]) and torch.equal(hw, b["hw"]) and torch.equal(pthw, b["pthw"]) and U.numel() == pth.numel() == 0
    args = (x, cell, ell.col, ell.shift, ell.cnt)
    bad = [lambda: ns.tersoff_multi_eval(x.double(), cell, ell.col, ell.shift, ell.cnt, tys, 2, tb, None, True, False),
           lambda: ns.tersoff_multi_eval(x.cpu(), cell, ell.col, ell.shift, ell.cnt, tys, 2, tb, None, True, False),
           lambda: ns.tersoff_multi_eval(x, cell, ell.col.long(), ell.shift, ell.cnt, tys, 2, tb, None, True, False),
           lambda: ns.tersoff_multi_eval(*args, tys.long(), 2, tb, None, True, False),
           lambda: ns.tersoff_multi_eval(*args, tys[:5].contiguous(), 2, tb, None, True, False),
           lambda: ns.tersoff_multi_eval(*args, tys.cpu(), 2, tb, None, True, False),
           lambda: ns.tersoff_multi_eval(*args, tys + 1, 2, tb, None, True, False),                 # a species = n_species
           lambda: ns.tersoff_multi_eval(*args, tys - 1, 2, tb, None, True, False),                 # a negative species
           lambda: ns.tersoff_multi_eval(*args, tys, 0, tb, None, True, False),
           lambda: ns.tersoff_multi_eval(*args, tys, 5, tb, None, True, False),
           lambda: ns.tersoff_multi_eval(*args, tys, 3, tb, None, True, False),                     # the table of another S
           lambda: ns.tersoff_multi_eval(*args, tys, 2, tb[:40].contiguous(), None, True, False),
           lambda: ns.tersoff_multi_eval(*args, tys, 2, tb.double(), None, True, False),
           lambda: ns.tersoff_multi_eval(*args, tys, 2, tb.cpu(), None, True, False),
           lambda: ns.tersoff_multi_eval(*args, tys, 2, tb, w[:5].contiguous(), True, False),
           lambda: ns.tersoff_multi_eval(*args, tys, 2, tb, w.double(), True, False)]
    for n, fn in enumerate(bad):
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
            pytest.fail("bad input %d was accepted" % n)
