"""K27: the tabulated embedded-atom term (EAM, mdg_eam_table_eval, csrc/eam_table.hip) against the float64 definition of
tests/eam_table_ref.py (pinned to an independent loop and to the properties of the interpolant by tests/test_eam_table_host.py),
against SuttonChen on the same list and, in a trajectory, against the CPU oracle's adjoint.

Tolerance of every kernel-vs-float64 comparison: K * 2^-24 * A per component with K = 64 (KTOL and `within` of
tests/test_gpu_eam.py), A = the float64 sum of the absolute values of what the kernel adds up (eam_table_ref.evaluate: the four
products of every lookup, the float32 uncertainty of its argument carried through its slope, products of scales for products).
`within` prints the largest observed err / (2^-24 A).

The second derivative of the interpolant jumps at the nodes, so H w and d(w.dU/dx)/dnodes are compared on 64-node tables and
only after `_margins` has asserted that no pair distance lies within 64 * 2^-24 r of an r node and no density within
512 * 2^-24 rho of a rho node (the reference and the kernel could otherwise pick different cells).

Observed on an MI355X, the largest err / (2^-24 A) over all cases of this file: U 0.24, dU/dx 0.06, dU/dnodes 3.43,
d(w.dU/dx)/dnodes 1.77 (all four on the triclinic 64-atom set), H.w below 0.005, the sum of the forces below 0.005; Cu-108 alone:
0.00 / 0.01 / 0.68 (64 nodes), 1.27 (1024), 2.36 (2048) / 0.64; three replicas 0.01 / 0.01 / 1.28 / 0.84; the node part of
force_vjp at w * 2^-30, 1, 2^30: 1.24 each.  Why the position derivatives sit so far below 64: a derivative of the interpolant
is a difference of node values over h (6 t (1 - t) (v_1 - v_0) / h and its kin, formed as two products), so the sum of absolute
values that A counts exceeds the result by about |v| / (h |f'|), 10 to 10^3 here, while the two products round almost alike;
the node gradients are sums of basis weights of one sign and have no such slack.  K is the project's and is not lowered for it:
a swapped species index moves dU/dx by 395 times the tolerance (case 3), and the Hessian parts are also pinned bit for bit to
autograd (case 7) and to the oracle's adjoint (case 10)."""
import numpy as np
import pytest
import torch

import eam_ref as SC
import eam_table_ref as R
import oracle as O
from conftest import load_golden
from test_gpu_eam import TOL, MARGIN, within, _gas37, _replicas24, TRAJ, traj_inputs
from test_gpu_parity import T, close, mk_system, DEV, oracle_run

pytestmark = pytest.mark.gpu
F32 = np.float32
CU = SC.PUBLISHED["copper"]
RC, RMIN = 5.2, 1.8
PAIR_MARGIN, RHO_MARGIN = 64.0, 512.0


def _functions(L):
    """Three phi, two f and two F, all different, at the length scale L; f_1 / f_0 >= 2.8 everywhere below 2 L."""
    pair = [lambda r: 0.9 * torch.exp(-1.3 * (r / L - 1.0)) - 0.2, lambda r: 1.4 * torch.exp(-1.1 * (r / L - 0.96)) - 0.3 * L / r,
            lambda r: 0.6 * torch.exp(-1.7 * (r / L - 1.04)) + 0.05 * r / L]
    density = [lambda r: 1.1 * torch.exp(-0.9 * (r / L - 1.0)), lambda r: 3.1 * torch.exp(-1.2 * (r / L - 1.0))]
    embed = [lambda p: -1.2 * torch.sqrt(p + 0.5) + 0.01 * p * p, lambda p: -0.8 * torch.log(p + 1.0) + 0.03 * p]
    return pair, density, embed


def _copper(x32, cell32, n=64, system=None, rc=RC, **kw):
    from mdgrad_amd.interface import EAM
    return EAM.from_sutton_chen(mk_system(x32, cell32) if system is None else system, "copper", cutoff=rc, r_min=RMIN, n_r=n, n_rho=n, **kw)


def _types(mod):
    return mod.types.cpu().long()


def _reference(mod, x32, cell32, w32=None, group=None):
    lst = R.pairs(x32, cell32, mod.cutoff, group=group)
    assert lst["margin"] >= MARGIN, "a pair sits on the cutoff: choose another seed"
    return lst, R.evaluate(x32, R.tables_of(mod), lst, cell32, _types(mod), R.grid_of(mod), w=w32, pin=mod.pin_cutoff)


def _margins(mod, x32, cell32, lst):
    m = R.node_margin(x32, R.tables_of(mod), lst, cell32, _types(mod), R.grid_of(mod))
    assert m["pairs"] >= PAIR_MARGIN, "a pair distance sits on a node of the r grid (%.1f): choose another seed" % m["pairs"]
    assert m["densities"] >= RHO_MARGIN, "a density sits on a node of the rho grid (%.1f): choose another seed" % m["densities"]
    return m


def _eval(mod, x, **kw):
    from mdgrad_amd import ops
    return ops.eam_table_eval(mod._ell, x, mod.types, mod._consts, mod._tables(), work=mod._work, fx=mod._fx, **kw)


def _check_outputs(mod, x32, cell32, tag, group=None, seed=0, second=True):
    """U, dU/dx, dU/dnodes (and, when `second`, H w and d(w.dU/dx)/dnodes behind the node-margin assertion) of one call each
    against float64; the energy-only call; the sum of the forces; LEVEL 1 and LEVEL 2 forces bit for bit."""
    w32 = np.random.default_rng(seed + 17).normal(0, 1, x32.shape).astype(F32)
    lst, ref = _reference(mod, x32, cell32, w32 if second else None, group)
    x, w = T(x32, DEV), T(w32, DEV)
    mod._reset_topology(x)
    o1 = _eval(mod, x, energy=True, grad=True, want_theta=True)
    o2 = _eval(mod, x, w=w, energy=False, grad=True, want_theta=True)
    tag += " "
    rs = dict(U=within(o1["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + "U"),
              grad=within(o1["grad"], ref["grad"], ref["A_grad"], tag + "dU/dx"),
              gtab=within(o1["gtab"], ref["gtab"], ref["A_gtab"], tag + "dU/dnodes"))
    if second:
        _margins(mod, x32, cell32, lst)
        rs["hw"] = within(o2["hw"], ref["hw"], ref["A_hw"], tag + "H.w")
        rs["gtabw"] = within(o2["gtabw"], ref["gtabw"], ref["A_gtabw"], tag + "d(w.dU/dx)/dnodes")
    assert torch.equal(o1["grad"], o2["grad"]) and o2["gtab"] is None and o1["gtabw"] is None
    assert bool(torch.isfinite(o2["hw"]).all()) and bool(torch.isfinite(o2["gtabw"]).all())
    e0 = _eval(mod, x, energy=True, grad=False)                                                      # LEVEL 0
    within(e0["energy"], ref["U"].reshape(1), ref["A_U"].reshape(1), tag + "U (energy-only call)")
    within(o1["grad"].sum(0), torch.zeros(3), ref["A_grad"].sum(0), tag + "sum_i dU/dx_i")
    if mod.pin_cutoff:
        m = R.pinned_mask(R.grid_of(mod)).to(DEV)
        assert float(o1["gtab"][m].abs().max()) == 0.0 and float(o2["gtabw"][m].abs().max()) == 0.0, "pinned entries are exact zeros"
    return lst, ref, o1, o2, rs


# ------------------------------------------------------------------------------------------------ 1: one species
def test_outputs_vs_float64_jittered_cu108_from_sutton_chen_tables():
    """3 x 3 x 3 fcc cells of copper jittered by 0.15 A, tables of Sutton-Chen copper: 64 nodes for every output; 1024 and 2048 nodes
    (either side of the size up to which the node gradient is summed per workgroup in LDS) for the continuous ones."""
    x32, cell32 = SC.jittered_fcc(3, 3.61, 0.15, 108)
    mod = _copper(x32, cell32, 64)
    lst, ref, o1, o2, _ = _check_outputs(mod, x32, cell32, "cu108/64")
    rows = lst["rows"]
    assert int(rows.min()) >= 40 and int(rows.max()) >= 54
    _check_outputs(_copper(x32, cell32, 1024), x32, cell32, "cu108/1024", second=False)    # 6144 words: the largest LDS copy
    _check_outputs(_copper(x32, cell32, 2048), x32, cell32, "cu108/2048", second=False)    # 12288 words: global atomics only


# ------------------------------------------------------------------------------------------------ 2: against SuttonChen
def test_table_term_equals_sutton_chen_within_the_measured_tabulation_error():
    from mdgrad_amd.interface import SuttonChen
    x32, cell32 = SC.jittered_fcc(3, 3.61, 0.15, 108)
    system = mk_system(x32, cell32)
    sc = SuttonChen.copper(system, cutoff=RC)
    for n in (64, 1024):
        mod = _copper(x32, cell32, n, system=system)
        lst, ref = _reference(mod, x32, cell32)
        k = SC.consts(9, 6, RC, "force")
        ref_sc = SC.evaluate(x32, [float(p.detach()) for p in (sc.epsilon, sc.a, sc.c)], lst, cell32, k)
        x = T(x32, DEV)
        mod._reset_topology(x)
        sc._reset_topology(x)
        ot = _eval(mod, x, energy=True, grad=True)
        from mdgrad_amd import ops
        os_ = ops.eam_eval(sc._ell, x, sc._consts, sc._theta(), work=sc._work, energy=True, grad=True)
        tab_U = abs(float(ref["U"]) - float(ref_sc["U"]))                     # tabulated float64 vs analytic float64
        tab_g = (ref["grad"] - ref_sc["grad"]).abs()
        dU = abs(float(ot["energy"]) - float(os_["energy"]))
        dg = (ot["grad"] - os_["grad"]).abs().cpu().double()
        floor_U, floor_g = TOL * float(ref["A_U"] + ref_sc["A_U"]), TOL * (ref["A_grad"] + ref_sc["A_grad"])
        print("table(%d) vs SuttonChen: |dU| %.3e (tabulation %.3e, float32 floor %.3e); max |dg| %.3e (tabulation %.3e)"
              % (n, dU, tab_U, floor_U, float(dg.max()), float(tab_g.max())))
        assert dU <= tab_U + floor_U
        assert bool((dg <= tab_g + floor_g).all())


# ------------------------------------------------------------------------------------------------ 3: two species, triclinic
def _tric64():
    from mdgrad_amd.interface import EAM
    g = load_golden("nbr_tric64")
    x32, cell32, rc = g["xyz"].astype(F32), g["cell"].astype(F32), float(g["cutoff"])
    types = np.arange(64) % 2
    mod = EAM.from_functions(mk_system(x32, cell32), types, *_functions(1.0), rc, 0.25, (0.5, 25.0), 64, 64)
    return mod, x32, cell32


def test_outputs_vs_float64_two_species_triclinic64_with_both_continuations():
    mod, x32, cell32 = _tric64()
    lst, ref, o1, o2, _ = _check_outputs(mod, x32, cell32, "tric64")
    m = R.node_margin(x32, R.tables_of(mod), lst, cell32, _types(mod), R.grid_of(mod))
    assert m["below"] >= 1 and m["above"] >= 2, "the closest pair lies below r_min and several densities above rho_max"
    assert int(lst["rows"].max()) > 16, "rows longer than the lanes of an atom"
    # a swapped species index is far outside the tolerance (observed: 395 times it at the worst component)
    tabs = R.tables_of(mod)
    wrong = R.evaluate(x32, (tabs[0], tabs[1].flip(0), tabs[2]), lst, cell32, _types(mod), R.grid_of(mod))
    assert float(((wrong["grad"] - ref["grad"]).abs() / ref["A_grad"]).max()) > 100 * TOL


# ------------------------------------------------------------------------------------------------ 4: empty row
def test_gas37_with_an_empty_row_and_an_isolated_pair():
    x32, box = _gas37()
    lst0 = R.pairs(x32, box, RC)
    k = SC.consts(9, 6, RC, "force")
    _, rho = SC.density(torch.tensor(x32).double(), CU[1], lst0, box, k)
    low = float(rho[rho > 0].min())
    mod = _copper(x32, box, 64, rho_range=(0.25 * low, 1.5 * float(rho.max())))
    assert low > mod.rho_range[0] + mod.h_rho, "every atom with a neighbour lies above the first cell of the rho grid"
    lst, ref, o1, o2, _ = _check_outputs(mod, x32, box, "gas37", second=False)
    rows = lst["rows"].tolist()
    assert rows[33] == 0 and rows[34] == rows[35] == 1 and max(rows) >= 8 and 37 % 16 != 0
    assert int(mod._ell.cnt[33]) == 0
    for o in (o1["grad"][33], o2["hw"][33]):
        assert bool(torch.isfinite(o).all()) and float(o.abs().max()) == 0.0, "the atom with the empty row"
    assert float(mod._work[33, 0]) == 0.0 and float(mod._work[33, 1]) == 0.0, "rho = 0"
    assert float(o1["grad"][34].abs().max()) > 0.0
    for o in (o1["energy"], o1["grad"], o1["gtab"], o2["hw"], o2["gtabw"]):
        assert bool(torch.isfinite(o).all())
    # node 0 of F: only the atom at rho = 0 reaches it -- exactly basis(0) = (1, t), t = (0 - rho_min) / h below the grid
    e0 = 2 * 2 * 64
    t0 = np.float32(1.0 / mod.h_rho) * (np.float32(0.0) - np.float32(mod.rho_range[0]))
    got = o1["gtab"][e0:e0 + 2].cpu().numpy()
    assert got[0] == np.float32(1.0) and got[1] == t0, (got, t0)
    assert float(o2["gtabw"][e0:e0 + 2].abs().max()) == 0.0, "d rho = 0: no directional derivative"


# ------------------------------------------------------------------------------------------------ 5: replicas
def _alloy_replicas():
    from mdgrad_amd.interface import EAM
    base, box, x32 = _replicas24()
    system = mk_system(base, box).replicate(3)
    mod = EAM.from_functions(system, np.arange(24) % 2, *_functions(2.5), RC, RMIN, (0.0, 12.0), 64, 64)
    return mod, x32, box


def test_node_gradients_on_three_replicas_bitwise_repeatable_and_permutable():
    mod, x32, box = _alloy_replicas()
    lst, ref, o1, o2, _ = _check_outputs(mod, x32, box, "3 x gas24", group=24, seed=5)
    assert int((lst["i"] // 24 != lst["j"] // 24).sum()) == 0
    x = T(x32, DEV)
    w = T(np.random.default_rng(22).normal(0, 1, x32.shape).astype(F32), DEV)
    a = mod.force_vjp(x, w)
    b = mod.force_vjp(x, w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))
    g1 = _eval(mod, x, energy=False, grad=True, want_theta=True)["gtab"]
    assert torch.equal(g1, _eval(mod, x, energy=False, grad=True, want_theta=True)["gtab"])
    # replicas (2, 0, 1): per-atom outputs move with their replica, the node gradients do not change, bit for bit
    perm = torch.cat([torch.arange(24) + 24 * r for r in (2, 0, 1)]).to(DEV)
    xp, wp = x[perm].contiguous(), w[perm].contiguous()
    mod._reset_topology(xp)
    p1 = _eval(mod, xp, energy=False, grad=True, want_theta=True)
    p2 = _eval(mod, xp, w=wp, energy=False, want_theta=True)
    mod._reset_topology(x)
    q1 = _eval(mod, x, energy=False, grad=True, want_theta=True)
    q2 = _eval(mod, x, w=w, energy=False, want_theta=True)
    assert torch.equal(p1["grad"], q1["grad"][perm]) and torch.equal(p2["hw"], q2["hw"][perm])
    assert torch.equal(p1["gtab"], q1["gtab"]) and torch.equal(p2["gtabw"], q2["gtabw"])


# ------------------------------------------------------------------------------------------------ 6: range of the scatter
def test_node_part_of_force_vjp_is_covariant_over_sixty_binades_of_w():
    mod, x32, box = _alloy_replicas()
    x = T(x32, DEV)
    w32 = np.random.default_rng(23).normal(0, 1, x32.shape).astype(F32)
    lst, ref = _reference(mod, x32, box, w32, group=24)
    _margins(mod, x32, box, lst)
    mod._reset_topology(x)
    base = None
    for s in (0, -30, 30):
        F, dq, gth = mod.force_vjp(x, T(w32, DEV) * 2.0 ** s)
        got = -torch.cat([t.reshape(-1) for t in gth])
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(dq).all())
        within(got * 2.0 ** -s, ref["gtabw"], ref["A_gtabw"], "force_vjp node part at w * 2^%d" % s)
        if base is None:
            base = F
        assert torch.equal(F, base), "the force does not depend on w"


# ------------------------------------------------------------------------------------------------ 7: autograd
def test_autograd_backward_and_double_backward_equal_force_vjp():
    x32, cell32 = SC.jittered_fcc(3, 3.61, 0.15, 108)
    mod = _copper(x32, cell32, 64)
    lst, ref = _reference(mod, x32, cell32)
    g = R.grid_of(mod)
    x = T(x32, DEV).requires_grad_(True)
    mod(x).backward()
    within(x.grad, ref["grad"], ref["A_grad"], "backward of model(xyz) in xyz")
    got = torch.cat([p.grad.reshape(-1) for p in mod.parameters()])
    within(got, ref["gtab"], ref["A_gtab"], "backward of model(xyz) in the nodes")
    w = torch.randn(108, 3, device=DEV)
    x2 = T(x32, DEV).requires_grad_(True)
    params = list(mod.parameters())
    (gx,) = torch.autograd.grad(mod(x2), x2, create_graph=True)
    hs = torch.autograd.grad((gx * w).sum(), [x2] + params)
    F, dq, gth = mod.force_vjp(x2.detach(), w)
    assert torch.equal(F, -gx.detach()) and torch.equal(dq, -hs[0])
    assert [t.shape for t in gth] == [p.shape for p in params] and len(gth) == 3
    assert all(torch.equal(a, -b) for a, b in zip(gth, hs[1:]))
    assert torch.equal(mod.force(x2.detach()), F)
    assert float(gth[0][:, -1].abs().max()) == 0.0 and float(gth[1][:, -1].abs().max()) == 0.0, "pinned entries are exact zeros"
    assert float(gth[0].abs().max()) > 0.0 and float(gth[2].abs().max()) > 0.0
    one = _copper(x32, cell32, 64, trainable=("embed",))
    assert [n for n, _ in one.named_parameters()] == ["embed_nodes"]
    t1 = one.force_vjp(x2.detach(), w)
    assert len(t1[2]) == 1 and torch.equal(t1[2][0], gth[2]) and torch.equal(t1[0], F) and torch.equal(t1[1], dq)
    (ge,) = torch.autograd.grad(one(x2), one.embed_nodes)
    assert torch.equal(ge.reshape(-1), got[2 * 2 * g["n_r"]:])
    frozen = _copper(x32, cell32, 64, trainable=False)
    assert list(frozen.parameters()) == []
    assert frozen.force_vjp(x2.detach(), w)[2] == [] and frozen.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    assert torch.equal(frozen.force_vjp(x2.detach(), w)[1], dq)
    assert mod.force_vjp(x2.detach(), w, want_theta=False)[2] is None
    (gf,) = torch.autograd.grad(frozen(x2), x2)
    assert torch.equal(gf, gx.detach())


# ------------------------------------------------------------------------------------------------ 8: into / scale / accum
def test_stack_sums_equal_the_members_separate_results():
    """Stack({"lj", "eam"}).force and .force_vjp (the force pass adds onto the pair term's buffers) against the sum of the
    members' separate results, to 2^-22 of the largest entry; the same for `accum` against the list return."""
    from mdgrad_amd import ops
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    x32, cell32 = SC.jittered_fcc(3, 3.61, 0.15, 66)
    system = mk_system(x32, cell32)
    eam = _copper(x32, cell32, 64, system=system)
    lj = PairPotentials(system, P.LJFamily(2.3, 0.1), cutoff=RC)
    stack = Stack({"lj": lj, "eam": eam})
    assert stack.supports_force_vjp() and stack.supports_static_topology()
    x, w = T(x32, DEV), torch.randn(108, 3, device=DEV)
    stack._reset_topology(x)
    assert lj._ell is eam._ell, "one search for both members"

    def same(a, b, what):
        assert float((a - b).abs().max()) <= 2.0 ** -22 * float(b.abs().max()), what
    same(stack.force(x), lj.force(x) + eam.force(x), "force")
    F, dq, gth = stack.force_vjp(x, w)
    f1, d1, g1 = lj.force_vjp(x, w)
    f2, d2, g2 = eam.force_vjp(x, w)
    same(F, f1 + f2, "force (vjp)")
    same(dq, d1 + d2, "d(w.F)/dx")
    params = list(stack.parameters())
    assert len(gth) == len(params) == 5
    by_id = {id(p): v for p, v in zip(list(lj.parameters()) + list(eam.parameters()), g1 + g2)}
    for p, v in zip(params, gth):
        same(v, by_id[id(p)], "parameter part")
    acc = ops.ThetaAccum(params)
    acc.flat.fill_(0.25)
    assert stack.force_vjp(x, w, accum=acc)[2] is None
    for v, want in zip(acc.views(), gth):
        assert float((v - 0.25 - want).abs().max()) <= 2.0 ** -22 * max(float(want.abs().max()), 0.25), "accum vs list"
    # a flat buffer in which the node tensors are neither adjacent nor in order
    acc2 = ops.ThetaAccum([eam.embed_nodes, lj.model.sigma, eam.pair_nodes, eam.density_nodes])
    assert eam.force_vjp(x, w, accum=acc2)[2] is None
    for v, want in zip(acc2.views(), [g2[2], torch.zeros(1, device=DEV), g2[0], g2[1]]):
        assert float((v - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max()), "accum, scattered offsets"
    F0, D0 = torch.randn_like(x), torch.randn_like(x)
    F1, D1, _ = eam.force_vjp(x, w, into=(F0.clone(), D0.clone()))
    same(F1 - F0, f2, "force added onto a buffer")
    same(D1 - D0, d2, "d(w.F)/dx added onto a buffer")


# ------------------------------------------------------------------------------------------------ 9: skin list
def test_evaluation_on_a_list_searched_with_a_skin_equals_a_fresh_exact_list():
    """rc = 5.0 here: rc + skin = 5.4 has to stay below half the 10.83 A cell."""
    from mdgrad_amd import _lib, ops
    x32, cell32 = SC.jittered_fcc(3, 3.61, 0.15, 67)
    rc, skin = 5.0, 0.4
    mod = _copper(x32, cell32, 64, rc=rc)
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
    A = {"energy": ref["A_U"].reshape(1), "grad": ref["A_grad"], "hw": ref["A_hw"], "gtab": ref["A_gtab"], "gtabw": ref["A_gtabw"]}
    run = lambda ell, **kw: ops.eam_table_eval(ell, x1, mod.types, mod._consts, mod._tables(), want_theta=True, **kw)
    for kw, keys in ((dict(energy=True), ("energy", "grad", "gtab")), (dict(w=w, energy=False), ("grad", "hw", "gtabw"))):
        a, b = run(vl.ell, **kw), run(exact, **kw)
        for key in keys:
            within(a[key], b[key].cpu(), A[key], "skin list vs exact list: " + key)
    within(a["grad"], ref["grad"], ref["A_grad"], "skin list vs float64: dU/dx")
    within(run(vl.ell, energy=True)["gtab"], ref["gtab"], ref["A_gtab"], "skin list vs float64: dU/dnodes")


# ------------------------------------------------------------------------------------------------ 10: trajectory + adjoint
_oracle_cache = {}


def _traj_module(system=None):
    x32, cell32, vel, mass = traj_inputs()
    system = mk_system(x32, cell32, vel, mass) if system is None else system
    return _copper(x32, cell32, 128, system=system, trainable=("density", "embed")), system


def oracle_traj(t, mod):
    if "run" not in _oracle_cache:
        x32, cell32, vel, mass = traj_inputs()
        cell = T(cell32)
        terms = [R.TableTerm(R.tables_of(mod), np.zeros(108, dtype=np.int64), R.grid_of(mod), cell32)]

        def loss_fn(Ls):
            _, _, gr = O.rdf_oracle(Ls[1][::2], cell, TRAJ["nbins"], TRAJ["r_range"])
            return gr.pow(2).mean() + Ls[0][-1].pow(2).mean() + 0.0 * Ls[2][-1].sum()
        _oracle_cache["run"] = oracle_run(x32, cell32, vel, mass, terms, TRAJ["T"], TRAJ["Q"], TRAJ["chains"], t, loss_fn)
    return _oracle_cache["run"]


@pytest.mark.parametrize("graphs_on", [True, False], ids=["graph_replay", "eager"])
def test_eam_term_in_a_stack_trajectory_and_adjoint_vs_oracle(graphs_on):
    """Stack(EAM, density and embed trainable, 128-node tables of Sutton-Chen copper) on 108 jittered copper atoms: 10 NHC steps
    through odeint_adjoint, the loss on rdf of q_t[::2] plus v_t[-1]^2 -- trajectories, adjoint of y0 and dL/dnodes against the
    oracle with eam_table_ref.TableTerm.  The stack stays on the analytic adjoint (force_vjp) and HIP-graph replay although the
    nodes require grad.  Tolerances: those of test_sc_term_in_a_stack_trajectory_and_adjoint_vs_oracle."""
    from mdgrad_amd import graphs
    from mdgrad_amd.interface import Stack
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.sovlers import odeint_adjoint
    eam, system = _traj_module()
    stack = Stack({"eam": eam})
    integ = NoseHooverChain(stack, system, T=TRAJ["T"], num_chains=TRAJ["chains"], Q=TRAJ["Q"], adjoint=True).to(DEV)
    assert integ.fused_spec("NH_verlet") is None, "a tabulated EAM member keeps the stack off the fused trajectory kernels"
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
    traj, lam, gth = oracle_traj(t, eam)
    close(q_t, traj[1], 0, 2e-5, "q_t")
    close(v_t, traj[0], 1e-3, 1e-4 * float(traj[0].abs().max()), "v_t")
    close(pv_t, traj[2], 2e-3, 1e-5, "pv_t")
    for x, l, nm in zip(y0, lam, ("adj v0", "adj q0", "adj pv0")):
        close(x.grad, l, 5e-3, 2e-3 * float(l.abs().max()) + 1e-9, nm)
    g = R.grid_of(eam)
    assert gth.numel() == 2 * (2 * g["n_r"] + g["n_rho"]) and eam.density_nodes.grad is not None and eam.embed_nodes.grad is not None
    want = gth[2 * g["n_r"]:].clone()
    want[:2 * g["n_r"]][-2:] = 0.0                                                   # the pinned last node of f
    got = torch.cat([eam.density_nodes.grad.reshape(-1), eam.embed_nodes.grad.reshape(-1)])
    close(got, want, 5e-3, 5e-4 * float(want.abs().max()), "dL/dnodes (density, embed)")


# ------------------------------------------------------------------------------------------------ 11: torch ops
def test_torch_ops_equal_ctypes_path_and_reject_bad_input():
    from mdgrad_amd import _torch_ops, ops
    ns = _torch_ops.get()
    assert ns is not None
    mod, x32, cell32 = _tric64()
    ell, k = mod._ell, mod._consts
    cell = _torch_ops.cell_args(ell.cell_struct)
    kk = [float(k.n_species), float(k.n_r), float(k.n_rho), k.r_min, k.rc, k.rho_min, mod.rho_range[1], float(k.pin_cutoff)]
    x, w, tab, ty = T(x32, DEV), torch.randn(64, 3, device=DEV), mod._tables(), mod.types
    a = ops.eam_table_eval(ell, x, ty, k, tab, energy=True, grad=True, want_theta=True)
    U, g, hw, gt, gtw = ns.eam_table_eval(x, cell, ell.col, ell.shift, ell.cnt, ty, kk, tab, None, True, True)
    assert torch.equal(U, a["energy"]) and torch.equal(g, a["grad"]) and torch.equal(gt, a["gtab"]) and hw.numel() == gtw.numel() == 0
    b = ops.eam_table_eval(ell, x, ty, k, tab, w=w, energy=False, grad=True, want_theta=True)
    U, g, hw, gt, gtw = ns.eam_table_eval(x, cell, ell.col, ell.shift, ell.cnt, ty, kk, tab, w, False, True)
    assert torch.equal(g, b["grad"]) and torch.equal(hw, b["hw"]) and torch.equal(gtw, b["gtabw"]) and U.numel() == gt.numel() == 0
    with pytest.raises(ValueError):
        ops.eam_table_eval(ell, x, ty, k, tab, work=torch.empty(63, 4, device=DEV))
    with pytest.raises(ValueError):
        ops.eam_table_eval(ell, x, ty, k, tab, want_theta=True, fx=torch.empty(8, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        ops.eam_table_eval(ell, x, ty, k, tab[:-1].contiguous())
    call = lambda **kw: ns.eam_table_eval(*[kw.get(n, v) for n, v in (("x", x), ("cell", cell), ("col", ell.col), ("shift", ell.shift),
                                                                     ("cnt", ell.cnt), ("ty", ty), ("kk", kk), ("tab", tab), ("w", None),
                                                                     ("e", True), ("t", False))])
    assert torch.equal(call()[1], a["grad"])
    bad = [dict(x=x.double()), dict(x=x.cpu()), dict(cell=cell[:5]), dict(col=ell.col.long()), dict(cnt=ell.cnt[:5].contiguous()),
           dict(kk=kk[:7]), dict(ty=ty.long()), dict(ty=ty[:5].contiguous()), dict(ty=ty + 1), dict(ty=ty.cpu()),
           dict(tab=tab[:-2].contiguous()), dict(tab=tab.double()), dict(tab=tab.cpu()), dict(w=w[:5].contiguous()), dict(w=w.double()),
           dict(kk=[0.0] + kk[1:]), dict(kk=[5.0] + kk[1:]), dict(kk=[2.5] + kk[1:]), dict(kk=kk[:1] + [3.0] + kk[2:]),
           dict(kk=kk[:2] + [4097.0] + kk[3:]), dict(kk=kk[:4] + [kk[3]] + kk[5:]), dict(kk=kk[:3] + [-0.5] + kk[4:]),
           dict(kk=kk[:6] + [kk[5]] + kk[7:]), dict(kk=kk[:7] + [2.0])]
    for n, kw in enumerate(bad):
        with pytest.raises((RuntimeError, NotImplementedError)):
            call(**kw)
            pytest.fail("bad input %d was accepted" % n)
