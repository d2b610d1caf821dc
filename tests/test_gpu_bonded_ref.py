"""csrc/bonded.hip (mdg_bonded_eval: BondPotentials / AnglePotentials) against the float64 definitions of tests/bonded_ref.py
(pinned to the reference's goldens, to finite differences and to the oracle by tests/test_bonded_host.py), at the edges the
24-atom golden chain does not reach: several workgroups, hubs, atoms in no term, empty tables, anisotropic and triclinic cells,
bond components of exactly +-L/2, angles down to 1e-5 of 0 and pi and exactly collinear ones, every output combination, `into`
buffers, autograd with an upstream gradient, and the torch route.

Error measure.  |got - ref64| per atom and component over that atom's scale (bonded_ref.scale: the sum over its incident terms
of the magnitude of the term's factors); energies over sum |U_term|.  The near-collinear cases bound err * sin(theta).

Tolerance.  Nothing is fixed in advance and nothing comes from the kernel: for every case the reference's own formulas are
evaluated in float32 on the CPU over exactly the case's float32 inputs; their distance from float64, in the same measure, is the
case's FLOOR (at least one unit roundoff, 2^-24), and a check allows MARGIN = 10 x the largest floor of its case group (the
margin of the pressure kernels: fused multiply-adds, reciprocals, another atan2).  The floors of the cases below, and what the kernel showed on an MI355X:

    group (floor = largest of its cases)          floor: energy  e_atom   grad     hw     | kernel: energy  e_atom   grad     hw
    A bond   chains 1..600, stars, extras                8.1e-7   1.8e-7   2.9e-7   7.3e-7 |         2.7e-7  1.8e-7   2.9e-7   7.2e-7
    A angle                                              1.5e-7   2.7e-7   3.8e-7   5.9e-7 |         1.8e-7  2.7e-7   4.9e-7   7.0e-7
    B bond   cell 3.0 x 4.5 x 7.0                        6.0e-8   9.1e-8   1.6e-7   1.9e-7 |         3.7e-10 8.3e-8   1.6e-7   1.9e-7
    B angle                                              1.7e-7   1.4e-7   2.1e-7   4.4e-7 |         5.5e-8  1.4e-7   2.4e-7   3.6e-7
    B triclinic System (through the modules)             9.9e-7   -        2.2e-7   7.4e-7 |         1.9e-7  -        1.8e-7   3.8e-7
    C exactly collinear rows                             6.0e-8   6.0e-8   6.6e-8   9.8e-8 |         5.3e-9  2.6e-8   6.6e-8   1.2e-7
    C rod, dy = 1e-3, theta0 = pi                        8.7e-5   6.0e-8   6.5e-8   1.9e-7 |         8.7e-5  3.5e-11  6.5e-8   1.9e-7
    D bond / angle   257-chain, cell 3.0 x 4.5 x 7.0     6.8e-7 / 1.1e-7   1.3e-7 / 1.1e-7   3.4e-7 / 4.2e-7   2.8e-7 / 5.9e-7
                                                         | kernel 1.9e-8 / 1.3e-8   1.3e-7 / 1.8e-7   3.4e-7 / 4.2e-7   3.2e-7 / 4.7e-7
    (the energy floor is the per-term sum of bonded_ref.Case.energy_floor: one scalar's own error is no floor)

    C sweep, largest over theta = delta and pi - delta, theta0 = 1.9 and pi (each of the four cases is held to its own floor);
    grad and hw as err * sin(theta):
    delta     floor: energy  grad     hw      | kernel: energy  grad     hw      | largest kernel / floor of a case
    1                7.2e-7  4.8e-7   7.0e-7  |         3.4e-7  5.2e-7   7.7e-7  | 0.8  1.2  1.1
    0.3              6.8e-7  1.4e-7   5.9e-7  |         8.8e-7  1.8e-7   7.9e-7  | 1.3  1.5  1.4
    0.1              1.2e-6  1.3e-7   8.5e-7  |         2.7e-6  2.1e-7   1.2e-6  | 2.7  1.7  4.5
    0.03             6.9e-6  1.2e-7   4.1e-6  |         7.6e-6  1.4e-7   4.1e-6  | 1.2  1.2  1.1
    0.01             2.0e-5  1.3e-7   9.7e-6  |         2.0e-5  1.2e-7   9.7e-6  | 1.0  1.0  1.3
    0.003            4.6e-5  1.2e-7   3.9e-5  |         4.7e-5  1.2e-7   3.9e-5  | 1.0  0.9  1.0
    0.001            1.7e-4  1.2e-7   1.3e-4  |         3.1e-4  1.9e-7   1.3e-4  | 2.1  1.5  1.8
    3e-4             5.6e-4  1.4e-7   4.2e-4  |         9.8e-4  1.9e-7   4.3e-4  | 2.0  1.4  1.2
    1e-4             9.4e-4  9.9e-8   8.9e-4  |         2.5e-3  2.0e-7   8.9e-4  | 3.9  2.0  2.8
    1e-5             1.5e-2  1.2e-7   2.2e-2  |         1.5e-2  1.2e-7   2.2e-2  | 1.0  1.0  1.0
    The force floor is flat in delta: the atan2 form loses nothing towards collinearity.  That of H w grows like 1 / delta (the
    direction of b1 x b2 is known to 2^-24 / sin theta and d^2 theta / db^2 ~ cot theta), that of the energy likewise for
    theta0 = pi at pi - delta, where theta - theta0 is a difference of two float32 numbers next to pi.  Kernel figures that equal
    their floor share its dominant rounding, the float32 difference of two positions.  The floors move by some 20 % between
    CPUs (vectorised float32 atan2); the figures above are from the host of the MI355X.

(Every test prints floor, tolerance and the kernel's figure per case and quantity; MDG_TEST_REPORT=<file> collects them.)

Before the angle term was rewritten on atan2 and the cross product, its acos form (the previous kernel, run once) failed group C
from delta = 0.3 inward: err * sin(theta) of the force at theta0 = 1.9 was 2.6e-7 (0.3), 5.6e-7 (0.1), 2.1e-6 (0.03), 4.0e-6
(0.01), 1.8e-5 (0.003), 4.7e-5 (0.001) against floors of 6e-8, that of H w 2.0e-6, 2.0e-5, 2.3e-4, 1.2e-3, 2.0e-2, 1.4e-1 against
floors of 2.1e-7 .. 3.3e-5 (first excess: H w at pi - 0.3, 6.2e-6 against 5.9e-6 allowed); at 3e-4, 1e-4 and 1e-5, on the exactly
collinear rows and on the straight rod the force and H w were not finite."""
import math
import os

import numpy as np
import pytest
import torch

import bonded_ref as R
from test_gpu_parity import T, mk_system, DEV

pytestmark = pytest.mark.gpu
MARGIN = 10.0
ULP = 2.0 ** -24
KINDS = {"bond": R.BOND, "angle": R.ANGLE}


def _report(line):
    print(line)
    if os.environ.get("MDG_TEST_REPORT"):
        with open(os.environ["MDG_TEST_REPORT"], "a") as fh:
            fh.write(line + "\n")


def _table(case):
    from mdgrad_amd import ops
    return ops.BondedTable(case.kind, case.top, case.n_atoms, [float(x) for x in case.L], case.k, case.x0, DEV)


def _launch(case, hvp=True):
    from mdgrad_amd import ops
    o = ops.bonded_eval(_table(case), T(case.pos, DEV), w=T(case.w, DEV) if hvp else None, energy=True)
    return dict(energy=o["e_atom"].double().sum().cpu(), e_atom=o["e_atom"], grad=o["grad"], hw=o["hw"])


def _floors(cases, sin_weighted=False):
    """The largest float32 floor of the group per quantity, with a cap that a broken reference or scale would break: the force
    of a few float32 operations lies within 64 ulp of its factor scale, H w within 64 ulp / sin(theta)."""
    fl = dict.fromkeys(R.QUANTITIES, ULP)       # (no float32 result is better than its own rounding, 2^-24: dyadic inputs
    #                                              that happen to evaluate exactly on the CPU are no licence for a zero tolerance)
    smin = 1.0
    for c in cases:
        ref, sc, r32 = c.reference()
        smin = min(smin, float(sc["sin"].min()))
        for q, v in R.ratios(r32, ref, sc, sin_weighted).items():
            fl[q] = max(fl[q], c.energy_floor() if q == "energy" else v)
    assert fl["grad"] <= 64 * ULP and fl["hw"] <= 64 * ULP / (smin if sin_weighted else 1.0), (fl, smin)
    return fl


def _check(cases, label, sin_weighted=False, outputs=None):
    """Both instantiations of the kernel (with and without H w) on every case against float64, at MARGIN x the group's floor.
    Every figure is printed before anything is asserted.  `outputs` (case -> list of dicts) replaces the two launches."""
    fl = _floors(cases, sin_weighted)
    bad = []
    for c in cases:
        ref, sc, _ = c.reference()
        outs = outputs(c) if outputs is not None else [_launch(c, True), _launch(c, False)]
        for o in outs:
            for q, v in R.ratios(o, ref, sc, sin_weighted).items():
                _report("%-12s %-40s %-7s floor %.3e  allowed %.3e  kernel %.3e%s" % (
                    label, c.name, q, fl[q], MARGIN * fl[q], v, "" if v <= MARGIN * fl[q] else "   <-- FAILS"))
                if not v <= MARGIN * fl[q]:
                    bad.append((c.name, q, v, MARGIN * fl[q]))
    assert not bad, "%s: %d figures above %g x floor, the first: %s" % (label, len(bad), MARGIN, bad[0])
    return fl


# ------------------------------------------------------------------------------------------------ A: grid and incidence lists
def _grid_cases(kind):
    cases = [R.chain_case(kind, n) for n in (1, 2, 3, 255, 256, 257)]
    cases.append(R.chain_case(kind, 500, free=100, extras=True))
    cases += [R.star_case(kind, n, hub_last) for n in (257, 600) for hub_last in (False, True)]
    return cases


@pytest.mark.parametrize("tag", ["bond", "angle"])
def test_grid_and_incidence_lists(tag):
    """N = 1, 2, 3 (no term, one term), 255, 256, 257 (the workgroup boundary) and 600 (three workgroups, 100 atoms in no term,
    five duplicated rows, five rows in the other direction, one in negative indices), and a hub of degree 64 at index 0 and at
    N - 1 -- for angles the hub is centre, first end and last end, 189 entries in its list.  Floors and the kernel's figures: see
    the file's docstring, group A."""
    cases = _grid_cases(KINDS[tag])
    assert [c.n_atoms for c in cases] == [1, 2, 3, 255, 256, 257, 600, 257, 257, 600, 600]
    tab = _table(cases[7])
    deg = (tab.inc_ptr[1:] - tab.inc_ptr[:-1]).cpu()
    assert int(deg[0]) == (64 if tag == "bond" else 189) and int(deg[200:].max()) == 0
    assert int((_table(cases[8]).inc_ptr[-1] - _table(cases[8]).inc_ptr[-2])) == int(deg[0]), "the hub as the last atom"
    _check(cases, "A " + tag)
    free = _launch(cases[6])
    for q in ("e_atom", "grad", "hw"):
        assert float(free[q][500:].abs().max()) == 0.0, "an atom in no term gets exact zeros"


@pytest.mark.parametrize("tag", ["bond", "angle"])
@pytest.mark.parametrize("n", [1, 3, 257])
def test_empty_table(tag, n):
    """n_terms = 0: every output is zero, and `into` buffers come back bitwise unchanged."""
    from mdgrad_amd import ops
    case = R.empty_case(KINDS[tag], n)
    tab = _table(case)
    assert tab.n_terms == 0
    o = ops.bonded_eval(tab, T(case.pos, DEV), w=T(case.w, DEV), energy=True)
    for q in ("e_atom", "grad", "hw"):
        assert o[q].shape[0] == n and float(o[q].abs().max()) == 0.0
    assert float(ops.bonded_eval(tab, T(case.pos, DEV))["grad"].abs().max()) == 0.0
    g = torch.Generator().manual_seed(n)
    F0, D0 = torch.randn(n, 3, generator=g).to(DEV), torch.randn(n, 3, generator=g).to(DEV)
    for s in (-1.0, 0.5):
        F1, D1 = F0.clone(), D0.clone()
        o = ops.bonded_eval(tab, T(case.pos, DEV), w=T(case.w, DEV), into=(F1, D1), scale=s)
        assert o["grad"] is F1 and o["hw"] is D1
        assert torch.equal(F1.view(torch.int32), F0.view(torch.int32)) and torch.equal(D1.view(torch.int32), D0.view(torch.int32))


# ------------------------------------------------------------------------------------------------ B: images
@pytest.mark.parametrize("tag", ["bond", "angle"])
def test_images_in_an_anisotropic_cell(tag):
    """Cell 3.0 x 4.5 x 7.0, positions unwrapped by up to one cell (raw bond components beyond +-0.9 L on every axis), and on
    every axis a raw bond component of exactly +L/2 (folded to -L/2), -L/2 (kept), +3L/2 and -3L/2 (left at +L/2 and -L/2: the
    single flag of topology.get_offsets folds once, and the reference applies the same rule), in dyadic coordinates.  Floors and
    the kernel's figures: group B."""
    case = R.image_case(KINDS[tag])
    L = case.L.astype(np.float64)
    x = case.pos.astype(np.float64)
    raw = x[case.top[:, 0]] - x[case.top[:, 1]]
    chain = raw[:-12]
    assert (chain.max(0) > 0.9 * L).all() and (chain.min(0) < -0.9 * L).all() and (np.abs(raw) <= 1.5 * L).all()
    b = R.bond_vectors(torch.tensor(x), case.top[:, :2], L).numpy()
    for a in range(3):
        for half, folded in ((0.5, -0.5), (-0.5, -0.5), (1.5, 0.5), (-1.5, -0.5)):      # +L/2 is folded, -L/2 is kept, once
            hit = raw[:, a] == half * L[a]
            assert hit.sum() == 1 and (b[hit, a] == folded * L[a]).all(), (a, half)
    _check([case], "B " + tag)


def test_a_triclinic_system_takes_the_diagonal_of_its_cell():
    """BondPotentials / AnglePotentials keep cell.diag() (torchmd/interface.py:429-431), also of a triclinic System; so does the
    reference here.  Through the modules: energy, force, force_vjp."""
    from mdgrad_amd.interface import AnglePotentials, BondPotentials
    cell = np.array([[5.0, 0.0, 0.0], [0.8, 5.5, 0.0], [0.3, -0.6, 6.0]])
    L = np.diag(cell)
    x = np.mod(R.random_chain(40, 41), L)
    system = mk_system(x, cell)
    for cls, kind in ((BondPotentials, R.BOND), (AnglePotentials, R.ANGLE)):
        case = R.Case("triclinic", kind, x, R.chain_rows(kind, 40), cell, seed=40)
        assert case.L.tolist() == [5.0, 5.5, 6.0]
        mod = cls(system, torch.as_tensor(case.top), case.k, case.x0)
        q, w = T(case.pos, DEV), T(case.w, DEV)

        def through_the_module(c):
            F, dq, gth = mod.force_vjp(q, w)
            assert gth == []
            return [dict(energy=mod(q).double().cpu(), grad=-F, hw=-dq), dict(grad=-mod.force(q))]
        _check([case], "B triclinic", outputs=through_the_module)


# ------------------------------------------------------------------------------------------------ C: angles near 0 and pi
@pytest.mark.parametrize("delta", R.SWEEP)
def test_angles_near_0_and_pi(delta):
    """64 isolated triplets at theta = delta and at pi - delta in random orientations, theta0 = 1.9 and pi: energy, force and
    H w, the last two as err * sin(theta) over the scale, each case against 10 x its own floor (file docstring, group C).  The
    force floor is flat in delta -- the atan2 form loses nothing towards collinearity -- and that of H w grows like 1 / delta
    (the direction of b1 x b2 is known to 2^-24 / sin theta, and d^2 theta / db^2 ~ cot theta)."""
    for at_pi in (False, True):
        for theta0 in (R.TH0, R.PI32):
            case = R.sweep_case(delta, at_pi, theta0)
            th, regular = R.angle_geometry(torch.tensor(case.pos).double(), case.top, case.L)[2:]
            off = (math.pi - th) if at_pi else th
            assert bool(regular.all()) and float((off / delta - 1).abs().max()) < 0.05, "the float32 inputs keep the angle"
            _check([case], "C sweep", sin_weighted=True)


@pytest.mark.parametrize("theta0", [R.TH0, R.PI32])
def test_exactly_collinear_triplets(theta0):
    """b2 = -2 b1 and b2 = b1 / 2 in dyadic coordinates (the cross product is exactly zero in float32), and a bond vector of
    length zero: everything is finite, the atoms of these rows alone get exact zeros in force and H w, the rows' energies are
    1/2 k (pi - theta0)^2, 1/2 k theta0^2 and 1/2 k theta0^2; the bent row on the centre of the first still acts."""
    case = R.collinear_case(theta0)
    _check([case], "C collinear", sin_weighted=True)
    for hvp in (True, False):
        o = _launch(case, hvp)
        for q in ("grad", "hw") if hvp else ("grad",):
            assert bool(torch.isfinite(o[q]).all()) and float(o[q][R.COLLINEAR_ONLY].abs().max()) == 0.0
            assert float(o[q][[1, 2, 12]].abs().min()) > 0.0
        e = o["e_atom"].cpu().double()
        want = [0.5 * case.k * (R.PI32 - theta0) ** 2, 0.5 * case.k * theta0 ** 2, 0.5 * case.k * theta0 ** 2]
        for atom, u in zip((0, 4, 9), want):             # role-0 atoms of the three collinear rows (atan2f(0, -x) is float32 pi)
            assert abs(float(e[atom]) - u) <= 4 * ULP * max(u, 0.5 * case.k * theta0 ** 2)


@pytest.mark.parametrize("dy", [1e-3, 0.0])
def test_rod_along_x_with_theta0_pi(dy):
    """A stiff chain as it is initialised: 16 atoms along x, theta0 = pi, alternate atoms displaced by 1e-3 in y (angles of
    pi - 4e-3) -- and not displaced at all: exactly collinear, zero force and H w, finite, zero energy."""
    case = R.rod_case(dy)
    _check([case], "C rod", sin_weighted=True)
    if dy == 0.0:
        o = _launch(case)
        for q in ("e_atom", "grad", "hw"):
            assert float(o[q].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ D: structure of H w
@pytest.mark.parametrize("tag", ["bond", "angle"])
def test_structure_of_the_hessian_vector_product(tag):
    """On the 257-chain in the anisotropic cell: u.(H w) = w.(H u), sum of the forces = 0, H (constant w) = 0 -- each within
    what 10 x the case's floor allows per entry: |u.(Hw) - w.(Hu)| <= tol sum_n s_n (|u_n|_1 + |w_n|_1), |sum_n g_n| <= tol
    sum_n s_n per component, |H const| <= tol s_n, s the per-atom scale.  (H w for random w against float64: groups A and B.)"""
    from mdgrad_amd import ops
    case = R.chain_case(KINDS[tag], 257, L=R.ANISO)
    fl = _check([case], "D " + tag)
    ref, sc, _ = case.reference()
    tab, q = _table(case), T(case.pos, DEV)
    u = torch.tensor(np.random.default_rng(2).normal(0, 1, case.pos.shape).astype(np.float32))
    w = torch.tensor(case.w)
    Hw = ops.bonded_eval(tab, q, w=w.to(DEV))["hw"].cpu().double()
    o = ops.bonded_eval(tab, q, w=u.to(DEV))
    Hu, g = o["hw"].cpu().double(), o["grad"].cpu().double()
    asym = abs(float((u.double() * Hw).sum() - (w.double() * Hu).sum()))
    allowed = MARGIN * fl["hw"] * float((sc["hw"] * (u.abs().sum(1) + w.abs().sum(1)).double()).sum())
    _report("D %-5s u.Hw - w.Hu %.3e allowed %.3e (u.Hw = %.3e)" % (tag, asym, allowed, float((u.double() * Hw).sum())))
    assert asym <= allowed
    net, net_allowed = float(g.sum(0).abs().max()), MARGIN * fl["grad"] * float(sc["grad"].sum())
    _report("D %-5s |sum F| %.3e allowed %.3e" % (tag, net, net_allowed))
    assert net <= net_allowed
    const = torch.tensor([0.3, -1.7, 0.9]).expand(case.n_atoms, 3).contiguous()
    Hc = ops.bonded_eval(tab, q, w=const.to(DEV))["hw"]
    rc = R.ratio(Hc, torch.zeros(case.n_atoms, 3), sc["hw"])
    _report("D %-5s H const %.3e allowed %.3e" % (tag, rc, MARGIN * fl["hw"]))
    assert rc <= MARGIN * fl["hw"]


# ------------------------------------------------------------------------------------------------ E: outputs and autograd
@pytest.mark.parametrize("tag", ["bond", "angle"])
def test_every_output_combination(tag):
    """energy x grad x w: what is not asked for is None, what is asked for equals, bit for bit, the launch of the same
    instantiation (with or without H w) that asks for everything -- grad=False with w is BondedGradFn.backward's call -- and
    asking for nothing is refused.  600 atoms: two launches are bitwise equal."""
    from mdgrad_amd import ops
    case = R.chain_case(KINDS[tag], 500, free=100, extras=True)
    tab, q, w = _table(case), T(case.pos, DEV), T(case.w, DEV)
    full = {True: ops.bonded_eval(tab, q, w=w, energy=True, grad=True), False: ops.bonded_eval(tab, q, energy=True, grad=True)}
    again = ops.bonded_eval(tab, q, w=w, energy=True, grad=True)
    for k in ("e_atom", "grad", "hw"):
        assert torch.equal(full[True][k], again[k]), "two launches are bitwise equal"
    assert full[False]["hw"] is None
    for energy in (False, True):
        for grad in (False, True):
            for hvp in (False, True):
                if not (energy or grad or hvp):
                    with pytest.raises(RuntimeError, match="no output"):
                        ops.bonded_eval(tab, q, energy=False, grad=False)
                    continue
                o = ops.bonded_eval(tab, q, w=w if hvp else None, energy=energy, grad=grad)
                for k, asked in (("e_atom", energy), ("grad", grad), ("hw", hvp)):
                    assert (o[k] is not None) == asked, (energy, grad, hvp, k)
                    if asked:
                        assert torch.equal(o[k], full[hvp][k]), (energy, grad, hvp, k)
    with pytest.raises(ValueError, match="w must be"):
        ops.bonded_eval(tab, q, w=w[:-1])


@pytest.mark.parametrize("tag", ["bond", "angle"])
@pytest.mark.parametrize("s", [-1.0, 0.5])
def test_into_buffers_and_scale(tag, s):
    """`into` = (F0, D0), scale s: the buffers hold F0 + s dU/dx and D0 + s H w -- each entry within 10 x the case's floor of
    |s| x its scale, plus the rounding of the one fused multiply-add that forms it, 2^-23 (|F0| + |s| scale)."""
    from mdgrad_amd import ops
    case = R.chain_case(KINDS[tag], 257, L=R.ANISO)
    fl = _floors([case])
    ref, sc, _ = case.reference()
    g = torch.Generator().manual_seed(3)
    F0, D0 = torch.randn(257, 3, generator=g), torch.randn(257, 3, generator=g)
    F1, D1 = F0.clone().to(DEV), D0.clone().to(DEV)
    o = ops.bonded_eval(_table(case), T(case.pos, DEV), w=T(case.w, DEV), into=(F1, D1), scale=s)
    assert o["grad"] is F1 and o["hw"] is D1
    for got, b0, q in ((F1, F0, "grad"), (D1, D0, "hw")):
        err = (got.cpu().double() - (b0.double() + s * ref[q])).abs()
        a = abs(s) * sc[q][:, None]
        allowed = MARGIN * fl[q] * a + 2.0 ** -23 * (b0.double().abs() + a)
        _report("E into %-5s s %+.1f %-4s worst err / allowed %.3f" % (tag, s, q, float((err / allowed).max())))
        assert bool((err <= allowed).all())


@pytest.mark.parametrize("tag", ["bond", "angle"])
def test_energy_fn_under_a_loss_with_an_upstream_gradient(tag):
    """BondedEnergyFn -> BondedGradFn through autograd: loss = U^2 + (dU/dx . w).sum(), so dloss/dx = 2 U dU/dx + H w -- an
    upstream gradient of 2 U on the energy and a second derivative -- against float64 autograd of the reference.  Allowed per
    entry, with the case's floors f: 10 (2 |U| f_grad s_grad + 2 f_energy sum|U_t| |dU/dx| + f_hw s_hw)."""
    from mdgrad_amd.interface import AnglePotentials, BondPotentials
    case = R.chain_case(KINDS[tag], 257, L=R.ANISO)
    fl = _floors([case])
    ref, sc, _ = case.reference()
    mod = (BondPotentials if tag == "bond" else AnglePotentials)(mk_system(case.pos, case.L), torch.as_tensor(case.top), case.k, case.x0)
    x, w = T(case.pos, DEV).requires_grad_(True), T(case.w, DEV)
    U = mod(x)
    (g,) = torch.autograd.grad(U, x, create_graph=True)
    loss = U * U + (g * w).sum()
    (dl,) = torch.autograd.grad(loss, x)
    x64 = torch.tensor(case.pos).double().requires_grad_(True)
    U64 = R.energy(x64, *case.args())
    (g64,) = torch.autograd.grad(U64, x64, create_graph=True)
    l64 = U64 * U64 + (g64 * torch.tensor(case.w).double()).sum()
    (dl64,) = torch.autograd.grad(l64, x64)
    u, su = abs(float(U64.detach())), float(sc["energy"])
    allowed = MARGIN * (2 * u * fl["grad"] * sc["grad"][:, None] + 2 * fl["energy"] * su * g64.detach().abs() + fl["hw"] * sc["hw"][:, None])
    err = (dl.cpu().double() - dl64).abs()
    _report("E loss %-5s U %.6e (ref %.6e) loss %.6e (ref %.6e) worst err / allowed %.3f" % (
        tag, float(U.detach()), float(U64.detach()), float(loss.detach()), float(l64.detach()), float((err / allowed).max())))
    assert abs(float(U.detach()) - float(U64.detach())) <= MARGIN * fl["energy"] * su
    assert bool(torch.isfinite(dl).all()) and bool((err <= allowed).all())


# ------------------------------------------------------------------------------------------------ F: the torch route
def _torch_route_cases():
    return [R.chain_case(R.BOND, 257, L=R.ANISO), R.chain_case(R.ANGLE, 257, L=R.ANISO), R.sweep_case(1e-3, False, R.TH0),
            R.sweep_case(1e-3, True, R.TH0), R.sweep_case(1e-3, True, R.PI32), R.collinear_case(R.TH0), R.collinear_case(R.PI32)]


def _module(case, k=None, x0=None):
    from mdgrad_amd.interface import AnglePotentials, BondPotentials
    cls = BondPotentials if case.kind == R.BOND else AnglePotentials
    return cls(mk_system(case.pos, case.L), torch.as_tensor(case.top), case.k if k is None else k, case.x0 if x0 is None else x0)


def _autograd_outputs(mod, x, w):
    U = mod(x)
    (g,) = torch.autograd.grad(U, x, create_graph=True, allow_unused=True)
    hw = torch.autograd.grad((g * w).sum(), x, allow_unused=True)[0] if g.requires_grad else torch.zeros_like(x)
    return dict(energy=U.detach().double().cpu(), grad=g.detach(), hw=torch.zeros_like(x) if hw is None else hw)


def test_torch_route_float64_positions():
    """float64 device positions take AnglePotentials / BondPotentials._torch_energy, the same function as the kernel and as the
    reference (itself float64 on the CPU): allowed 10 x the case's float32 floor x 2^-29, the ratio of the unit roundoffs.
    The chain, theta = 1e-3 and pi - 1e-3 (err * sin theta), and the exactly collinear rows."""
    bad = []
    for case in _torch_route_cases():
        mod = _module(case)
        x = T(case.pos, DEV).double().requires_grad_(True)
        assert not mod._hip_ok(x)
        out = _autograd_outputs(mod, x, T(case.w, DEV).double())
        ref, sc, _ = case.reference()
        fl = _floors([case], True)
        for q, v in R.ratios(out, ref, sc, True).items():
            _report("F float64   %-40s %-7s allowed %.3e  torch route %.3e" % (case.name, q, MARGIN * fl[q] * 2.0 ** -29, v))
            if not v <= MARGIN * fl[q] * 2.0 ** -29:
                bad.append((case.name, q, v))
    assert not bad, bad


def _constant_gradients(case, dtype):
    k = torch.tensor(case.k, dtype=dtype, requires_grad=True)
    x0 = torch.tensor(case.x0, dtype=dtype, requires_grad=True)
    return torch.autograd.grad(R.energy(torch.tensor(case.pos).to(dtype), case.kind, case.top, k, x0, case.L), (k, x0))


def test_torch_route_constants_that_require_grad():
    """k and ro / theta0 as device tensors that require grad switch the term to the torch route in float32: U, dU/dx and H w at
    10 x the float32 floor like the kernel, dU/dk and dU/dx0 against float64 autograd of the reference at 10 x their own float32
    floor, over the scales sum_t 1/2 m_t^2 and sum_t k m_t, m_t = max(|b|^2, ro) resp. max(theta, theta0)."""
    bad = []
    for case in _torch_route_cases():
        k = torch.tensor(case.k, device=DEV, requires_grad=True)
        x0 = torch.tensor(case.x0, device=DEV, requires_grad=True)
        mod = _module(case, k, x0)
        assert not mod._hip_ok() and not mod.supports_force_vjp()
        x = T(case.pos, DEV).requires_grad_(True)
        out = _autograd_outputs(mod, x, T(case.w, DEV))
        ref, sc, _ = case.reference()
        fl = _floors([case], True)
        for q, v in R.ratios(out, ref, sc, True).items():
            _report("F trainable %-40s %-7s allowed %.3e  torch route %.3e" % (case.name, q, MARGIN * fl[q], v))
            if not v <= MARGIN * fl[q]:
                bad.append((case.name, q, v))
        x64 = torch.tensor(case.pos).double()
        m = (R.bond_vectors(x64, case.top, case.L).pow(2).sum(-1).clamp(min=case.x0) if case.kind == R.BOND
             else R.angle_geometry(x64, case.top, case.L)[2].clamp(min=case.x0))
        scales = (float(0.5 * m.pow(2).sum()), float(case.k * m.sum()))
        got = torch.autograd.grad(mod(x), (k, x0))
        r64, r32 = _constant_gradients(case, torch.float64), _constant_gradients(case, torch.float32)
        for name, a, b, c, s in zip(("dU/dk", "dU/dx0"), got, r64, r32, scales):
            floor, v = max(abs(float(c) - float(b)) / s, ULP), abs(float(a) - float(b)) / s
            _report("F trainable %-40s %-7s floor %.3e  allowed %.3e  torch route %.3e" % (case.name, name, floor, MARGIN * floor, v))
            assert floor <= 64 * ULP
            if not v <= MARGIN * floor:
                bad.append((case.name, name, v))
    assert not bad, bad
