"""Tersoff term, host side: tests/tersoff_ref.py -- the float64 definition the GPU tests compare the kernels with -- against an
independent loop, finite differences, the diamond lattice in closed form and the model's own limits; Tersoff's torch
restatement against it; the argument checks and the validation of the C entry points; and the input conditions of every
configuration that tests/test_gpu_tersoff.py evaluates."""
import ctypes
import math

import numpy as np
import pytest
import torch

import oracle as O
import tersoff_ref as R

SI, CA = R.SILICON, R.CARBON
KSI, KCA = R.consts(**SI), R.consts(**CA)


def _cpu_system(pos, cell):
    from mdgrad_amd.system import System
    return System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
                  masses=np.full(len(pos), 28.0855), device="cpu")


def _f64(v):
    return torch.tensor(np.asarray(v, dtype=np.float64))


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("name", ["si64", "c64", "gas37", "tric64", "lam3", "replicas"])
def test_energy_equals_an_independent_loop(name):
    x32, cell32, p, group = R.gpu_cases()[name]
    for m in ((3, 1) if name == "lam3" else (p.get("m", 3),)):
        k = R.consts(**dict(p, m=m))
        lst = R.bonds_and_triplets(x32, cell32, k["rc"], group=group)
        uR, uA, zeta = R.energy(_f64(x32), _f64(R.theta_of(p)), lst, cell32, k, parts=True)
        lR, lA = R.energy_loops(x32, R.theta_of(p), cell32, k, group=group)
        assert abs(float(uR) - lR) <= 1e-12 * abs(lR) and abs(float(uA) - lA) <= 1e-12 * abs(lA), (float(uR), lR, float(uA), lA)
        assert lR > 0.0 and lA < 0.0
    if group is not None:
        assert int((lst["bc"] // group != lst["be"] // group).sum()) == 0, "replicas do not see each other"


def test_sum_of_the_per_piece_contributions_equals_autograd_and_bounds_it():
    x32, cell32, p, _ = R.gpu_cases()["si64"]
    lst = R.bonds_and_triplets(x32, cell32, KSI["rc"])
    w = np.random.default_rng(3).normal(0, 1, x32.shape)
    ref = R.evaluate(x32, R.theta_of(p), lst, cell32, KSI, w=w)
    for key in ("grad", "hw", "dth", "dthw"):
        assert bool((ref[key].abs() <= ref["A_" + key] * (1 + 1e-12)).all()), key
    assert float(ref["A_U"]) >= abs(float(ref["U"]))
    assert abs(float(ref["A_dth"][0]) * SI["A"] + float(ref["A_dth"][1]) * SI["B"] - float(ref["A_U"])) <= 1e-12 * float(ref["A_U"])
    # translation invariance
    assert float(ref["grad"].sum(0).abs().max()) <= 1e-13 * float(ref["A_grad"].sum(0).max())
    assert float(ref["hw"].sum(0).abs().max()) <= 1e-13 * float(ref["A_hw"].sum(0).max())


@pytest.mark.parametrize("name", ["si64", "lam3", "gas37"])
def test_finite_differences_of_the_float64_energy(name):
    """Central differences of U along a random direction (step 1e-5 A: truncation ~ 1e-10 relative, rounding ~ 1e-11 A_U / step)
    against w . dU/dx, and of w . dU/dx along a second direction against its H w; the same in theta."""
    x32, cell32, p, group = R.gpu_cases()[name]
    k = R.consts(**p)
    lst = R.bonds_and_triplets(x32, cell32, k["rc"], group=group)
    rng = np.random.default_rng(11)
    w, v = rng.normal(0, 1, x32.shape), rng.normal(0, 1, x32.shape)
    th = R.theta_of(p)
    ref = R.evaluate(x32, th, lst, cell32, k, w=w)
    x = _f64(x32)
    U = lambda xx, tt=th: float(R.energy(xx, _f64(tt), lst, cell32, k))
    e = 1e-5
    fd = (U(x + e * _f64(w)) - U(x - e * _f64(w))) / (2 * e)
    an = float((ref["grad"] * _f64(w)).sum())
    assert abs(fd - an) <= 1e-7 * float((ref["A_grad"] * _f64(w).abs()).sum()), (fd, an)

    def wg(xx):
        xx = xx.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(R.energy(xx, _f64(th), lst, cell32, k), xx)
        return float((g * _f64(w)).sum())
    fd2 = (wg(x + e * _f64(v)) - wg(x - e * _f64(v))) / (2 * e)
    an2 = float((ref["hw"] * _f64(v)).sum())
    assert abs(fd2 - an2) <= 1e-6 * float((ref["A_hw"] * _f64(v).abs()).sum()), (fd2, an2)
    for c, step in enumerate((1e-3, 1e-3, 1e-7)):
        tp, tm = list(th), list(th)
        tp[c] += step
        tm[c] -= step
        fd = (U(x, tp) - U(x, tm)) / (2 * step)
        assert abs(fd - float(ref["dth"][c])) <= 1e-6 * float(ref["A_dth"][c]), (c, fd, float(ref["dth"][c]))


@pytest.mark.parametrize("p,a,u_n,a_min", [(SI, 5.432, -4.62960, 5.432), (CA, 3.566, -7.37051, 3.5656)], ids=["silicon", "carbon"])
def test_perfect_diamond_in_closed_form(p, a, u_n, a_min):
    """Four neighbours at a sqrt(3) / 4 inside R - D, the second shell beyond R + D, lam3 = 0: zeta = 3 g(-1/3), and
    U / N = 2 [A exp(-lam1 r0) - b B exp(-lam2 r0)].  The values were computed from the published constants."""
    k = R.consts(**p)
    pos, cell = O.diamond_lattice(2, a)
    lst = R.bonds_and_triplets(pos, cell, k["rc"])
    assert lst["rows"].tolist() == [4] * 64 and lst["tb"].numel() == 64 * 12
    x = _f64(pos).requires_grad_(True)
    uR, uA, zeta = R.energy(x, _f64(R.theta_of(p)), lst, cell, k, parts=True)
    U = float((uR + uA).detach()) / 64
    closed, z, b = R.diamond_closed_form(p, a)
    assert abs(U - u_n) <= 1e-5 and abs(closed - u_n) <= 1e-5 and abs(U - closed) <= 1e-6
    assert float((zeta.detach() - z).abs().max()) <= 1e-6 * z, "every bond has zeta = 3 g(-1/3)"
    if p is SI:
        assert abs(z - 30673.6) <= 0.1 and abs(b - 0.958303) <= 1e-6
    (g,) = torch.autograd.grad(uR + uA, x)
    assert float(g.abs().max()) <= 1e-9, "the forces vanish by symmetry"
    # the minimum over the lattice constant: golden-section search on the closed form, which the lattice sum equals
    lo, hi = a_min - 0.05, a_min + 0.05
    f = lambda s: R.diamond_closed_form(p, s)[0]
    gr = (math.sqrt(5.0) - 1.0) / 2.0
    for _ in range(60):
        c, d = hi - gr * (hi - lo), lo + gr * (hi - lo)
        lo, hi = (lo, d) if f(c) < f(d) else (c, hi)
    assert abs(0.5 * (lo + hi) - a_min) <= 1e-3, 0.5 * (lo + hi)
    for s in (a_min - 0.02, a_min + 0.02):
        pos_s, cell_s = O.diamond_lattice(2, s)
        lst_s = R.bonds_and_triplets(pos_s, cell_s, k["rc"])
        Us = float(R.energy(_f64(pos_s), _f64(R.theta_of(p)), lst_s, cell_s, k)) / 64
        assert abs(Us - f(s)) <= 1e-9 and Us > f(a_min) - 1e-12


def test_cutoff_function_is_continuous_with_its_derivative():
    for k in (KSI, KCA):
        for edge, want in ((k["R"] - k["D"], 1.0), (k["R"] + k["D"], 0.0)):
            r = torch.tensor([edge - 1e-9, edge + 1e-9], dtype=torch.float64, requires_grad=True)
            v = R.fc(r, k)
            (dv,) = torch.autograd.grad(v.sum(), r)
            assert float((v.detach() - want).abs().max()) <= 1e-15 and float(dv.abs().max()) <= 1e-7, (edge, v, dv)
        mid = torch.tensor([k["R"]], dtype=torch.float64, requires_grad=True)
        (dm,) = torch.autograd.grad(R.fc(mid, k).sum(), mid)
        assert abs(float(R.fc(mid, k).detach()) - 0.5) <= 1e-15 and abs(float(dm) + 0.25 * math.pi / k["D"]) <= 1e-12
        assert float(R.fc(torch.tensor([k["rc"], k["rc"] + 1.0], dtype=torch.float64), k).abs().max()) == 0.0


def test_a_dimer_has_zeta_zero_bond_order_one_and_finite_derivatives():
    cell = np.array([14.0, 15.0, 16.0])
    x = np.array([[3.0, 3.0, 3.0], [3.0, 3.0, 5.35]])
    lst = R.bonds_and_triplets(x, cell, KSI["rc"])
    assert lst["bc"].numel() == 2 and lst["tb"].numel() == 0
    ref = R.evaluate(x, R.theta_of(SI), lst, cell, KSI, w=np.array([[0.3, -0.2, 0.5], [0.1, 0.4, -0.7]]))
    assert float(ref["zeta"].abs().max()) == 0.0
    r = 2.35
    want = SI["A"] * math.exp(-SI["lam1"] * r) - SI["B"] * math.exp(-SI["lam2"] * r)              # b = 1
    assert abs(float(ref["U"]) - want) <= 1e-13 * abs(want)
    for key in ("grad", "hw", "dth", "dthw"):
        assert bool(torch.isfinite(ref[key]).all()), key
    assert float(ref["dth"][2]) == 0.0 and float(ref["dthw"][2]) == 0.0, "nothing depends on h"
    assert float(ref["grad"].abs().max()) > 0.0


def test_a_trimer_is_not_symmetric_in_the_bond_order():
    """i - j - k bent, with k bonded to j only: zeta_ij = 0 (i has no other neighbour), zeta_ji = fc g(cos theta_ijk) > 0."""
    cell = np.array([14.0, 15.0, 16.0])
    c = np.array([5.0, 5.0, 5.0])
    ang = np.deg2rad(100.0)
    x = np.array([c + 2.3 * np.array([1.0, 0.0, 0.0]), c, c + 2.4 * np.array([np.cos(ang), np.sin(ang), 0.0])])
    lst = R.bonds_and_triplets(x, cell, KSI["rc"])
    assert lst["rows"].tolist() == [1, 2, 1]
    _, _, zeta = R.energy(_f64(x), _f64(R.theta_of(SI)), lst, cell, KSI, parts=True)
    b = R.bond_order(zeta, KSI)
    ij = int(((lst["bc"] == 0) & (lst["be"] == 1)).nonzero())
    ji = int(((lst["bc"] == 1) & (lst["be"] == 0)).nonzero())
    assert float(zeta[ij]) == 0.0 and float(b[ij]) == 1.0 and float(zeta[ji]) > 0.0 and float(b[ji]) < 1.0 - 1e-3


# ------------------------------------------------------------------------------------------------ the module on the host
@pytest.mark.parametrize("name,extra", [("si64", {}), ("c64", {}), ("lam3", dict(m=3)), ("lam3", dict(m=1))],
                         ids=["silicon", "carbon", "lam3_m3", "lam3_m1"])
def test_torch_energy_equals_the_float64_reference(name, extra):
    from mdgrad_amd.interface import Tersoff
    x32, cell32, p, _ = R.gpu_cases()[name]
    p = dict(p, **extra)
    k = R.consts(**p)
    mod = Tersoff(_cpu_system(x32, cell32), **p)
    assert [n for n, _ in mod.named_parameters()] == ["A", "B", "h"] and not mod.supports_force_vjp()
    assert abs(mod.cutoff - k["rc"]) <= 1e-12
    theta = [float(q.detach()) for q in (mod.A, mod.B, mod.h)]                                    # (float32 parameters)
    lst = R.bonds_and_triplets(x32, cell32, k["rc"])
    w = torch.tensor(np.random.default_rng(7).normal(0, 1, x32.shape))
    ref = R.evaluate(x32, theta, lst, cell32, k, w=w)
    x = torch.tensor(x32).double().requires_grad_(True)
    U = mod(x)
    assert U.dtype == torch.float64
    gx, gA, gB, gh = torch.autograd.grad(U, (x, mod.A, mod.B, mod.h), create_graph=True)
    (hw,) = torch.autograd.grad((gx * w).sum(), x)
    assert abs(float(U.detach()) - float(ref["U"])) <= 1e-12 * float(ref["A_U"])
    assert float((gx.detach() - ref["grad"]).abs().max()) <= 1e-11 * float(ref["A_grad"].max())
    assert float((hw - ref["hw"]).abs().max()) <= 1e-11 * float(ref["A_hw"].max())
    got = torch.stack([t.detach().reshape(()) for t in (gA, gB, gh)]).double()
    assert bool(((got - ref["dth"]).abs() <= 1e-6 * ref["A_dth"]).all())                         # (float32 parameters)


def test_torch_energy_on_replicas_and_frozen_parameters():
    from mdgrad_amd.interface import Tersoff
    base, box, x3 = R.replicas16(R.SEEDS["replicas"])
    mod = Tersoff.silicon(_cpu_system(base, box).replicate(3), trainable=False)
    assert list(mod.parameters()) == [] and set(dict(mod.named_buffers())) >= {"A", "B", "h"}
    th = [float(mod.A), float(mod.B), float(mod.h)]
    assert th == [float(np.float32(v)) for v in (1830.8, 471.18, -0.59825)]
    lst = R.bonds_and_triplets(x3, box, KSI["rc"], group=16)
    got = float(mod(torch.tensor(x3).double()))
    want = float(R.energy(torch.tensor(x3).double(), _f64(th), lst, box, KSI))
    assert abs(got - want) <= 1e-12 * abs(want)
    car = Tersoff.carbon(_cpu_system(*O.diamond_lattice(2, 3.566)))
    assert {n: getattr(car._consts, n) for n in ("lam1", "lam2", "beta", "n", "c", "d", "R", "D")} == \
        {n: CA[n] for n in ("lam1", "lam2", "beta", "n", "c", "d", "R", "D")} and Tersoff.PUBLISHED == dict(silicon=SI, carbon=CA)


def test_argument_checks_raise_value_error():
    from mdgrad_amd.interface import Tersoff
    pos, cell = O.diamond_lattice(2, 5.432)
    s = _cpu_system(pos, cell)
    for kw, word in ((dict(index_tuple=([0], [1])), "index_tuple"), (dict(ex_pairs=[[0, 1]]), "ex_pairs"),
                     (dict(R=5.4, D=0.15), "half the shortest cell height"), (dict(m=2), "m must be 1 or 3"),
                     (dict(A=0.0), "A and B"), (dict(A=-3.0), "A and B"), (dict(B=0.0), "A and B"), (dict(lam1=0.0), "lam1"),
                     (dict(D=0.0), "D > 0"), (dict(R=0.1), "R > D"), (dict(n=0.0), "n must be positive"), (dict(d=0.0), "d must")):
        with pytest.raises(ValueError, match=word):
            Tersoff(s, **dict(SI, **kw))
    tric = _cpu_system(pos, np.array([[10.864, 0, 0], [0, 10.864, 0], [9.0, 0, 5.9]]))
    with pytest.raises(ValueError, match="half the shortest cell height"):
        Tersoff.silicon(tric)                                          # the height along z is 5.9 < 2 (R + D)
    assert "not covered" in Tersoff.__doc__.lower() and "several species" in Tersoff.__doc__


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_entry_points_validate_their_arguments():
    from mdgrad_amd import _lib, ops
    lib = _lib.load()
    p = ctypes.c_void_p(64)                  # never dereferenced: every call below fails its checks first
    cell = _lib.make_cell([11.0, 11.0, 11.0])
    k = ops.tersoff_consts(**SI)

    def broken(**kw):
        b = ops.tersoff_consts(**SI)
        for name, v in kw.items():
            setattr(b, name, v)
        return ctypes.byref(b)

    def fails(rc, word):
        msg = lib.mdg_last_error()
        assert rc == -1 and word.encode() in msg, (rc, word, msg)

    ev, C, Kc = lib.mdg_tersoff_eval, ctypes.byref(cell), ctypes.byref(k)
    #                 pos n cell col shift cnt max consts theta w  energy grad hw pth pthw partial work scale acc stream
    fails(ev(None, 8, C, p, p, p, 8, Kc, None, None, None, p, None, None, None, None, p, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, None, p, p, p, 8, Kc, None, None, None, p, None, None, None, None, p, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, C, p, None, p, 8, Kc, None, None, None, p, None, None, None, None, p, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, C, p, p, p, 8, None, None, None, None, p, None, None, None, None, p, 1.0, 0, None), "consts is null")
    fails(ev(p, 0, C, p, p, p, 8, Kc, None, None, None, p, None, None, None, None, p, 1.0, 0, None), "bad sizes")
    fails(ev(p, 8, C, p, p, p, 0, Kc, None, None, None, p, None, None, None, None, p, 1.0, 0, None), "bad sizes")
    for kw, word in ((dict(A=0.0), "A > 0"), (dict(B=-1.0), "B > 0"), (dict(lam1=0.0), "lam1 > 0"), (dict(lam2=-1.0), "lam2 > 0"),
                     (dict(D=0.0), "D > 0"), (dict(R=0.1), "R > D"), (dict(m=2), "m must be 1 or 3"), (dict(m=0), "m must be 1 or 3"),
                     (dict(n=0.0), "n > 0"), (dict(d=0.0), "d must not be 0")):
        fails(ev(p, 8, C, p, p, p, 8, broken(**kw), None, None, None, p, None, None, None, None, p, 1.0, 0, None), word)
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, None, p, p, None, None, None, p, 1.0, 0, None), "need w")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, None, p, None, None, p, None, p, 1.0, 0, None), "need w")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, p, None, p, None, None, None, None, p, 1.0, 0, None), "without hw")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, None, None, None, None, None, None, p, 1.0, 0, None), "no output")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, p, None, None, None, None, None, p, 1.0, 0, None), "partial")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, None, p, None, None, None, None, None, 1.0, 0, None), "bond_work")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, p, None, None, p, None, None, None, None, 1.0, 0, None), "bond_work")
    assert lib.mdg_tersoff_partial_size(64) == 4 and lib.mdg_tersoff_partial_size(37) == 3 and lib.mdg_tersoff_partial_size(0) == 0
    assert lib.mdg_tersoff_work_size(64, 8) == 4 * 64 * 8 and lib.mdg_tersoff_work_size(0, 8) == 0
    assert lib.mdg_tersoff_work_size(1 << 20, 1 << 10) == 4 << 30, "64-bit"
    assert ctypes.sizeof(_lib.MdgTersoffConsts) == 13 * 8 + 8
    for bad in (dict(A=0.0), dict(B=-1.0), dict(lam1=0.0), dict(D=0.0), dict(R=0.1), dict(m=2), dict(m=1.5), dict(n=0.0), dict(d=0.0)):
        with pytest.raises(ValueError):
            ops.tersoff_consts(**dict(SI, **bad))


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
@pytest.mark.parametrize("name", ["si64", "c64", "gas37", "tric64", "lam3", "replicas", "skin", "traj"])
def test_input_conditions_of_the_gpu_configurations(name):
    """At least 10 directed bonds strictly inside the taper (R - D, R + D); no pair separation within 0.01 A of R - D or
    R + D (a bond there would make the comparison depend on the rounding of r against the edge); a bond with zeta = 0 in the
    sets whose tests speak of one."""
    x32, cell32, p, group = R.gpu_cases()[name]
    k = R.consts(**p)
    inside, gap = R.taper_census(x32, cell32, k, group=group)
    assert inside >= 10, inside
    assert gap >= 0.01, gap
    if name in ("gas37", "replicas"):
        lst = R.bonds_and_triplets(x32, cell32, k["rc"], group=group)
        _, _, zeta = R.energy(_f64(x32), _f64(R.theta_of(p)), lst, cell32, k, parts=True)
        assert int((zeta == 0).sum()) >= 1
    if name == "gas37":
        rows = lst["rows"].tolist()
        assert rows[31] == 0 and rows[32] == rows[33] == 1 and rows[34:37] == [2, 1, 1] and rows[0] > 16
        pair = (lst["bc"] == 32) & (lst["be"] == 33)
        assert int(pair.sum()) == 1 and float(zeta[pair]) == 0.0, "the isolated dimer"
