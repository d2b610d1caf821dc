"""Sutton-Chen term, host side: tests/eam_ref.py -- the float64 definition the GPU tests compare the kernels with -- against an
independent loop, the fcc lattice sums and its own invariances; SuttonChen's torch restatement against it; the argument checks
and the validation of the C entry points."""
import ctypes
import math

import numpy as np
import pytest
import torch

import eam_ref as R
import oracle as O

CU = R.PUBLISHED["copper"]
TH = torch.tensor(CU[:3], dtype=torch.float64)
RC = 5.2


def _k(shift="force", n=CU[3], m=CU[4], rc=RC):
    return R.consts(n, m, rc, shift)


def _cpu_system(pos, cell):
    from mdgrad_amd.system import System
    return System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
                  masses=np.full(len(pos), 63.546), device="cpu")


def _cu108(seed=108, jit=0.15):
    x32, cell32 = R.jittered_fcc(3, 3.61, jit, seed)
    return x32, cell32, R.pairs(x32, cell32, RC)


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("shift", ["force", "none"])
def test_energy_equals_an_independent_double_loop(shift):
    k = _k(shift)
    x32, cell32, lst = _cu108()
    assert int(lst["rows"].min()) >= 40 and int(lst["rows"].max()) >= 54
    up, ue = R.energy(torch.tensor(x32).double(), TH, lst, cell32, k, parts=True)
    lp, le = R.energy_loops(x32, CU[:3], cell32, k)
    assert abs(float(up) - lp) <= 1e-12 * abs(lp) and abs(float(ue) - le) <= 1e-12 * abs(le), (float(up), lp, float(ue), le)
    assert lp > 0.0 and le < 0.0
    # the same on three replicas that must not see each other
    x3 = np.concatenate([x32, R.jittered_fcc(3, 3.61, 0.15, 109)[0], R.jittered_fcc(3, 3.61, 0.1, 110)[0]])
    lst3 = R.pairs(x3, cell32, RC, group=108)
    assert int((lst3["i"] // 108 != lst3["j"] // 108).sum()) == 0
    u = float(R.energy(torch.tensor(x3).double(), TH, lst3, cell32, k))
    l = sum(R.energy_loops(x3, CU[:3], cell32, k, group=108))
    assert abs(u - l) <= 1e-12 * abs(l)


def test_perfect_fcc_copper_equals_the_truncated_lattice_sums_and_is_stationary_at_their_c():
    """3 x 3 x 3 cells of fcc copper at a0 = a = 3.61, rc = 5.2, as published: four shells, 54 neighbours.  U / N =
    eps (S_n / 2 - c sqrt(S_m)) of the truncated sums (-3.38955 eV); the forces vanish by symmetry; with c = n S_n / (m sqrt(S_m))
    of the truncated sums (40.2099) the uniformly scaled lattice is stationary."""
    k = _k("none")
    pos, cell = O.fcc_lattice(3, 3.61)
    lst = R.pairs(pos, cell, RC)
    assert lst["rows"].tolist() == [54] * 108
    eps, a, c = CU[:3]
    Sn, Sm, sites = R.fcc_sums(9, 6, a0=float(cell[0]) / 3, a=a, rc=RC)
    assert sites == 54
    x = torch.tensor(pos, requires_grad=True)
    U = R.energy(x, TH, lst, cell, k)
    want = eps * (0.5 * Sn - c * math.sqrt(Sm))
    assert abs(float(U.detach()) / 108 - want) <= 1e-12 * abs(want)
    assert abs(want + 3.38955) <= 1e-5, want
    (g,) = torch.autograd.grad(U, x)
    # 54 pair forces of up to 0.6 eV / A each cancel; coordinates are multiples of a0 / 2 rounded to 2^-53 * 10.83
    assert float(g.abs().max()) <= 1e-12, "the forces vanish"
    c0 = 9 * Sn / (6 * math.sqrt(Sm))
    assert abs(c0 - 40.2099) <= 2e-4, c0
    s = torch.ones((), dtype=torch.float64, requires_grad=True)
    th0 = torch.tensor([eps, a, c0], dtype=torch.float64)
    # r -> s r with the pair set fixed (rc is not scaled: as published there is no dependence on it inside the support)
    Us = R.energy(torch.tensor(pos) * s, th0, dict(lst, off=lst["off"] * s), cell, k)
    (dUds,) = torch.autograd.grad(Us, s)
    assert abs(float(dUds)) <= 1e-11 * 108 * eps * 0.5 * 9 * Sn, float(dUds)


@pytest.mark.parametrize("metal", sorted(R.PUBLISHED))
def test_published_constants_reproduce_their_c_from_the_full_lattice_sums(metal):
    """c = n S_n / (m sqrt(S_m)) (the lattice at a0 = a is stationary) with the sums over the whole fcc lattice: 40 a plus
    the integral tail.  -U / N = eps S_n (2 n - m) / (2 m) is the published cohesive energy."""
    eps, a, c, n, m = R.PUBLISHED[metal]
    Sn, Sm, _ = R.fcc_sums(n, m)
    assert abs(n * Sn / (m * math.sqrt(Sm)) - c) <= 1e-4 * c
    ecoh = eps * Sn * (2 * n - m) / (2 * m)
    assert abs(ecoh - dict(copper=3.500, nickel=4.440, silver=2.960, gold=3.780)[metal]) <= 2e-3, ecoh


@pytest.mark.parametrize("shift", ["force", "none"])
def test_scales_bound_the_values(shift):
    k = _k(shift)
    x32, cell32, lst = _cu108(seed=3)
    w = np.random.default_rng(3).normal(0, 1, x32.shape)
    ref = R.evaluate(x32, CU[:3], lst, cell32, k, w=w)
    for key in ("grad", "hw", "dth", "dthw"):
        assert bool((ref[key].abs() <= ref["A_" + key] * (1 + 1e-12)).all()), key
    assert float(ref["A_U"]) >= abs(float(ref["U"]))
    assert float(ref["kappa"].min()) >= 1.0 - 1e-12
    if shift == "none":
        assert float((ref["kappa"] - 1).abs().max()) <= 1e-12
    else:
        assert float(ref["rho"].min()) > 0.0 and float(ref["kappa"].max()) > 1.1


@pytest.mark.parametrize("shift", ["force", "none"])
def test_translation_invariance(shift):
    x32, cell32, lst = _cu108(seed=5)
    w = np.random.default_rng(5).normal(0, 1, x32.shape)
    ref = R.evaluate(x32, CU[:3], lst, cell32, _k(shift), w=w)
    assert float(ref["grad"].sum(0).abs().max()) <= 1e-13 * float(ref["A_grad"].sum(0).max())
    assert float(ref["hw"].sum(0).abs().max()) <= 1e-13 * float(ref["A_hw"].sum(0).max())


@pytest.mark.parametrize("shift", ["force", "none"])
def test_scaling_identities(shift):
    k = _k(shift)
    x32, cell32, lst = _cu108(seed=6)
    x, th = torch.tensor(x32).double(), TH.clone()
    U = float(R.energy(x, th, lst, cell32, k))
    U2 = float(R.energy(x, th * torch.tensor([2.5, 1.0, 1.0], dtype=torch.float64), lst, cell32, k))
    assert abs(U2 - 2.5 * U) <= 1e-13 * abs(U2), "U is linear in epsilon at fixed c"
    s = 1.37
    xs, cs = x * s, cell32.astype(np.float64) * s
    ks = _k(shift, rc=RC * s)
    lst_s = R.pairs(xs, cs, RC * s)
    assert lst_s["i"].numel() == lst["i"].numel()
    Us = float(R.energy(xs, th * torch.tensor([1.0, s, 1.0], dtype=torch.float64), lst_s, cs, ks))
    assert abs(Us - U) <= 1e-12 * abs(U), "U(s x, s a, s cell, s rc) = U"
    # a dU/da = sum_i (n/2 sum_j phi + m rho_i F'(rho_i)): S_k is homogeneous of degree k in a
    ref = R.evaluate(x32, CU[:3], lst, cell32, k)
    r, rho = R.density(x, th[1], lst, cell32, k)
    eps, a, c = CU[:3]
    hom = k["n"] * eps * float(R.shape(r, a, k["n"], k).sum()) + k["m"] * float((rho * (-eps * c / (2 * rho.sqrt()))).sum())
    assert abs(a * float(ref["dth"][1]) - hom) <= 1e-12 * float(ref["A_dth"][1]) * a


# ------------------------------------------------------------------------------------------------ the module on the host
@pytest.mark.parametrize("shift", ["force", "none"])
def test_torch_energy_equals_the_float64_reference(shift):
    from mdgrad_amd.interface import SuttonChen
    k = _k(shift)
    x32, cell32, lst = _cu108(seed=7)
    mod = SuttonChen.copper(_cpu_system(x32, cell32), cutoff=RC, shift=shift)
    assert [n for n, _ in mod.named_parameters()] == ["epsilon", "a", "c"] and not mod.supports_force_vjp()
    assert (mod.n, mod.m, mod.cutoff, mod.shift) == (9, 6, RC, shift)
    theta = [float(p.detach()) for p in (mod.epsilon, mod.a, mod.c)]                      # (float32 parameters)
    w = torch.tensor(np.random.default_rng(7).normal(0, 1, x32.shape))
    ref = R.evaluate(x32, theta, lst, cell32, k, w=w)
    x = torch.tensor(x32).double().requires_grad_(True)
    U = mod(x)
    assert U.dtype == torch.float64
    gx, ge, ga, gc = torch.autograd.grad(U, (x, mod.epsilon, mod.a, mod.c), create_graph=True)
    (hw,) = torch.autograd.grad((gx * w).sum(), x)
    assert abs(float(U.detach()) - float(ref["U"])) <= 1e-12 * float(ref["A_U"])
    assert float((gx.detach() - ref["grad"]).abs().max()) <= 1e-12 * float(ref["A_grad"].max())
    assert float((hw - ref["hw"]).abs().max()) <= 1e-12 * float(ref["A_hw"].max())
    got = torch.stack([ge.detach().reshape(()), ga.detach().reshape(()), gc.detach().reshape(())]).double()
    assert bool(((got - ref["dth"]).abs() <= 1e-6 * ref["A_dth"]).all())               # (float32 parameters)


def test_torch_energy_on_three_replicas_with_frozen_parameters():
    from mdgrad_amd.interface import SuttonChen
    x32, cell32, _ = _cu108(seed=7)
    rep = _cpu_system(x32, cell32).replicate(3)
    x3 = np.concatenate([x32, R.jittered_fcc(3, 3.61, 0.15, 8)[0], R.jittered_fcc(3, 3.61, 0.1, 9)[0]])
    for shift in ("force", "none"):
        au = SuttonChen.gold(rep, cutoff=RC, shift=shift, trainable=False)
        assert list(au.parameters()) == [] and set(dict(au.named_buffers())) >= {"epsilon", "a", "c"}
        th = [float(au.epsilon), float(au.a), float(au.c)]
        assert th == [float(np.float32(v)) for v in R.PUBLISHED["gold"][:3]] and (au.n, au.m) == (10, 8)
        lst3 = R.pairs(x3, cell32, RC, group=108)
        U3 = float(au(torch.tensor(x3).double()))
        want = float(R.energy(torch.tensor(x3).double(), torch.tensor(th, dtype=torch.float64), lst3, cell32, _k(shift, 10, 8)))
        assert abs(U3 - want) <= 1e-12 * abs(want)


def test_an_isolated_atom_has_no_embedding_energy_and_finite_derivatives():
    from mdgrad_amd.interface import SuttonChen
    pos = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 4.0], [9.0, 9.0, 9.0]])
    mod = SuttonChen.copper(_cpu_system(pos, [16.0, 16.0, 16.0]), cutoff=5.0)
    x = torch.tensor(pos, requires_grad=True)
    U = mod(x)
    g = torch.autograd.grad(U, (x, mod.epsilon, mod.a, mod.c), create_graph=True)
    w = torch.tensor([[0.3, -0.2, 0.5], [0.1, 0.4, -0.6], [1.0, 1.0, 1.0]], dtype=torch.float64)
    (hw,) = torch.autograd.grad((g[0] * w).sum(), x)
    assert all(bool(torch.isfinite(t).all()) for t in g + (hw,))
    gx = g[0].detach()
    assert float(gx[2].abs().max()) == 0.0 and float(hw[2].abs().max()) == 0.0 and float(gx[0].abs().max()) > 0.0


def test_published_class_methods_and_default_cutoff():
    from mdgrad_amd.interface import SuttonChen
    pos = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 4.0]])
    s = _cpu_system(pos, [20.0, 20.0, 20.0])
    for name, (eps, a, c, n, m) in R.PUBLISHED.items():
        mod = getattr(SuttonChen, name)(s)
        assert mod.cutoff == 2.0 * a and (mod.n, mod.m, mod.shift) == (n, m, "force")
        assert [float(p.detach()) for p in (mod.epsilon, mod.a, mod.c)] == [float(np.float32(v)) for v in (eps, a, c)]
        assert SuttonChen.PUBLISHED[name] == R.PUBLISHED[name]
    assert SuttonChen.silver(s, cutoff=6.0, shift="none").cutoff == 6.0


def test_argument_checks_raise_value_error():
    from mdgrad_amd.interface import SuttonChen
    x32, cell32 = R.jittered_fcc(3, 3.61, 0.0)
    s = _cpu_system(x32, cell32)
    for kw, word in ((dict(epsilon=0.0), "epsilon"), (dict(epsilon=-1.0), "epsilon"), (dict(a=0.0), "length a"),
                     (dict(a=-2.0), "length a"), (dict(c=-0.1), "c must be"), (dict(n=6, m=6), "exponents"),
                     (dict(n=17), "exponents"), (dict(m=0), "exponents"), (dict(n=9.5), "exponents"), (dict(m=5.5), "exponents"),
                     (dict(cutoff=0.0), "cutoff must be positive"), (dict(cutoff=-1.0), "cutoff must be positive"),
                     (dict(cutoff=5.5), "half the shortest cell height"), (dict(shift="energy"), "shift"),
                     (dict(index_tuple=([0], [1])), "index_tuple"), (dict(ex_pairs=[[0, 1]]), "ex_pairs")):
        args = dict(epsilon=CU[0], a=CU[1], c=CU[2], n=9, m=6, cutoff=RC)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            SuttonChen(s, **args)
    tric = _cpu_system(x32, np.array([[10.83, 0, 0], [0, 10.83, 0], [9.0, 0, 6.0]]))
    with pytest.raises(ValueError, match="half the shortest cell height"):
        SuttonChen.copper(tric, cutoff=RC)                            # the height along z is 6.0 < 2 rc
    with pytest.raises(ValueError, match="half the shortest cell height"):
        SuttonChen.copper(s)                                          # the default 2 a = 7.22 > 5.415
    assert SuttonChen(s, CU[0], CU[1], 0.0, 9, 6, RC).cutoff == RC, "c = 0 (a pair potential) is allowed"


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_entry_points_validate_their_arguments():
    from mdgrad_amd import _lib, ops
    lib = _lib.load()
    p = ctypes.c_void_p(64)                  # never dereferenced: every call below fails its checks first
    cell = _lib.make_cell([11.0, 11.0, 11.0])
    k = ops.eam_consts(*CU, cutoff=RC)

    def broken(**kw):
        b = ops.eam_consts(*CU, cutoff=RC)
        for name, v in kw.items():
            setattr(b, name, v)
        return ctypes.byref(b)

    def fails(rc, word):
        msg = lib.mdg_last_error()
        assert rc == -1 and word.encode() in msg, (rc, word, msg)

    ev, C, Kc = lib.mdg_eam_eval, ctypes.byref(cell), ctypes.byref(k)
    fails(ev(None, 8, C, p, p, p, 8, Kc, None, None, None, p, None, None, None, None, p, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, None, p, p, p, 8, Kc, None, None, None, p, None, None, None, None, p, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, C, p, None, p, 8, Kc, None, None, None, p, None, None, None, None, p, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, C, p, p, p, 8, None, None, None, None, p, None, None, None, None, p, 1.0, 0, None), "consts is null")
    fails(ev(p, 0, C, p, p, p, 8, Kc, None, None, None, p, None, None, None, None, p, 1.0, 0, None), "bad sizes")
    fails(ev(p, 8, C, p, p, p, 0, Kc, None, None, None, p, None, None, None, None, p, 1.0, 0, None), "bad sizes")
    fails(ev(p, 8, C, p, p, p, 8, broken(a=0.0), None, None, None, p, None, None, None, None, p, 1.0, 0, None), "a > 0")
    fails(ev(p, 8, C, p, p, p, 8, broken(epsilon=-1.0), None, None, None, p, None, None, None, None, p, 1.0, 0, None), "epsilon > 0")
    fails(ev(p, 8, C, p, p, p, 8, broken(c=-1.0), None, None, None, p, None, None, None, None, p, 1.0, 0, None), "c >= 0")
    fails(ev(p, 8, C, p, p, p, 8, broken(rc=0.0), None, None, None, p, None, None, None, None, p, 1.0, 0, None), "rc > 0")
    fails(ev(p, 8, C, p, p, p, 8, broken(n=17), None, None, None, p, None, None, None, None, p, 1.0, 0, None), "exponents")
    fails(ev(p, 8, C, p, p, p, 8, broken(m=9), None, None, None, p, None, None, None, None, p, 1.0, 0, None), "exponents")
    fails(ev(p, 8, C, p, p, p, 8, broken(m=0), None, None, None, p, None, None, None, None, p, 1.0, 0, None), "exponents")
    fails(ev(p, 8, C, p, p, p, 8, broken(shift=2), None, None, None, p, None, None, None, None, p, 1.0, 0, None), "shift must be")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, None, p, p, None, None, None, p, 1.0, 0, None), "need w")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, None, p, None, None, p, None, p, 1.0, 0, None), "need w")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, p, None, p, None, None, None, None, p, 1.0, 0, None), "without hw")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, None, None, None, None, None, None, p, 1.0, 0, None), "no output")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, p, None, None, None, None, None, p, 1.0, 0, None), "partial")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, None, p, None, None, None, None, None, 1.0, 0, None), "atom_work is null")
    assert lib.mdg_eam_partial_size(64) == 4 and lib.mdg_eam_partial_size(37) == 3 and lib.mdg_eam_partial_size(0) == 0
    assert ctypes.sizeof(_lib.MdgEAMConsts) == 48
    for bad in (dict(epsilon=0.0), dict(a=-1.0), dict(c=-1.0), dict(n=6, m=6), dict(n=17), dict(m=0), dict(cutoff=0.0),
                dict(shift="energy")):
        args = dict(epsilon=1.0, a=1.0, c=1.0, n=9, m=6, cutoff=2.0)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.eam_consts(**args)
