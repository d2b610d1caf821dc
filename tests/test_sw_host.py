"""Stillinger-Weber term, host side: tests/sw_ref.py -- the float64 definition the GPU tests compare the kernel with -- against
an independent loop, the diamond-lattice ground state and its own invariances; StillingerWeber's torch restatement against
it; the argument checks, the cutoff rule of a trainable sigma and the validation of the C entry points."""
import ctypes

import numpy as np
import pytest
import torch

import oracle as O
import sw_ref as R

K = R.consts()
SI = [R.SILICON["epsilon"], R.SILICON["sigma"], R.SILICON["lam"]]
TH = torch.tensor(SI, dtype=torch.float64)


def _cpu_system(pos, cell):
    from mdgrad_amd.system import System
    return System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
                  masses=np.full(len(pos), 28.0855), device="cpu")


def _si64(seed=64, jit=0.3):
    x32, cell32 = R.jittered_diamond(2, 5.431, jit, seed)
    return x32, cell32, R.pairs_and_triplets(x32, cell32, K["a"] * SI[1])


# ------------------------------------------------------------------------------------------------ the definition
def test_energy_equals_an_independent_triple_loop():
    x32, cell32, lst = _si64()
    assert lst["tc"].numel() > 2000 and int(lst["rows"].min()) >= 4 and int(lst["rows"].max()) >= 12
    u2, u3 = R.energy(torch.tensor(x32).double(), TH, lst, cell32, K, parts=True)
    l2, l3 = R.energy_loops(x32, SI, cell32, K)
    assert abs(float(u2) - l2) <= 1e-12 * abs(l2) and abs(float(u3) - l3) <= 1e-12 * abs(l3), (float(u2), l2, float(u3), l3)
    assert l3 > 0.0 and l2 < 0.0
    # the same on three replicas that must not see each other
    x3 = np.concatenate([x32, R.jittered_diamond(2, 5.431, 0.3, 65)[0], R.jittered_diamond(2, 5.431, 0.2, 66)[0]])
    lst3 = R.pairs_and_triplets(x3, cell32, K["a"] * SI[1], group=64)
    u = float(R.energy(torch.tensor(x3).double(), TH, lst3, cell32, K))
    l = sum(R.energy_loops(x3, SI, cell32, K, group=64))
    assert abs(u - l) <= 1e-12 * abs(l)


def test_perfect_diamond_silicon_is_the_ground_state():
    """2 x 2 x 2 cells of diamond at a0 = 5.431: four neighbours per atom at the tetrahedral angle, so the three-body part
    vanishes and the pair part sits in its minimum, -epsilon per bond: U / N = -2 epsilon (float64 gives -1.9999999977)."""
    pos, cell = O.diamond_lattice(2, 5.431)
    lst = R.pairs_and_triplets(pos, cell, K["a"] * SI[1])
    assert lst["rows"].tolist() == [4] * 64 and lst["tc"].numel() == 64 * 6
    x = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
    u2, u3 = R.energy(x, TH, lst, cell, K, parts=True)
    eps = SI[0]
    assert abs(float((u2 + u3).detach()) / 64 + 2 * eps) <= 1e-8 * 2 * eps, float((u2 + u3).detach()) / 64 / eps
    assert abs(float(u3.detach())) <= 1e-12 * eps
    (g,) = torch.autograd.grad(u2 + u3, x)
    # the four bond forces of an atom cancel by symmetry, up to the rounding of the coordinates (2^-53 * 10.9 A) times the
    # bond stiffness (about 30 epsilon / sigma^2): 1e-12 epsilon / sigma leaves two orders of magnitude
    assert float(g.abs().max()) <= 1e-12 * eps / SI[1], "the forces vanish"


def test_sum_of_the_per_term_contributions_equals_autograd_and_bounds_it():
    x32, cell32, lst = _si64(seed=3)
    w = np.random.default_rng(3).normal(0, 1, x32.shape)
    ref = R.evaluate(x32, SI, lst, cell32, K, w=w)
    for key in ("grad", "hw", "dth", "dthw"):
        assert bool((ref[key].abs() <= ref["A_" + key] * (1 + 1e-12)).all()), key
    assert float(ref["A_U"]) >= abs(float(ref["U"]))
    assert float(ref["A_dth"][0]) >= float(ref["A_U"]) / SI[0] * (1 - 1e-12), "U is linear in epsilon"


def test_translation_invariance():
    x32, cell32, lst = _si64(seed=5)
    w = np.random.default_rng(5).normal(0, 1, x32.shape)
    ref = R.evaluate(x32, SI, lst, cell32, K, w=w)
    assert float(ref["grad"].sum(0).abs().max()) <= 1e-13 * float(ref["A_grad"].sum(0).max())
    assert float(ref["hw"].sum(0).abs().max()) <= 1e-13 * float(ref["A_hw"].sum(0).max())


def test_scaling_identities():
    x32, cell32, lst = _si64(seed=6)
    x, th = torch.tensor(x32).double(), TH.clone()
    U = float(R.energy(x, th, lst, cell32, K))
    U2 = float(R.energy(x, th * torch.tensor([2.5, 1.0, 1.0], dtype=torch.float64), lst, cell32, K))
    assert abs(U2 - 2.5 * U) <= 1e-13 * abs(U2), "U is linear in epsilon"
    s = 1.37
    xs, cs = x * s, cell32.astype(np.float64) * s
    lst_s = R.pairs_and_triplets(xs, cs, K["a"] * SI[1] * s)
    assert lst_s["tc"].numel() == lst["tc"].numel()
    Us = float(R.energy(xs, th * torch.tensor([1.0, s, 1.0], dtype=torch.float64), lst_s, cs, K))
    assert abs(Us - U) <= 1e-12 * abs(U), "U(x, sigma) = U(s x, s sigma) with the cell scaled"


# ------------------------------------------------------------------------------------------------ the module on the host
def test_torch_energy_equals_the_float64_reference():
    from mdgrad_amd.interface import StillingerWeber
    x32, cell32, lst = _si64(seed=7)
    mod = StillingerWeber.silicon(_cpu_system(x32, cell32))
    assert [n for n, _ in mod.named_parameters()] == ["epsilon", "sigma", "lam"] and not mod.supports_force_vjp()
    theta = [float(p.detach()) for p in (mod.epsilon, mod.sigma, mod.lam)]                 # (float32 parameters)
    lst = R.pairs_and_triplets(x32, cell32, K["a"] * theta[1])
    w = torch.tensor(np.random.default_rng(7).normal(0, 1, x32.shape))
    ref = R.evaluate(x32, theta, lst, cell32, K, w=w)
    x = torch.tensor(x32).double().requires_grad_(True)
    U = mod(x)
    assert U.dtype == torch.float64
    gx, ge, gs, gl = torch.autograd.grad(U, (x, mod.epsilon, mod.sigma, mod.lam), create_graph=True)
    (hw,) = torch.autograd.grad((gx * w).sum(), x)
    assert abs(float(U.detach()) - float(ref["U"])) <= 1e-12 * float(ref["A_U"])
    assert float((gx.detach() - ref["grad"]).abs().max()) <= 1e-12 * float(ref["A_grad"].max())
    assert float((hw - ref["hw"]).abs().max()) <= 1e-12 * float(ref["A_hw"].max())
    got = torch.stack([ge.detach().reshape(()), gs.detach().reshape(()), gl.detach().reshape(())]).double()
    assert bool(((got - ref["dth"]).abs() <= 1e-6 * ref["A_dth"]).all())              # (float32 parameters)
    # three replicas, frozen parameters, the mW constants
    rep = _cpu_system(x32, cell32).replicate(3)
    x3 = np.concatenate([x32, R.jittered_diamond(2, 5.431, 0.3, 8)[0], R.jittered_diamond(2, 5.431, 0.2, 9)[0]])
    mw = StillingerWeber.mW(rep, trainable=False)
    assert list(mw.parameters()) == [] and set(dict(mw.named_buffers())) >= {"epsilon", "sigma", "lam"}
    th = [float(mw.epsilon), float(mw.sigma), float(mw.lam)]
    assert abs(th[0] - R.MW["epsilon"]) <= 1e-7 * th[0] and abs(th[0] - 0.26838) <= 1e-5 and th[2] == np.float32(23.15)
    lst3 = R.pairs_and_triplets(x3, cell32, K["a"] * th[1], group=64)
    U3 = float(mw(torch.tensor(x3).double()))
    want = float(R.energy(torch.tensor(x3).double(), torch.tensor(th, dtype=torch.float64), lst3, cell32, K))
    assert abs(U3 - want) <= 1e-12 * abs(want)


def test_argument_checks_raise_value_error():
    from mdgrad_amd.interface import StillingerWeber
    pos, cell = O.diamond_lattice(2, 5.431)
    s = _cpu_system(pos, cell)
    for kw, word in ((dict(epsilon=0.0), "epsilon"), (dict(epsilon=-1.0), "epsilon"), (dict(sigma=0.0), "sigma"),
                     (dict(sigma=-2.0), "sigma"), (dict(lam=-0.1), "lam"), (dict(p=4, q=4), "exponents"),
                     (dict(p=13), "exponents"), (dict(q=-1), "exponents"), (dict(p=4.5), "exponents"),
                     (dict(sigma=3.1), "half the shortest cell height"), (dict(index_tuple=([0], [1])), "index_tuple"),
                     (dict(ex_pairs=[[0, 1]]), "ex_pairs")):
        args = dict(epsilon=2.1683, sigma=2.0951)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            StillingerWeber(s, **args)
    tric = _cpu_system(pos, np.array([[10.862, 0, 0], [0, 10.862, 0], [9.0, 0, 6.0]]))
    with pytest.raises(ValueError, match="half the shortest cell height"):
        StillingerWeber(tric, 2.1683, 2.0951)                         # the height along z is 6.0 < 2 a sigma
    assert StillingerWeber(s, 2.1683, 2.0951, lam=0.0).cutoff > 0.0


def test_cutoff_rule_keeps_grows_and_shrinks_the_list_cutoff():
    """a sigma <= cutoff <= 1.05 a sigma: kept, with static_version() unchanged; otherwise reset to 1.02 a sigma with a new
    static_version().  sigma is read only when its version counter moved."""
    from mdgrad_amd.interface import StillingerWeber
    pos, cell = O.diamond_lattice(2, 5.431)
    mod = StillingerWeber(_cpu_system(pos, cell), 2.1683, 2.0, a=1.8)
    assert (mod.cutoff_reset, mod.cutoff_keep) == (1.02, 1.05)
    rc0 = 1.8 * 2.0
    assert abs(mod.cutoff - 1.02 * rc0) <= 1e-6
    v0, c0 = mod.static_version(), mod.cutoff
    assert mod._sync_cutoff() is False and mod.static_version() == v0, "nothing moved"
    with torch.no_grad():
        mod.sigma.mul_(1.01)                                  # a sigma = 3.636 <= 3.672: the list is still sufficient
    mod.prepare_pass()
    assert mod.cutoff == c0 and mod.static_version() == v0
    with torch.no_grad():
        mod.sigma.mul_(1.02)                                  # a sigma = 3.709 > 3.672: grow
    mod.prepare_pass()
    v1 = mod.static_version()
    assert abs(mod.cutoff - 1.02 * rc0 * 1.01 * 1.02) <= 1e-5 and v1 != v0
    with torch.no_grad():
        mod.sigma.mul_(0.98)                                  # cutoff / (a sigma) = 1.0408 <= 1.05: kept
    mod.prepare_pass()
    assert mod.static_version() == v1
    with torch.no_grad():
        mod.sigma.mul_(0.97)                                  # cutoff / (a sigma) = 1.073 > 1.05: shrink
    mod.prepare_pass()
    v2 = mod.static_version()
    assert abs(mod.cutoff - 1.02 * 1.8 * float(mod.sigma.detach())) <= 1e-5 and v2 not in (v0, v1)
    mod.prepare_pass()
    assert mod.static_version() == v2
    with torch.no_grad():
        mod.epsilon.mul_(2.0), mod.lam.mul_(0.5)              # the other parameters do not touch the list
    mod.prepare_pass()
    assert mod.static_version() == v2
    with torch.no_grad():
        mod.sigma.mul_(-1.0)
    with pytest.raises(ValueError, match="sigma"):
        mod.prepare_pass()


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_entry_points_validate_their_arguments():
    from mdgrad_amd import _lib, ops
    lib = _lib.load()
    p = ctypes.c_void_p(64)                  # never dereferenced: every call below fails its checks first
    cell = _lib.make_cell([11.0, 11.0, 11.0])
    k = ops.sw_consts(2.1683, 2.0951)

    def broken(**kw):
        b = ops.sw_consts(2.1683, 2.0951)
        for name, v in kw.items():
            setattr(b, name, v)
        return ctypes.byref(b)

    def fails(rc, word):
        msg = lib.mdg_last_error()
        assert rc == -1 and word.encode() in msg, (rc, word, msg)

    ev, C, Kc = lib.mdg_sw_eval, ctypes.byref(cell), ctypes.byref(k)
    fails(ev(None, 8, C, p, p, p, 8, Kc, None, None, None, p, None, None, None, None, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, None, p, p, p, 8, Kc, None, None, None, p, None, None, None, None, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, C, p, None, p, 8, Kc, None, None, None, p, None, None, None, None, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, C, p, p, p, 8, None, None, None, None, p, None, None, None, None, 1.0, 0, None), "consts is null")
    fails(ev(p, 0, C, p, p, p, 8, Kc, None, None, None, p, None, None, None, None, 1.0, 0, None), "bad sizes")
    fails(ev(p, 8, C, p, p, p, 0, Kc, None, None, None, p, None, None, None, None, 1.0, 0, None), "bad sizes")
    fails(ev(p, 8, C, p, p, p, 8, broken(sigma=0.0), None, None, None, p, None, None, None, None, 1.0, 0, None), "sigma > 0")
    fails(ev(p, 8, C, p, p, p, 8, broken(epsilon=-1.0), None, None, None, p, None, None, None, None, 1.0, 0, None), "epsilon > 0")
    fails(ev(p, 8, C, p, p, p, 8, broken(lam=-1.0), None, None, None, p, None, None, None, None, 1.0, 0, None), "lam >= 0")
    fails(ev(p, 8, C, p, p, p, 8, broken(a=0.0), None, None, None, p, None, None, None, None, 1.0, 0, None), "a > 0")
    fails(ev(p, 8, C, p, p, p, 8, broken(p=13), None, None, None, p, None, None, None, None, 1.0, 0, None), "exponents")
    fails(ev(p, 8, C, p, p, p, 8, broken(q=4), None, None, None, p, None, None, None, None, 1.0, 0, None), "exponents")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, None, p, p, None, None, None, 1.0, 0, None), "need w")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, None, p, None, None, p, None, 1.0, 0, None), "need w")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, p, None, p, None, None, None, None, 1.0, 0, None), "without hw")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, None, None, None, None, None, None, 1.0, 0, None), "no output")
    fails(ev(p, 8, C, p, p, p, 8, Kc, None, None, p, None, None, None, None, None, 1.0, 0, None), "partial")
    assert lib.mdg_sw_partial_size(64) == 4 and lib.mdg_sw_partial_size(37) == 3 and lib.mdg_sw_partial_size(0) == 0
    assert ctypes.sizeof(_lib.MdgSWConsts) == 72
    for bad in (dict(epsilon=0.0), dict(sigma=-1.0), dict(lam=-1.0), dict(p=3, q=3), dict(p=14), dict(a=0.0)):
        args = dict(epsilon=1.0, sigma=1.0)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.sw_consts(**args)
