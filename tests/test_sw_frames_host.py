"""thermo.StillingerWeberEnergy without a GPU: the host / float64 path (the model's torch restatement frame by frame) against the
float64 definition of tests/sw_ref.py, the shapes it accepts, its refusals, and the argument checks of the C entry points of
csrc/sw_frames.hip (K34).

Tolerance: float64 torch against the float64 reference, 1e-12 relative to the frame's energy (the parameters are float32 in
the module and are handed to the reference as the module holds them)."""
import ctypes

import numpy as np
import pytest
import torch

import sw_ref as R

K = R.consts()
N = 64


def _cpu_system(pos, cell):
    from mdgrad_amd.system import System
    return System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
                  masses=np.full(len(pos), 28.0855), device="cpu")


def _frames(n, first_seed=64):
    xs = [R.jittered_diamond(2, 5.431, 0.3, first_seed + s) for s in range(n)]
    return np.stack([x for x, _ in xs]), xs[0][1]


def _energy(system):
    from mdgrad_amd.interface import StillingerWeber
    from mdgrad_amd.thermo import StillingerWeberEnergy
    model = StillingerWeber.silicon(system)
    return model, StillingerWeberEnergy(system, model)


def _reference(model, frames, cell):
    th = torch.tensor([float(p.detach()) for p in (model.epsilon, model.sigma, model.lam)], dtype=torch.float64)
    out = []
    for x in frames:
        lst = R.pairs_and_triplets(x, cell, K["a"] * float(th[1]))
        out.append(float(R.energy(torch.tensor(x).double(), th, lst, cell, K)))
    return np.array(out)


def test_float64_host_frames_equal_the_reference_per_frame():
    frames, cell = _frames(3)
    model, energy = _energy(_cpu_system(frames[0], cell))
    want = _reference(model, frames, cell)
    q = torch.tensor(frames).double().requires_grad_(True)
    U = energy(q)
    assert U.shape == (3,) and U.dtype == torch.float64
    err = np.abs(U.detach().numpy() - want) / np.abs(want)
    print("StillingerWeberEnergy float64 host: largest relative error %.3e (allowed 1e-12)" % err.max())
    assert err.max() <= 1e-12
    assert len(set(np.round(want, 6))) == 3, "three different frames"
    # differentiable in the frames and the parameters; U[f] is what the model gives for the frame
    gq, gs = torch.autograd.grad(U.sum(), (q, model.sigma))
    assert gq.shape == q.shape and bool(torch.isfinite(gq).all()) and float(gq.abs().max()) > 0 and float(gs.abs()) > 0
    for f in range(3):
        assert float(model(q[f].detach()).detach()) == float(U[f].detach())
    assert model._n_rep == 1


def test_shapes():
    frames, cell = _frames(4, first_seed=70)
    system = _cpu_system(frames[0], cell)
    model, energy = _energy(system)
    q = torch.tensor(frames).double()
    U = energy(q)
    assert energy(q[2]).shape == () and float(energy(q[2])) == float(U[2])                      # [N, 3]
    assert U.shape == (4,)                                                                       # [T, N, 3]
    two = energy(q.reshape(2, 2, N, 3))                                                          # [R, T, N, 3]
    assert two.shape == (2, 2) and torch.equal(two.reshape(4), U)
    st = energy(torch.cat([q[:2], q[2:]], dim=1))                                                # [T, 2 N, 3]: q[t], q[t + 2]
    assert st.shape == (2, 2) and torch.equal(st[:, 0], U[:2]) and torch.equal(st[:, 1], U[2:])
    # a replicated system: the model sees k replicas, the observable one frame at a time
    from mdgrad_amd.interface import StillingerWeber
    from mdgrad_amd.thermo import StillingerWeberEnergy
    rep = _cpu_system(frames[0], cell).replicate(2)
    m2 = StillingerWeber.silicon(rep)
    e2 = StillingerWeberEnergy(rep, m2)
    st2 = e2(torch.cat([q[:2], q[2:]], dim=1))
    assert st2.shape == (2, 2) and torch.allclose(st2, st, rtol=1e-14, atol=0) and m2._n_rep == 2
    with pytest.raises(ValueError, match="k \\* 64"):
        energy(torch.zeros(3, 50, 3))
    # float32 host frames take the same path in float32
    assert energy(q.float()).dtype == torch.float32


def test_refusals():
    from mdgrad_amd.interface import PairPotentials, StillingerWeber, StillingerWeberMulti
    from mdgrad_amd.thermo import StillingerWeberEnergy
    frames, cell = _frames(1)
    system = _cpu_system(frames[0], cell)
    pair = PairPotentials.__new__(PairPotentials)                           # (the refusal looks at the type alone, and a
    multi = StillingerWeberMulti.__new__(StillingerWeberMulti)              #  PairPotentials cannot be built without a device)
    with pytest.raises(NotImplementedError, match="StillingerWeber \\(one species\\); got PairPotentials"):
        StillingerWeberEnergy(system, pair)
    with pytest.raises(NotImplementedError, match="StillingerWeberMulti"):
        StillingerWeberEnergy(system, multi)
    tric = _cpu_system(frames[0], np.array([[10.862, 0, 0], [1.0, 10.862, 0], [0, 0, 10.862]]))
    with pytest.raises(ValueError, match="diagonal"):
        StillingerWeberEnergy(tric, StillingerWeber.silicon(tric))
    big = _cpu_system(np.random.default_rng(0).uniform(0, 30.0, (1025, 3)), np.full(3, 30.0))
    with pytest.raises(ValueError, match="1024 atoms"):
        StillingerWeberEnergy(big, StillingerWeber.silicon(big))
    # a sigma beyond half the box: at construction, and after sigma has moved
    model, energy = _energy(system)
    with torch.no_grad():
        model.sigma.mul_(1.5)                                               # a sigma = 5.66 > 5.431
    with pytest.raises(ValueError, match="half the shortest cell"):
        energy(torch.tensor(frames).double())
    with pytest.raises(ValueError, match="half the shortest cell"):
        StillingerWeberEnergy(system, model)


def test_sigma_is_read_only_when_it_moved():
    frames, cell = _frames(1)
    model, energy = _energy(_cpu_system(frames[0], cell))
    key = energy._sig_key
    energy(torch.tensor(frames).double())
    assert energy._sig_key == key
    with torch.no_grad():
        model.sigma.mul_(1.03)
    energy(torch.tensor(frames).double())
    assert energy._sig_key != key


def test_c_entry_points_validate_their_arguments():
    from mdgrad_amd import _lib, ops
    lib = _lib.load()
    p = ctypes.c_void_p(64)                  # never dereferenced: every call below fails its checks first
    cell, tric = _lib.make_cell([11.0, 11.0, 11.0]), _lib.make_cell([[11.0, 0, 0], [1.0, 11.0, 0], [0, 0, 11.0]])
    k = ops.sw_consts(2.1683, 2.0951)

    def broken(**kw):
        b = ops.sw_consts(2.1683, 2.0951)
        for name, v in kw.items():
            setattr(b, name, v)
        return ctypes.byref(b)

    def fails(rc, word):
        msg = lib.mdg_last_error()
        assert rc == -1 and word.encode() in msg, (rc, word, msg)

    fw, C, Kc = lib.mdg_sw_frames_fwd, ctypes.byref(cell), ctypes.byref(k)
    fails(fw(None, 2, 8, C, Kc, p, p, None, None), "null argument")
    fails(fw(p, 2, 8, None, Kc, p, p, None, None), "null argument")
    fails(fw(p, 2, 8, C, None, p, p, None, None), "null argument")
    fails(fw(p, 2, 8, C, Kc, None, p, None, None), "theta is null")
    fails(fw(p, 2, 8, C, Kc, p, None, None, None), "null output")
    fails(fw(p, 0, 8, C, Kc, p, p, None, None), "empty")
    fails(fw(p, 2, 0, C, Kc, p, p, None, None), "empty")
    fails(fw(p, 2, 1025, C, Kc, p, p, None, None), "at most 1024 atoms")
    fails(fw(p, 2, 8, ctypes.byref(tric), Kc, p, p, None, None), "diagonal")
    fails(fw(p, 2, 8, C, broken(a=0.0), p, p, None, None), "a > 0")
    fails(fw(p, 2, 8, C, broken(gamma=-1.0), p, p, None, None), "gamma >= 0")
    fails(fw(p, 2, 8, C, broken(p=13), p, p, None, None), "exponents")
    fails(fw(p, 2, 8, C, broken(q=4), p, p, None, None), "exponents")
    bw = lib.mdg_sw_frames_theta_bwd
    fails(bw(None, p, 2, p, None), "null argument")
    fails(bw(p, None, 2, p, None), "null argument")
    fails(bw(p, p, 2, None, None), "null argument")
    fails(bw(p, p, 0, p, None), "empty")
    assert ops.sw_frames_row_cap() == 64 and ops.SW_FRAMES_MAX_ATOMS == 1024
