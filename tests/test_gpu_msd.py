"""MSD observable on the GPU (csrc/msd.hip, ops.MsdFn, observable.msd) against the float64 definition (tests/msd_ref.py:
torch float64 on the CPU from the same float32 positions).

Tolerances are derived, not measured.  Kernel and reference see identical float32 inputs; a float32 subtraction carries a
relative error of 2^-24; every forward term is non-negative, so a summation chain of depth n carries at most n 2^-24 relative
error.  The forward's chain is: the origins of one (atom, lag) in sequence (<= T = 64 here), the shuffle tree over the 16
atoms of a tile (4), the tiles and the normalisation in double (2), on top of ~4 roundings in |d|^2 (~8 in |d|^4):
  |M2 - M2_64| <= 2e-5 M2_64        |M4 - M4_64| <= 4e-5 M4_64                     (335 and 671 x 2^-24)
The backward sums 2 (L - 1) terms in sequence per element, each with ~5 roundings of its own (coefficient, subtraction,
|d|^2, two fused multiply-adds), the weight once; gabs is the same sum with every term replaced by its absolute value:
  |gx - gx_64| <= 1e-5 gabs + 1e-12 elementwise                                    ((2 L + 4) 2^-24 = 7.9e-6 at L = 64)
Every comparison prints its figure before it asserts.  The largest figures an MI355X showed over the cases below: M2 1.5e-7,
M4 2.5e-7, gx 1.8e-7 of gabs (rounding errors do not line up as the worst case assumes); the bounds stay the derived ones."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from msd_ref import msd64, random_walk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL2, TOL4, TOLG = 2e-5, 4e-5, 1e-5


def _const(name):
    """The kernels' tile constants, from the one place that defines them."""
    src = open(os.path.join(ROOT, "mdgrad_amd", "csrc", "msd.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


TILE, WINDOW = 1 << _const("MSD_TILE_SHIFT"), _const("MSD_WINDOW")


def figure(what, observed, allowed):
    print("FIGURE %-72s observed %.3e  allowed %.3e" % (what, observed, allowed))


def mk_system(n_atoms, n_rep=0):
    from mdgrad_amd.system import System
    pos = np.random.default_rng(0).uniform(0, 5.0, (n_atoms, 3))
    s = System(positions=pos, cell=np.array([5.0, 5.0, 5.0]), masses=np.full(n_atoms, 1.008), device=DEV)
    return s.replicate(n_rep) if n_rep else s


_walks = {}


def walk(T, N, k=1, R=1):
    """float32 [R, T, k N, 3]: an independent random walk per column, |x| ~ 50 (computed once per shape, never modified)."""
    key = (T, N, k, R)
    if key not in _walks:
        x = random_walk(T, R * k * N, seed=1000 * T + 10 * N + k + R).reshape(T, R, k * N, 3).transpose(1, 0, 2, 3)
        _walks[key] = np.ascontiguousarray(x)
    return _walks[key]


def run(obs, x, G2, G4):
    """(M2, M4, d(sum G2 M2 + sum G4 M4)/dx) through the kernels; M4 / G4 None without the fourth moment."""
    q = torch.as_tensor(np.asarray(x)).to(DEV).requires_grad_(True)
    m2, m4 = obs.moments_per_replica(q)
    loss = (m2 * torch.as_tensor(G2, dtype=torch.float32).to(DEV).reshape(m2.shape)).sum()
    if m4 is not None:
        loss = loss + (m4 * torch.as_tensor(G4, dtype=torch.float32).to(DEV).reshape(m4.shape)).sum()
    (g,) = torch.autograd.grad(loss, q)
    return m2.detach(), (m4.detach() if m4 is not None else None), g


def check_rows(what, x4, N, L, stride, w, fourth, m2, m4, g, G2, G4):
    """Every (batch, replica) row of the kernels' results against msd64 on that row's slice."""
    R, T, C = x4.shape[0], x4.shape[1], x4.shape[2]
    k = C // N
    m2 = m2.reshape(R * k, L).cpu().double().numpy()
    m4 = m4.reshape(R * k, L).cpu().double().numpy() if fourth else None
    g = g.reshape(R, T, C, 3).cpu().double().numpy()
    worst2 = worst4 = worstg = 0.0
    for r in range(R):
        for c in range(k):
            row = r * k + c
            xs = x4[r][:, c * N:(c + 1) * N]
            M2, M4, gx, gabs = msd64(xs, L, stride, w, G2[row], G4[row] if fourth else None)
            assert m2[row, 0] == 0.0 and np.isfinite(m2[row]).all()
            worst2 = max(worst2, float((np.abs(m2[row, 1:] - M2[1:]) / M2[1:]).max()) if L > 1 else 0.0)
            ok = (np.abs(m2[row] - M2) <= TOL2 * M2).all()
            if fourth:
                assert m4[row, 0] == 0.0 and np.isfinite(m4[row]).all()
                worst4 = max(worst4, float((np.abs(m4[row, 1:] - M4[1:]) / M4[1:]).max()) if L > 1 else 0.0)
                ok = ok and (np.abs(m4[row] - M4) <= TOL4 * M4).all()
            gs = g[r][:, c * N:(c + 1) * N]
            assert np.isfinite(gs).all()
            err = np.abs(gs - gx)
            worstg = max(worstg, float((err / (gabs + 1e-300)).max()))
            ok = ok and (err <= TOLG * gabs + 1e-12).all()
            if w is not None:
                assert (gs[:, np.asarray(w) == 0] == 0).all(), "%s: an atom of weight 0 has a gradient" % what
            if not ok:
                figure(what + " row %d: M2, M4, gx" % row, max(worst2 / TOL2, worst4 / TOL4, worstg / TOLG), 1.0)
            assert ok, "%s row %d: M2 %.3e (allowed %.1e), M4 %.3e (%.1e), gx %.3e of gabs (%.1e)" % (
                what, row, worst2, TOL2, worst4, TOL4, worstg, TOLG)
    figure(what + " |M2 - M2_64| / M2_64", worst2, TOL2)
    if fourth:
        figure(what + " |M4 - M4_64| / M4_64", worst4, TOL4)
    figure(what + " |gx - gx_64| / gabs", worstg, TOLG)


def weights_with_zeros(N, seed):
    w = np.random.default_rng(seed).uniform(0.25, 2.0, N).astype(np.float32)
    w[::3] = 0.0
    if N < 2:
        w[:] = 1.5
    return w


# (N, T, L, stride, k, R)
CASES = ([(N, 20, 20, 1, 1, 1) for N in (1, 63, 64, 65, 108, TILE + 1)] +
         [(TILE + 1, T, L, 1, 1, 1) for T in (1, 2, WINDOW - 1, WINDOW, WINDOW + 1, 64) for L in sorted({1, T})] +
         [(TILE + 1, 2 * WINDOW + 1, L, s, 1, 1) for s in (3, 2 * WINDOW + 2) for L in (1, 2 * WINDOW + 1)] +
         [(5, 20, 20, 1, 2, 1), (5, 20, 20, 3, 3, 1), (5, WINDOW + 1, 7, 1, 3, 2), (108, 64, 64, 3, 1, 2), (TILE, 64, 64, 1, 1, 2)])


@pytest.mark.parametrize("mode", ["plain", "weights+fourth"])
@pytest.mark.parametrize("N,T,L,stride,k,R", CASES)
def test_shape_boundaries_against_float64(N, T, L, stride, k, R, mode):
    from mdgrad_amd.observable import msd
    fourth = mode != "plain"
    w = weights_with_zeros(N, seed=N + T) if fourth else None
    obs = msd(mk_system(N, k if k > 1 else 0), L, weights=w, origin_stride=stride, fourth_moment=fourth)
    x4 = walk(T, N, k, R)
    x = x4 if R > 1 else x4[0]
    rng = np.random.default_rng(7 * N + T + L)
    G2, G4 = rng.uniform(-1, 1, (R * k, L)), rng.uniform(-1, 1, (R * k, L)) / 50.0
    m2, m4, g = run(obs, x, G2, G4)
    lead = ((R,) if R > 1 else ()) + ((k,) if k > 1 else ())
    assert m2.shape == lead + (L,) and g.shape == x.shape and (m4 is None) == (not fourth)
    check_rows("N %d T %d L %d s %d k %d R %d %s" % (N, T, L, stride, k, R, mode), x4, N, L, stride, w, fourth, m2, m4, g, G2, G4)


def test_leading_shapes_and_bitwise_repeatability():
    from mdgrad_amd.observable import msd
    N, T, L, k, R = 5, 20, 9, 3, 2
    x4 = torch.as_tensor(walk(T, N, k, R)).to(DEV)                      # [R, T, k N, 3]
    one = msd(mk_system(N), L, origin_stride=2, fourth_moment=True)
    stk = msd(mk_system(N, k), L, origin_stride=2, fourth_moment=True)
    full2, full4 = stk.moments_per_replica(x4)
    assert full2.shape == (R, k, L) and full4.shape == (R, k, L)
    assert stk.per_replica(x4[0]).shape == (k, L) and torch.equal(stk.per_replica(x4[0]), full2[0])
    for r in range(R):
        for c in range(k):
            xs = x4[r][:, c * N:(c + 1) * N]
            a2, a4 = one.moments_per_replica(xs)
            assert a2.shape == (L,) and torch.equal(a2, full2[r, c]) and torch.equal(a4, full4[r, c])
    xb = torch.stack([x4[0][:, :N], x4[1][:, N:2 * N]])                # [R, T, N, 3]
    b2 = one.per_replica(xb)
    assert b2.shape == (R, L) and torch.equal(b2[0], full2[0, 0]) and torch.equal(b2[1], full2[1, 1])
    assert torch.equal(stk(x4), full2.reshape(-1, L).mean(0)) and stk(x4).shape == (L,)
    m2, m4 = stk.moments(x4)
    assert torch.equal(m2, full2.reshape(-1, L).mean(0)) and torch.equal(m4, full4.reshape(-1, L).mean(0))
    a2 = stk.non_gaussian(x4)
    assert a2.shape == (L,) and float(a2[0]) == 0.0 and torch.isfinite(a2).all()
    assert torch.allclose(a2[1:], 3 * m4[1:] / (5 * m2[1:] ** 2) - 1)
    G2, G4 = np.random.default_rng(5).uniform(-1, 1, (R * k, L)), np.random.default_rng(6).uniform(-1, 1, (R * k, L))
    a, b = run(stk, x4.cpu().numpy(), G2, G4), run(stk, x4.cpu().numpy(), G2, G4)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_random_walk_is_gaussian_and_diffuses():
    """4 096 walkers x 64 frames, unit steps per component: |alpha_2| < 0.1 and D = 1/2 per unit time from the slope."""
    from mdgrad_amd.observable import diffusion_coefficient, msd
    obs = msd(mk_system(4096), 64, fourth_moment=True)
    q = torch.as_tensor(random_walk(64, 4096, seed=11)).to(DEV)
    a2 = obs.non_gaussian(q)
    D = float(diffusion_coefficient(obs(q), 1.0, fit_range=(1, 32)))
    figure("random walk: largest |alpha_2|", float(a2.abs().max()), 0.1)
    figure("random walk: |D - 1/2|", abs(D - 0.5), 0.02)
    assert float(a2.abs().max()) < 0.1 and abs(D - 0.5) < 0.02


def test_non_contiguous_input_and_the_leaf_gets_the_gradient():
    from mdgrad_amd.observable import msd
    N, T, L = TILE + 1, 2 * WINDOW + 2, 9
    x = walk(T, N)[0]
    obs = msd(mk_system(N), L)
    leaf = torch.as_tensor(x).to(DEV).requires_grad_(True)
    G2 = np.random.default_rng(8).uniform(-1, 1, (1, L))
    m2 = obs(leaf[::2])
    (m2 * torch.as_tensor(G2[0], dtype=torch.float32).to(DEV)).sum().backward()
    assert leaf.grad.shape == leaf.shape and (leaf.grad[1::2] == 0).all()
    check_rows("every second frame of a leaf", x[None, ::2], N, L, 1, None, False, m2.detach(), None, leaf.grad[::2], G2, None)
    assert torch.equal(m2.detach(), obs(torch.as_tensor(np.ascontiguousarray(x[::2])).to(DEV)))
    cols = torch.as_tensor(walk(T, N, 2)[0]).to(DEV)[:, N:]             # a slice in the atom dimension
    assert not cols.is_contiguous() and torch.equal(obs(cols), obs(cols.contiguous()))


# ---------------------------------------------------------------------------------------------- through a trajectory
def composite(q_t, n_atoms, L):
    """The per-lag torch composition: slice, subtract, square, mean."""
    return torch.stack([q_t.new_zeros(())] + [(q_t[tau:] - q_t[:-tau]).pow(2).sum(-1).mean() for tau in range(1, L)])


def traj_run(n_rep, use_kernels, L=10):
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NoseHooverChain, Simulations
    from mdgrad_amd.observable import msd
    from mdgrad_amd.system import System
    g = load_golden("pressure_p3")
    s = System(positions=np.asarray(g["pos"], dtype=np.float64), cell=np.asarray(g["cell"], dtype=np.float64),
               masses=np.asarray(g["mass"], dtype=np.float64), device=DEV)
    s.set_velocities(np.asarray(g["vel"], dtype=np.float64))
    system = s.replicate(n_rep) if n_rep else s
    mdl = P.LennardJones(1.0, 1.0)
    model = Stack({"pair": PairPotentials(system, mdl, cutoff=float(g["cutoff"]))})
    integ = NoseHooverChain(model, system, T=float(g["T"]), num_chains=int(g["chains"]), Q=float(g["Q"])).to(DEV)
    assert integ.fused_spec("NH_verlet") is not None
    n = int(g["n_steps"])
    v_t, q_t, pv_t = Simulations(system, integ).simulate(steps=n, frequency=n, dt=float(g["dt"]))
    m = msd(system, L)(q_t) if use_kernels else composite(q_t, 108, L)
    m[1:].sum().backward()
    return m.detach(), q_t.detach(), torch.stack([mdl.sigma.grad.reshape(()), mdl.epsilon.grad.reshape(())]).cpu().double()


@pytest.mark.parametrize("n_rep", [0, 2])
def test_through_the_fused_trajectory(n_rep):
    """108-atom LJ, 20 steps: msd(q_t)[1:].sum().backward() reaches the potential's parameters, and gives what the torch
    composite on the q_t of a fresh identical run gives (a check of the autograd wiring; the accuracy pins are above)."""
    m, q, grads = traj_run(n_rep, True)
    m_c, q_c, grads_c = traj_run(n_rep, False)
    figure("trajectory n_rep %d: largest |q_t - q_t of the second run|" % n_rep, float((q - q_c).abs().max()), float("nan"))
    assert torch.isfinite(grads).all() and (grads != 0).all()
    top = float(grads_c.abs().max())
    figure("trajectory n_rep %d: |dL/dtheta - composite| / largest" % n_rep, float((grads - grads_c).abs().max()) / top, 1e-4)
    figure("trajectory n_rep %d: |M2 - composite| / M2" % n_rep, float(((m - m_c).abs()[1:] / m_c[1:]).max()), 1e-5)
    assert ((grads - grads_c).abs() <= 1e-4 * top).all(), (grads, grads_c)
    assert torch.allclose(m, m_c, rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------------- torch ops and autograd
def test_torch_ops_equal_the_ctypes_path(tmp_path):
    """MsdFn goes through torch.ops.mdgrad.msd_fwd / msd_bwd when the op library is loaded and through ctypes when
    MDG_TORCH_OPS=0: the same kernels, the same bits.  The switch is read once per process, hence the child."""
    from mdgrad_amd import _torch_ops
    from mdgrad_amd.observable import msd
    ns = _torch_ops.get()
    assert ns is not None and hasattr(ns, "msd_fwd") and hasattr(ns, "msd_bwd")
    N, T, L, k, R = TILE + 1, WINDOW + 3, 11, 2, 2
    x, w = walk(T, N, k, R), weights_with_zeros(N, 3)
    G2, G4 = np.random.default_rng(1).uniform(-1, 1, (R * k, L)), np.random.default_rng(2).uniform(-1, 1, (R * k, L))
    np.savez(tmp_path / "in.npz", x=x, w=w, G2=G2, G4=G4)
    here = run(msd(mk_system(N, k), L, weights=w, origin_stride=2, fourth_moment=True), x, G2, G4)
    q = torch.as_tensor(x).to(DEV)
    wd, g2d, g4d = torch.as_tensor(w).to(DEV), torch.as_tensor(G2, dtype=torch.float32).to(DEV), torch.as_tensor(G4, dtype=torch.float32).to(DEV)
    m2, m4 = ns.msd_fwd(q, N, wd, L, 2, True)
    assert torch.equal(m2.reshape(here[0].shape), here[0]) and torch.equal(m4.reshape(here[1].shape), here[1])
    assert torch.equal(ns.msd_bwd(q, N, wd, L, 2, g2d, g4d), here[2])
    with pytest.raises(RuntimeError, match="multiple of group"):
        ns.msd_fwd(q, N + 1, None, L, 2, False)
    with pytest.raises(RuntimeError, match="n_lags"):
        ns.msd_fwd(q, N, None, T + 1, 1, False)
    script = tmp_path / "child.py"
    script.write_text(
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from mdgrad_amd import _torch_ops\n"
        "from mdgrad_amd.observable import msd\n"
        "from test_gpu_msd import mk_system, run\n"
        "assert _torch_ops.get() is None\n"
        "d = np.load(sys.argv[1])\n"
        "obs = msd(mk_system(%d, %d), %d, weights=d['w'], origin_stride=2, fourth_moment=True)\n"
        "m2, m4, g = run(obs, d['x'], d['G2'], d['G4'])\n"
        "np.savez(sys.argv[2], m2=m2.cpu().numpy(), m4=m4.cpu().numpy(), g=g.cpu().numpy())\n"
        % (os.path.join(ROOT, "tests"), ROOT, N, k, L))
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       env=dict(os.environ, MDG_TORCH_OPS="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    there = np.load(tmp_path / "out.npz")
    for name, t in zip(("m2", "m4", "g"), here):
        assert np.array_equal(there[name], t.cpu().numpy()), "%s differs between torch.ops and ctypes" % name


def test_second_backward_raises():
    from mdgrad_amd.observable import msd
    N, T = 5, 8
    q = torch.as_tensor(walk(T, N)[0]).to(DEV).requires_grad_(True)
    m = msd(mk_system(N), 4)(q)
    (g,) = torch.autograd.grad(m.sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
