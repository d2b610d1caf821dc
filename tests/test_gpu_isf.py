"""Intermediate scattering functions on the GPU (csrc/isf.hip, ops.IsfFn, observable.intermediate_scattering) against the
float64 definition (tests/isf_ref.py: torch float64 on the CPU from the same float32 positions and cell lengths).

Tolerances are derived, not measured; kernel and reference see identical float32 inputs.
  Coherent forward: the measure of tests/test_gpu_sk.py with the static envelope, |F - F64| <= TOL (sqrt(N_eff F64[b, 0]) + 1),
    TOL = 10 x 8.1e-8: the phase code is K16's, a product of two rho carries the same 2 |rho| N eps bound as |rho|^2, and the
    origin sums run in double.
  Coherent gradient: the rule of test_gpu_sk.grad_close, |g - g64| <= 10 x 4.8e-7 max|g64| + 1e-4 |g64|.
  Self forward, absolute: |F_s - F_s64| <= 5e-7 + D 2^-24.  5e-7: two positions at ~3e-8 turns each times 2 pi, plus the 1-ulp
    polynomials.  D, the float32 chain of one value: the origins of one (pair, lag) in sequence (|O_tau| <= T additions of
    terms of size <= 1, normalised by |O_tau|, so T), two roundings per product z conj z' (2), w^2 and its product (2), the
    shuffle tree over the 16 atoms of a tile (4); tiles, vectors and the normalisation are in double: D = T + 8.
  Self gradient: |gs - gs64| <= (5e-7 + Dg 2^-24) gabs + 1e-12 elementwise, gabs of tests/isf_ref.py.  Dg: 2 (L - 1) lags in
    sequence, the 8 vectors of a chunk, ceil(M / 8) chunks, and 8 roundings of a term (coefficient, two fused multiply-adds
    twice, the final product, w^2, 2 pi / L): Dg = 2 (L - 1) + ceil(M / 8) + 16.
Neither bound is let above 1e-5, the cap tests/test_gpu_sk.py sets itself: at the lag limit (L = 75, Dg = 167) the derived
1.05e-5 is cut to it.  Every comparison prints its figure before it asserts.  The largest figures an MI355X showed over
test_shape_boundaries_against_float64 and test_atom_blocks_beyond_1024 (the FIGURE lines of `pytest -s`), as fractions of the
allowed error: coherent forward 0.035, coherent gradient 0.042, self forward 0.115, self gradient 0.091.  Rounding errors do
not line up as the worst case assumes; the bounds stay the derived ones."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from isf_ref import isf64, random_walk
from sk_ref import n_eff
from test_isf_host import WALK, walk_expected

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, A_TOL, R_TOL = 10 * 8.1e-8, 10 * 4.8e-7, 1e-4
CELL = 5.0


def _const(name):
    """The kernels' tile constants, from the one place that defines them."""
    src = open(os.path.join(ROOT, "mdgrad_amd", "csrc", "isf.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


TILE, WINDOW, BWD_VECS = 1 << _const("ISF_TILE_SHIFT"), _const("ISF_WINDOW"), _const("ISF_BWD_VECS")
CONF = (5, (1.0, 6.0), 4)                    # nbins, k_range, max_per_bin: 20 vectors


def figure(what, observed, allowed):
    print("FIGURE %-72s observed %.3e  allowed %.3e" % (what, observed, allowed))


def mk_system(n_atoms, n_rep=0):
    from mdgrad_amd.system import System
    pos = np.random.default_rng(0).uniform(0, CELL, (n_atoms, 3))
    s = System(positions=pos, cell=np.array([CELL] * 3), masses=np.full(n_atoms, 1.008), device=DEV)
    return s.replicate(n_rep) if n_rep else s


def mk_obs(N, L, kind, conf=CONF, k=1, weights=None, stride=1):
    from mdgrad_amd.observable import intermediate_scattering
    return intermediate_scattering(mk_system(N, k if k > 1 else 0), conf[0], conf[1], L, kind=kind, weights=weights,
                                   max_per_bin=conf[2], origin_stride=stride)


_walks = {}


def walk(T, N, k=1, R=1):
    """float32 [R, T, k N, 3]: an independent random walk per column, steps of 0.3, |x| up to ~50 = ten cells (computed once
    per shape, never modified)."""
    key = (T, N, k, R)
    if key not in _walks:
        x = random_walk(T, R * k * N, seed=1000 * T + 10 * N + k + R, step=0.3).reshape(T, R, k * N, 3).transpose(1, 0, 2, 3)
        _walks[key] = np.ascontiguousarray(x)
    return _walks[key]


def run(obs, x, G):
    """(F, d sum(G F) / dx) through the kernels."""
    q = torch.as_tensor(np.asarray(x)).to(DEV).requires_grad_(True)
    F = obs.per_replica(q)
    (g,) = torch.autograd.grad((F * torch.as_tensor(G, dtype=torch.float32).to(DEV).reshape(F.shape)).sum(), q)
    return F.detach(), g


def check_rows(what, obs, x4, N, w, F, g, G):
    """Every (batch, replica) row of the kernels' results against isf64 on that row's slice."""
    R, T, C = x4.shape[0], x4.shape[1], x4.shape[2]
    k, B, L, M = C // N, obs.nbins, obs.t_range, len(obs.kvecs)
    coh = obs.kind == "coherent"
    F = F.reshape(R * k, B, L).cpu().double().numpy()
    g = g.reshape(R, T, C, 3).cpu().double().numpy()
    G = np.asarray(G).reshape(R * k, B, L)
    neff = n_eff(w, N)
    tol_s = min(5e-7 + (T + 8) * 2.0 ** -24, 1e-5)
    tol_gs = min(5e-7 + (2 * (L - 1) + -(-M // BWD_VECS) + 16) * 2.0 ** -24, 1e-5)
    worst_f = worst_g = 0.0
    for r in range(R):
        for c in range(k):
            row = r * k + c
            ref = isf64(x4[r][:, c * N:(c + 1) * N], [CELL] * 3, obs.kvecs.numpy(), obs._seg_host, L, obs.origin_stride, w, G[row],
                        coherent=coh, self_part=not coh)
            gs = g[r][:, c * N:(c + 1) * N]
            assert np.isfinite(F[row]).all() and np.isfinite(gs).all()
            assert (F[row][obs.n_vectors.numpy() == 0] == 0).all(), "%s: an empty bin is not 0" % what
            if coh:
                ef = np.abs(F[row] - ref["F"]) / (TOL * (np.sqrt(neff * np.abs(ref["F"][:, :1])) + 1.0))
                eg = np.abs(gs - ref["g"]) / (A_TOL * np.abs(ref["g"]).max() + R_TOL * np.abs(ref["g"]) + 1e-300)
            else:
                ef = np.abs(F[row] - ref["Fs"]) / tol_s
                eg = np.abs(gs - ref["gs"]) / (tol_gs * ref["gabs"] + 1e-12)
            if w is not None:
                assert (gs[:, np.asarray(w) == 0] == 0).all(), "%s: an atom of weight 0 has a gradient" % what
            worst_f, worst_g = max(worst_f, float(ef.max())), max(worst_g, float(eg.max()))
    figure(what + " forward error / allowed", worst_f, 1.0)
    figure(what + " gradient error / allowed", worst_g, 1.0)
    assert worst_f <= 1.0 and worst_g <= 1.0, "%s: forward %.3e, gradient %.3e of the allowed error" % (what, worst_f, worst_g)


def weights_with_zeros(N, seed):
    w = np.random.default_rng(seed).uniform(0.25, 2.0, N).astype(np.float32)
    w[::3] = 0.0
    if N < 2:
        w[:] = 1.5
    return w


def vec_conf(M):
    """One bin holding the first M vectors of the cell (M = 1: the shell |n| = 1 alone)."""
    return (1, (1.0, 1.5), 1) if M == 1 else (1, (1.0, 14.0), M)


EMPTY = (8, (1.0, 2.0), None)               # |k| = 1.26 and 1.78 only: six empty bins
# (N, T, L, stride, k, R, conf)
CASES = ([(N, 12, 12, 1, 1, 1, CONF) for N in (1, TILE - 1, TILE, TILE + 1, 63, 64, 65, 128, 129)] +
         [(TILE + 1, T, L, 1, 1, 1, CONF) for T in (1, 2, WINDOW - 1, WINDOW, WINDOW + 1, 40) for L in sorted({1, T})] +
         [(TILE + 1, 2 * WINDOW + 1, L, s, 1, 1, CONF) for s in (3, 2 * WINDOW + 2) for L in (1, 2 * WINDOW + 1)] +
         [(TILE + 1, WINDOW + 1, WINDOW + 1, 1, 1, 1, vec_conf(M)) for M in (1, 63, 64, 65, 257)] +
         [(TILE + 1, WINDOW + 1, 5, 2, 1, 1, EMPTY)] +
         [(TILE + 1, 36, L, 1, 1, 1, CONF) for L in (15, 16, 35, 36)] +       # the pair tile shrinks: 256 -> 128 -> 64
         [(5, 75, 75, 1, 1, 1, CONF), (TILE + 1, 70, 20, 3, 1, 1, CONF)] +    # the lag limit; two frame windows of the self backward
         [(5, 12, 12, 1, 2, 1, CONF), (5, 12, 12, 3, 3, 1, CONF), (5, WINDOW + 1, 7, 1, 3, 2, CONF), (TILE + 1, 12, 12, 1, 1, 2, CONF)])


def one_case(N, T, L, stride, k, R, conf, kind, weighted):
    w = weights_with_zeros(N, seed=N + T) if weighted else None
    obs = mk_obs(N, L, kind, conf, k, w, stride)
    if conf[2] is not None and conf[0] == 1 and conf[2] > 1:
        assert len(obs.kvecs) == conf[2]
    x4 = walk(T, N, k, R)
    x = x4 if R > 1 else x4[0]
    G = np.random.default_rng(7 * N + T + L).uniform(-1, 1, (R * k, obs.nbins, L))
    F, g = run(obs, x, G)
    lead = ((R,) if R > 1 else ()) + ((k,) if k > 1 else ())
    assert F.shape == lead + (obs.nbins, L) and g.shape == x.shape
    check_rows("%s N %d T %d L %d s %d k %d R %d M %d %s" % (kind, N, T, L, stride, k, R, len(obs.kvecs), "w" if weighted else "-"),
               obs, x4, N, w, F, g, G)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights"])
@pytest.mark.parametrize("kind", ["coherent", "self"])
@pytest.mark.parametrize("N,T,L,stride,k,R,conf", CASES)
def test_shape_boundaries_against_float64(N, T, L, stride, k, R, conf, kind, weighted):
    one_case(N, T, L, stride, k, R, conf, kind, weighted)


@pytest.mark.parametrize("kind", ["coherent", "self"])
def test_atom_blocks_beyond_1024(kind):
    one_case(1025, 3, 3, 1, 1, 1, CONF, kind, True)


# ---------------------------------------------------------------------------------------------- consistency on the device
def test_consistency_on_the_device():
    from mdgrad_amd.observable import structure_factor
    N, T, L = 65, 12, 6
    x = walk(T, N)[0]
    q = torch.as_tensor(x).to(DEV)
    for w in (None, weights_with_zeros(N, 3)):
        coh, slf = mk_obs(N, L, "coherent", weights=w), mk_obs(N, L, "self", weights=w)
        k, F = coh(q)
        ks, Fs = slf(q)
        sk = structure_factor(mk_system(N), CONF[0], CONF[1], weights=w, max_per_bin=CONF[2])
        kk, S = sk(q)
        assert torch.equal(k, kk) and torch.equal(ks, kk) and F.shape == (CONF[0], L)
        F, Fs, S = F.cpu().double().numpy(), Fs.cpu().double().numpy(), S.cpu().double().numpy()
        e = float((np.abs(F[:, 0] - S) / (np.sqrt(n_eff(w, N) * np.abs(S)) + 1.0)).max())
        figure("F[:, 0] against structure_factor", e, 2 * TOL)
        assert e <= 2 * TOL
        tol_s = 5e-7 + (T + 8) * 2.0 ** -24
        figure("F_s[:, 0] against 1", float(np.abs(Fs[:, 0] - 1).max()), tol_s)
        assert np.abs(Fs[:, 0] - 1).max() <= tol_s
        # whole cells added to some atoms of some frames: +7 L and -3 L
        xs = x.copy()
        xs[3:7, ::2] += np.float32(7 * CELL)
        xs[5:, 1::3, 1] -= np.float32(3 * CELL)
        qs = torch.as_tensor(xs).to(DEV)
        e = float((np.abs(coh(qs)[1].cpu().double().numpy() - F) / (np.sqrt(n_eff(w, N) * np.abs(F[:, :1])) + 1.0)).max())
        figure("coherent: displaced by whole cells", e, TOL)
        assert e <= TOL
        e = float(np.abs(slf(qs)[1].cpu().double().numpy() - Fs).max())
        figure("self: displaced by whole cells", e, tol_s)
        assert e <= tol_s
    x1 = walk(T, 1)[0]
    q1 = torch.as_tensor(x1).to(DEV)
    F1, Fs1 = mk_obs(1, L, "coherent")(q1)[1].cpu().double().numpy(), mk_obs(1, L, "self")(q1)[1].cpu().double().numpy()
    e = float(np.abs(F1 - Fs1).max())
    figure("N = 1: coherent against self", e, TOL * 2 + 5e-7 + (T + 8) * 2.0 ** -24)
    assert e <= TOL * 2 + 5e-7 + (T + 8) * 2.0 ** -24                   # envelope sqrt(1 x 1) + 1 = 2


@pytest.mark.parametrize("kind", ["coherent", "self"])
def test_leading_shapes_repeatability_and_chunking(kind, monkeypatch):
    from mdgrad_amd import ops
    N, T, L, k, R = 5, 12, 7, 3, 2
    x4 = torch.as_tensor(walk(T, N, k, R)).to(DEV)                      # [R, T, k N, 3]
    one, stk = mk_obs(N, L, kind, stride=2), mk_obs(N, L, kind, k=k, stride=2)
    full = stk.per_replica(x4)
    B = stk.nbins
    assert full.shape == (R, k, B, L)
    assert stk.per_replica(x4[0]).shape == (k, B, L) and torch.equal(stk.per_replica(x4[0]), full[0])
    for r in range(R):
        for c in range(k):
            a = one.per_replica(x4[r][:, c * N:(c + 1) * N])
            assert a.shape == (B, L) and torch.equal(a, full[r, c])
    xb = torch.stack([x4[0][:, :N], x4[1][:, N:2 * N]])                # [R, T, N, 3]
    b = one.per_replica(xb)
    assert b.shape == (R, B, L) and torch.equal(b[0], full[0, 0]) and torch.equal(b[1], full[1, 1])
    kk, mean = stk(x4)
    assert torch.equal(mean, full.reshape(-1, B, L).mean(0)) and kk.shape == (B,)
    G = np.random.default_rng(5).uniform(-1, 1, (R * k, B, L))
    xn = x4.cpu().numpy()
    first, second = run(stk, xn, G), run(stk, xn, G)
    assert all(torch.equal(p, q) for p, q in zip(first, second))
    calls = []
    real = ops.IsfFn._chunks
    monkeypatch.setattr(ops.IsfFn, "_chunks", staticmethod(lambda *a: calls.append(real(*a)) or calls[-1]))
    for limit, n_calls in ((4 * int(ops._lib.load().mdg_isf_workspace(stk.KINDS[kind], 1, T, N, len(stk.kvecs), L)), R * k),
                           (4 * int(ops._lib.load().mdg_isf_workspace(stk.KINDS[kind], k, T, N, len(stk.kvecs), L)), R),
                           (1, R * k)):
        monkeypatch.setattr(ops, "ISF_WS_BYTES", limit)
        del calls[:]
        chunked = run(stk, xn, G)
        assert len(calls) == 2 and all(len(c) == n_calls for c in calls), (limit, calls)
        assert all(torch.equal(p, q) for p, q in zip(first, chunked)), "the result depends on the chunking (%d calls)" % n_calls


@pytest.mark.parametrize("kind", ["coherent", "self"])
def test_non_contiguous_input_and_the_leaf_gets_the_gradient(kind):
    N, T, L = TILE + 1, 2 * WINDOW + 2, 5
    x = walk(T, N)[0]
    obs = mk_obs(N, L, kind)
    leaf = torch.as_tensor(x).to(DEV).requires_grad_(True)
    G = np.random.default_rng(8).uniform(-1, 1, (1, obs.nbins, L))
    F = obs.per_replica(leaf[::2])
    (F * torch.as_tensor(G[0], dtype=torch.float32).to(DEV)).sum().backward()
    assert leaf.grad.shape == leaf.shape and (leaf.grad[1::2] == 0).all()
    check_rows(kind + " every second frame of a leaf", obs, x[None, ::2], N, None, F.detach(), leaf.grad[::2], G)
    assert torch.equal(F.detach(), obs.per_replica(torch.as_tensor(np.ascontiguousarray(x[::2])).to(DEV)))
    cols = torch.as_tensor(walk(T, N, 2)[0]).to(DEV)[:, N:]             # a slice in the atom dimension
    assert not cols.is_contiguous() and torch.equal(obs.per_replica(cols), obs.per_replica(cols.contiguous()))


@pytest.mark.parametrize("kind", ["coherent", "self"])
def test_second_backward_raises(kind):
    q = torch.as_tensor(walk(8, 5)[0]).to(DEV).requires_grad_(True)
    F = mk_obs(5, 4, kind)(q)[1]
    (g,) = torch.autograd.grad(F.sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_random_walk_decays_as_a_gaussian():
    """The 4 096-walker case of tests/test_isf_host.py on the device: |F_s - exp(-k^2 sigma^2 tau / 2)| < 0.05."""
    from mdgrad_amd.observable import intermediate_scattering
    from mdgrad_amd.system import System
    W = WALK
    s = System(positions=np.zeros((W["N"], 3)), cell=np.asarray(W["cell"]), masses=np.full(W["N"], 1.008), device=DEV)
    obs = intermediate_scattering(s, W["nbins"], W["k_range"], W["T"], kind="self", max_per_bin=W["max_per_bin"])
    q = torch.as_tensor(random_walk(W["T"], W["N"], W["seed"], step=W["sigma"])).to(DEV)
    Fs = obs(q)[1].cpu().double().numpy()
    lengths = np.asarray(W["cell"], dtype=np.float32).astype(np.float64)
    kabs = np.sqrt(((2 * np.pi * obs.kvecs.numpy() / lengths) ** 2).sum(1))
    err = float(np.abs(Fs - walk_expected(kabs, obs._seg_host, W["T"], W["sigma"])).max())
    figure("random walk: largest |F_s - exp(-k^2 sigma^2 tau / 2)|", err, 0.05)
    assert err < 0.05


# ---------------------------------------------------------------------------------------------- through a trajectory
TRAJ = (6, (2.0, 10.0), 6, 8)                # nbins, k_range, max_per_bin, t_range


def composite(q_t, obs, n_atoms):
    """The torch composition in float64: cos / sin of q_t @ k.T, a slice per lag; mean over the replicas."""
    k = (2 * np.pi * obs.kvecs.double() / obs.cell.cpu().double()).to(q_t.device)
    T, L = q_t.shape[0], obs.t_range
    q = q_t.double().reshape(T, -1, n_atoms, 3)
    ph = q @ k.t()                                                      # [T, reps, N, M]
    c, s = ph.cos(), ph.sin()
    rows = []
    for tau in range(L):
        if obs.kind == "self":
            f = (c[tau:] * c[:T - tau] + s[tau:] * s[:T - tau]).sum(2)
        else:
            re, im = c.sum(2), s.sum(2)
            f = re[tau:] * re[:T - tau] + im[tau:] * im[:T - tau]
        rows.append(f.mean(0).mean(0) / n_atoms)                        # [M]
    Fk = torch.stack(rows, 1)                                           # [M, L]
    seg = obs._seg_host
    return torch.stack([Fk[seg[b]:seg[b + 1]].mean(0) if seg[b + 1] > seg[b] else Fk.new_zeros(L) for b in range(obs.nbins)])


def traj_run(n_rep, kind, use_kernels):
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NoseHooverChain, Simulations
    from mdgrad_amd.observable import intermediate_scattering, relaxation, structure_factor
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
    obs = intermediate_scattering(system, TRAJ[0], TRAJ[1], TRAJ[3], kind=kind, max_per_bin=TRAJ[2])
    F = obs(q_t)[1] if use_kernels else composite(q_t, obs, 108)
    peak = int(structure_factor(system, TRAJ[0], TRAJ[1], max_per_bin=TRAJ[2])(q_t.detach())[1].argmax())      # the first peak of S(k)
    relaxation(F)[peak, 1:].sum().backward()
    return F.detach(), q_t.detach(), torch.stack([mdl.sigma.grad.reshape(()), mdl.epsilon.grad.reshape(())]).cpu().double()


@pytest.mark.parametrize("kind", ["coherent", "self"])
@pytest.mark.parametrize("n_rep", [0, 2])
def test_through_the_fused_trajectory(n_rep, kind):
    """108-atom LJ, 20 steps: relaxation(F)[first-peak bin, 1:].sum().backward() reaches the potential's parameters, and
    gives what the torch composite on the q_t of a fresh identical run gives (a check of the autograd wiring)."""
    F, q, grads = traj_run(n_rep, kind, True)
    F_c, q_c, grads_c = traj_run(n_rep, kind, False)
    top = float(grads_c.abs().max())
    figure("trajectory %s n_rep %d: smallest |dL/dtheta| (must be finite and not 0)" % (kind, n_rep), float(grads.abs().min()), 0.0)
    figure("trajectory %s n_rep %d: |dL/dtheta - composite| / largest" % (kind, n_rep), float((grads - grads_c).abs().max()) / top, 1e-4)
    F = F.double()
    figure("trajectory %s n_rep %d: |F - composite| / |F|" % (kind, n_rep), float(((F - F_c).abs() / F_c.abs()).max()), 1e-5)
    assert torch.isfinite(grads).all() and (grads != 0).all()
    assert ((grads - grads_c).abs() <= 1e-4 * top).all(), (grads, grads_c)
    assert torch.allclose(F, F_c, rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------------- torch ops and ctypes
def test_torch_ops_equal_the_ctypes_path(tmp_path):
    """IsfFn goes through torch.ops.mdgrad.isf_fwd / isf_bwd when the op library is loaded and through ctypes when
    MDG_TORCH_OPS=0: the same kernels, the same bits.  The switch is read once per process, hence the child."""
    from mdgrad_amd import _torch_ops
    ns = _torch_ops.get()
    assert ns is not None and hasattr(ns, "isf_fwd") and hasattr(ns, "isf_bwd")
    N, T, L, k, R = TILE + 1, WINDOW + 3, 6, 2, 2
    x, w = walk(T, N, k, R), weights_with_zeros(N, 3)
    G = np.random.default_rng(1).uniform(-1, 1, (R * k, CONF[0], L))
    np.savez(tmp_path / "in.npz", x=x, w=w, G=G)
    here = {kind: run(mk_obs(N, L, kind, k=k, weights=w, stride=2), x, G) for kind in ("coherent", "self")}
    obs = mk_obs(N, L, "self", k=k, weights=w, stride=2)
    q = torch.as_tensor(x).to(DEV)
    cell = _torch_ops.cell_args(obs._cell_struct)
    F = ns.isf_fwd(q, 1, N, 0, k, cell, obs.weights, obs._norm, obs._kvec, obs._seg, obs._seg_host, L, 2)
    assert torch.equal(F.reshape(here["self"][0].shape), here["self"][0])
    with pytest.raises(RuntimeError, match="multiple of group"):
        ns.isf_fwd(q, 1, N + 1, 0, 1, cell, None, obs._norm, obs._kvec, obs._seg, obs._seg_host, L, 2)
    with pytest.raises(RuntimeError, match="n_lags"):
        ns.isf_fwd(q, 0, N, 0, k, cell, obs.weights, obs._norm, obs._kvec, obs._seg, obs._seg_host, T + 1, 1)
    script = tmp_path / "child.py"
    script.write_text(
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from mdgrad_amd import _torch_ops\n"
        "from test_gpu_isf import mk_obs, run\n"
        "assert _torch_ops.get() is None\n"
        "d = np.load(sys.argv[1])\n"
        "out = {}\n"
        "for kind in ('coherent', 'self'):\n"
        "    F, g = run(mk_obs(%d, %d, kind, k=%d, weights=d['w'], stride=2), d['x'], d['G'])\n"
        "    out['F_' + kind], out['g_' + kind] = F.cpu().numpy(), g.cpu().numpy()\n"
        "np.savez(sys.argv[2], **out)\n"
        % (os.path.join(ROOT, "tests"), ROOT, N, L, k))
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       env=dict(os.environ, MDG_TORCH_OPS="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    there = np.load(tmp_path / "out.npz")
    for kind in ("coherent", "self"):
        assert np.array_equal(there["F_" + kind], here[kind][0].cpu().numpy()), "%s F differs between torch.ops and ctypes" % kind
        assert np.array_equal(there["g_" + kind], here[kind][1].cpu().numpy()), "%s g differs between torch.ops and ctypes" % kind
