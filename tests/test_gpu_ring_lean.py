"""The full-ring sweep of the wave-per-replica kernels (ring_sweep<..., FULL>, csrc/traj_ring.hpp: even N, no per-pair
existence flags) against the general sweep of the same build (MDG_RING_LEAN=0): forward + adjoint through ops.fused_traj with
block = 64, with and without the fused RDF, NHC and NVE -- v_t, q_t, pv_t, the per-frame forces, g(r), the three costates and the
parameter gradient are the same bits.  The switch is read where a launch is built, so each setting runs in a child process of
its own (this file, run as a script, is the worker); both children compute every case once and the tests compare what they saved.

The shapes: N = 108 (nl = 54: the antipodal step runs; the headline), 106 (nl = 53: no antipodal step), 128 (every lane owns
atoms: nobody is kept out of the sweep), 2 (nl = 1: step 0 only), 4 (nl = 2: step 0 and the antipodal step, no ring step),
107 (odd: must not take the full ring; equal trivially -- guards the dispatch), `far` (N = 108, one atom of one replica moved
by +2 cell lengths: the window vote fails there, general minimum image) and `twin` (N = 108, two atoms of one replica at the same
place with the same velocity: d2 = 0 at every frame is rejected, the outputs stay finite)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_parity import T, mk_system, DEV

pytestmark = pytest.mark.gpu

R, NT = 6, 6
SHAPES = [("n108", 108), ("n106", 106), ("n128", 128), ("n2", 2), ("n4", 4), ("n107", 107), ("far", 108), ("twin", 108)]
CASES = [(s, "lj", ens, rdf) for s, _ in SHAPES for ens in ("nhc", "nve") for rdf in (False, True)]
CASES += [("n108", "yukawa", ens, False) for ens in ("nhc", "nve")]
NAMES = ("v_t", "q_t", "pv_t", "f_t", "g", "adj_v0", "adj_q0", "adj_pv0", "adj_theta")


def _key(shape, form, ens, rdf):
    return "%s-%s-%s-%s" % (shape, form, ens, "rdf" if rdf else "plain")


def _positions(shape, n_atoms, g):
    """[R, N, 3] positions and velocities: the golden fcc box (a bcc lattice of the same box for 128 atoms), jittered"""
    cell = float(g["cell"][0])                           # (cubic)
    if n_atoms <= g["pos"].shape[0]:
        base = g["pos"][:n_atoms]
    else:
        a = cell / 4.0
        c = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3) * a
        base = np.concatenate([c + 0.25 * a, c + 0.75 * a])[:n_atoms].astype(np.float32)
    rng = np.random.default_rng(n_atoms + len(shape))
    pos = np.mod(base[None] + rng.normal(0, 0.02, (R,) + base.shape), cell).astype(np.float32)
    vel = rng.normal(0, 0.5, pos.shape).astype(np.float32)
    if shape == "far":
        pos[2, 5, 1] += 2.0 * cell
    if shape == "twin":
        pos[3, 11] = pos[3, 10]
        vel[3, 11] = vel[3, 10]
    return base, pos, vel


def _run_case(shape, n_atoms, form, ens, rdf):
    from mdgrad_amd import ops
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NVE, NoseHooverChain
    from mdgrad_amd.observable import rdf as rdf_obs
    g = load_golden("nhc_traj_lj")
    base, pos, vel = _positions(shape, n_atoms, g)
    mass = np.resize(g["mass"], n_atoms)
    if shape == "twin":
        mass[11] = mass[10]
    system = mk_system(base, g["cell"], vel[0], mass)
    mdl = P.LennardJones(1.0, 1.0) if form == "lj" else P.Yukawa(1.0, 1.2)
    stack = Stack({"pair": PairPotentials(system, mdl, cutoff=2.5)})
    nhc = ens == "nhc"
    integ = (NoseHooverChain(stack, system, T=1.0, num_chains=5, Q=50.0) if nhc else NVE(stack, system)).to(DEV)
    integ.fuse_observables = rdf
    spec = integ.fused_spec("NH_verlet" if nhc else "verlet")
    assert spec is not None and not spec.large
    spec.block = 64
    t = torch.Tensor([0.004 * i for i in range(NT)]).to(DEV)
    obs = rdf_obs(system, nbins=100, r_range=(0.75, 2.5))
    params = list(mdl.parameters())
    out = {}
    for launch in range(2 if rdf else 1):                # (the first launch registers the observable, the second one fuses it)
        v0, q0 = T(vel, DEV).requires_grad_(True), T(pos, DEV).requires_grad_(True)
        pv0 = torch.zeros(R, 5, device=DEV, requires_grad=True) if nhc else None
        res = ops.fused_traj(v0, q0, pv0, t, spec.flat_params(), spec)
        v_t, q_t = res[0], res[1]
        assert (q_t._mdg_traj[3] is not None) == (rdf and launch == 1), "fused observable: launch %d" % launch
        f_t = getattr(v_t.grad_fn, "f_t", None)
        assert f_t is not None, "the wave-per-replica kernels keep the per-frame forces"
        gr = obs(q_t)[2]
        wgt = torch.linspace(0.5, 1.5, gr.shape[0], device=DEV)
        loss = (gr * wgt).pow(2).sum() + q_t[:, ::2].pow(2).sum() / 100.0 + v_t[:, -1].pow(2).sum() / 50.0
        if nhc:
            loss = loss + res[2][:, -1].sum()
        for p in params:
            p.grad = None
        f_keep = f_t[:, 1:].detach().clone()
        loss.backward()
        out = {"v_t": v_t, "q_t": q_t, "pv_t": res[2] if nhc else None, "f_t": f_keep, "g": gr, "adj_v0": v0.grad, "adj_q0": q0.grad,
               "adj_pv0": pv0.grad if nhc else None,
               "adj_theta": torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params])}
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in out.items() if v is not None}


def _worker(path):
    n_of = dict(SHAPES)
    res = {}
    for shape, form, ens, rdf in CASES:
        for k, v in _run_case(shape, n_of[shape], form, ens, rdf).items():
            res[_key(shape, form, ens, rdf) + "/" + k] = v
    np.savez(path, **res)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """{setting: arrays}: one child process per setting of MDG_RING_LEAN, started together"""
    d = tmp_path_factory.mktemp("ring_lean")
    procs = {}
    for name, val in (("lean", None), ("general", "0")):
        env = dict(os.environ)
        env.pop("MDG_RING_LEAN", None)
        if val is not None:
            env["MDG_RING_LEAN"] = val
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), str(d / (name + ".npz"))], env=env,
                                       cwd=os.path.dirname(os.path.abspath(__file__)), stdout=subprocess.PIPE,
                                       stderr=subprocess.STDOUT, text=True)
    out = {}
    for name, p in procs.items():
        log, _ = p.communicate()
        assert p.returncode == 0, "worker (%s) failed:\n%s" % (name, log[-4000:])
        out[name] = dict(np.load(str(d / (name + ".npz")), allow_pickle=False))
    return out


@pytest.mark.parametrize("shape,form,ens,rdf", CASES, ids=[_key(*c) for c in CASES])
def test_full_ring_sweep_is_bitwise_the_general_one(both, shape, form, ens, rdf):
    key = _key(shape, form, ens, rdf)
    seen = 0
    for nm in NAMES:
        a, b = both["lean"].get(key + "/" + nm), both["general"].get(key + "/" + nm)
        assert (a is None) == (b is None), nm
        if a is None:
            assert nm in ("pv_t", "adj_pv0") and ens == "nve", nm
            continue
        seen += 1
        assert np.isfinite(b).all(), "%s %s: the general sweep's output is not finite" % (key, nm)
        assert torch.equal(torch.from_numpy(a), torch.from_numpy(b)), "%s %s: max |diff| %.3e" % (
            key, nm, float(np.abs(a.astype(np.float64) - b).max()))
    assert seen == (9 if ens == "nhc" else 7)
    assert float(np.abs(both["lean"][key + "/adj_q0"]).max()) > 0 and float(np.abs(both["lean"][key + "/adj_theta"]).max()) > 0


if __name__ == "__main__":
    _worker(sys.argv[1])
