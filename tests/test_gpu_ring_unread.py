"""The ring adjoint leaves out the work whose results nobody reads (csrc/traj_ring.hpp, TrajArgs::skip_unread): without the
gradient of the initial state -- a fit of the potential's parameters -- FusedTrajFn.backward passes null adj_v0 / adj_q0 /
adj_pv0, the kernel skips the geometry-only sweep of frame 0 and the final stores, and where no dL/dv arrives (g_v null) the first
evaluation of the last interval runs the geometry-only sweep instead of H.w with w = 0.  MDG_RING_SKIP_UNREAD=0 keeps all of that
work (null outputs are just not stored); the switch is read where a launch is built, so each setting runs in a child process of
its own (this file, run as a script, is the worker).

block = 64, R = 6, T = 5; N = 108 (the headline's sweeps) and N = 4 (in-lane and antipodal operations only); NHC and NVE; the
fused RDF on every frame, and on frames 1, 3 only (strided, without frame 0: no frame-0 sweep in either setting); the loss fed by
g(r) alone (g_v, g_q null: the last interval's first evaluation is the geometry-only one) or by g(r) and v_t (g_v arrives).

  * the parameter gradient is the same bits with and without MDG_RING_SKIP_UNREAD=0;
  * the same bits with and without requires_grad on the initial state; the costates are returned when asked for -- the same
    bits in both settings -- and None when not."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (run as a script: this puts the repository root on sys.path)
from conftest import load_golden
from test_gpu_parity import T, mk_system, DEV

pytestmark = pytest.mark.gpu

R, NT = 6, 5
SIZES = (108, 4)
CASES = [(n, ens, sel, feed) for n in SIZES for ens in ("nhc", "nve") for sel in ("all", "odd") for feed in ("g", "g+v")]


def _key(n, ens, sel, feed, state):
    return "n%d-%s-%s-%s-%s" % (n, ens, sel, feed, "state" if state else "theta")


def _run_case(n_atoms, ens, sel, feed, state):
    from mdgrad_amd import ops
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NVE, NoseHooverChain
    from mdgrad_amd.observable import rdf as rdf_obs
    g = load_golden("nhc_traj_lj")
    cell = float(g["cell"][0])
    base = g["pos"][:n_atoms]
    rng = np.random.default_rng(n_atoms)
    pos = np.mod(base[None] + rng.normal(0, 0.02, (R,) + base.shape), cell).astype(np.float32)
    vel = rng.normal(0, 0.5, pos.shape).astype(np.float32)
    system = mk_system(base, g["cell"], vel[0], g["mass"][:n_atoms])
    mdl = P.LennardJones(1.0, 1.0)
    stack = Stack({"pair": PairPotentials(system, mdl, cutoff=2.5)})
    nhc = ens == "nhc"
    integ = (NoseHooverChain(stack, system, T=1.0, num_chains=5, Q=50.0) if nhc else NVE(stack, system)).to(DEV)
    integ.fuse_observables = True
    spec = integ.fused_spec("NH_verlet" if nhc else "verlet")
    assert spec is not None and not spec.large
    spec.block = 64
    t = torch.Tensor([0.004 * i for i in range(NT)]).to(DEV)
    obs = rdf_obs(system, nbins=100, r_range=(0.75, 2.5))
    params = list(mdl.parameters())
    out = {}
    for launch in range(2):                              # (the first launch registers the observable, the second one fuses it)
        v0, q0 = T(vel, DEV).requires_grad_(state), T(pos, DEV).requires_grad_(state)
        pv0 = torch.zeros(R, 5, device=DEV, requires_grad=state) if nhc else None
        res = ops.fused_traj(v0, q0, pv0, t, spec.flat_params(), spec)
        v_t, q_t = res[0], res[1]
        assert (q_t._mdg_traj[3] is not None) == (launch == 1), "fused observable: launch %d" % launch
        assert getattr(v_t.grad_fn, "f_t", None) is not None, "the wave-per-replica kernels must run"
        gr = obs(q_t if sel == "all" else q_t[:, 1::2])[2]
        wgt = torch.linspace(0.5, 1.5, gr.shape[0], device=DEV)
        loss = (gr * wgt).pow(2).sum()
        if feed == "g+v":
            loss = loss + v_t[:, -1].pow(2).sum() / 50.0
        for p in params:
            p.grad = None
        loss.backward()
        out = {"adj_theta": torch.cat([p.grad.reshape(-1) for p in params])}
        if state:
            out.update(adj_v0=v0.grad, adj_q0=q0.grad)
            if nhc:
                out["adj_pv0"] = pv0.grad
        else:
            assert v0.grad is None and q0.grad is None and (pv0 is None or pv0.grad is None)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def _worker(path):
    res = {}
    for case in CASES:
        for state in (False, True):
            for k, v in _run_case(*case, state).items():
                res[_key(*case, state) + "/" + k] = v
    np.savez(path, **res)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """{setting: arrays}: one child process per setting of MDG_RING_SKIP_UNREAD, started together"""
    d = tmp_path_factory.mktemp("ring_unread")
    procs = {}
    for name, val in (("skip", None), ("keep", "0")):
        env = dict(os.environ)
        env.pop("MDG_RING_SKIP_UNREAD", None)
        if val is not None:
            env["MDG_RING_SKIP_UNREAD"] = val
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), str(d / (name + ".npz"))], env=env,
                                       cwd=os.path.dirname(os.path.abspath(__file__)), stdout=subprocess.PIPE,
                                       stderr=subprocess.STDOUT, text=True)
    out = {}
    for name, p in procs.items():
        log, _ = p.communicate()
        assert p.returncode == 0, "worker (%s) failed:\n%s" % (name, log[-4000:])
        out[name] = dict(np.load(str(d / (name + ".npz")), allow_pickle=False))
    return out


def _same_bits(a, b, what):
    assert a.shape == b.shape and np.isfinite(a).all(), what
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: max |diff| %.3e" % (
        what, float(np.abs(a.astype(np.float64) - b).max()))


@pytest.mark.parametrize("n,ens,sel,feed", CASES, ids=["n%d-%s-%s-%s" % c for c in CASES])
def test_parameter_gradient_does_not_depend_on_the_skipped_work(both, n, ens, sel, feed):
    ref = both["keep"][_key(n, ens, sel, feed, True) + "/adj_theta"]
    assert float(np.abs(ref).max()) > 0
    for setting in ("skip", "keep"):
        for state in (False, True):
            _same_bits(both[setting][_key(n, ens, sel, feed, state) + "/adj_theta"], ref,
                       "dL/dtheta, %s, %s" % (setting, "with the costates" if state else "parameters only"))


@pytest.mark.parametrize("n,ens,sel,feed", CASES, ids=["n%d-%s-%s-%s" % c for c in CASES])
def test_costates_are_returned_when_asked_for_and_only_then(both, n, ens, sel, feed):
    names = ("adj_v0", "adj_q0") + (("adj_pv0",) if ens == "nhc" else ())
    for nm in names:
        for setting in ("skip", "keep"):
            assert _key(n, ens, sel, feed, False) + "/" + nm not in both[setting], nm
        a, b = (both[s][_key(n, ens, sel, feed, True) + "/" + nm] for s in ("skip", "keep"))
        _same_bits(a, b, nm)
    # (the fused observable's frame gradient reaches adj_q0 in every case; frame 0's own share only where it is selected)
    assert float(np.abs(both["skip"][_key(n, ens, sel, feed, True) + "/adj_q0"]).max()) > 0


if __name__ == "__main__":
    _worker(sys.argv[1])
