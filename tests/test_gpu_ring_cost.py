"""The ring sweeps after their cycle-cost trim (csrc/traj_ring.hpp): the visitor of a ring step is read through one running byte
address per lane (ring_visitor_at: a compare with the scalar step, a select, a subtraction; the rows are DS offset fields) in
ring_sweep -- general, near, FULL, masked, the antipodal read -- and in ring_sweep_lj_multi, and the two cubics of the fused RDF
derivative table are six scalar fmas.  Integer addressing and the same fmas: no output bit moves against the parent commit
(`python tests/test_gpu_ring_cost.py --dump DIR` writes every output array of the cases below as DIR/<case>__<name>.npy; the
same script runs in the parent's tree; profiles/ring_cost_ab.txt carries the comparison).

block = 64, R = 6, T = 5, NHC and NVE, with and without the fused RDF.
  N = 2, 3, 4, 6, 8: nl = ceil(N/2) = 1 .. 4 ring lanes -- a lane passes entry 0 of the visitor rows at its first step or never,
    odd and even nl (with and without the antipodal step), a last lane with one atom (N = 3);
  N = 107, 108 with the re-ordered lattice of tests/test_gpu_ring_antipodal.py (antipodal pairs interact).

  * trajectory, costates and parameter gradient against the CPU oracle with the tolerances of tests/test_gpu_pins.py and, at
    the sizes tests/test_gpu_ring_antipodal.py has figures for, within twice those (its own bound);
  * the fused histogram is the bits of rdf_fwd_fine_kernel on the same frames, and the fused frame gradient equals the separate
    observable launches within that file's bound.  N = 2, 3 have no figure there: the figure is the interpolation error of the
    derivative table relative to the gradient, a property of the table (the same 100 bins over the same range for every
    cluster below 64 atoms), so they take the largest of that file's small-cluster figures (N = 4: 7.298e-04), doubled as
    that file does;
  * the default build equals MDG_RING_LEAN=0 (the general sweep) bit for bit, every output (one child process per setting);
  * one stack of two masked LJ 12-6 terms at N = 8 (ring_sweep_lj_multi) against the oracle, tolerances of
    tests/test_gpu_pins.py test_ring_kernels_with_several_masked_terms_vs_oracle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (run as a script: this puts the repository root on sys.path)
import oracle as O
from test_gpu_parity import T, close, mk_system, oracle_run, DEV
from test_gpu_ring_antipodal import (ENSEMBLES, NT, PARENT_FRAME_GRAD, PARENT_ORACLE, R, _inputs, _run_fused, _setup,
                                     frame_gradient_figure, measure_oracle)

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 4, 6, 8, 107, 108)
CASES = [(n, ens) for n in SIZES for ens in ENSEMBLES]
SMALL_FRAME_GRAD = max(v for (n, _), v in PARENT_FRAME_GRAD.items() if n < 64)      # (4, 'nhc'): 7.298e-04


def _key(n_atoms, ens, fused):
    return "n%d-%s-%s" % (n_atoms, ens, "rdf" if fused else "plain")


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("n_atoms,ens", CASES)
def test_trajectory_costates_and_parameter_gradient_vs_oracle(n_atoms, ens):
    fig = measure_oracle(n_atoms, ens, check=True)          # (the asserts of tests/test_gpu_pins.py inside)
    print("N = %d %s: max |gpu - oracle| / max |oracle|: " % (n_atoms, ens) + "  ".join("%s %.3e" % kv for kv in sorted(fig.items())))
    for nm, e in fig.items():
        if (n_atoms, ens) in PARENT_ORACLE:
            assert e <= 2.0 * PARENT_ORACLE[(n_atoms, ens)][nm], "%s: %.3e against twice %.3e" % (nm, e, PARENT_ORACLE[(n_atoms, ens)][nm])


def _masked_stack():
    """two masked LJ 12-6 terms on 8 atoms: one shared sweep (ring_sweep_lj_multi); the launch's outputs and what the oracle
    needs to repeat it"""
    from mdgrad_amd import _lib, ops, potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NoseHooverChain
    n_atoms = 8
    g, base, pos, vel = _inputs(n_atoms)
    mass = g["mass"][:n_atoms]
    system = mk_system(base, g["cell"], vel[0], mass)
    A_, B_ = list(range(0, n_atoms, 2)), list(range(1, n_atoms, 2))
    specs = [(P.LennardJones(1.0, 1.0), dict(index_tuple=(A_, A_)), 2.5, [1.0, 1.0]),
             (P.LennardJones(0.9, 0.8), dict(index_tuple=(A_, B_)), 2.2, [0.9, 0.8])]
    stack = Stack({"t%d" % k: PairPotentials(system, sp[0], cutoff=sp[2], **sp[1]) for k, sp in enumerate(specs)})
    integ = NoseHooverChain(stack, system, T=1.0, num_chains=5, Q=50.0).to(DEV)
    spec = integ.fused_spec("NH_verlet")
    assert spec is not None and not spec.large
    spec.block = 64
    prm = spec.params(R, NT)
    assert _lib.load().mdg_traj_ring_taken(C.byref(prm), C.byref(spec.cell_struct), C.byref(spec.terms)), \
        "the wave-per-replica kernels must run"
    t = torch.Tensor([0.004 * i for i in range(NT)])
    v0, q0 = T(vel, DEV).requires_grad_(True), T(pos, DEV).requires_grad_(True)
    pv0 = torch.zeros(R, 5, device=DEV, requires_grad=True)
    out = ops.FusedTrajFn.apply(v0, q0, pv0, t.to(DEV), spec.flat_params(), spec)
    for sp in specs:
        sp[0].zero_grad()
    nrm = n_atoms * 3
    loss = (out[1][:, ::2].pow(2).sum((1, 2, 3)) / (3 * nrm) + out[0][:, -1].pow(2).sum((1, 2)) / nrm).sum() + out[2][:, -1].sum()
    loss.backward()
    torch.cuda.synchronize()
    arrays = {"v_t": out[0], "q_t": out[1], "pv_t": out[2], "adj_v0": v0.grad, "adj_q0": q0.grad, "adj_pv0": pv0.grad,
              "adj_theta": torch.cat([p.grad.reshape(-1) for sp in specs for p in sp[0].parameters()])}
    return {k: v.detach().cpu().numpy() for k, v in arrays.items()}, (g, pos, vel, mass, specs, t, nrm)


def test_two_masked_lj_terms_in_one_sweep_vs_oracle():
    a, (g, pos, vel, mass, specs, t, nrm) = _masked_stack()
    gth_sum = np.zeros(4)
    for r in range(R):
        terms = [O.PairTerm("lj", torch.tensor(sp[3]), sp[2], T(g["cell"]), **sp[1], p=12, q=6, c=1) for sp in specs]
        traj, lam, gth = oracle_run(pos[r], g["cell"], vel[r], mass, terms, 1.0, 50.0, 5, t,
                                    lambda L: L[1][::2].pow(2).sum() / (3 * nrm) + L[0][-1].pow(2).sum() / nrm + L[2][-1].sum())
        close(a["q_t"][r], traj[1], 0, 3e-5, "q_t[%d]" % r)
        close(a["v_t"][r], traj[0], 0, 3e-4, "v_t[%d]" % r)
        close(a["adj_v0"][r], lam[0], 2e-3, 3e-4 * float(lam[0].abs().max()), "adj v0[%d]" % r)
        close(a["adj_q0"][r], lam[1], 2e-3, 3e-4 * float(lam[1].abs().max()), "adj q0[%d]" % r)
        gth_sum += gth.numpy()
    close(a["adj_theta"], gth_sum, 2e-3, 3e-4 * np.abs(gth_sum).max(), "dL/dtheta")


# ------------------------------------------------------------------------------------------------ every output array
def _run_plain(n_atoms, ens):
    """the launch of measure_oracle (no fused observable): its outputs"""
    from mdgrad_amd import ops
    g, system, mdl, spec, pos, vel, t, nhc = _setup(n_atoms, ens, False)
    v0, q0 = T(vel, DEV).requires_grad_(True), T(pos, DEV).requires_grad_(True)
    pv0 = torch.zeros(R, 5, device=DEV, requires_grad=True) if nhc else None
    out = ops.FusedTrajFn.apply(v0, q0, pv0, t.to(DEV), spec.flat_params(), spec)
    assert getattr(out[0].grad_fn, "f_t", None) is not None, "the wave-per-replica kernels must run"
    mdl.zero_grad()
    nrm = n_atoms * 3
    loss = (out[1][:, ::2].pow(2).sum((1, 2, 3)) / (3 * nrm) + out[0][:, -1].pow(2).sum((1, 2)) / nrm).sum()
    if nhc:
        loss = loss + out[2][:, -1].sum()
    loss.backward()
    torch.cuda.synchronize()
    arrays = {"v_t": out[0], "q_t": out[1], "pv_t": out[2] if nhc else None, "adj_v0": v0.grad, "adj_q0": q0.grad,
              "adj_pv0": pv0.grad if nhc else None, "adj_theta": torch.stack([mdl.sigma.grad.reshape(()), mdl.epsilon.grad.reshape(())])}
    return {k: v.detach().cpu().numpy() for k, v in arrays.items() if v is not None}


def produce():
    """{case/name: array}: every output of every case"""
    res = {}
    for n_atoms, ens in CASES:
        for k, v in _run_plain(n_atoms, ens).items():
            res[_key(n_atoms, ens, False) + "/" + k] = v
        for k, v in _run_fused(n_atoms, ens).items():
            res[_key(n_atoms, ens, True) + "/" + k] = v
    for k, v in _masked_stack()[0].items():
        res["n8-nhc-masked2/" + k] = v
    return res


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """{setting: arrays}: one child process per setting of MDG_RING_LEAN, started together"""
    d = tmp_path_factory.mktemp("ring_cost")
    procs = {}
    for name, val in (("lean", None), ("general", "0")):
        env = dict(os.environ)
        env.pop("MDG_RING_LEAN", None)
        if val is not None:
            env["MDG_RING_LEAN"] = val
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--npz", str(d / (name + ".npz"))], env=env,
                                       cwd=os.path.dirname(os.path.abspath(__file__)), stdout=subprocess.PIPE,
                                       stderr=subprocess.STDOUT, text=True)
    out = {}
    for name, p in procs.items():
        log, _ = p.communicate()
        assert p.returncode == 0, "worker (%s) failed:\n%s" % (name, log[-4000:])
        out[name] = dict(np.load(str(d / (name + ".npz")), allow_pickle=False))
    return out


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_default_build_is_bitwise_the_general_sweep(both):
    assert sorted(both["lean"]) == sorted(both["general"])
    assert len(both["lean"]) >= len(CASES) * (5 + 9) + 7
    for k in sorted(both["lean"]):
        a, b = both["lean"][k], both["general"][k]
        assert np.isfinite(b).all(), "%s: not finite" % k
        assert _bits_equal(a, b), "%s: max |diff| %.3e" % (k, float(np.abs(a.astype(np.float64) - b).max()))
    for n_atoms, ens in CASES:
        for fused in (False, True):
            key = _key(n_atoms, ens, fused)
            assert float(np.abs(both["lean"][key + "/adj_q0"]).max()) > 0 and float(np.abs(both["lean"][key + "/adj_theta"]).max()) > 0, key


@pytest.mark.parametrize("n_atoms,ens", CASES)
def test_fused_histogram_is_bitwise_the_many_frame_kernel(both, n_atoms, ens):
    key = _key(n_atoms, ens, True)
    for setting in ("lean", "general"):
        a, b = both[setting][key + "/raw"], both[setting][key + "/raw_fine"]
        assert float(a.max()) > 0, "no pair fed the histogram"
        assert _bits_equal(a, b), "%s (%s): max |diff| %.3e" % (key, setting, float(np.abs(a.astype(np.float64) - b).max()))


@pytest.mark.parametrize("n_atoms,ens", CASES)
def test_fused_frame_gradient_equals_separate_launches(both, n_atoms, ens):
    arrays = {"n%d-%s/%s" % (n_atoms, ens, nm): both["lean"][_key(n_atoms, ens, True) + "/" + nm] for nm in ("adj_q0", "sep_adj_q0")}
    e = frame_gradient_figure(arrays, n_atoms, ens)
    bound = 2.0 * PARENT_FRAME_GRAD.get((n_atoms, ens), SMALL_FRAME_GRAD)
    print("frame gradient N = %d %s: max |fused - separate| / max |separate| = %.3e (bound %.3e)" % (n_atoms, ens, e, bound))
    assert e <= bound


if __name__ == "__main__":
    if sys.argv[1:2] == ["--dump"]:
        os.makedirs(sys.argv[2], exist_ok=True)
        for k, v in produce().items():
            np.save(os.path.join(sys.argv[2], k.replace("/", "__") + ".npy"), v)
    elif sys.argv[1:2] == ["--npz"]:
        np.savez(sys.argv[2], **produce())
    else:
        raise SystemExit("usage: test_gpu_ring_cost.py --dump DIR | --npz FILE")
