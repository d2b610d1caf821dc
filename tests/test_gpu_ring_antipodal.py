"""The antipodal step of the ring sweep evaluates each pair once (ring_sweep, csrc/traj_ring.hpp: for an even number of ring
lanes nl = ceil(N/2), lane l and lane l + nl/2 meet from both sides; the lower one takes the straight pairs, the upper one
the crossed pairs through the same operation on swapped visitor halves, and the visitors' sums are handed to the antipode in one
ds_bpermute_b32 per register).  Summation order moves against the directed form at rounding level; the pair set does not.

block = 64, R = 6, T = 5.  N = 108 (nl = 54, the headline), 8 (nl = 4: one ring step and the antipodal step), 4 (nl = 2: the
antipodal step is the only step between lanes), 107 (odd N with even nl: the last lane owns one atom, general sweep), 6
(nl = 3, odd: no antipodal step -- the code of the directed form, guards the dispatch).

  * trajectory, costates and parameter gradient against the CPU oracle, NHC and NVE, with the tolerances of
    tests/test_gpu_pins.py, and each figure max |gpu - oracle| / max |oracle| within twice what the directed form gave
    (`python tests/test_gpu_ring_antipodal.py --measure` prints every figure without asserting; the same script runs in the
    parent commit's tree; profiles/ring_antipodal_ab.txt carries both builds' figures);
  * one evaluation (force, H.w, parameter sums) at N = 108 against float64, within twice the directed form's figures;
  * the fused histogram is the bits of rdf_fwd_fine_kernel on the same frames (the many-frame kernel takes >= 1 024 frames
    of >= 64 atoms: 1 024 frames with every atom at the origin are appended -- d = 0 feeds no bin -- and below 64 atoms the
    missing atoms sit at one point beyond the observable's cutoff from every atom, _many_frames);
  * the fused frame gradient against the separate observable launches: max |adj_q0(fused) - adj_q0(separate)| / max |separate|
    within twice the directed form's figure;
  * lean equals MDG_RING_LEAN=0 bit for bit (one child process per setting: this file, run as a script, is the worker);
  * the adjoint that reads the stored forces equals the one that rebuilds them bit for bit (the check of
    tests/test_gpu_ring_force_frames.py at these sizes, with that test's own nine frames)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (run as a script: this puts the repository root on sys.path)
import oracle as O
from conftest import load_golden
from test_gpu_parity import T, close, mk_system, oracle_run, DEV
from test_gpu_ring_force_frames import test_ring_adjoint_with_stored_forces_is_bitwise_the_rebuilt_one as stored_forces_check
from test_gpu_ring_trim import measure_one_evaluation

pytestmark = pytest.mark.gpu

R, NT = 6, 5
SIZES = (108, 8, 4, 107, 6)
ENSEMBLES = ("nhc", "nve")
CASES = [(n, ens) for n in SIZES for ens in ENSEMBLES]
NAMES = ("v_t", "q_t", "pv_t", "f_t", "g", "adj_v0", "adj_q0", "adj_pv0", "adj_theta")
# The figures of the parent commit (the directed antipodal step): python tests/test_gpu_ring_antipodal.py --measure there.
# {(N, ensemble): {quantity: max |gpu - oracle| / max |oracle|}}, the frame gradient and one evaluation against float64.
PARENT_ORACLE = {
    (108, 'nhc'): {'q_t': 9.937e-08, 'v_t': 6.562e-07, 'adj_v0': 3.598e-07, 'adj_q0': 6.916e-07, 'theta': 2.464e-07},
    (108, 'nve'): {'q_t': 4.968e-08, 'v_t': 5.15e-07, 'adj_v0': 5.469e-07, 'adj_q0': 5.966e-07, 'theta': 4.305e-07},
    (8, 'nhc'): {'q_t': 1.553e-09, 'v_t': 4.321e-07, 'adj_v0': 3.327e-07, 'adj_q0': 1.57e-06, 'theta': 5.255e-07},
    (8, 'nve'): {'q_t': 1.238e-08, 'v_t': 3.125e-07, 'adj_v0': 2.361e-07, 'adj_q0': 6.919e-07, 'theta': 1.587e-07},
    (4, 'nhc'): {'q_t': 1.249e-08, 'v_t': 2.402e-07, 'adj_v0': 2.023e-07, 'adj_q0': 1.033e-06, 'theta': 8.228e-08},
    (4, 'nve'): {'q_t': 7.798e-10, 'v_t': 3.66e-07, 'adj_v0': 3.127e-07, 'adj_q0': 1.2e-06, 'theta': 6.409e-07},
    (107, 'nhc'): {'q_t': 2.483e-08, 'v_t': 3.006e-07, 'adj_v0': 1.678e-07, 'adj_q0': 7.43e-07, 'theta': 2.907e-07},
    (107, 'nve'): {'q_t': 9.929e-08, 'v_t': 3.66e-07, 'adj_v0': 3.479e-07, 'adj_q0': 5.74e-07, 'theta': 3.434e-07},
    (6, 'nhc'): {'q_t': 1.553e-09, 'v_t': 1.749e-07, 'adj_v0': 1.18e-07, 'adj_q0': 7.014e-07, 'theta': 1.048e-07},
    (6, 'nve'): {'q_t': 1.245e-08, 'v_t': 2.518e-07, 'adj_v0': 3.04e-07, 'adj_q0': 5.07e-07, 'theta': 3.91e-07},
}
PARENT_FRAME_GRAD = {(108, 'nhc'): 1.827e-05, (108, 'nve'): 1.950e-05, (8, 'nhc'): 6.172e-04, (8, 'nve'): 4.995e-04, (4, 'nhc'): 7.298e-04,
                     (4, 'nve'): 6.161e-04, (107, 'nhc'): 2.704e-05, (107, 'nve'): 2.298e-05, (6, 'nhc'): 2.556e-04, (6, 'nve'): 6.309e-04}
PARENT_EVAL = {'force': 2.799e-06, 'hw': 2.379e-06, 'theta': 4.403e-06}


def _inputs(n_atoms):
    g = load_golden("nhc_traj_lj")
    base = g["pos"][:n_atoms]
    if n_atoms > 100:
        # In lattice order atom i and atom i + 54 -- the atoms of antipodal lanes -- sit 2.77 apart, beyond the cutoff: the
        # antipodal step would add zeros.  Even atoms first, then the odd ones: antipodal lanes hold lattice neighbours.
        base = base[np.concatenate([np.arange(0, n_atoms, 2), np.arange(1, n_atoms, 2)])]
    rng = np.random.default_rng(1000 + n_atoms)
    pos = np.mod(base[None] + rng.normal(0, 0.02, (R,) + base.shape), g["cell"]).astype(np.float32)
    vel = rng.normal(0, 0.5, pos.shape).astype(np.float32)
    nl = (n_atoms + 1) // 2
    if nl % 2 == 0:                                      # the antipodal step must have pairs inside the cutoff to add up
        cell = np.asarray(g["cell"], np.float64)
        d = base[nl:].astype(np.float64)[None, :, :] - base[:nl].astype(np.float64)[:, None, :]
        d -= cell * np.rint(d / cell)
        dist = np.sqrt((d * d).sum(-1))                  # [atoms of the lower lanes, atoms of the upper lanes]
        close_ = [dist[2 * l + a, 2 * l + b] < 2.0 for l in range(nl // 2) for a in (0, 1) for b in (0, 1) if 2 * l + b < n_atoms - nl]
        assert sum(close_) >= nl // 2, "N = %d: %d antipodal pairs inside the cutoff" % (n_atoms, sum(close_))
    return g, base, pos, vel


def _setup(n_atoms, ens, fuse):
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NVE, NoseHooverChain
    g, base, pos, vel = _inputs(n_atoms)
    system = mk_system(base, g["cell"], vel[0], g["mass"][:n_atoms])
    mdl = P.LennardJones(1.0, 1.0)
    stack = Stack({"pair": PairPotentials(system, mdl, cutoff=2.5)})
    nhc = ens == "nhc"
    integ = (NoseHooverChain(stack, system, T=1.0, num_chains=5, Q=50.0) if nhc else NVE(stack, system)).to(DEV)
    integ.fuse_observables = fuse
    spec = integ.fused_spec("NH_verlet" if nhc else "verlet")
    assert spec is not None and not spec.large
    spec.block = 64
    t = torch.Tensor([0.004 * i for i in range(NT)])
    return g, system, mdl, spec, pos, vel, t, nhc


# ------------------------------------------------------------------------------------------------ against the oracle
def measure_oracle(n_atoms, ens, check=False):
    """{quantity: max |gpu - oracle| / max |oracle| over the replicas}; check: also the asserts of tests/test_gpu_pins.py"""
    from mdgrad_amd import ops
    g, system, mdl, spec, pos, vel, t, nhc = _setup(n_atoms, ens, False)
    v0, q0 = T(vel, DEV).requires_grad_(True), T(pos, DEV).requires_grad_(True)
    pv0 = torch.zeros(R, 5, device=DEV, requires_grad=True) if nhc else None
    out = ops.FusedTrajFn.apply(v0, q0, pv0, t.to(DEV), spec.flat_params(), spec)
    v_t, q_t = out[0], out[1]
    assert getattr(v_t.grad_fn, "f_t", None) is not None, "the wave-per-replica kernels must run"
    mdl.zero_grad()
    nrm = n_atoms * 3
    loss = (q_t[:, ::2].pow(2).sum((1, 2, 3)) / (3 * nrm) + v_t[:, -1].pow(2).sum((1, 2)) / nrm).sum()
    if nhc:
        loss = loss + out[2][:, -1].sum()
    loss.backward()
    fig = {k: 0.0 for k in ("q_t", "v_t", "adj_v0", "adj_q0")}
    gth_sum = np.zeros(2)

    def rel(a, b):
        a, b = a.detach().cpu().numpy().astype(np.float64), b.detach().numpy().astype(np.float64)
        return float(np.abs(a - b).max() / np.abs(b).max())

    for r in range(R):
        term = O.PairTerm("lj", torch.tensor([1.0, 1.0]), 2.5, T(g["cell"]), p=12, q=6, c=1)
        traj, lam, gth = oracle_run(
            pos[r], g["cell"], vel[r], g["mass"][:n_atoms], [term], 1.0, 50.0, 5, t,
            lambda L: L[1][::2].pow(2).sum() / (3 * nrm) + L[0][-1].pow(2).sum() / nrm + (L[2][-1].sum() if nhc else 0.0),
            ensemble=ens)
        if check:
            close(q_t[r], traj[1], 0, 2e-5, "q_t[%d]" % r)
            close(v_t[r], traj[0], 0, 2e-4, "v_t[%d]" % r)
            close(v0.grad[r], lam[0], 1e-3, 2e-4 * float(lam[0].abs().max()), "adj v0[%d]" % r)
            close(q0.grad[r], lam[1], 1e-3, 2e-4 * float(lam[1].abs().max()), "adj q0[%d]" % r)
            if nhc:
                close(out[2][r], traj[2], 1e-4, 1e-4, "pv_t[%d]" % r)
                close(pv0.grad[r], lam[2], 1e-3, 2e-4 * float(lam[2].abs().max()) + 1e-6, "adj pv0[%d]" % r)
        for k, a, b in (("q_t", q_t[r], traj[1]), ("v_t", v_t[r], traj[0]), ("adj_v0", v0.grad[r], lam[0]),
                        ("adj_q0", q0.grad[r], lam[1])):
            fig[k] = max(fig[k], rel(a, b))
        gth_sum += gth.numpy()
    got = np.array([float(mdl.sigma.grad), float(mdl.epsilon.grad)])
    if check:
        close(got, gth_sum, 1e-3, 2e-4 * np.abs(gth_sum).max() + 1e-7, "dL/dtheta")
    fig["theta"] = float(np.abs(got - gth_sum).max() / np.abs(gth_sum).max())
    return fig


@pytest.mark.parametrize("n_atoms,ens", CASES)
def test_trajectory_costates_and_parameter_gradient_vs_oracle(n_atoms, ens):
    fig = measure_oracle(n_atoms, ens, check=True)
    print("N = %d %s: max |gpu - oracle| / max |oracle|: " % (n_atoms, ens) + "  ".join("%s %.3e" % kv for kv in sorted(fig.items())))
    for nm, e in fig.items():
        assert e <= 2.0 * PARENT_ORACLE[(n_atoms, ens)][nm], "%s: %.3e against twice the parent's %.3e" % (
            nm, e, PARENT_ORACLE[(n_atoms, ens)][nm])


def test_one_evaluation_matches_float64_within_twice_the_parent():
    err = measure_one_evaluation()
    print("one evaluation, N = 108, max |gpu - float64| / max |float64|: " + "  ".join("%s %.3e" % kv for kv in sorted(err.items())))
    for nm, e in err.items():
        assert e <= 2.0 * PARENT_EVAL[nm], "%s: %.3e against twice the parent's %.3e" % (nm, e, PARENT_EVAL[nm])


# ------------------------------------------------------------------------------------------------ fused observable
def _many_frames(frames, cell, cutoff):
    """The frames as rdf_fwd_fine_kernel takes them (>= 1 024 frames of >= 64 atoms) with the same pair counts: 1 024 more
    frames with every atom at the origin (d = 0 feeds no bin) and, below 64 atoms, the missing atoms all at ONE point that
    is farther than the observable's cutoff from every atom of every frame (and at d = 0 from one another)."""
    n_frames, n_atoms = frames.shape[0], frames.shape[1]
    if n_atoms < 64:
        x = frames.reshape(-1, 3).cpu().numpy().astype(np.float64)
        c = (np.arange(16) + 0.5) * cell / 16
        cand = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
        d = cand[:, None, :] - x[None, :, :]
        d -= cell * np.rint(d / cell)
        dmin = np.sqrt((d * d).sum(-1)).min(1)
        assert float(dmin.max()) > cutoff + 0.02, "no point beyond the cutoff from every atom (%.3f)" % float(dmin.max())
        p = torch.as_tensor(cand[int(np.argmax(dmin))], dtype=torch.float32, device=frames.device)
        frames = torch.cat([frames, p.expand(n_frames, 64 - n_atoms, 3)], 1)
    return torch.cat([frames, torch.zeros(1024, frames.shape[1], 3, device=frames.device)]).contiguous()


def _run_fused(n_atoms, ens):
    """two launches with the fused observable asked for (the first registers it and runs the separate observable launches, the
    second fuses it): the second launch's outputs, the first launch's adj_q0 and the many-frame kernel's histogram of the
    second launch's frames"""
    from mdgrad_amd import ops
    from mdgrad_amd.observable import rdf as rdf_obs
    g, system, mdl, spec, pos, vel, t, nhc = _setup(n_atoms, ens, True)
    t = t.to(DEV)
    # (below 64 atoms the observable ends at 2.0, cutoff 2.5: _many_frames needs a point beyond it from every atom of the cluster)
    obs = rdf_obs(system, nbins=100, r_range=(0.75, 2.5 if n_atoms >= 64 else 2.0))
    params = list(mdl.parameters())
    sep_q0 = None
    for launch in range(2):
        v0, q0 = T(vel, DEV).requires_grad_(True), T(pos, DEV).requires_grad_(True)
        pv0 = torch.zeros(R, 5, device=DEV, requires_grad=True) if nhc else None
        res = ops.fused_traj(v0, q0, pv0, t, spec.flat_params(), spec)
        v_t, q_t = res[0], res[1]
        raw = q_t._mdg_traj[3]
        assert (raw is not None) == (launch == 1), "fused observable: launch %d" % launch
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
        if launch == 0:
            sep_q0 = q0.grad.detach().clone()
    with torch.no_grad():
        frames = _many_frames(q_t.detach().reshape(-1, n_atoms, 3), float(g["cell"][0]), float(obs.cutoff_boundary))
        fine = ops.RdfRawFn.apply(frames, obs.offsets, obs.coeff, obs.cutoff_boundary, obs._cell_struct, None, obs.spacing)
    out = {"v_t": v_t, "q_t": q_t, "pv_t": res[2] if nhc else None, "f_t": f_keep, "g": gr, "adj_v0": v0.grad, "adj_q0": q0.grad,
           "adj_pv0": pv0.grad if nhc else None, "adj_theta": torch.cat([p.grad.reshape(-1) for p in params]),
           "raw": raw, "raw_fine": fine, "sep_adj_q0": sep_q0}
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in out.items() if v is not None}


def _key(n_atoms, ens):
    return "n%d-%s" % (n_atoms, ens)


def _worker(path):
    res = {}
    for n_atoms, ens in CASES:
        for k, v in _run_fused(n_atoms, ens).items():
            res[_key(n_atoms, ens) + "/" + k] = v
    np.savez(path, **res)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """{setting: arrays}: one child process per setting of MDG_RING_LEAN, started together"""
    d = tmp_path_factory.mktemp("ring_antipodal")
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


@pytest.mark.parametrize("n_atoms,ens", CASES)
def test_lean_is_bitwise_the_general_sweep(both, n_atoms, ens):
    key = _key(n_atoms, ens)
    for nm in NAMES + ("raw",):
        a, b = both["lean"].get(key + "/" + nm), both["general"].get(key + "/" + nm)
        assert (a is None) == (b is None), nm
        if a is None:
            assert nm in ("pv_t", "adj_pv0") and ens == "nve", nm
            continue
        assert np.isfinite(b).all(), "%s %s: not finite" % (key, nm)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s %s: max |diff| %.3e" % (
            key, nm, float(np.abs(a.astype(np.float64) - b).max()))
    assert float(np.abs(both["lean"][key + "/adj_q0"]).max()) > 0 and float(np.abs(both["lean"][key + "/adj_theta"]).max()) > 0


@pytest.mark.parametrize("n_atoms,ens", CASES)
def test_fused_histogram_is_bitwise_the_many_frame_kernel(both, n_atoms, ens):
    key = _key(n_atoms, ens)
    for setting in ("lean", "general"):
        a, b = both[setting][key + "/raw"], both[setting][key + "/raw_fine"]
        assert float(a.max()) > 0, "no pair fed the histogram"
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s (%s): max |diff| %.3e" % (
            key, setting, float(np.abs(a.astype(np.float64) - b).max()))


def frame_gradient_figure(arrays, n_atoms, ens):
    key = _key(n_atoms, ens)
    fus, sep = arrays[key + "/adj_q0"].astype(np.float64), arrays[key + "/sep_adj_q0"].astype(np.float64)
    return max(float(np.abs(fus[r] - sep[r]).max() / np.abs(sep[r]).max()) for r in range(R))


@pytest.mark.parametrize("n_atoms,ens", CASES)
def test_fused_frame_gradient_equals_separate_launches_within_twice_the_parent(both, n_atoms, ens):
    e = frame_gradient_figure(both["lean"], n_atoms, ens)
    print("frame gradient N = %d %s: max |fused - separate| / max |separate| = %.3e (parent %.3e)" % (
        n_atoms, ens, e, PARENT_FRAME_GRAD[(n_atoms, ens)]))
    assert e <= 2.0 * PARENT_FRAME_GRAD[(n_atoms, ens)]


@pytest.mark.parametrize("n_atoms,ens", CASES)
@pytest.mark.parametrize("rdf", [False, True])
def test_stored_force_is_bitwise_the_rebuilt_one(n_atoms, ens, rdf):
    stored_forces_check("lj126", ens, n_atoms, rdf)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--measure"]:                   # [--measure [FILE]]: FILE receives the N = 6 arrays (odd nl: the parent's bits)
        import tempfile
        for n, e in CASES:
            print("oracle (%d, %r): %r," % (n, e, {k: float("%.3e" % v) for k, v in measure_oracle(n, e).items()}), flush=True)
        print("eval: %r" % {k: float("%.3e" % v) for k, v in measure_one_evaluation().items()}, flush=True)
        path = os.path.join(tempfile.mkdtemp(), "measure.npz")
        _worker(path)
        arrays = dict(np.load(path, allow_pickle=False))
        for n, e in CASES:
            print("frame gradient (%d, %r): %.3e," % (n, e, frame_gradient_figure(arrays, n, e)), flush=True)
            a, b = arrays[_key(n, e) + "/raw"], arrays[_key(n, e) + "/raw_fine"]
            print("histogram (%d, %r): bitwise the many-frame kernel %s" % (n, e, np.array_equal(a.view(np.uint32), b.view(np.uint32))), flush=True)
        if len(sys.argv) > 2:
            np.savez(sys.argv[2], **{k: v for k, v in arrays.items() if k.startswith("n6-")})
    else:
        _worker(sys.argv[1])
