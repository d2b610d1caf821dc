"""reweight.Reweighting on the GPU: thermo.PotentialEnergy's and rdf.per_frame's kernels under the weights, and the example
examples/fit_rdf_reweight.py end to end.

The parameter gradient of a reweighted RDF is compared with the float64 host path of the same computation on the same frames;
allowed = MARGIN x the distance of the float32 host path from the float64 one (at least 2^-24), MARGIN = 10, over the largest
entry of the float64 gradient of that parameter.  16 frames of 108 atoms (rdf_ref.draw_frames; no fragile pair at the RDF's
cutoff_boundary nor at the LJ cutoff, asserted), Lennard-Jones at (1.003, 0.98) with frames that count as sampled at (1, 1)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import pair_forms_ref as PF
from test_rdf_frames_host import BOX, _report, frames_for, observable

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 10.0
N, F, KT = 108, 16, 1.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Path:
    """the whole computation on one device in one dtype: frames -> weights -> reweighted g(r) -> three linear functionals"""

    def __init__(self, frames, device, dtype):
        from mdgrad_amd import potentials as P
        from mdgrad_amd.reweight import Reweighting
        from mdgrad_amd.system import System
        from mdgrad_amd.thermo import PotentialEnergy
        self.obs = observable(N, device=device)
        system = System(positions=frames[0].astype(np.float64), cell=BOX.astype(np.float64), masses=np.ones(N), device=device)
        self.lj = P.LennardJones(1.0, 1.0).to(dtype)
        self.energy = PotentialEnergy.from_terms(system, [(self.lj, 2.5)])
        self.q = torch.as_tensor(frames).to(device=device, dtype=dtype)
        self.rw = Reweighting(self.energy, KT, self.q)
        with torch.no_grad():
            self.rows = self.obs.per_frame(self.q)
        k = torch.arange(100, dtype=torch.float64)
        self.c = torch.stack([torch.linspace(-1, 1, 100, dtype=torch.float64), torch.cos(k / 7.0), (k == 18).double()]).to(device)

    def set_theta(self, sigma, epsilon):
        with torch.no_grad():
            self.lj.sigma.fill_(sigma)
            self.lj.epsilon.fill_(epsilon)

    def gradients(self):
        """[3, 2]: d(c_j . g)/d(sigma, epsilon), g the reweighted normalised RDF"""
        g = self.obs.normalise(self.rw.average(self.rows))[2].double()
        out = [torch.stack(torch.autograd.grad((cj * g).sum(), [self.lj.sigma, self.lj.epsilon], retain_graph=True)).reshape(2)
               for cj in self.c]
        return torch.stack(out).double().cpu().numpy(), g.detach().cpu().numpy()


@pytest.fixture(scope="module")
def frames():
    obs = observable(N)
    fr = frames_for(obs, N, F, seed=31)
    for x in fr:
        assert len(PF.fragile_pairs(x, BOX, [PF.Term("lj", 2.5)])) == 0
    return fr


def test_weights_are_exactly_uniform_at_theta_ref(frames):
    p = Path(frames, DEV, torch.float32)
    w = p.rw.weights()
    assert w.dtype == torch.float64 and w.is_cuda
    assert torch.equal(w, torch.full((F,), 1.0 / F, dtype=torch.float64, device=DEV))
    assert p.rw.n_eff() == pytest.approx(F, rel=1e-15) and not p.rw.stale()
    # pooled replicas: [R, T] frames
    from mdgrad_amd.reweight import Reweighting
    rw2 = Reweighting(p.energy, KT, p.q.reshape(4, 4, N, 3))
    assert rw2.weights().shape == (4, 4) and torch.equal(rw2.weights().reshape(-1), w)
    assert rw2.average(p.rows.reshape(4, 4, 100)).shape == (100,)


def test_gradient_of_a_reweighted_rdf_against_the_float64_host_path(frames):
    from mdgrad_amd import ops
    dev32, cpu32, cpu64 = Path(frames, DEV, torch.float32), Path(frames, "cpu", torch.float32), Path(frames, "cpu", torch.float64)
    for p in (dev32, cpu32, cpu64):
        p.set_theta(1.003, 0.98)
    ops.EnergyFramesFn.last_route = None
    G, g = dev32.gradients()
    # the backward pass ran no position kernel: the frames are detached and the op took the parameters-only sweep
    assert dev32.rw.q_ref.grad is None and not dev32.rw.q_ref.requires_grad and ops.EnergyFramesFn.last_route == "theta"
    G32, g32 = cpu32.gradients()
    G64, g64 = cpu64.gradients()
    w = dev32.rw.weights().detach().cpu().numpy()
    assert w.max() / w.min() > 1.5, "the weights are meant to be far from uniform here"
    bad = []
    for what, got, r32, r64, scale in (("g(r)", g, g32, g64, np.abs(g64).max()),
                                       ("d/dsigma", G[:, 0], G32[:, 0], G64[:, 0], np.abs(G64[:, 0]).max()),
                                       ("d/depsilon", G[:, 1], G32[:, 1], G64[:, 1], np.abs(G64[:, 1]).max())):
        floor = max(float(np.abs(r32 - r64).max() / scale), 2.0 ** -24)
        err = float(np.abs(got - r64).max() / scale)
        _report("reweighted RDF on the device, %-10s floor %.3e  allowed %.3e  kernel %.3e%s"
                % (what, floor, MARGIN * floor, err, "" if err <= MARGIN * floor else "   <-- FAILS"))
        if not err <= MARGIN * floor:
            bad.append((what, err, MARGIN * floor))
    assert not bad, bad


def example():
    spec = importlib.util.spec_from_file_location("fit_rdf_reweight", os.path.join(ROOT, "examples", "fit_rdf_reweight.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_recovers_the_parameters_end_to_end():
    """examples/fit_rdf_reweight.main with --replicas 16 --epochs 40 --frames 60 --seed 0 (defaults otherwise: lr 0.002, resample
    below 0.9 F, start at sigma 0.92, epsilon 0.8; target sigma = epsilon = 1).

    Observed on an MI355X (the same figures in two runs): loss 0.42337 -> 0.28340, sigma 0.9200 -> 0.9918, epsilon 0.8000 ->
    0.8809, 19 resamples in the 40 steps (n_eff of the last step: 640.0 of 640 frames, i.e. right after a resample); about 2 s."""
    hist = example().main(["--replicas", "16", "--epochs", "40", "--frames", "60", "--seed", "0", "--device", DEV])
    first, last = hist[0], hist[-1]
    _report("fit_rdf_reweight: loss %.5f -> %.5f, sigma %.4f -> %.4f, epsilon %.4f -> %.4f, resamples %d, n_eff of the last step %.1f"
            % (first[0], last[0], 0.92, last[1], 0.8, last[2], last[4], last[3]))
    assert last[0] < first[0]
    assert abs(last[1] - 1.0) < abs(0.92 - 1.0) and abs(last[2] - 1.0) < abs(0.8 - 1.0)
    assert last[4] >= 1
    assert all(np.isfinite(h).all() for h in hist)


def test_example_with_the_langevin_sampler():
    """The estimator is indifferent to the thermostat: the same fit sampled with md.Langevin (BAOAB, generic path), --thermostat
    langevin --replicas 8 --epochs 12 --frames 50 --seed 0: both parameters move towards the target and nothing is non-finite.

    Observed on an MI355X: sigma 0.9200 -> 0.9399, epsilon 0.8000 -> 0.8197, 5 resamples; the loss went 0.31347 -> 0.43088 -- over
    its first dozen steps it rises with the default sampler too (0.42 -> 0.54 at step 9, then down to 0.28 at step 40): the
    target is the RDF of 30 frames after a 20-frame burn-in from the lattice, and so is every sample.  No assertion on it."""
    hist = example().main(["--thermostat", "langevin", "--replicas", "8", "--epochs", "12", "--frames", "50", "--seed", "0",
                           "--device", DEV])
    first, last = hist[0], hist[-1]
    _report("fit_rdf_reweight --thermostat langevin: loss %.5f -> %.5f, sigma 0.9200 -> %.4f, epsilon 0.8000 -> %.4f, resamples %d"
            % (first[0], last[0], last[1], last[2], last[4]))
    assert all(np.isfinite(h).all() for h in hist)
    assert abs(last[1] - 1.0) < abs(0.92 - 1.0) and abs(last[2] - 1.0) < abs(0.8 - 1.0)
