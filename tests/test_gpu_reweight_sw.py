"""reweight.Reweighting with the three-body model on the GPU: thermo.StillingerWeberEnergy's kernel (K34) under the weights with
the per-frame angle histogram (K35) as the observable, and examples/fit_adf_reweight_sw.py end to end.

The gradient of the reweighted, un-normalised angle histogram with respect to (epsilon, sigma, lam) at theta_ref is the
covariance identity; it is compared with reweight_ref.gradient fed with the float64 U and dU/dtheta of tests/sw_ref.py and the
float64 host rows of the same frames.  Tolerance: the rule of tests/test_gpu_reweight.py for the same identity with the pair
energy -- allowed = MARGIN x the distance of the float32 host path from the float64 one (at least 2^-24), MARGIN = 10, over the
largest entry of the float64 gradient of that parameter.  40 frames of the 64-atom jittered diamond (seeds 200 ...).

Observed on an MI355X, d/d(epsilon, sigma, lam): float32 floor 7.8e-07, 9.4e-07, 1.2e-06; kernel path 8.8e-07, 6.7e-07, 1.1e-06 (the
float64 host path itself is 1.0e-07 ... 2.2e-07 from the reference: its parameters are float32)."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import reweight_ref as RW
import sw_ref as R
from test_rdf_frames_host import _report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 10.0
F, N, KT = 40, 64, 0.05
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = R.consts()


def frames40():
    xs = [R.jittered_diamond(2, 5.431, 0.3, 200 + s) for s in range(F)]
    return np.stack([x for x, _ in xs]), xs[0][1]


class Path:
    """the whole computation on one device in one dtype: frames -> weights -> reweighted angle histogram"""

    def __init__(self, frames, cell, device, dtype):
        from mdgrad_amd.interface import StillingerWeber
        from mdgrad_amd.observable import angle_distribution
        from mdgrad_amd.reweight import Reweighting
        from mdgrad_amd.system import System
        from mdgrad_amd.thermo import StillingerWeberEnergy
        system = System(positions=frames[0].astype(np.float64), cell=cell.astype(np.float64), masses=np.full(N, 28.0855),
                        device=device)
        self.model = StillingerWeber.silicon(system)
        self.energy = StillingerWeberEnergy(system, self.model)
        self.obs = angle_distribution(system, nbins=32, angle_range=(0.0, math.pi), cutoff=3.0, keep_angles=False)
        self.q = torch.as_tensor(frames).to(device=device, dtype=dtype)
        self.rw = Reweighting(self.energy, KT, self.q)
        with torch.no_grad():
            self.rows = self.obs.per_frame(self.q)

    def gradients(self):
        """[32, 3]: d<raw_b>/d(epsilon, sigma, lam) at theta_ref, and <raw>"""
        avg = self.rw.average(self.rows).double()
        ps = [self.model.epsilon, self.model.sigma, self.model.lam]
        G = torch.stack([torch.cat(torch.autograd.grad(avg[b], ps, retain_graph=True)) for b in range(avg.shape[0])])
        return G.double().cpu().numpy(), avg.detach().cpu().numpy()


def test_gradient_of_a_reweighted_adf_is_the_covariance_identity():
    from mdgrad_amd import ops
    frames, cell = frames40()
    dev32 = Path(frames, cell, DEV, torch.float32)
    cpu32, cpu64 = Path(frames, cell, "cpu", torch.float32), Path(frames, cell, "cpu", torch.float64)
    # the reference: float64 U and dU/dtheta per frame, the float64 host rows, uniform weights at theta_ref
    th = [float(p.detach()) for p in (cpu64.model.epsilon, cpu64.model.sigma, cpu64.model.lam)]
    dU = []
    for x in frames:
        lst = R.pairs_and_triplets(x, cell, K["a"] * th[1])
        dU.append(R.evaluate(x, th, lst, cell, K)["dth"].numpy())
    w = np.full(F, 1.0 / F)
    want = RW.gradient(w, cpu64.rows.numpy(), np.stack(dU), KT)                      # [32, 3]
    ops.SWFramesFn.last_route = None
    calls = []
    real = ops.sw_eval
    ops.sw_eval = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        G, avg = dev32.gradients()
    finally:
        ops.sw_eval = real
    # no adjoint and no force kernel: the frames are detached, the backward pass is the weighted sum of the emitted dU/dtheta
    assert ops.SWFramesFn.last_route == "theta" and not calls and not dev32.rw.q_ref.requires_grad
    assert torch.equal(dev32.rw.weights().detach(), torch.full((F,), 1.0 / F, dtype=torch.float64, device=DEV))
    G32, _ = cpu32.gradients()
    G64, avg64 = cpu64.gradients()
    bad = []
    for k, name in enumerate(("d/depsilon", "d/dsigma", "d/dlam")):
        scale = np.abs(want[:, k]).max()
        host = float(np.abs(G64[:, k] - want[:, k]).max() / scale)
        floor = max(float(np.abs(G32[:, k] - want[:, k]).max() / scale), 2.0 ** -24)
        err = float(np.abs(G[:, k] - want[:, k]).max() / scale)
        _report("reweighted ADF on the device, %-10s float64 host path %.3e  floor %.3e  allowed %.3e  kernel %.3e%s"
                % (name, host, floor, MARGIN * floor, err, "" if err <= MARGIN * floor else "   <-- FAILS"))
        assert host <= 1e-6, "the float64 host path is the identity itself (float32 parameters)"
        if not err <= MARGIN * floor:
            bad.append((name, err, MARGIN * floor))
    assert not bad, bad
    assert np.abs(avg - avg64).max() <= 2e-6 * np.abs(avg64).max()


def example():
    spec = importlib.util.spec_from_file_location("fit_adf_reweight_sw", os.path.join(ROOT, "examples", "fit_adf_reweight_sw.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_recovers_lam_end_to_end():
    """examples/fit_adf_reweight_sw.main with --replicas 8 --epochs 12 --frames 50 --burn 20 --seed 0 (defaults otherwise: the
    64-molecule mW box, lr 0.3, resample below 0.9 F, start at lam = 18; target lam = 23.15).

    Observed on an MI355X: loss 4.731e-04 -> 1.554e-05 (it jumps after a resample, 1.15e-03 at epoch 4: every sample is 30
    frames of 8 replicas), lam 18.300 -> 21.098, 3 resamples, n_eff between 220 and 240 of 240 frames; about 1 s."""
    hist = example().main(["--replicas", "8", "--epochs", "12", "--frames", "50", "--burn", "20", "--seed", "0", "--device", DEV])
    first, last = hist[0], hist[-1]
    for k, h in enumerate(hist):
        _report("fit_adf_reweight_sw: epoch %2d  loss %.4e  lam %.3f  n_eff %.1f  resamples %d" % ((k,) + tuple(h)))
    assert all(np.isfinite(h).all() for h in hist)
    assert last[0] < first[0]
    assert abs(last[1] - 23.15) < abs(18.0 - 23.15) and last[1] > 18.0
