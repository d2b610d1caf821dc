"""reweight.Reweighting with the bond-order model on the GPU: thermo.TersoffEnergy's kernel (K38) under the weights with the
per-frame angle histogram (K35) as the observable, and examples/fit_adf_reweight_tersoff.py end to end.

The gradient of the reweighted, un-normalised angle histogram with respect to (A, B, h) at theta_ref is the covariance
identity; it is compared with reweight_ref.gradient fed with the float64 U and dU/dtheta of tests/tersoff_ref.py and the float64
host rows of the same frames.  Tolerance: the rule of tests/test_gpu_reweight_sw.py for the same identity -- allowed = MARGIN x
the distance of the float32 host path from the float64 one (at least 2^-24), MARGIN = 10, over the largest entry of the float64
gradient of that parameter.  40 frames of the 64-atom jittered diamond (tersoff_frames_cases.si_frames), kT = 0.05.

Observed on an MI355X, d/d(A, B, h): float32 floor 1.0e-06, 8.0e-06, 4.8e-05; kernel path 6.0e-07, 3.4e-06, 6.9e-07 (the
float64 host path itself is about 3e-08 from the reference: its parameters are float32 and are cast once)."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import reweight_ref as RW
import tersoff_frames_cases as TC
from test_rdf_frames_host import _report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 10.0
F, N, KT = 40, 64, 0.05
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Path:
    """the whole computation on one device in one dtype: frames -> weights -> reweighted angle histogram"""

    def __init__(self, case, device, dtype):
        from mdgrad_amd.observable import angle_distribution
        from mdgrad_amd.reweight import Reweighting
        from mdgrad_amd.system import System
        system = System(positions=case.frames[0].astype(np.float64), cell=case.cell.astype(np.float64),
                        masses=np.full(N, 28.0855), device=device)
        self.model, self.energy = case.modules(system)
        self.obs = angle_distribution(system, nbins=32, angle_range=(0.0, math.pi), cutoff=3.0, keep_angles=False)
        self.q = torch.as_tensor(case.frames).to(device=device, dtype=dtype)
        self.rw = Reweighting(self.energy, KT, self.q)
        with torch.no_grad():
            self.rows = self.obs.per_frame(self.q)

    def gradients(self):
        """[32, 3]: d<raw_b>/d(A, B, h) at theta_ref, and <raw>"""
        avg = self.rw.average(self.rows).double()
        ps = [self.model.A, self.model.B, self.model.h]
        G = torch.stack([torch.cat(torch.autograd.grad(avg[b], ps, retain_graph=True)) for b in range(avg.shape[0])])
        return G.double().cpu().numpy(), avg.detach().cpu().numpy()


def test_gradient_of_a_reweighted_adf_is_the_covariance_identity():
    from mdgrad_amd import ops
    case = TC.si_frames(F)
    dev32 = Path(case, DEV, torch.float32)
    cpu32, cpu64 = Path(case, "cpu", torch.float32), Path(case, "cpu", torch.float64)
    # the reference: float64 U and dU/dtheta per frame, the float64 host rows, uniform weights at theta_ref
    dU = case.reference(cpu64.model)["dth"].numpy()
    w = np.full(F, 1.0 / F)
    want = RW.gradient(w, cpu64.rows.numpy(), dU, KT)                                # [32, 3]
    ops.TersoffFramesFn.last_route = None
    calls = []
    real = ops.tersoff_eval
    ops.tersoff_eval = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        G, avg = dev32.gradients()
    finally:
        ops.tersoff_eval = real
    # no adjoint and no force kernel: the frames are detached, the backward pass is the weighted sum of the emitted dU/dtheta
    assert ops.TersoffFramesFn.last_route == "theta" and not calls and not dev32.rw.q_ref.requires_grad
    assert torch.equal(dev32.rw.weights().detach(), torch.full((F,), 1.0 / F, dtype=torch.float64, device=DEV))
    G32, _ = cpu32.gradients()
    G64, avg64 = cpu64.gradients()
    bad = []
    for k, name in enumerate(("d/dA", "d/dB", "d/dh")):
        scale = np.abs(want[:, k]).max()
        host = float(np.abs(G64[:, k] - want[:, k]).max() / scale)
        floor = max(float(np.abs(G32[:, k] - want[:, k]).max() / scale), 2.0 ** -24)
        err = float(np.abs(G[:, k] - want[:, k]).max() / scale)
        _report("reweighted ADF on the device, %-6s float64 host path %.3e  floor %.3e  allowed %.3e  kernel %.3e%s"
                % (name, host, floor, MARGIN * floor, err, "" if err <= MARGIN * floor else "   <-- FAILS"))
        assert host <= 1e-6, "the float64 host path is the identity itself (float32 parameters)"
        if not err <= MARGIN * floor:
            bad.append((name, err, MARGIN * floor))
    assert not bad, bad
    assert np.abs(avg - avg64).max() <= 2e-6 * np.abs(avg64).max()


def example():
    spec = importlib.util.spec_from_file_location("fit_adf_reweight_tersoff",
                                                  os.path.join(ROOT, "examples", "fit_adf_reweight_tersoff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_moves_h_towards_the_target_end_to_end():
    """examples/fit_adf_reweight_tersoff.main with --replicas 8 --epochs 12 --frames 50 --burn 20 --seed 0 (defaults
    otherwise: the 64-atom silicon box at 1200 K, dt 0.2, lr 0.01, resample below 0.9 F, start at h = -0.45; target
    h = -0.59825).

    Observed on an MI355X: loss 7.782e-04 -> 2.283e-04 (it jumps after a resample, 8.13e-04 at epoch 3: every sample is 30
    frames of 8 replicas), h -0.46000, -0.46999, -0.47997, -0.48997, -0.50001, -0.51003, -0.51982, -0.52937, -0.53868,
    -0.54773, -0.55627, -0.56437 after the twelve epochs, 3 resamples, n_eff between 219 and 240 of 240 frames; about 5 s."""
    mod = example()
    hist = mod.main(["--replicas", "8", "--epochs", "12", "--frames", "50", "--burn", "20", "--seed", "0", "--device", DEV])
    first, last = hist[0], hist[-1]
    for k, h in enumerate(hist):
        _report("fit_adf_reweight_tersoff: epoch %2d  loss %.4e  h %.5f  n_eff %.1f  resamples %d" % ((k,) + tuple(h)))
    assert all(np.isfinite(h).all() for h in hist)
    assert last[0] < first[0]
    assert abs(last[1] - mod.H_TRUE) < abs(-0.45 - mod.H_TRUE)
