"""reweight.Reweighting with the embedded-atom models on the GPU: thermo.EAMEnergy's kernels (K36, K37) under the weights with the
per-frame RDF rows (K32) as the observable, and examples/fit_rdf_reweight_eam.py end to end in both of its modes.

The gradient of the reweighted, un-normalised RDF rows with respect to (epsilon, a, c) of SuttonChen and with respect to the
embedding nodes of the tabulated EAM at theta_ref is the covariance identity; it is compared with reweight_ref.gradient fed with
the float64 U and dU/dtheta of tests/eam_ref.py / tests/eam_table_ref.py and the float64 host rows of the same frames.
Tolerance: the rule of tests/test_gpu_reweight_sw.py for the same identity -- allowed = MARGIN x the distance of the float32
host path from the float64 one (at least 2^-24), MARGIN = 10, over the largest entry of the float64 gradient of that parameter
(of the whole block for the nodes).  40 frames of the 108-atom jittered copper box (seeds 300 ...).

Observed on an MI355X, d/d(epsilon, a, c): float32 floor 1.5e-05, 1.6e-05, 1.7e-05; kernel path 1.1e-06, 6.1e-07, 1.0e-06;
d/d embed_nodes: floor 2.8e-05, kernel path 9.5e-06 (the float64 host path itself is 1.6e-08 ... 3.4e-08 from the reference: its
parameters are float32).  That the kernel path is closer than the float32 host path is expected, not measured apart: K37's
weighted sum over the frames runs in double and K36b adds the node terms as integers, while the float32 host path rounds every
frame's term to float32 before a covariance cancels most of it."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import eam_ref as SC
import eam_table_ref as R
import reweight_ref as RW
from test_rdf_frames_host import _report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 10.0
F, N, KT, RC, NB = 40, 108, 0.0862, 5.2, 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CU = SC.PUBLISHED["copper"]


def frames40():
    xs = [SC.jittered_fcc(3, 3.61, 0.15, 300 + s) for s in range(F)]
    return np.stack([x for x, _ in xs]), xs[0][1]


class Path:
    """the whole computation on one device in one dtype: frames -> weights -> reweighted RDF rows"""

    def __init__(self, frames, cell, device, dtype, tabulated):
        from mdgrad_amd.interface import EAM, SuttonChen
        from mdgrad_amd.observable import rdf
        from mdgrad_amd.reweight import Reweighting
        from mdgrad_amd.system import System
        from mdgrad_amd.thermo import EAMEnergy
        system = System(positions=frames[0].astype(np.float64), cell=cell.astype(np.float64), masses=np.full(N, 63.546),
                        device=device)
        if tabulated:
            self.model = EAM.from_sutton_chen(system, "copper", cutoff=RC, r_min=1.8, n_r=64, n_rho=64, trainable=("embed",))
            self.params = [self.model.embed_nodes]
        else:
            eps, a, c, n, m = CU
            self.model = SuttonChen(system, eps, a, c, n, m, RC)
            self.params = [self.model.epsilon, self.model.a, self.model.c]
        self.energy = EAMEnergy(system, self.model)
        self.obs = rdf(system, nbins=NB, r_range=(2.0, RC))
        self.q = torch.as_tensor(frames).to(device=device, dtype=dtype)
        self.rw = Reweighting(self.energy, KT, self.q)
        with torch.no_grad():
            self.rows = self.obs.per_frame(self.q)

    def gradients(self):
        """[NB, P]: d<raw_b>/dparams at theta_ref, and <raw>"""
        avg = self.rw.average(self.rows).double()
        G = torch.stack([torch.cat([g.reshape(-1) for g in torch.autograd.grad(avg[b], self.params, retain_graph=True)])
                         for b in range(avg.shape[0])])
        return G.double().cpu().numpy(), avg.detach().cpu().numpy()


@pytest.mark.parametrize("kind", ["sutton-chen", "tabulated"])
def test_gradient_of_a_reweighted_rdf_is_the_covariance_identity(kind):
    from mdgrad_amd import ops
    tab = kind == "tabulated"
    frames, cell = frames40()
    dev32 = Path(frames, cell, DEV, torch.float32, tab)
    cpu32, cpu64 = Path(frames, cell, "cpu", torch.float32, tab), Path(frames, cell, "cpu", torch.float64, tab)
    # the reference: float64 dU/dtheta per frame, the float64 host rows, uniform weights at theta_ref
    m = cpu64.model
    dU = []
    for x in frames:
        if tab:
            lst = R.pairs(x, cell, RC)
            ref = R.evaluate(x, R.tables_of(m), lst, cell, m.types.cpu().long(), R.grid_of(m), pin=m.pin_cutoff)
            dU.append(ref["gtab"].numpy()[-m.embed_nodes.numel():])
        else:
            lst = SC.pairs(x, cell, RC)
            dU.append(SC.evaluate(x, [float(p.detach()) for p in cpu64.params], lst, cell, SC.consts(m.n, m.m, RC, "force"))["dth"].numpy())
    want = RW.gradient(np.full(F, 1.0 / F), cpu64.rows.numpy(), np.stack(dU), KT)        # [NB, P]
    fn = ops.EAMTableFramesFn if tab else ops.EAMFramesFn
    fn.last_route = None
    calls = []
    real = (ops.eam_table_eval, ops.eam_eval)
    ops.eam_table_eval = lambda *a, **k: calls.append(1) or real[0](*a, **k)
    ops.eam_eval = lambda *a, **k: calls.append(1) or real[1](*a, **k)
    try:
        G, avg = dev32.gradients()
    finally:
        ops.eam_table_eval, ops.eam_eval = real
    # no adjoint and no force kernel: the frames are detached
    assert fn.last_route == ("nodes" if tab else "theta") and not calls and not dev32.rw.q_ref.requires_grad
    assert torch.equal(dev32.rw.weights().detach(), torch.full((F,), 1.0 / F, dtype=torch.float64, device=DEV))
    G32, _ = cpu32.gradients()
    G64, avg64 = cpu64.gradients()
    blocks = [("d/d embed_nodes", slice(None))] if tab else [("d/depsilon", slice(0, 1)), ("d/da", slice(1, 2)), ("d/dc", slice(2, 3))]
    bad = []
    for name, k in blocks:
        scale = np.abs(want[:, k]).max()
        host = float(np.abs(G64[:, k] - want[:, k]).max() / scale)
        floor = max(float(np.abs(G32[:, k] - want[:, k]).max() / scale), 2.0 ** -24)
        err = float(np.abs(G[:, k] - want[:, k]).max() / scale)
        _report("reweighted RDF on the device (%s), %-16s float64 host path %.3e  floor %.3e  allowed %.3e  kernel %.3e%s"
                % (kind, name, host, floor, MARGIN * floor, err, "" if err <= MARGIN * floor else "   <-- FAILS"))
        assert host <= 1e-6, "the float64 host path is the identity itself (float32 parameters)"
        if not err <= MARGIN * floor:
            bad.append((name, err, MARGIN * floor))
    assert not bad, bad
    assert np.abs(avg - avg64).max() <= 2e-6 * np.abs(avg64).max()


def example():
    spec = importlib.util.spec_from_file_location("fit_rdf_reweight_eam", os.path.join(ROOT, "examples", "fit_rdf_reweight_eam.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ARGS = ["--replicas", "4", "--epochs", "10", "--frames", "40", "--burn", "15", "--seed", "0", "--device", DEV]


def test_example_sutton_chen_end_to_end():
    """examples/fit_rdf_reweight_eam.main with ARGS (defaults otherwise: lr 0.003, off 0.05, resample below 0.9 F; start at
    epsilon = 1.30011e-2, a = 3.4295; target a = 3.61).

    Observed on an MI355X: loss 2.484e-01 -> 4.805e-02 (one rise, 1.110e-01 -> 1.124e-01 at epoch 6), a 3.4403 -> 3.5360, epsilon
    1.30382e-2 -> 1.33671e-2 (barely determined, as in examples/fit_rdf_sc.py), a resample after every epoch (a step of 0.011 in
    the stiff a drops n_eff below 90 of the 100 frames); the four tests of this file took 6 s together."""
    hist = example().main(ARGS)
    for k, h in enumerate(hist):
        _report("fit_rdf_reweight_eam: epoch %2d  loss %.4e  epsilon %.5e  a %.4f  n_eff %.1f  resamples %d" % ((k,) + tuple(h)))
    assert all(np.isfinite(h).all() for h in hist)
    assert hist[-1][0] < hist[0][0]
    assert abs(hist[-1][2] - 3.61) < abs(3.61 * 0.95 - 3.61)


def test_example_tabulated_end_to_end():
    """examples/fit_rdf_reweight_eam.main with ARGS + --tabulated: the embedding nodes fitted to the same target.

    Observed on an MI355X: loss 2.484e-01 -> 1.681e-01, falling at every epoch, the largest change of a node entry 1.5e-3 -> 1.45e-2,
    3 resamples, n_eff between 93.4 and 100 of 100 frames."""
    hist = example().main(ARGS + ["--tabulated"])
    for k, h in enumerate(hist):
        _report("fit_rdf_reweight_eam --tabulated: epoch %2d  loss %.4e  max |d embed| %.3e  n_eff %.1f  resamples %d" % ((k,) + tuple(h)))
    assert all(np.isfinite(h).all() for h in hist)
    assert hist[-1][0] < hist[0][0] and hist[-1][1] > 0.0
