"""reweight.Reweighting without a GPU: the weights, n_eff, the average and its parameter gradient against the float64 numpy
reference tests/reweight_ref.py (fed by tests/pair_forms_ref.py and tests/rdf_ref.py) and against central differences.

Setup of the gradient tests: F = 6 frames of 48 atoms in the 4.8 cell (rdf_ref.draw_frames; no fragile pair at the RDF's
cutoff_boundary 3.0 nor at the LJ cutoff 2.5, asserted), Lennard-Jones, kT = 1, everything in float64 on the host:
thermo.PotentialEnergy's and rdf.per_frame's torch restatements."""
import os

import numpy as np
import pytest
import torch

import pair_forms_ref as PF
import rdf_ref as R
import reweight_ref as W
from test_rdf_frames_host import BOX, frames_for, inputs, observable

TOL64 = 1e-12
N, F, KT = 48, 6, 1.0
THETA_REF = (1.0, 1.0)                   # sigma, epsilon the frames count as sampled at


def _report(line):
    print(line)
    if os.environ.get("MDG_TEST_REPORT"):
        with open(os.environ["MDG_TEST_REPORT"], "a") as fh:
            fh.write(line + "\n")


class Setup:
    def __init__(self):
        from mdgrad_amd import potentials as P
        from mdgrad_amd.system import System
        from mdgrad_amd.thermo import PotentialEnergy
        self.obs = observable(N)
        self.frames = frames_for(self.obs, N, F, seed=29)
        for x in self.frames:
            assert len(PF.fragile_pairs(x, BOX, [PF.Term("lj", 2.5)])) == 0
        mu, coeff, cut = inputs(self.obs)
        self.rows = np.stack([R.rdf_reference(self.frames[f:f + 1], BOX, mu, coeff, cut).raw for f in range(F)])   # [F, nbins]
        system = System(positions=self.frames[0].astype(np.float64), cell=BOX.astype(np.float64), masses=np.ones(N), device="cpu")
        self.lj = P.LennardJones(*THETA_REF).double()
        self.energy = PotentialEnergy.from_terms(system, [(self.lj, 2.5)])
        self.q = torch.as_tensor(self.frames, dtype=torch.float64)

    def set_theta(self, sigma, epsilon):
        with torch.no_grad():
            self.lj.sigma.fill_(sigma)
            self.lj.epsilon.fill_(epsilon)

    def reference(self, sigma, epsilon):
        """per frame (U, sU, dU/dtheta [2], its scale [2]) in float64 from pair_forms_ref"""
        term = [PF.Term("lj", 2.5, theta=(sigma, epsilon))]
        term[0].theta = (float(sigma), float(epsilon))                       # (the float64 values, not rounded to float32)
        res = [PF.evaluate(x, np.zeros_like(x), BOX, term) for x in self.frames]
        return (np.array([r.U for r in res]), np.array([r.sU for r in res]), np.stack([r.dU[0] for r in res]),
                np.stack([r.sdU[0] for r in res]))


@pytest.fixture(scope="module")
def setup():
    return Setup()


def test_uniform_weights_and_n_eff_at_theta_ref(setup):
    from mdgrad_amd.reweight import Reweighting
    setup.set_theta(*THETA_REF)
    rw = Reweighting(setup.energy, KT, setup.q)
    w = rw.weights()
    assert w.dtype == torch.float64 and w.shape == (F,)
    assert torch.equal(w, torch.full((F,), 1.0 / F, dtype=torch.float64))       # exactly: every energy difference is 0
    assert rw.n_eff() == pytest.approx(F, rel=1e-15) and not rw.stale()
    assert not rw.q_ref.requires_grad and not rw.u_ref.requires_grad
    # pooled leading dimensions: [2, 3] frames give [2, 3] weights that sum to 1 over all of them
    rw2 = Reweighting(setup.energy, KT, setup.q.reshape(2, 3, N, 3))
    assert rw2.weights().shape == (2, 3) and torch.equal(rw2.weights().reshape(-1), w) and rw2.n_frames == F
    with pytest.raises(ValueError, match="kT"):
        Reweighting(setup.energy, 0.0, setup.q)


def test_weights_against_the_reference_and_resample(setup):
    from mdgrad_amd.reweight import Reweighting
    setup.set_theta(*THETA_REF)
    rw = Reweighting(setup.energy, KT, setup.q)
    U0, sU0, _, _ = setup.reference(*THETA_REF)
    assert np.abs(rw.u_ref.numpy() - U0).max() <= TOL64 * sU0.max()
    setup.set_theta(1.004, 0.97)
    U1, sU1, _, _ = setup.reference(1.004, 0.97)
    w, want = rw.weights().detach().numpy(), W.weights(U1, U0, KT)
    # ln w carries the energies' absolute error over kT: 1e-12 of the sums of |phi|, twice
    tol = 2 * TOL64 * (sU0.max() + sU1.max()) / KT + 1e-15
    _report("weights vs reference: max |w - ref| / ref %.3e, allowed %.3e" % (np.abs(w / want - 1).max(), tol))
    assert np.abs(w / want - 1).max() <= tol
    assert 1.0 < rw.n_eff() < F and rw.n_eff() == pytest.approx(W.n_eff(want), rel=tol * 10)
    assert rw.stale(fraction=1.0) and not rw.stale(fraction=1.0 / F)
    rw.resample(setup.q[:4])                                                 # new reference at the current parameters
    assert rw.n_frames == 4 and torch.equal(rw.weights(), torch.full((4,), 0.25, dtype=torch.float64))
    assert np.abs(rw.u_ref.numpy() - U1[:4]).max() <= TOL64 * sU1.max()


def test_weights_of_any_callable_constant_shift_and_extremes():
    from mdgrad_amd.reweight import Reweighting
    q = torch.zeros(5, 3, 3)
    base = torch.tensor([0.3, -1.2, 0.8, 2.0, -0.4], dtype=torch.float64)
    state = {"shift": torch.zeros(5, dtype=torch.float64), "const": 0.0}
    energy = lambda x: base + state["shift"] + state["const"]               # noqa: E731
    rw = Reweighting(energy, 0.5, q)
    state["shift"] = torch.tensor([0.1, -0.2, 0.05, 0.0, 0.3], dtype=torch.float64)
    w = rw.weights()
    du = (base + state["shift"]) - base
    assert np.abs(w.numpy() - W.weights(du.numpy(), 0 * du.numpy(), 0.5)).max() <= 1e-15
    # a constant added to every U_f changes no weight (beyond the float64 rounding of U + const: 2^-52 |U| / kT)
    for const in (4.0, -1234.5, 1.0e6):
        state["const"] = const
        assert np.abs(rw.weights().numpy() - w.numpy()).max() <= 4 * 2.0 ** -52 * (abs(const) + 3.0) / 0.5
    state["const"] = 0.0
    # Delta U / kT = +-1e4: finite one-hot weights, n_eff = 1
    for sign in (1.0, -1.0):
        state["shift"] = torch.tensor([0.0, sign * 5000.0, 0.0, 0.0, 0.0], dtype=torch.float64)   # kT = 0.5
        w = rw.weights()
        assert torch.isfinite(w).all() and float(w.sum()) == pytest.approx(1.0, abs=1e-15)
        if sign < 0:
            assert torch.equal(w, torch.tensor([0.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64)) and rw.n_eff() == 1.0
        else:
            assert float(w[1]) == 0.0 and rw.n_eff() == pytest.approx(W.n_eff(w.numpy()), rel=1e-14)
        assert rw.stale()


def test_average_with_trailing_dimensions():
    from mdgrad_amd.reweight import Reweighting
    rng = np.random.default_rng(3)
    base = torch.as_tensor(rng.normal(size=(2, 3)))
    state = {"shift": torch.zeros(2, 3, dtype=torch.float64)}
    rw = Reweighting(lambda x: base + state["shift"], 0.7, torch.zeros(2, 3, 4, 3))
    state["shift"] = torch.as_tensor(rng.normal(size=(2, 3)))
    w = W.weights((base + state["shift"]).numpy(), base.numpy(), 0.7)
    for shape in ((2, 3), (2, 3, 7), (2, 3, 4, 5)):
        v = rng.normal(size=shape)
        out = rw.average(torch.as_tensor(v))
        assert out.shape == shape[2:] and np.abs(out.numpy() - W.average(w, v)).max() <= 1e-14
    v32 = torch.as_tensor(rng.normal(size=(2, 3, 7)), dtype=torch.float32)
    assert rw.average(v32).dtype == torch.float32
    with pytest.raises(ValueError, match="lead"):
        rw.average(torch.zeros(6, 7))


@pytest.mark.parametrize("theta", [THETA_REF, (1.003, 0.98)], ids=["at theta_ref", "away from theta_ref"])
def test_gradient_of_a_reweighted_rdf_against_the_reference(setup, theta):
    """d<raw_k>/d(sigma, epsilon) of every bin by autograd through the weights against the covariance identity evaluated in
    numpy.  Scale of a bin and parameter: sum_f w_f (|O_fk| + |<O_k>|) s_f / kT with s_f the sum over the pairs of
    |dphi/dtheta| -- what is added up -- and the allowance 1e-12 of it; for the average itself times (1 + the amplification through ln w): the weights
    themselves carry 2e-12 (sum |phi|) / kT (the gradient is held to the plain 1e-12 of its scale)."""
    from mdgrad_amd.reweight import Reweighting
    setup.set_theta(*THETA_REF)
    rw = Reweighting(setup.energy, KT, setup.q)
    setup.set_theta(*theta)
    rows = setup.obs.per_frame(setup.q)
    avg = rw.average(rows)
    assert avg.shape == (setup.obs.nbins,) and avg.dtype == torch.float64
    jac = torch.stack([torch.stack(torch.autograd.grad(avg[k], [setup.lj.sigma, setup.lj.epsilon], retain_graph=True)).reshape(2)
                       for k in range(setup.obs.nbins)]).numpy()
    U0, sU0, _, _ = setup.reference(*THETA_REF)
    U1, sU1, G, sG = setup.reference(*theta)
    w = W.weights(U1, U0, KT)
    if theta == THETA_REF:
        assert (w == 1.0 / F).all()
    want = W.gradient(w, setup.rows, G, KT)
    mean = W.average(w, setup.rows)
    scale = ((w[:, None, None] * (np.abs(setup.rows)[:, :, None] + np.abs(mean)[None, :, None]) * sG[:, None, :]).sum(0)) / KT
    amp = 1.0 + 2 * (sU0.max() + sU1.max()) / KT
    err = (np.abs(jac - want) / scale).max()
    _report("reweighted RDF gradient vs reference (%s): figure %.3e allowed %.3e" % (theta, err, TOL64 * amp))
    assert np.abs(avg.detach().numpy() - mean).max() <= TOL64 * amp * np.abs(setup.rows).max()
    assert err <= TOL64                  # (the amplification through ln w is allowed for in the average, not needed here)


def test_gradient_against_central_differences(setup):
    """The same gradient against (A(theta + h) - A(theta - h)) / 2h, A_k = <raw_k>, in float64 with h = 2e-7 (the
    truncation bound below is loose by three orders of magnitude, so the step is chosen where it is still a thousand times
    below the gradient while the roundoff, which grows as 1 / h, stays smaller still).

    Allowed error = truncation + roundoff.  Truncation: h^2 / 6 |A'''|.  With g = U'/kT etc. (derivatives with respect to the
    parameter) and cumulants under the weights, A' = -k(O, g), A'' = k(O, g, g) - k(O, g'), A''' = -k(O, g, g, g) + 3 k(O, g, g')
    - k(O, g''); for centred variables bounded by dO, a, b, c (the largest deviations over the frames of O_k, U'/kT, U''/kT,
    U'''/kT) |k(O,g,g,g)| <= 4 dO a^3, |k(O,g,g')| <= 2 dO a b ... so |A'''| <= dO (4 a^3 + 6 a b + c).  For LJ, U = 4 eps
    (sigma^12 S12 - sigma^6 S6) with S_n = sum r^-n: the sigma-derivatives are closed forms of S12, S6; in epsilon U'' = 0.
    The deviations are taken at theta and enlarged by 10 % for the interval [theta - h, theta + h].
    Roundoff: the two averages carry 2^-52 |A| each, amplified by the energies' own error in ln w, over 2h."""
    from mdgrad_amd.reweight import Reweighting
    h = 2e-7
    theta = (1.003, 0.98)
    setup.set_theta(*THETA_REF)
    rw = Reweighting(setup.energy, KT, setup.q)
    rows = setup.obs.per_frame(setup.q)
    setup.set_theta(*theta)
    avg = rw.average(rows)
    jac = torch.stack([torch.stack(torch.autograd.grad(avg[k], [setup.lj.sigma, setup.lj.epsilon], retain_graph=True)).reshape(2)
                       for k in range(setup.obs.nbins)]).numpy()
    # S12, S6 per frame from the reference's pair set
    term = [PF.Term("lj", 2.5)]
    S12, S6 = np.zeros(F), np.zeros(F)
    for f, x in enumerate(setup.frames):
        m = PF.membership(x, BOX, term)[0]
        d2 = PF._images(x, BOX, np.dtype(np.float64))[2][np.triu(m, 1)]
        S12[f], S6[f] = (d2 ** -6).sum(), (d2 ** -3).sum()
    sg, ep = theta
    dev = lambda v: 1.1 * np.abs(v - v.mean()).max() * 2 / KT                # noqa: E731  (|v_f - <v>| <= max - min <= 2 max dev)
    d_sigma = [4 * ep * (12 * sg ** 11 * S12 - 6 * sg ** 5 * S6), 4 * ep * (132 * sg ** 10 * S12 - 30 * sg ** 4 * S6),
               4 * ep * (1320 * sg ** 9 * S12 - 120 * sg ** 3 * S6)]
    d_eps = [4 * (sg ** 12 * S12 - sg ** 6 * S6), 0 * S12, 0 * S12]
    dO = 2 * np.abs(setup.rows - setup.rows.mean(0)).max(0)                   # [nbins]
    _, sU, _, _ = setup.reference(*theta)
    for p, ders in enumerate((d_sigma, d_eps)):
        a, b, c = (dev(v) for v in ders)
        trunc = h * h / 6 * dO * (4 * a ** 3 + 6 * a * b + c)
        vals = []
        for s in (+1, -1):
            th = list(theta)
            th[p] += s * h
            setup.set_theta(*th)
            with torch.no_grad():
                vals.append(rw.average(rows).numpy())
        cd = (vals[0] - vals[1]) / (2 * h)
        roundoff = 2.0 ** -52 * (1 + 4 * sU.max() / KT) * np.abs(setup.rows).max(0) * 2 / (2 * h)
        allowed = trunc + roundoff
        err = np.abs(jac[:, p] - cd)
        k = int(np.argmax(err / allowed))
        _report("central differences, parameter %d: worst bin %d |autograd - cd| %.3e, allowed %.3e (truncation %.3e, roundoff %.3e),"
                " |gradient| up to %.3e" % (p, k, err[k], allowed[k], trunc[k], roundoff[k], np.abs(jac[:, p]).max()))
        assert (err <= allowed).all()
        assert allowed.max() <= 1e-3 * np.abs(jac[:, p]).max()               # (the check is a thousand times finer than the gradient)
    setup.set_theta(*THETA_REF)
