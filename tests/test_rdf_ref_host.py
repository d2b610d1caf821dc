"""CPU-only: tests/rdf_ref.py, the float64 reference of the RDF kernels, pinned four ways -- to the reference project's
recorded results (tests/golden/rdf.npz), to central finite differences, to oracle.rdf_raw_oracle on float64 tensors, and each
variant model to the exact sum -- and every input of tests/test_gpu_rdf_ref.py built and checked, so that a bad seed or a
case that misses its edge is found here and not on the GPU."""
import numpy as np
import pytest
import torch

import oracle as O
import rdf_ref as R
from conftest import load_golden


def _golden_inputs():
    g = load_golden("rdf")
    mu = torch.linspace(0.75, float(g["bins"][-1]), 100).numpy()
    return g, mu, float(-0.5 / float(mu[1] - mu[0]) ** 2)


def _normalised(raw, vol_bins, V, upstream_of_g):
    """count, g(r) and dL/d raw of rdf.forward (observable.py:71-76): count = raw / sum raw, g = count V / vol_bins."""
    S = raw.sum()
    count = raw / S
    gr = count * V / vol_bins
    c = upstream_of_g(gr) * V / vol_bins                     # dL/d count
    return count, gr, c / S - (c * raw).sum() / S ** 2


def test_golden_of_the_reference_project():
    """count, g and grad_xyz of 4 frames x 108 atoms, and the species-selected single frame (40 bins, width 0.07), as the
    reference project recorded them in float32: within a few float32 roundings of the float64 reference."""
    g, mu, coeff = _golden_inputs()
    first = R.rdf_reference(g["xyz"], g["cell"], mu, coeff, 3.0)
    count, gr, g_raw = _normalised(first.raw, g["vol_bins"].astype(np.float64), float(g["V"]), lambda gr: g["wgt"].astype(np.float64))
    ref = R.rdf_reference(g["xyz"], g["cell"], mu, coeff, 3.0, g_raw.astype(np.float32))
    assert np.abs(count - g["count"]).max() <= 2e-6 * count.max()
    assert np.abs(gr - g["g"]).max() <= 2e-6 * gr.max()
    # (g_raw is rounded to float32 on the way in: 6e-8 relative per bin)
    assert np.abs(ref.g_xyz - g["grad_xyz"]).max() <= 2e-5 * np.abs(g["grad_xyz"]).max()
    assert len(ref.fragile) == 0 or ref.fragile.shape[1] == 3
    # species-selected, explicit width, one frame, loss sum g^2
    mu2 = torch.linspace(0.5, float(g["sel_bins"][-1]), 40).numpy()
    c2 = -0.5 / 0.07 ** 2
    it = (g["idx_a"].tolist(), g["idx_b"].tolist())
    b = g["sel_bins"].astype(np.float64)
    vb, V = 4 * np.pi / 3 * (b[1:] ** 3 - b[:-1] ** 3), 4 / 3 * np.pi * 2.2 ** 3
    x1 = g["xyz"][:1]
    sel = R.rdf_reference(x1, g["cell"], mu2, c2, 2.7, index_tuple=it)
    count, gr, g_raw = _normalised(sel.raw, vb, V, lambda gr: 2 * gr)
    assert np.abs(count - g["sel_count"]).max() <= 2e-6 * count.max()
    assert np.abs(gr - g["sel_g"]).max() <= 2e-6 * gr.max()
    # the upstream gradient is passed in float64 here through two float32 halves: g_xyz is linear in it
    hi = g_raw.astype(np.float32)
    lo = (g_raw - hi).astype(np.float32)
    gx = R.rdf_reference(x1, g["cell"], mu2, c2, 2.7, np.stack([hi, lo]), index_tuple=it).g_xyz.sum(0)[0]
    assert np.abs(gx - g["sel_grad"]).max() <= 2e-5 * np.abs(g["sel_grad"]).max()
    # the mask form of the same selection
    m = R.pair_mask(108, index_tuple=it)
    assert np.array_equal(R.rdf_reference(x1, g["cell"], mu2, c2, 2.7, mask=m).raw, sel.raw)


@pytest.mark.parametrize("tri", [False, True])
def test_central_finite_differences(tri):
    """g_xyz against (L(x + h e) - L(x - h e)) / 2h of L = sum_k g_k raw_k on float32-representable displacements, for 40
    coordinates of 2 frames x 24 atoms, h = 2^-12.  The truncation is h^2 L''' / 6 with |L'''| <= 3 |L'| / sigma^2 for
    Gaussians of width sigma: allowed h^2 / (2 sigma^2) = 9.5e-5 of the largest component."""
    g, mu, coeff = _golden_inputs()
    cell = np.array(R.TRI_CELL, np.float32) if tri else g["cell"]
    cut = 2.3 if tri else 3.0
    x = (g["xyz"][:2, :24].astype(np.float64)).round(3).astype(np.float32)
    w = np.linspace(-1, 1, 100, dtype=np.float32)
    ref = R.rdf_reference(x, cell, mu, coeff, cut, w)
    assert len(ref.fragile) == 0
    rng = np.random.default_rng(3)
    h = np.float32(2.0 ** -12)
    worst = 0.0
    for _ in range(40):
        f, a, c = rng.integers(2), rng.integers(24), rng.integers(3)
        vals = []
        for sgn in (1, -1):
            y = x.copy()
            y[f, a, c] += sgn * h
            vals.append(float(R.rdf_reference(y, cell, mu, coeff, cut).raw @ w.astype(np.float64)))
        step = float(np.float32(x[f, a, c] + h)) - float(np.float32(x[f, a, c] - h))
        worst = max(worst, abs((vals[0] - vals[1]) / step - ref.g_xyz[f, a, c]))
    print("finite differences: worst %.3e of %.3e" % (worst, np.abs(ref.g_xyz).max()))
    assert worst <= float(h) ** 2 * abs(coeff) * np.abs(ref.g_xyz).max()            # coeff = -1 / (2 sigma^2)
    assert (ref.A >= np.abs(ref.g_xyz).max(-1) * (1 - 1e-12)).all(), "|g| <= sum |dL/dd| over the atom's pairs"


@pytest.mark.parametrize("tri", [False, True])
def test_oracle_on_float64_tensors(tri):
    """raw and its gradient against oracle.rdf_raw_oracle (torch, the reference project's formulas) run on float64 tensors:
    the same float32 centres, cutoff end + 0.5 = 3.0, and width 2^-6 so that coeff = -2048 is what a kernel would receive."""
    g, mu, _ = _golden_inputs()
    cell = np.array(R.TRI_CELL, np.float32) if tri else g["cell"]
    x = g["xyz"][:3, :60]
    w = np.linspace(-1, 1, 100, dtype=np.float32)
    xo = torch.tensor(x).double().requires_grad_(True)
    raw_o = O.rdf_raw_oracle(xo, torch.tensor(cell).double(), 100, (0.75, 2.5), width=2.0 ** -6)
    (gx_o,) = torch.autograd.grad((raw_o * torch.tensor(w).double()).sum(), xo)
    ref = R.rdf_reference(x, cell, mu, -2048.0, 3.0, w)
    assert np.abs(ref.raw - raw_o.detach().numpy()).max() <= 1e-12 * ref.raw.max()
    assert np.abs(ref.g_xyz - gx_o.numpy()).max() <= 1e-11 * np.abs(gx_o.numpy()).max()


# ------------------------------------------------------------------------------------------------ the variant models
def _small(case, n_frames=96):
    """The case's own inputs cut to a few frames: cheap enough for the CPU suite."""
    import copy
    c = copy.copy(case)
    c._refs = {"frames": (case.frames()[0][:n_frames], 0)}
    return c


MODEL_CASES = ["half/table R=6", "lane/table R=11", "lane/table R=11 triclinic", "lane/frame R=6 width 0.4",
               "lane/frame R=11 500 centres", "fine/table 65 atoms masked", "low and high edge", "cell sweep"]


@pytest.mark.parametrize("name", MODEL_CASES)
def test_models_against_the_exact_sum(name):
    """Every variant model in float64 against the exact float64 sum on 96 frames of the case; floor and model_gap are
    printed per quantity.  Asserted: the forward models stay within what rdf.hip documents for them -- the fine
    histogram's per-term bound of 1.1e-5 three widths out times the < 3 centres' worth of pairs that reach a bin, 3e-5 of
    the largest bin (the lane kernels' left-out terms, "a relative 3e-7 of a bin's count", are far inside) --; the backward models are finite and agree with the exact gradient to 1e-3 of an atom's scale with
    linspace weights (a model that restated another kernel would be off by O(1)).  The Hermite table's own stated bound is
    asserted in test_hermite_table_is_below_2e6_of_a_unit_contribution."""
    case = _small(R.BY_NAME[name])
    route, fwd, bwd, model = R.plan_of(case)
    assert model is not None and route[0] == case.expect[0]
    al = case.allowances(model)
    for q, (floor, gap) in al.items():
        print("%-34s %-8s floor %.3e  model_gap %.3e" % (name, q, floor, gap))
        assert np.isfinite(floor) and np.isfinite(gap)
    assert al["raw"][1] <= 3e-5
    assert al["linspace"][1] <= 1e-3
    assert (al["raw"][1] > 0) == (model["fwd"] is not None), "an approximate forward differs from the exact sum"


def test_hermite_table_is_below_2e6_of_a_unit_contribution():
    """rdf.hip states for the derivative table an interpolation error below 2e-6 of a unit contribution at width = spacing.
    One centre with g = 1, a dense sweep of distances, the library's nodes per spacing (mdg_rdf_fine_grid); the unit is
    g / sigma, in which dL/dd = -t exp(-t^2 / 2), t = (d - mu) / sigma.  The Hermite bound is (hf / sigma)^4 / 384 times the
    largest fourth derivative of t exp(-t^2 / 2), 5.8 at t = 0.6: 1.5e-6 with ten nodes per spacing.  (With the eight nodes the
    table had before, and 3 taken for that derivative, the same sweep measured 3.64e-6: the reason it has ten now.)"""
    case = R.BY_NAME["half/table R=6"]
    sub = R.plan_of(case)[2]["table_sub"]
    mu, coeff = case.centres().astype(np.float64), float(np.float32(case.coeff()))
    sigma = (-0.5 / coeff) ** 0.5
    g = np.zeros((1, 100))
    g[0, 50] = 1.0
    d = np.linspace(mu[50] - 0.2, mu[50] + 0.2, 20001)
    got = R._dldd_hermite(6, sub, d, mu, coeff, g, np.float64)[0]
    x = d - mu[50]
    exact = 2 * coeff * x * np.exp(coeff * x * x)
    err = np.abs(got - exact).max() * sigma
    print("hermite table, %d nodes per spacing: %.3e of g / sigma (%.3e of the largest |dL/dd| of the term)" % (
        sub, err, err / (np.abs(exact).max() * sigma)))
    assert abs((mu[1] - mu[0]) / sub / sigma - 1.0 / sub) < 1e-6, "width = spacing"
    assert err < 2e-6


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
def _geometry(case):
    """Accepted minimum-image distances of the first 64 frames and the fractional pair coordinates, in float64."""
    x = case.frames()[0][:64].astype(np.float64)
    h, inv, diag = R._cell(case.cell(), np.float64)
    iu, ju = R._pairs(case.n_atoms, R.pair_mask(case.n_atoms, index_tuple=case.index_tuple()))
    D, s, _ = R._images(x, h, inv, diag, iu, ju)
    d = np.sqrt((D * D).sum(-1))
    return d, s, x @ inv


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_inputs_of_the_gpu_cases(name):
    """Every case of tests/test_gpu_rdf_ref.py: the plan the library reports is the one the case means to run; at most 5 %
    of its frames were redrawn for a fragile pair and none is left; and the case reaches its edge."""
    case = R.BY_NAME[name]
    route, fwd, bwd, model = R.plan_of(case)
    want = case.expect
    assert route == want[:3], (route, want)
    if want[0] == "frames":
        if want[3] is not None:
            assert (fwd["R"], fwd["waves"], int(fwd["rows128"])) == want[3]
        assert bwd["R"] == want[4]
    frames, redrawn = case.frames()
    assert frames.dtype == np.float32 and frames.shape == (case.n_frames, case.n_atoms, 3)
    print("%-36s redrawn %d of %d frames" % (name, redrawn, case.n_frames))
    assert redrawn <= 0.05 * case.n_frames and len(case.check(frames)) == 0
    mu = case.centres().astype(np.float64)
    d, s, frac = _geometry(case)
    ok = (d > 0) & (d < case.cutoff())
    dmu = (mu[-1] - mu[0]) / (mu.size - 1)
    assert (ok & (np.abs(d - mu[mu.size // 2]) < dmu)).any() or case.n_atoms == 2, "pairs near the middle centre"
    if name == "low and high edge":
        R_ = min(fwd["R"], bwd["R"])
        kc = np.rint((d - mu[0]) / dmu)
        assert (ok & (d < mu[0]) & (kc >= -R_) & (kc < 0)).any() and (ok & (kc > mu.size - 1) & (kc <= mu.size - 1 + R_)).any()
        assert (ok & (kc < -bwd["R"] - 1)).any() and (ok & (kc > mu.size + bwd["R"])).any(), "and pairs beyond the table's ends"
    if "not a linspace" in name:
        assert case.spacing() == 0.0 and np.abs(np.diff(mu) - dmu).max() > 0.1 * dmu
    if "triclinic" in name:
        assert (np.abs(d - 2.3) < 0.05).any(), "pairs next to the cutoff, which lies inside the centres' range"
    if "masked" in name:
        a, b = case.index_tuple()
        assert 0 < len(a) < len(b) and len(a) + len(b) == case.n_atoms
    if "1025" in name:
        assert case.n_frames % fwd["waves"] == 1 and case.n_frames % bwd["waves"] == 1
    if "65 atoms" in name:
        assert case.n_atoms % 2 == 1 and case.n_atoms > 64
    if "translated" in name:
        assert frac.max() > 1.24 and frac.min() > 0.29, "outside the window of the unclamped minimum image"
    if "unwrapped" in name:
        assert np.abs(s).max() > 1.5 and frac.max() > 1.9, "raw separations beyond 1.5 cells: the shift is clamped to one cell"
    if "coincident" in name:
        assert (d == 0).sum() == d.shape[0], "one pair at distance exactly zero in every frame"
    if case.liquid:
        assert case.n_atoms == 512 and 3 * case.cutoff() <= case.box()[0]
    if case.n_atoms in (2, 7):
        assert ok.sum() >= 64 and R.plan_of(case)[1]["stride"] == 128, "accepted pairs; the pair table is mostly padding"


def test_plan_reports_the_fine_grid():
    """ops.rdf_plan("fwd", ...): the fine integer grid it reports (mdg_rdf_fine_grid) is mdg_rdf_fine_plan's -- h = 0.004 / s,
    reach = 5.3 / s, bins = ceil(((nbins - 1) spacing + 2 reach) / h) + 1, s = sqrt(-coeff log2 e) -- whatever variant the
    shape takes, and 0 bins where the grid exceeds the 36 864 bins of the workgroup's LDS histogram."""
    from mdgrad_amd import _lib, ops
    cs = _lib.make_cell([4.8] * 3)
    for nbins, width, fits in ((100, 1.0, True), (100, 1.6, True), (60, 1.0, True), (100, 0.4, False), (500, 1.6, False)):
        sp = float(np.float32(1.75 / (nbins - 1)))
        coeff = -0.5 / (width * sp) ** 2
        s = float(np.sqrt(np.float32(-np.float32(coeff) * np.float32(1.4426950408889634))))
        for frames, atoms in ((1024, 48), (1024, 108), (8, 48)):
            p = ops.rdf_plan("fwd", frames, atoms, nbins, sp, coeff, cs, None)
            assert abs(p["fine_h"] * s / 0.004 - 1) < 1e-6 and abs(p["fine_reach"] * s / 5.3 - 1) < 1e-6
            want = R.fine_bins(nbins, np.float32(sp), p["fine_h"], p["fine_reach"])
            assert p["fine_bins"] == (want if fits else 0) and (want <= 36864) == fits, (nbins, width, p, want)
            assert (p["variant"] == "fine") == (fits and frames >= 1024 and atoms >= 64)
    b = ops.rdf_plan("bwd", 1024, 48, 100, float(np.float32(1.75 / 99)), -0.5 / (1.75 / 99) ** 2, cs, None)
    assert b["variant"] == "table" and b["R"] == 6 and b["table_sub"] == 10 and b["cells"] == (99 + 14) * 10
    assert ops.rdf_plan("fwd", 1024, 1, 100, 0.0177, -1600.0, cs, None) is None
