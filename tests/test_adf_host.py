"""Bond-angle distribution, host side: the angle list against the reference's (golden A1, A2) and the observable's grid
and Gaussian constants against the reference's GaussianSmearing (nff/nn/layers.py:14-31, torchmd/observable.py:120-139)."""
import numpy as np
import pytest
import torch

from conftest import load_golden


@pytest.mark.parametrize("case", ["c15_", "c20_", "c25_"])
def test_generate_angle_list_matches_reference(case):
    from mdgrad_amd.topology import generate_angle_list, make_directed
    g = load_golden("adf_a1")
    nbr = torch.as_tensor(g[case + "nbr"].astype(np.int64))
    d = make_directed(nbr)
    assert d.shape == (2 * len(nbr), 3)
    assert torch.equal(d[len(nbr):], nbr[:, [0, 2, 1]])
    got = generate_angle_list(nbr)
    assert len(got) == int(g[case + "n_angles"])
    want = torch.as_tensor(g[case + "angle_list"].astype(np.int64))
    if case + "sub_idx" in g:
        got = got[torch.as_tensor(g[case + "sub_idx"])]
    assert torch.equal(got, want)


def test_generate_angle_list_masked_and_empty():
    from mdgrad_amd.topology import generate_angle_list
    g = load_golden("adf_a2")
    got = generate_angle_list(torch.as_tensor(g["nbr"].astype(np.int64)))
    assert torch.equal(got, torch.as_tensor(g["angle_list"].astype(np.int64)))
    assert generate_angle_list(torch.zeros(0, 3, dtype=torch.long)).shape == (0, 4)


def test_generate_angle_list_refuses_beyond_the_limit(monkeypatch):
    from mdgrad_amd import topology
    g = load_golden("adf_a1")
    monkeypatch.setattr(topology, "ANGLE_LIST_MAX", 1000)
    with pytest.raises(ValueError, match="keep_angles=False"):
        topology.generate_angle_list(torch.as_tensor(g["c15_nbr"].astype(np.int64)))


def _cpu_system():
    from mdgrad_amd.system import System
    g = load_golden("adf_a1")
    return System(positions=np.asarray(g["c15_xyz"][0], dtype=np.float64), cell=np.asarray(g["cell"], dtype=np.float64),
                  masses=np.full(108, 1.008), device="cpu")


@pytest.mark.parametrize("nbins,rng,width", [(60, (0.0, np.pi), None), (40, (0.5, 2.8), 0.05), (7, (2.0, 1.0), None)])
def test_grid_and_gaussian_constants_match_reference(nbins, rng, width):
    from mdgrad_amd.observable import angle_distribution, Angles
    obs = angle_distribution(_cpu_system(), nbins, rng, cutoff=1.5, width=width)
    bins = torch.linspace(rng[0], rng[1], nbins + 1)
    centres = torch.linspace(rng[0], float(bins[-1]), nbins)
    w = torch.FloatTensor((centres[1] - centres[0]) * torch.ones_like(centres)) if width is None else \
        torch.FloatTensor(width * torch.ones_like(centres))
    assert torch.equal(obs.bins.cpu(), bins)
    assert torch.equal(obs.smear.offsets.cpu(), centres)
    assert obs.width == w[0].item()
    assert obs.coeff == float(-0.5 / torch.pow(w, 2)[0])
    assert obs.spacing == float(centres[1] - centres[0])
    assert obs.cutoff == 1.5 and obs.index_tuple is None and obs.device == torch.device("cpu")
    assert obs.keep_angles is True
    a = Angles(_cpu_system(), nbins, rng, cutoff=1.5, width=width)
    assert torch.equal(a.bins.cpu(), bins) and a.width == obs.width


def test_golden_widths_agree():
    from mdgrad_amd.observable import angle_distribution
    g1, g2 = load_golden("adf_a1"), load_golden("adf_a2")
    assert angle_distribution(_cpu_system(), 60, (0.0, np.pi), cutoff=1.5).width == float(g1["c15_width"])
    assert angle_distribution(_cpu_system(), 40, (0.5, 2.8), cutoff=1.5, width=0.05).width == float(g2["width"])


@pytest.mark.parametrize("nbins,rng,width", [(0, (0.0, 3.0), None), (1, (0.0, 3.0), None), (-3, (0.0, 3.0), None),
                                             (10, (0.0,), None)])
def test_invalid_arguments_raise_as_the_reference(nbins, rng, width):
    from mdgrad_amd.observable import angle_distribution
    with pytest.raises((IndexError, RuntimeError)):
        angle_distribution(_cpu_system(), nbins, rng, cutoff=1.5, width=width)


def test_zero_width_is_refused():
    from mdgrad_amd.observable import angle_distribution
    with pytest.raises(ValueError, match="width"):
        angle_distribution(_cpu_system(), 10, (0.0, 3.0), cutoff=1.5, width=0.0)
