"""Dihedral terms, host side: the topology helpers, the OPLS mapping, compute_dihe and DihedralPotentials' torch restatement
against the reference's goldens (D1, D2: tests/golden/make_dihedral_goldens.py), the sign convention of phi, the grid of
dihedral_distribution, and the argument validation of the C entry points.  Also pins tests/dihedral_ref.py -- the float64
definitions the GPU tests compare the kernels with -- to the same goldens."""
import ctypes
import math

import numpy as np
import pytest
import torch

import dihedral_ref as R
from conftest import load_golden


def _cpu_system(pos, cell):
    from mdgrad_amd.system import System
    return System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
                  masses=np.full(len(pos), 1.008), device="cpu")


# ------------------------------------------------------------------------------------------------ topology
def test_chain_dihedrals():
    from mdgrad_amd.topology import chain_dihedrals
    assert chain_dihedrals(5).tolist() == [[0, 1, 2, 3], [1, 2, 3, 4]]
    assert chain_dihedrals(6, start=10).tolist() == [[10, 11, 12, 13], [11, 12, 13, 14], [12, 13, 14, 15]]
    for n in (0, 3):
        assert chain_dihedrals(n).shape == (0, 4) and chain_dihedrals(n).dtype == torch.long


def test_dihedrals_from_bonds():
    from mdgrad_amd.topology import chain_dihedrals, dihedrals_from_bonds
    chain = [[i, i + 1] for i in range(4)]
    assert torch.equal(dihedrals_from_bonds(torch.tensor(chain)), chain_dihedrals(5))
    assert torch.equal(dihedrals_from_bonds(torch.tensor(chain[::-1])[:, [1, 0]]), chain_dihedrals(5)), "order and direction of the bonds"
    # a 4-ring: one torsion about every bond, j < k, ordered by (j, k, i, l)
    ring = dihedrals_from_bonds([[0, 1], [1, 2], [2, 3], [3, 0]])
    assert ring.tolist() == [[3, 0, 1, 2], [1, 0, 3, 2], [0, 1, 2, 3], [1, 2, 3, 0]]
    # branched: 0-1, 1-2, 1-3, 3-4, 3-5 (two centres of degree 3): torsions only about 1-3
    br = dihedrals_from_bonds([[0, 1], [1, 2], [1, 3], [3, 4], [3, 5]])
    assert br.tolist() == [[0, 1, 3, 4], [0, 1, 3, 5], [2, 1, 3, 4], [2, 1, 3, 5]]
    # a triangle has no proper torsion (i == l), a pendant atom on it has two
    assert dihedrals_from_bonds([[0, 1], [1, 2], [2, 0]]).shape == (0, 4)
    assert dihedrals_from_bonds([[0, 1], [1, 2], [2, 0], [2, 3]]).tolist() == [[1, 0, 2, 3], [0, 1, 2, 3]]
    assert dihedrals_from_bonds(torch.zeros(0, 2, dtype=torch.long)).shape == (0, 4)
    for row in ring.tolist() + br.tolist():
        assert len(set(row)) == 4 and row[1] < row[2]


def test_dihedral_table_incidence_and_refusals():
    from mdgrad_amd import ops
    top = [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5], [3, 4, 5, 6], [6, 5, 4, 3]]
    tab = ops.DihedralTable(top, 8, [5.0, 5.0, 5.0], "cpu")
    ptr, inc = tab.inc_ptr.tolist(), tab.inc.tolist()
    assert ptr[0] == 0 and ptr[-1] == 20 and len(ptr) == 9 and ptr[8] == ptr[7], "atom 7 takes part in nothing"
    for a in range(8):
        own = inc[ptr[a]:ptr[a + 1]]
        assert own == sorted(own) and all(top[c >> 2][c & 3] == a for c in own)
    assert sorted(inc) == list(range(20)) and ptr[4] - ptr[3] == 5 and ptr[1] - ptr[0] == 1
    assert ops.DihedralTable(torch.zeros(0, 4, dtype=torch.long), 4, [5.0] * 3, "cpu").n_terms == 0
    for bad in ([[0, 1, 2, 8]], [[-1, 1, 2, 3]]):
        with pytest.raises(ValueError, match="outside"):
            ops.DihedralTable(bad, 8, [5.0] * 3, "cpu")
    for bad in ([[0, 1, 2, 0]], [[0, 1, 1, 3]], [[2, 1, 2, 3]]):
        with pytest.raises(ValueError, match="twice"):
            ops.DihedralTable(bad, 8, [5.0] * 3, "cpu")
    with pytest.raises(ValueError, match="types"):
        ops.DihedralTable(top, 8, [5.0] * 3, "cpu", types=[0, 1, 2, 0, 0], n_types=2)
    with pytest.raises(ValueError, match="types"):
        ops.DihedralTable(top, 8, [5.0] * 3, "cpu", types=[0, 1], n_types=2)


# ------------------------------------------------------------------------------------------------ OPLS
def test_opls_to_multiharmonic_equals_the_trigonometric_form():
    from mdgrad_amd.interface import DihedralPotentials
    V = torch.tensor([[0.7, -1.3, 0.4, 0.9], [1.9, 0.0, -2.2, 0.35]], dtype=torch.float64)
    A = DihedralPotentials.opls_to_multiharmonic(V)
    assert A.shape == (2, 5) and A.dtype == torch.float64
    c = torch.linspace(-1, 1, 101, dtype=torch.float64)
    phi = torch.acos(c)
    for v, a in zip(V, A):
        trig = sum(v[m - 1] / 2 * (1 + (-1) ** (m + 1) * torch.cos(m * phi)) for m in range(1, 5))
        poly = sum(a[m] * c ** m for m in range(5))
        assert float((trig - poly).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ goldens
def test_compute_dihe_and_the_float64_reference_match_d1():
    from mdgrad_amd.observable import compute_dihe
    g = load_golden("dihedral_d1")
    top = g["dihes"].astype(np.int64)
    x32 = torch.tensor(g["xyz"])
    assert x32.shape[0] != 3 and top.shape[0] != 3
    c64 = compute_dihe(x32.double(), torch.as_tensor(top))
    assert c64.shape == (5, 21) and float((c64 - torch.tensor(g["cos64"])).abs().max()) <= 1e-13
    c32 = compute_dihe(x32, torch.as_tensor(top))
    assert c32.dtype == torch.float32 and float((c32.double() - torch.tensor(g["cos64"])).abs().max()) <= 10 * float(g["err32"])
    # three rows: the reference's dim-less cross would take the wrong axis; this one does not
    assert float((compute_dihe(x32.double(), torch.as_tensor(top[:3])) - torch.tensor(g["cos64"][:, :3])).abs().max()) <= 1e-13
    cr, pr, ok = R.geometry(x32.double(), top)
    assert bool(ok.all()) and float((cr - torch.tensor(g["cos64"])).abs().max()) <= 1e-13
    assert float((pr.cos() - cr).abs().max()) <= 1e-13 and float(pr.abs().max()) <= math.pi
    # imaging: the wrapped frames give the same angles with the cell, not without
    L = g["cell"].astype(np.float64)
    cw = R.cos_phi(torch.tensor(np.mod(g["xyz"].astype(np.float64), L)), top, L)
    assert float((cw - torch.tensor(g["cos64"])).abs().max()) <= 1e-12


def _wrapped_d2():
    g = load_golden("dihedral_d2")
    L = g["cell"].astype(np.float64)
    pos = g["pos"].astype(np.float64)
    wrapped = np.mod(pos, L)
    b = np.diff(wrapped, axis=0)
    assert int((np.abs(b) >= 0.5 * L).any(1).sum()) >= 3, "at least three bonds must cross the boundary"
    return g, wrapped, L


def test_torch_energy_and_the_float64_reference_match_d2_on_the_wrapped_chain():
    from mdgrad_amd.interface import DihedralPotentials
    g, wrapped, L = _wrapped_d2()
    top, types = g["dihes"].astype(np.int64), g["types"].astype(np.int64)
    mod = DihedralPotentials(_cpu_system(wrapped, L), torch.as_tensor(top), torch.tensor(g["coeffs"]), types=torch.as_tensor(types))
    assert [n for n, _ in mod.named_parameters()] == ["coeffs"] and mod.coeffs.shape == (2, 5) and mod.coeffs.dtype == torch.float32
    assert not mod._hip_ok(torch.zeros(24, 3, dtype=torch.float64)) and not mod._hip_ok(torch.zeros(24, 3))
    frozen = DihedralPotentials(_cpu_system(wrapped, L), torch.as_tensor(top), torch.tensor(g["coeffs"]), types=torch.as_tensor(types),
                                trainable=False)
    assert list(frozen.parameters()) == [] and "coeffs" in dict(frozen.named_buffers())
    w = torch.tensor(g["w"]).double()
    fmax, hmax = float(np.abs(g["force"]).max()), float(np.abs(g["hw"]).max())

    def check(energy_of, A):
        q = torch.tensor(wrapped, requires_grad=True)
        U = energy_of(q)
        gq, gA = torch.autograd.grad(U, (q, A), create_graph=True)
        dq, dA = torch.autograd.grad(-(gq * w).sum(), (q, A))
        assert abs(float(U.detach()) - float(g["energy"][0])) <= 1e-6 * abs(float(g["energy"][0]))       # (float32 coefficients)
        assert float((-gq.detach() - torch.tensor(g["force"])).abs().max()) <= 1e-6 * fmax
        assert float((-dq - torch.tensor(g["hw"])).abs().max()) <= 1e-6 * hmax
        assert float((gA.detach().double() - torch.tensor(g["dU_dA"])).abs().max()) <= 1e-6 * float(np.abs(g["dU_dA"]).max())
        assert float((dA.double() - torch.tensor(g["dwF_dA"])).abs().max()) <= 1e-6 * float(np.abs(g["dwF_dA"]).max())

    check(mod.forward, mod.coeffs)                     # float64 host positions: the torch restatement
    A = torch.tensor(g["coeffs"], dtype=torch.float64, requires_grad=True)
    check(lambda q: R.energy(q, top, A, types, L), A)
    # the oracle-protocol term on top of it
    term = R.DihedralTerm(top, g["coeffs"], L, types)
    F, dq, dth = term.force_vjp(torch.tensor(wrapped), w)
    assert term.n_theta == 10 and float((F - torch.tensor(g["force"])).abs().max()) <= 1e-6 * fmax
    assert float((-dq - torch.tensor(g["hw"])).abs().max()) <= 1e-6 * hmax
    assert float((dth.reshape(2, 5) - torch.tensor(g["dwF_dA"])).abs().max()) <= 1e-6 * float(np.abs(g["dwF_dA"]).max())
    assert float((term.force(torch.tensor(wrapped)) - F).abs().max()) == 0.0


def test_from_opls_builds_the_same_term():
    from mdgrad_amd.interface import DihedralPotentials
    g, wrapped, L = _wrapped_d2()
    top = torch.as_tensor(g["dihes"].astype(np.int64))
    V = torch.tensor([0.7, -1.3, 0.4, 0.9])
    a = DihedralPotentials.from_opls(_cpu_system(wrapped, L), top, V)
    b = DihedralPotentials(_cpu_system(wrapped, L), top, DihedralPotentials.opls_to_multiharmonic(V))
    q = torch.tensor(wrapped)
    assert a.coeffs.shape == (5,) and float(a(q)) == float(b(q))
    ph = R.phi(q, top.numpy(), L)
    trig = sum(float(V[m - 1]) / 2 * (1 + (-1) ** (m + 1) * torch.cos(m * ph)) for m in range(1, 5)).sum()
    assert abs(float(a(q)) - float(trig)) <= 1e-6 * abs(float(trig))
    with pytest.raises(ValueError, match="coeffs"):
        DihedralPotentials(_cpu_system(wrapped, L), top, torch.zeros(4))


def test_degenerate_terms_are_skipped_by_the_restatements():
    from mdgrad_amd.interface import DihedralPotentials
    pos = np.array([[0.5, 0.5, 0.5], [1.0, 0.5, 0.5], [1.5, 0.5, 0.5], [1.5, 1.0, 1.0], [2.0, 1.5, 0.5], [2.5, 1.0, 1.5]])
    top = np.array([[0, 1, 2, 3], [2, 3, 4, 5]])
    L = np.array([8.0, 8.0, 8.0])
    mod = DihedralPotentials(_cpu_system(pos, L), torch.as_tensor(top), [0.3, -1.1, 0.8, 0.5, -0.4])
    q = torch.tensor(pos, requires_grad=True)
    U = mod(q)
    (gq,) = torch.autograd.grad(U, q)
    c, ph, ok = R.geometry(q.detach(), top, L)
    assert ok.tolist() == [False, True] and float(c[0]) == 0.0 and float(ph[0]) == 0.0
    assert bool(torch.isfinite(gq).all()) and float(gq[:2].abs().max()) == 0.0, "atoms of the skipped term alone feel nothing"
    assert abs(float(U) - float(R.energy(q.detach(), top, mod.coeffs.detach().double(), None, L))) <= 1e-12


# ------------------------------------------------------------------------------------------------ sign convention
def test_phi_is_minus_the_signed_dihedral_of_the_polymer_demo():
    """d_i of compute_intcoord (demo/fold.py:57-72) restated in float64: with u_i the unit vectors x_i - x_{i+1} and
    n_i = u_i x u_{i+1} normalised, d_i = acos(clamp(n_i.n_{i+1}, +-0.99)) sign(u_i.n_{i+1}).  phi = -d_i off the clamp."""
    g = load_golden("dihedral_d1")
    x = g["xyz"].astype(np.float64)
    u = x[:, :-1] - x[:, 1:]
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    n = np.cross(u[:, :-1], u[:, 1:])
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    cosd = (n[:, :-1] * n[:, 1:]).sum(-1)
    d = np.arccos(np.clip(cosd, -0.99, 0.99)) * np.sign((u[:, :-2] * n[:, 1:]).sum(-1))
    phi = R.phi(torch.tensor(x), g["dihes"].astype(np.int64)).numpy()
    free = np.abs(cosd) < 0.99
    assert free.sum() >= 50 and np.abs(phi[free] + d[free]).max() <= 1e-9
    assert (np.sign(phi[0]) == -np.sign(d[0])).all(), "opposite on all 21 terms of frame 0"


# ------------------------------------------------------------------------------------------------ observable grid
@pytest.mark.parametrize("nbins,width", [(36, None), (50, None), (36, 0.1), (50, 0.5)])
def test_distribution_grid_centres_and_width(nbins, width):
    from mdgrad_amd.observable import dihedral_distribution
    g = load_golden("dihedral_d1")
    obs = dihedral_distribution(_cpu_system(g["xyz"][0], g["cell"]), g["dihes"].astype(np.int64), nbins, width=width)
    delta = 2 * math.pi / nbins
    assert torch.equal(obs.bins.cpu(), torch.linspace(-math.pi, math.pi, nbins + 1))
    assert float((obs.offsets.cpu().double() - R.centres(nbins)).abs().max()) <= 2.5e-7
    assert float((0.5 * (obs.bins[1:] + obs.bins[:-1]).cpu() - obs.offsets.cpu()).abs().max()) <= 1e-6
    assert obs.width == (delta if width is None else width) and obs.coeff == -0.5 / obs.width ** 2
    assert obs.spacing == delta and obs.nbins == nbins and obs.n_terms == 21 and obs.keep_angles is True


def test_distribution_refuses_bad_arguments():
    from mdgrad_amd.observable import dihedral_distribution
    g = load_golden("dihedral_d1")
    s, top = _cpu_system(g["xyz"][0], g["cell"]), g["dihes"].astype(np.int64)
    for kw in (dict(nbins=36, width=0.51), dict(nbins=36, width=0.0), dict(nbins=36, width=-0.1), dict(nbins=8)):
        with pytest.raises(ValueError, match="width"):
            dihedral_distribution(s, top, **kw)
    for nbins in (0, -4, 4097, 2.5):
        with pytest.raises(ValueError, match="nbins"):
            dihedral_distribution(s, top, nbins)
    with pytest.raises(ValueError, match="outside"):
        dihedral_distribution(s, [[0, 1, 2, 24]], 36)


def test_a_table_over_the_stacked_system_keeps_the_stacked_atom_count():
    from mdgrad_amd.observable import Dihedrals
    g = load_golden("dihedral_d1")
    s = _cpu_system(g["xyz"][0], g["cell"])
    assert Dihedrals(s, g["dihes"].astype(np.int64)).natoms == 24
    s.group_size, s.n_replicas = 12, 2               # two stacked replicas of 12
    assert Dihedrals(s, [[0, 1, 2, 3]]).natoms == 12 and Dihedrals(s, [[12, 13, 14, 15]]).natoms == 24


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_entry_points_validate_their_arguments():
    from mdgrad_amd import _lib
    lib = _lib.load()
    L = (ctypes.c_float * 3)(6.0, 6.0, 6.0)
    p = ctypes.c_void_p(64)                  # never dereferenced: every call below fails its checks first

    def fails(rc, word):
        msg = lib.mdg_last_error()
        assert rc == -1 and word.encode() in msg, (rc, word, msg)

    ev = lib.mdg_dihedral_eval
    fails(ev(None, 8, L, p, 2, p, None, 1, p, p, None, None, p, None, None, None, 1.0, 0, None), "pos")
    fails(ev(p, 8, None, p, 2, p, None, 1, p, p, None, None, p, None, None, None, 1.0, 0, None), "cell_len")
    fails(ev(p, 0, L, p, 2, p, None, 1, p, p, None, None, p, None, None, None, 1.0, 0, None), "n_atoms")
    fails(ev(p, 8, L, p, -1, p, None, 1, p, p, None, None, p, None, None, None, 1.0, 0, None), "n_terms")
    fails(ev(p, 8, L, None, 2, p, None, 1, p, p, None, None, p, None, None, None, 1.0, 0, None), "top")
    fails(ev(p, 8, L, p, 2, None, None, 1, p, p, None, None, p, None, None, None, 1.0, 0, None), "coeff")
    fails(ev(p, 8, L, p, 2, p, None, 0, p, p, None, None, p, None, None, None, 1.0, 0, None), "n_types")
    fails(ev(p, 8, L, p, 2, p, None, 1, None, p, None, None, p, None, None, None, 1.0, 0, None), "inc_ptr")
    fails(ev(p, 8, L, p, 2, p, None, 1, p, p, None, None, p, p, None, None, 1.0, 0, None), "needs w")
    fails(ev(p, 8, L, p, 2, p, None, 1, p, p, None, None, None, None, None, None, 1.0, 0, None), "no output")
    cg = lib.mdg_dihedral_coeff_grad
    fails(cg(None, None, None, 2, 1, p, None, None), "c_term")
    fails(cg(p, None, None, -1, 1, p, None, None), "n_terms")
    fails(cg(p, None, None, 2, 0, p, None, None), "n_types")
    fails(cg(p, None, None, 2, 1, None, None, None), "no output")
    fails(cg(p, None, None, 2, 1, None, p, None), "cd_term")
    pf = lib.mdg_dihedral_phi_fwd
    fails(pf(None, 2, 8, L, p, 2, p, p, None), "pos")
    fails(pf(p, 0, 8, L, p, 2, p, p, None), "n_frames")
    fails(pf(p, 2, 8, L, p, -3, p, p, None), "n_terms")
    fails(pf(p, 2, 8, L, None, 2, p, p, None), "top")
    fails(pf(p, 2, 8, L, p, 2, None, None, None), "no output")
    pb = lib.mdg_dihedral_phi_bwd
    fails(pb(None, 2, 8, L, p, 2, p, p, p, None, p, None), "pos")
    fails(pb(p, 2, 8, None, p, 2, p, p, p, None, p, None), "cell_len")
    fails(pb(p, 2, 8, L, p, 2, None, p, p, None, p, None), "inc_ptr")
    fails(pb(p, 2, 8, L, p, 2, p, p, None, None, p, None), "g_phi")
    fails(pb(p, 2, 8, L, p, 2, p, p, p, None, None, None), "g_xyz")
    hf, hb = lib.mdg_dihedral_hist_fwd, lib.mdg_dihedral_hist_bwd
    fails(hf(None, None, 10, 36, 0.1, p, p, None), "phi")
    fails(hf(p, None, -1, 36, 0.1, p, p, None), "n must")
    for nbins in (0, 4097):
        fails(hf(p, None, 10, nbins, 0.1, p, p, None), "nbins")
        fails(hb(p, None, 10, nbins, 0.1, p, p, None), "nbins")
    for width in (0.0, -0.2, 0.6):
        fails(hf(p, None, 10, 36, width, p, p, None), "width")
        fails(hb(p, None, 10, 36, width, p, p, None), "width")
    fails(hf(p, None, 10, 36, 0.1, None, p, None), "raw")
    fails(hf(p, None, 10, 36, 0.1, p, None, None), "scratch")
    fails(hb(p, None, 10, 36, 0.1, None, p, None), "g_raw")
    fails(hb(p, None, 10, 36, 0.1, p, None, None), "g_phi")
    assert lib.mdg_dihedral_hist_scratch(1000, 36) == 38
