"""thermo.TabulatedEnergy without a GPU: the float64 reference of tests/energy_table_ref.py checked against itself and the LJ
energy of tests/pair_forms_ref.py, the torch restatement (host / float64 positions) against that reference, the tabulation, the
interpolation error of the default table, the C entry points' argument checks and the constructor's refusals.

Tolerance of the float64 torch path against the float64 reference: error over the reference's scale <= 1e-12, as in
tests/test_energy_frames_host.py.  Every fixture is free of fragile pairs at the cutoff used (asserted)."""
import numpy as np
import pytest
import torch

import energy_table_ref as ER
import pair_forms_ref as PF
from test_energy_frames_host import _report, frames_108, mk_system

TOL64 = 1e-12
CUT = 2.5


def example_mlp(dtype=torch.float32):
    """the pairMLP of examples/fit_rdf_pairmlp.py at its initial weights"""
    from mdgrad_amd import potentials as P
    torch.manual_seed(0)
    mlp = P.pairMLP(n_gauss=25, r_start=0.0, r_end=2.5, n_layers=2, n_width=64, nonlinear="ELU")
    with torch.no_grad():
        mlp.layers[-1].weight.mul_(0.1)
    return mlp.to(dtype)


def small_mlp(seed=1, dtype=torch.float32):
    from mdgrad_amd import potentials as P
    torch.manual_seed(seed)
    return P.pairMLP(n_gauss=8, r_start=0.3, r_end=2.5, n_layers=1, n_width=8, nonlinear="ELU").to(dtype)


def interpolation_error(table32, u0, du, module64, cutoff, per_cell=8):
    """max |phi~ - phi| in float64 over a dense grid in u (per_cell points in every cell of the table), phi~ interpolated from
    the float32 table as the kernel receives it; also max |phi| there"""
    p = len(table32) // 2
    u = u0 + du * (np.arange((p - 1) * per_cell + 1, dtype=np.float64) / per_cell)
    u = u[u < cutoff * cutoff]
    with torch.no_grad():
        phi = module64(torch.as_tensor(u).sqrt()[:, None]).reshape(-1).numpy()
    got, _ = ER.interpolate(table32, u0, du, u)
    return float(np.abs(got - phi).max()), float(np.abs(phi).max())


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_interpolates_its_nodes_and_matches_a_fine_lj_table():
    rng = np.random.default_rng(0)
    p = 9
    u0, du = ER.grid(CUT, p, 0.3)
    tab = rng.standard_normal(2 * p).astype(np.float32)
    nodes = np.float64(np.float32(u0)) + np.float64(np.float32(du)) * np.arange(p)
    v, s = ER.interpolate(tab, u0, du, nodes)
    # (the node positions are products in float64 of the float32 grid values; 1 / du is the kernel's float32 value, so a node
    #  sits within 1e-6 of a cell from fr = 0)
    assert np.abs(v - tab[0::2]).max() <= 1e-5 and np.abs(s * du - tab[1::2]).max() <= 1e-4
    assert ER.interpolate(tab, u0, du, [u0 - 0.1])[0][0] == np.float64(tab[0])
    fx = PF.liquid(108)
    p = 4096
    u0, du = ER.grid(CUT, p, 0.2)
    fine = ER.lj_energy_table(u0, du, p)
    assert len(ER.fragile(fx.x, fx.cell, CUT)) == 0
    got = ER.evaluate(fx.x, fx.cell, fine, u0, du, CUT)
    lj = PF.evaluate(fx.x, np.zeros_like(fx.x), fx.cell, [PF.Term("lj", CUT, theta=(1.0, 1.0))])
    eU = abs(got.U - lj.U) / lj.sU
    eF = float((np.abs(-got.dq - lj.F) / lj.sF).max())
    _report("fine LJ energy table against the LJ form: U %.3e, dU/dq %.3e of the scale" % (eU, eF))
    # (the nodes are float32 roundings of LJ, 2^-24 of a value; the cubic on 4 096 nodes adds less.  The slope of the interpolant
    #  sees a node's rounding over the cell width, 1.5 / du of it: 1.5 x 2^-24 |phi| / (du |dphi/du|), and |phi / (dphi/du)| <=
    #  u / 3 ~ 2 in the tail, which holds most pairs: 1.2e-4 of the scale)
    assert eU <= 1e-6 and eF <= 1.5 * 2.0 ** -24 * 2.0 / du and got.n_below == 0 and got.n_pairs > 3000


# ------------------------------------------------------------------------------------------------ the torch restatement
def masks_108():
    A, B = PF.species(108)
    return {"none": None, "masked": dict(index_tuple=(A, B), ex_pairs=PF.excluded_list(108))}


@pytest.mark.parametrize("which", ["none", "masked"])
def test_float64_torch_path_against_the_reference(which):
    from mdgrad_amd.thermo import TabulatedEnergy
    fx, xyz = frames_108()
    sel = masks_108()[which]
    mask = None if sel is None else PF.select_mask(108, **sel)
    p = 64
    obs = TabulatedEnergy.from_terms(mk_system(fx.x, fx.cell), [(small_mlp(), CUT, (sel or {}).get("index_tuple"),
                                                                 (sel or {}).get("ex_pairs"))], nodes=p, r_min=0.2)
    u0, du, _ = obs.grid()
    assert (u0, du) == ER.grid(CUT, p, 0.2)
    tab = ER.lj_energy_table(u0, du, p, seed=3, noise=0.04)
    q = torch.as_tensor(xyz, dtype=torch.float64).requires_grad_(True)
    T = torch.as_tensor(tab).double().requires_grad_(True)
    U, nb = obs._torch_table_energy(q, T, obs._groups[0])
    assert int(nb) == 0
    for f, x in enumerate(xyz):
        assert len(ER.fragile(x, fx.cell, CUT, mask)) == 0
        ref = ER.evaluate(x, fx.cell, tab, u0, du, CUT, mask)
        gq, gT = torch.autograd.grad(U[f], [q, T], retain_graph=True)
        figs = {"U": PF.error(float(U[f].detach()), ref, "U"), "dq": PF.error(gq[f].numpy(), ref, "dq"), "dT": PF.error(gT.numpy(), ref, "dT")}
        _report("%s frame %d: %s" % (which, f, figs))
        assert all(v <= TOL64 for v in figs.values()), figs
        assert float(gq[1 - f].abs().max()) == 0.0
    # the whole class: its own table of the module, float32 nodes
    tab_m = obs.tabulate().detach().numpy()
    assert tab_m.dtype == np.float32 and tab_m.shape == (2 * p,)
    Um = obs(torch.as_tensor(xyz, dtype=torch.float64))
    assert Um.dtype == torch.float64 and int(obs.last_below) == 0
    for f, x in enumerate(xyz):
        ref = ER.evaluate(x, fx.cell, tab_m, u0, du, CUT, mask)
        assert PF.error(float(Um[f]), ref, "U") <= TOL64


def test_shapes_stacked_replicas_and_the_exact_prior():
    from mdgrad_amd import potentials as P
    from mdgrad_amd.thermo import PotentialEnergy, TabulatedEnergy
    fx, xyz = frames_108()
    mlp, prior = small_mlp(), P.ExcludedVolume(sigma=0.9, epsilon=1.0, power=12)
    terms = [(mlp, CUT), (prior, CUT)]
    obs = TabulatedEnergy.from_terms(mk_system(fx.x, fx.cell), terms, nodes=256)
    q = torch.as_tensor(xyz, dtype=torch.float64)
    U_T = obs(q)
    assert U_T.shape == (2,) and obs(q[1]).shape == () and torch.equal(obs(q[1]), U_T[1])
    U_RT = obs(torch.stack([q, q.flip(0), q]))
    assert U_RT.shape == (3, 2) and torch.equal(U_RT[1], U_T.flip(0))
    # the prior is the exact route, the module the tabulated one
    only = TabulatedEnergy.from_terms(mk_system(fx.x, fx.cell), [(mlp, CUT)], nodes=256)
    exact = PotentialEnergy.from_terms(mk_system(fx.x, fx.cell), [(prior, CUT)])
    assert torch.allclose(U_T, only(q) + exact(q), rtol=0, atol=1e-12 * float(U_T.abs().max()))
    k = 3
    obs_k = TabulatedEnergy.from_terms(mk_system(fx.x, fx.cell, n_rep=k), terms, nodes=256)
    qs = torch.stack([torch.cat([q[(t + r) % 2] for r in range(k)]) for t in range(2)])
    U_k = obs_k(qs)
    assert U_k.shape == (2, k)
    for t in range(2):
        for r in range(k):
            assert torch.equal(U_k[t, r], U_T[(t + r) % 2])
    with pytest.raises(ValueError, match="k \\* 108"):
        obs(torch.zeros(2, 100, 3))
    # two modules with one cutoff and no mask share a table; another cutoff is a group of its own
    two = TabulatedEnergy.from_terms(mk_system(fx.x, fx.cell), [(mlp, CUT), (small_mlp(2), CUT), (small_mlp(3), 1.8)], nodes=64)
    assert [len(g["mods"]) for g in two._groups] == [2, 1]


# ------------------------------------------------------------------------------------------------ the tabulation
def test_tabulated_nodes_are_the_module_and_the_slopes_its_derivative():
    from mdgrad_amd.thermo import TabulatedEnergy
    fx = PF.liquid(108)
    mlp = small_mlp(dtype=torch.float64)
    p = 128
    obs = TabulatedEnergy.from_terms(mk_system(fx.x, fx.cell), [(mlp, CUT)], nodes=p, r_min=0.2)
    u0, du, _ = obs.grid()
    tab = obs.tabulate()
    assert tab.dtype == torch.float64 and tab.requires_grad
    u = (u0 + du * torch.arange(p, dtype=torch.float32)).double()
    with torch.no_grad():
        phi = mlp(u.sqrt()[:, None]).reshape(-1)
        h = 1e-5
        cd = (mlp((u + h).sqrt()[:, None]) - mlp((u - h).sqrt()[:, None])).reshape(-1) / (2 * h)
    assert torch.equal(tab.detach()[0::2], phi)
    err = float((tab.detach()[1::2] - du * cd).abs().max() / (du * cd).abs().max())
    _report("tabulated slopes against a central difference: %.3e of the largest" % err)
    assert err <= 1e-7                                 # (h^2 / 6 |phi'''| / |phi'| ~ 1e-10, rounding 1e-16 / h ~ 1e-11 of phi)
    # the node gradient flows into the module parameters
    g = torch.autograd.grad((tab * torch.linspace(0, 1, 2 * p, dtype=torch.float64)).sum(), list(mlp.parameters()))
    assert all(torch.isfinite(x).all() for x in g) and any(float(x.abs().max()) > 0 for x in g)


def test_interpolation_error_of_the_default_table():
    """nodes = 2048, r_min = 0.2 (the defaults), the pairMLP of examples/fit_rdf_pairmlp.py at its initial weights: the figure
    recorded in docs/KERNELS.md (K33).  Measured, printed, not bounded in advance."""
    from mdgrad_amd.thermo import TabulatedEnergy
    fx = PF.liquid(108)
    mlp = example_mlp()
    obs = TabulatedEnergy.from_terms(mk_system(fx.x, fx.cell), [(mlp, CUT)])
    assert obs.nodes == 2048 and obs.r_min == 0.2
    u0, du, p = obs.grid()
    tab32 = obs.tabulate().detach().numpy()
    import copy
    err, mag = interpolation_error(tab32, u0, du, copy.deepcopy(mlp).double(), CUT)
    tab64 = TabulatedEnergy.from_terms(mk_system(fx.x, fx.cell), [(copy.deepcopy(mlp).double(), CUT)]).tabulate().detach().numpy()
    err64, _ = interpolation_error(tab64.astype(np.float32), u0, du, copy.deepcopy(mlp).double(), CUT)
    _report("default table (2048 nodes, r_min 0.2), example pairMLP: max |phi~ - phi| = %.3e (float32 tabulation), %.3e "
            "(float64 tabulation rounded to float32); max |phi| = %.3e" % (err, err64, mag))
    assert np.isfinite(err) and np.isfinite(err64)


# ------------------------------------------------------------------------------------------------ the C entry points
def test_library_validates_energy_table_arguments():
    """Argument errors return -1 with a message, before anything is launched (no device needed)."""
    import ctypes as C
    from mdgrad_amd import _lib
    lib = _lib.load()
    cell, tric = _lib.make_cell([5.0, 5.0, 5.0]), _lib.make_cell([[5.0, 0, 0], [1.0, 5.0, 0], [0, 0, 5.0]])
    buf = C.c_void_p(256)                # never dereferenced: every call below fails its checks
    p = 16
    u0, du = ER.grid(2.5, p, 0.2)

    def fwd(n_frames=2, n_atoms=8, c=cell, table=buf, n_nodes=p, u0=u0, du=du, cutoff=2.5, U=buf, below=buf, ws=buf, pos=buf):
        return lib.mdg_energy_table_fwd(pos, n_frames, n_atoms, C.byref(c), table, n_nodes, u0, du, cutoff, None, U, below, ws, None)

    def bwd(gU=buf, g_pos=buf, g_table=buf, ws=buf, n_nodes=p, du=du, c=cell):
        return lib.mdg_energy_table_bwd(buf, 2, 8, C.byref(c), buf, n_nodes, u0, du, 2.5, None, gU, g_pos, g_table, ws, None)

    for call, word in ((lambda: fwd(pos=None), "null"), (lambda: fwd(table=None), "null"), (lambda: fwd(U=None), "null"),
                       (lambda: fwd(below=None), "null"), (lambda: fwd(ws=None), "null"),
                       (lambda: fwd(n_frames=0), "empty"), (lambda: fwd(n_atoms=0), "empty"),
                       (lambda: fwd(n_nodes=3), "nodes"), (lambda: fwd(n_nodes=4097), "nodes"),
                       (lambda: fwd(du=0.0), "du > 0"), (lambda: fwd(du=-du), "du > 0"),
                       (lambda: fwd(du=du * 1.001), "last node"), (lambda: fwd(cutoff=2.4), "last node"),
                       (lambda: fwd(u0=u0 + 0.01), "last node"),
                       (lambda: fwd(c=tric), "diagonal"), (lambda: fwd(n_atoms=40000), "atoms"),
                       (lambda: fwd(n_frames=1 << 24), "2^24"),
                       (lambda: bwd(gU=None), "null"), (lambda: bwd(ws=None), "null"), (lambda: bwd(n_nodes=2), "nodes"),
                       (lambda: bwd(du=0.0), "du > 0"), (lambda: bwd(c=tric), "diagonal"),
                       (lambda: bwd(g_pos=None, g_table=None), "both null")):
        rc = call()
        assert rc == -1 and word in lib.mdg_last_error().decode(), (rc, word, lib.mdg_last_error())
    # the scale and 2 p int64 words, then one partial per tile of a tiled frame
    assert lib.mdg_energy_table_workspace(8192, 108, 2048) == 4 + 4 * 2048
    assert lib.mdg_energy_table_workspace(64, 4096, 16) == 4 + 4 * 16 + 64 * 16 * 9


# ------------------------------------------------------------------------------------------------ refusals
def test_constructor_refusals():
    from mdgrad_amd import potentials as P
    from mdgrad_amd.thermo import TabulatedEnergy
    fx = PF.liquid(108)
    system = mk_system(fx.x, fx.cell)
    mlp = small_mlp()
    with pytest.raises(NotImplementedError, match="GNN, bonded, many-body and charge"):
        TabulatedEnergy(system, torch.nn.Linear(2, 2))
    with pytest.raises(NotImplementedError, match="PotentialEnergy"):
        TabulatedEnergy.from_terms(system, [(P.LennardJones(1.0, 1.0), CUT)])
    with pytest.raises(NotImplementedError, match="four built-in"):
        TabulatedEnergy.from_terms(system, [(mlp, CUT)] + [(P.LennardJones(1.0, 1.0), CUT)] * 5)
    tric = mk_system(fx.x, np.array([[4.8, 0, 0], [0.6, 4.8, 0], [0, 0, 4.8]]))
    with pytest.raises(ValueError, match="diagonal"):
        TabulatedEnergy.from_terms(tric, [(mlp, 2.0)])
    for bad in (3, 4097):
        with pytest.raises(ValueError, match="nodes"):
            TabulatedEnergy.from_terms(system, [(mlp, CUT)], nodes=bad)
    with pytest.raises(ValueError, match="r_min"):
        TabulatedEnergy.from_terms(system, [(mlp, CUT)], r_min=1.0)
    big = mk_system(np.random.default_rng(0).uniform(0, 40.0, (32769, 3)), [40.0] * 3)
    with pytest.raises(ValueError, match="32768 atoms"):
        TabulatedEnergy.from_terms(big, [(mlp, CUT)])


def test_pairs_below_the_first_node():
    """a pair closer than r_min * cutoff: refused with check_range (the message names r_min), counted and continued by the
    constant first node value without it"""
    from mdgrad_amd.thermo import TabulatedEnergy
    fx = PF.liquid(108)
    x = fx.x.copy()
    x[1] = x[0] + np.float32([0.3, 0.0, 0.0])                   # r = 0.3 < 0.2 * 2.5
    assert len(ER.fragile(x, fx.cell, CUT)) == 0
    mlp = small_mlp()
    q = torch.as_tensor(x[None], dtype=torch.float64)
    with pytest.raises(RuntimeError, match="r_min"):
        TabulatedEnergy.from_terms(mk_system(fx.x, fx.cell), [(mlp, CUT)], nodes=64)(q)
    obs = TabulatedEnergy.from_terms(mk_system(fx.x, fx.cell), [(mlp, CUT)], nodes=64, check_range=False)
    U = obs(q)
    u0, du, _ = obs.grid()
    ref = ER.evaluate(x, fx.cell, obs.tabulate().detach().numpy(), u0, du, CUT)
    assert ref.n_below == 1 and int(obs.last_below) == 1
    assert PF.error(float(U[0]), ref, "U") <= TOL64
