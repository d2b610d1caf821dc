"""thermo.PotentialEnergy without a GPU: the torch restatement (host / float64 positions) against the float64 reference of
tests/pair_forms_ref.py, the shapes, the constructor's refusals, the C entry points' argument checks and the compiled
wave-per-frame kernels' registers read from the gfx950 code object that build() made (as tests/test_pressure_host.py does for
the virial kernels).

Tolerance: the float64 torch path against the float64 reference, error over the reference's scale (per atom and component the
sum of the absolute summands; for U and dU/dtheta over all pairs) <= 1e-12, as in tests/test_pair_forms_ref_host.py.  Every
fixture is free of fragile pairs at the cutoffs used (asserted), so the references are exact on them and no case is left out.
On a host the model is given through PotentialEnergy.from_terms (a PairPotentials needs a device for its neighbour list); the
equality with model(q[f]) is tests/test_gpu_energy_frames.py's."""
import os

import numpy as np
import pytest
import torch

import pair_forms_ref as PF
import test_pressure_host as TP

TOL64 = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(line):
    print(line)
    if os.environ.get("MDG_TEST_REPORT"):
        with open(os.environ["MDG_TEST_REPORT"], "a") as fh:
            fh.write(line + "\n")


def mk_system(x, cell, device="cpu", n_rep=0):
    from mdgrad_amd.system import System
    s = System(positions=np.asarray(x, np.float64), cell=np.asarray(cell, np.float64), masses=np.full(len(x), 1.008), device=device)
    return s.replicate(n_rep) if n_rep else s


def members_of(name, n):
    """[(form, theta or None, cutoff, selection or None)] of a single form of PF.FORMS or of a stack of PF.stack"""
    return [(name, None, 2.5, None)] if name in PF.FORMS else PF.stack(name, n)


def observable(fx, members, device="cpu", dtype=torch.float64, n_rep=0):
    """(PotentialEnergy, modules) for the members; the modules hold the float32 parameter values in `dtype`"""
    from mdgrad_amd.thermo import PotentialEnergy
    mods = [PF.module(f, th).to(dtype) for f, th, _, _ in members]
    terms = [(m, rc, (sel or {}).get("index_tuple"), (sel or {}).get("ex_pairs")) for m, (_, _, rc, sel) in zip(mods, members)]
    return PotentialEnergy.from_terms(mk_system(fx.x, fx.cell, device, n_rep), terms), mods


def frames_108():
    """two frames of 108 atoms in the 4.8 cell: liquid(108) and unwrapped() (every third atom a whole cell away)"""
    a, b = PF.liquid(108), PF.unwrapped()
    assert (a.cell == b.cell).all()
    return a, np.stack([a.x, b.x])


def references(xyz, cell, terms):
    """per frame the float64 Result of pair_forms_ref.evaluate; the fixture must carry no fragile pair"""
    out = []
    for x in xyz:
        assert len(PF.fragile_pairs(x, cell, terms)) == 0, "the fixture has a fragile pair at these cutoffs"
        out.append(PF.evaluate(x, np.zeros_like(x), cell, terms))
    return out


def compare(what, U, gq, gth, refs, tol, floors=None):
    """U [F], gq [F][N,3] = dU_f/dq_f, gth [F] = list of dU_f/dtheta per term: errors over the reference's scales <= tol
    (tol = a number, or MARGIN with per-frame `floors`)"""
    worst = {}
    for f, ref in enumerate(refs):
        figs = {"U": PF.error(U[f], ref, "U"), "F": PF.error(-np.asarray(gq[f], np.float64), ref, "F"),
                "dU": PF.error([np.asarray(g, np.float64) for g in gth[f]], ref, "dU")}
        for q, v in figs.items():
            allowed = tol if floors is None else tol * floors[f][q]
            _report("%-40s frame %d %-3s floor %.3e allowed %.3e figure %.3e%s" % (
                what, f, q, 0.0 if floors is None else floors[f][q], allowed, v, "" if v <= allowed else "   <-- FAILS"))
            worst[(f, q)] = (v, allowed)
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, "%s: %s" % (what, bad)


def run(obs, mods, q):
    """U, and per frame dU_f/dq_f and dU_f/dtheta (one list entry per term)"""
    q = q.clone().requires_grad_(True)
    U = obs(q)
    ps = [p for m in mods for p in m.mdg_params()]
    gq, gth = [], []
    for f in range(q.shape[0]):
        g = torch.autograd.grad(U[f], [q] + ps, retain_graph=True, allow_unused=True)
        assert all(float(g[0][k].abs().max()) == 0.0 for k in range(q.shape[0]) if k != f)
        gq.append(g[0][f].detach().cpu().numpy())
        it = iter(g[1:])
        gth.append([np.array([float(next(it)) for _ in m.mdg_params()]) for m in mods])
    return U.detach().cpu().numpy(), gq, gth


@pytest.mark.parametrize("name", list(PF.FORMS) + ["three_term"])
def test_float64_host_path_against_the_reference(name):
    fx, xyz = frames_108()
    members = members_of(name, 108)
    terms = PF.terms_of(members, 108)
    refs = references(xyz, fx.cell, terms)
    obs, mods = observable(fx, members)
    U, gq, gth = run(obs, mods, torch.as_tensor(xyz, dtype=torch.float64))
    compare(name + " float64 host", U, gq, gth, refs, TOL64)


def test_float32_host_path_runs_and_agrees_to_its_floor():
    """the same restatement in float32 (what a float32 host tensor takes): within MARGIN = 10 x the float32 floor"""
    fx, xyz = frames_108()
    members = members_of("two_cutoffs", 108)
    terms = PF.terms_of(members, 108)
    refs = references(xyz, fx.cell, terms)
    floors = [PF.floors(x, np.zeros_like(x), fx.cell, terms, ref) for x, ref in zip(xyz, refs)]
    obs, mods = observable(fx, members, dtype=torch.float32)
    U, gq, gth = run(obs, mods, torch.as_tensor(xyz))
    assert U.dtype == np.float32
    compare("two_cutoffs float32 host", U, gq, gth, refs, 10.0, floors)


def test_shapes_and_stacked_replicas():
    fx, xyz = frames_108()
    members = members_of("lj", 108)
    obs, _ = observable(fx, members)
    q = torch.as_tensor(xyz, dtype=torch.float64)
    U_T = obs(q)
    assert U_T.shape == (2,) and U_T.dtype == torch.float64
    one = obs(q[1])
    assert one.shape == () and torch.equal(one, U_T[1])
    U_RT = obs(torch.stack([q, q.flip(0), q]))
    assert U_RT.shape == (3, 2) and torch.equal(U_RT[0], U_T) and torch.equal(U_RT[1], U_T.flip(0))
    k = 3
    obs_k, _ = observable(fx, members, n_rep=k)
    qs = torch.stack([torch.cat([q[(t + r) % 2] for r in range(k)]) for t in range(2)])        # [2, 3 N, 3]
    U_k = obs_k(qs)
    assert U_k.shape == (2, k)
    for t in range(2):
        for r in range(k):
            assert torch.equal(U_k[t, r], U_T[(t + r) % 2])
    assert obs_k(qs[0]).shape == (k,)
    with pytest.raises(ValueError, match="k \\* 108"):
        obs(torch.zeros(2, 100, 3))
    with pytest.raises(ValueError):
        obs(torch.zeros(108, 2))


def test_constructor_rejections():
    from mdgrad_amd import potentials as P
    from mdgrad_amd.thermo import PotentialEnergy
    fx = PF.liquid(108)
    system = mk_system(fx.x, fx.cell)
    lj = P.LennardJones(1.0, 1.0)
    # a GNN or any other module is no PairPotentials / Stack of them
    with pytest.raises(NotImplementedError, match="Reweighting accepts any callable"):
        PotentialEnergy(system, torch.nn.Linear(2, 2))
    # a tabulated user module (pairMLP): the kernels tabulate its force, not its energy
    mlp = P.pairMLP(n_gauss=8, r_start=0.5, r_end=2.5, n_layers=1, n_width=8, nonlinear="ELU")
    with pytest.raises(NotImplementedError, match="Reweighting accepts any callable"):
        PotentialEnergy.from_terms(system, [(mlp, 2.5)])
    with pytest.raises(NotImplementedError, match="one to four"):
        PotentialEnergy.from_terms(system, [(P.LennardJones(1.0, 1.0), 2.5)] * 5)
    with pytest.raises(NotImplementedError):
        PotentialEnergy.from_terms(system, [])
    tric = mk_system(fx.x, np.array([[4.8, 0, 0], [0.6, 4.8, 0], [0, 0, 4.8]]))
    with pytest.raises(ValueError, match="diagonal"):
        PotentialEnergy.from_terms(tric, [(lj, 2.0)])
    obs = PotentialEnergy.from_terms(system, [(lj, 2.5, None, [[0, 1]])])
    assert obs._terms.n_terms == 1 and obs._terms.n_theta_total == 2 and obs._masks[0].shape == (108, 108)


def test_library_validates_energy_arguments():
    """Argument errors return -1 with a message, before anything is launched (no device needed)."""
    import ctypes as C
    from mdgrad_amd import _lib, ops
    lib = _lib.load()
    cell, tric = _lib.make_cell([5.0, 5.0, 5.0]), _lib.make_cell([[5.0, 0, 0], [1.0, 5.0, 0], [0, 0, 5.0]])
    lj = ops.make_term(dict(kind=_lib.PAIR_LJ, p=12, q=6, c=1.0), 2.5, 0, 2)
    one = ops.make_terms([lj], 2)
    morse = ops.make_terms([ops.make_term(dict(kind=_lib.PAIR_MORSE, a=3.0, phi=1.5), 2.5, 0, 0)], 0)
    buf = C.c_void_p(256)                # never dereferenced: every call below fails its checks

    def fwd(n_frames=2, n_atoms=8, c=cell, terms=one, theta=buf, U=buf, ws=buf, pos=buf):
        return lib.mdg_energy_frames_fwd(pos, n_frames, n_atoms, C.byref(c), C.byref(terms), theta, U, ws, None)

    def bwd(terms=one, gU=buf, g_pos=buf, g_theta=buf, ws=buf):
        return lib.mdg_energy_frames_bwd(buf, 2, 8, C.byref(cell), C.byref(terms), buf, gU, g_pos, g_theta, ws, None)

    table = ops.make_terms([ops.make_term(dict(kind=4, p=8), 2.5, 0, 16)], 16)
    shifted = ops.make_terms([ops.make_term(dict(kind=_lib.PAIR_LJ, p=12, q=6), 2.5, 1, 2)], 2)
    for call, word in ((lambda: fwd(c=tric), "diagonal"), (lambda: fwd(n_frames=0), "empty"), (lambda: fwd(n_atoms=0), "empty"),
                       (lambda: fwd(n_atoms=40000), "atoms"), (lambda: fwd(n_frames=1 << 24), "2^24"),
                       (lambda: fwd(theta=None), "theta"), (lambda: fwd(pos=None), "null"), (lambda: fwd(U=None), "null"),
                       (lambda: fwd(ws=None), "null"), (lambda: fwd(terms=ops.make_terms([], 0)), "terms"),
                       (lambda: fwd(terms=table), "built-in"), (lambda: bwd(terms=table), "built-in"),
                       (lambda: fwd(terms=shifted), "offset"), (lambda: bwd(gU=None), "null"), (lambda: bwd(ws=None), "null"),
                       (lambda: bwd(g_pos=None, g_theta=None), "both null"),
                       (lambda: bwd(terms=morse, g_pos=None), "without parameters")):
        rc = call()
        assert rc == -1 and word in lib.mdg_last_error().decode(), (rc, word, lib.mdg_last_error())
    assert lib.mdg_energy_frames_workspace(8192, 108, 2) == 8192 * 2
    # 16 i-blocks x 9 shells of tiles per frame, each with its row of parameter partials in the parameters-only sweep
    assert lib.mdg_energy_frames_workspace(64, 4096, 2) == 64 * 16 * 9 * 2
    assert lib.mdg_energy_frames_workspace(64, 4096, 0) == 64 * 16 * 9
    assert lib.mdg_energy_frames_workspace(3, 108, 0) == 1


@pytest.mark.skipif(not os.path.exists(TP.READELF), reason="llvm-readelf of the ROCm toolchain is needed")
def test_energy_kernels_use_no_scratch_and_the_wave_kernels_keep_four_waves(tmp_path, monkeypatch):
    monkeypatch.setattr(TP, "OBJ", os.path.join(ROOT, "mdgrad_amd", "lib", "obj", "energy.hip.o"))
    ks = TP._kernels(tmp_path)
    names = sorted(ks)
    wave = [n for n in names if "fp_frame_kernel" in n and "EnergyVisitELi64E" in n]
    assert len(wave) == 3, names                       # value, parameters-only, full rows
    for stem in ("EnergyVisitELi256ELi0E", "EnergyVisitELi256ELi1E", "EnergyVisitELi256ELi2E", "fp_tile_once_kernel",
                 "fp_tile_rows_kernel", "fp_row_sum_kernel", "fp_col_sum_kernel"):
        assert any(stem in n for n in names), "kernel %s is missing from energy.hip.o: %s" % (stem, names)
    for n, (vgprs, scratch) in ks.items():
        print("%-110s %3d VGPRs, %d B scratch" % (n, vgprs, scratch))
        assert scratch == 0, "%s uses %d B of scratch per lane" % (n, scratch)
        if n in wave:
            assert vgprs <= TP.WAVE_VGPRS, "%s: %d VGPRs" % (n, vgprs)


def test_new_sources_have_no_floating_point_atomics():
    """energy.hip and the shared sweeps have no atomics at all; rdf_frames.hip adds integers in LDS only"""
    def code(name):
        src = open(os.path.join(ROOT, "mdgrad_amd", "csrc", name)).read()
        return "\n".join(line.split("//")[0] for line in src.splitlines())
    for name in ("energy.hip", "frame_pairs.hpp"):
        assert "atomic" not in code(name).lower(), name
    rf = code("rdf_frames.hip")
    assert "unsafeAtomicAdd" not in rf and rf.count("atomicAdd(") == 1 and "atomicAdd(&hist[b], fx64(" in rf
