"""Multi-species Tersoff term, host side: tests/tersoff_multi_ref.py -- the float64 definition the GPU tests compare the kernels
with -- against an independent loop, the zincblende and diamond lattices in closed form and the one-species definition of
tests/tersoff_ref.py; TersoffMulti's torch restatement and argument checks; the table image and the validation of the C entry
points; and the input conditions of every configuration that tests/test_gpu_tersoff_multi.py evaluates."""
import ctypes
import math

import numpy as np
import pytest
import torch

import oracle as O
import tersoff_multi_ref as M
import tersoff_ref as R1


def _cpu_system(pos, cell):
    from mdgrad_amd.system import System
    return System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
                  masses=np.full(len(pos), 28.0855), device="cpu")


def _f64(v):
    return torch.tensor(np.asarray(v, dtype=np.float64))


def _tile(types, x, group):
    return np.tile(types, len(x) // (group or len(x)))


CASE_NAMES = ["sic_alloy64", "tric64", "gas37", "s3_64", "replicas", "skin", "traj", "zb_perfect"]


# ------------------------------------------------------------------------------------------------ 1: the definition
@pytest.mark.parametrize("name", CASE_NAMES)
def test_energy_equals_an_independent_loop(name):
    x32, cell32, ty, tab, group = M.gpu_cases()[name]
    ty = _tile(ty, x32, group)
    lst = M.bonds_and_triplets(x32, cell32, tab, group=group)
    uR, uA, _ = M.energy(_f64(x32), ty, tab, lst, cell32, parts=True)
    lR, lA = M.energy_loops(x32, ty, tab, cell32, group=group)
    assert abs(float(uR) - lR) <= 1e-11 * abs(lR) and abs(float(uA) - lA) <= 1e-11 * abs(lA), (float(uR), lR, float(uA), lA)
    assert lR > 0.0 and lA < 0.0


# ------------------------------------------------------------------------------------------------ 2: closed forms
def test_mixing_rules_and_closed_forms_of_sic_ge_and_sige():
    """The mixed Si-C constants, zincblende SiC at a = 4.32 (four unlike neighbours inside R - D, the second shell beyond R + D of
    the like pairs, zeta = 3 g(-1/3)), diamond germanium and zincblende SiGe at their minima; the figures are those computed
    from the published constants in float64 (Tersoff 1989 reports 6.165 eV and 4.32 A for SiC, 3.85 eV and 5.657 A for Ge)."""
    t = M.sic()
    for got, want in ((t["R"][0, 1], 2.357260), (t["D"][0, 1], 0.152720), (t["A"][0, 1], 1597.3111), (t["B"][0, 1], 395.1451)):
        assert abs(got - want) <= 1e-4 * want, (got, want)
    for k in M.PAIR_KEYS:
        assert np.array_equal(t[k], t[k].T)
    assert t["A"][0, 0] == R1.SILICON["A"] and t["B"][1, 1] == R1.CARBON["B"] and abs(t["R"][1, 1] - 1.95) < 1e-12 and abs(t["D"][0, 0] - 0.15) < 1e-12
    u, b_sic, b_csi = M.zincblende_closed_form(t, 4.32)
    assert abs(u + 6.164662) <= 2e-6 and abs(b_sic - 0.958303) <= 1e-6 and abs(b_csi - 0.883754) <= 1e-6
    a_min, u_min = M.closed_form_minimum(t, 4.32)
    assert abs(a_min - 4.3211) <= 1e-3 and abs(u_min + 6.164666) <= 2e-6
    ge = M.mixed([M.GERMANIUM])
    u, b0, b1 = M.zincblende_closed_form(ge, 5.6567, 0, 0)
    assert abs(u + 3.850600) <= 2e-6 and b0 == b1
    a_min, u_min = M.closed_form_minimum(ge, 5.6567, 0, 0)
    assert abs(a_min - 5.6567) <= 1e-3 and abs(u_min + 3.850600) <= 2e-6
    a_min, u_min = M.closed_form_minimum(M.sige(), 5.5416)
    assert abs(a_min - 5.5416) <= 1e-3 and abs(u_min + 4.231139) <= 2e-6
    # the lattice sum equals the closed form
    ty = M.zincblende(4.32)[2]
    pos, cellf = O.diamond_lattice(2, 4.32)
    lst = M.bonds_and_triplets(pos, cellf, t)
    xg = _f64(pos).requires_grad_(True)
    U = M.energy(xg, ty, t, lst, cellf)
    assert abs(float(U.detach()) / 64 - M.zincblende_closed_form(t, 4.32)[0]) <= 1e-9
    (g,) = torch.autograd.grad(U, xg)
    assert float(g.abs().max()) <= 1e-9, "the forces vanish by symmetry"
    live = M.census(pos, ty, t, cellf)
    assert live["classes"].tolist() == [[[0, 0], [0, 64 * 6]], [[64 * 6, 0], [0, 0]]], "only unlike neighbours are inside their cutoffs"


# ------------------------------------------------------------------------------------------------ 3: single-species limits
@pytest.mark.parametrize("S", [1, 2])
def test_identical_species_reduce_to_the_one_species_definition(S):
    x32, cell32, p, _ = R1.gpu_cases()["si64"]
    k = R1.consts(**p)
    lst1 = R1.bonds_and_triplets(x32, cell32, k["rc"])
    want = float(R1.energy(_f64(x32), _f64(R1.theta_of(p)), lst1, cell32, k))
    tab = M.mixed([p] * S)
    ty = np.random.default_rng(5).integers(0, S, 64)
    assert S == 1 or 0 < int(ty.sum()) < 64
    lst = M.bonds_and_triplets(x32, cell32, tab)
    got = float(M.energy(_f64(x32), ty, tab, lst, cell32))
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    if S == 2:                       # relabelling the species changes nothing either
        sw = float(M.energy(_f64(x32), 1 - ty, M.relabelled(tab, [1, 0]), lst, cell32))
        assert abs(sw - got) <= 1e-13 * abs(got)


def test_relabelled_tables_give_the_same_energy_for_unlike_species():
    x32, cell32, ty, tab, _ = M.gpu_cases()["sic_alloy64"]
    lst = M.bonds_and_triplets(x32, cell32, tab)
    a = M.evaluate(x32, ty, tab, lst, cell32)
    b = M.evaluate(x32, 1 - ty, M.relabelled(tab, [1, 0]), lst, cell32)
    assert abs(float(a["U"]) - float(b["U"])) <= 1e-13 * float(a["A_U"])
    assert float((a["grad"] - b["grad"]).abs().max()) <= 1e-13 * float(a["A_grad"].max())
    perm = torch.tensor([3, 2, 1, 0, 7, 6, 5, 4, 9, 8])          # (A, B [2, 2] transposed in both indices, h swapped)
    assert bool(((a["dth"][perm] - b["dth"]).abs() <= 1e-13 * b["A_dth"]).all()) and float(a["dth"][1]) != float(a["dth"][2])


# ------------------------------------------------------------------------------------------------ 4: the module on the host
@pytest.mark.parametrize("name", ["sic_alloy64", "s3_64", "replicas"])
def test_torch_energy_equals_the_float64_reference(name):
    from mdgrad_amd.interface import TersoffMulti
    x32, cell32, ty, tab, group = M.gpu_cases()[name]
    S = tab["S"]
    if group is None:
        system = _cpu_system(x32, cell32)
    else:
        system = _cpu_system(M.replicas16(M.SEEDS["replicas"])[0], cell32).replicate(len(x32) // group)
    mod = TersoffMulti.from_tables(system, ty, *M.pair_centre(tab))
    assert [(n, tuple(p.shape)) for n, p in mod.named_parameters()] == [("A", (S, S)), ("B", (S, S)), ("h", (S,))]
    assert not mod.supports_force_vjp() and abs(mod.cutoff - M.rc_max(tab)) <= 1e-12 and mod.n_species == S
    assert mod.types.dtype == torch.int32 and mod.types.tolist() == _tile(ty, x32, group).tolist()
    tab32 = dict(tab, **{k: getattr(mod, k).detach().double().numpy() for k in ("A", "B", "h")})       # (float32 parameters)
    lst = M.bonds_and_triplets(x32, cell32, tab, group=group)
    w = torch.tensor(np.random.default_rng(7).normal(0, 1, x32.shape))
    ref = M.evaluate(x32, _tile(ty, x32, group), tab32, lst, cell32, w=w)
    x = torch.tensor(x32).double().requires_grad_(True)
    U = mod(x)
    assert U.dtype == torch.float64
    gx, gA, gB, gh = torch.autograd.grad(U, (x, mod.A, mod.B, mod.h), create_graph=True)
    (hw,) = torch.autograd.grad((gx * w).sum(), x)
    assert abs(float(U.detach()) - float(ref["U"])) <= 1e-12 * float(ref["A_U"])
    assert float((gx.detach() - ref["grad"]).abs().max()) <= 1e-11 * float(ref["A_grad"].max())
    assert float((hw - ref["hw"]).abs().max()) <= 1e-11 * float(ref["A_hw"].max())
    got = torch.cat([t.detach().reshape(-1) for t in (gA, gB, gh)]).double()
    assert bool(((got - ref["dth"]).abs() <= 1e-6 * ref["A_dth"]).all())                              # (float32 parameters)


def test_constructors_mixing_and_frozen_parameters():
    from mdgrad_amd.interface import Tersoff, TersoffMulti
    x32, cell32, ty, tab, _ = M.gpu_cases()["sic_alloy64"]
    s = _cpu_system(x32, cell32)
    mod = TersoffMulti.silicon_carbide(s, ty, trainable=False)
    assert list(mod.parameters()) == [] and set(dict(mod.named_buffers())) >= {"A", "B", "h"}
    for k in M.PAIR_KEYS:
        assert np.allclose(mod._pair[k], tab[k], rtol=1e-14, atol=0), k
    for k in M.CENTRE_KEYS:
        assert np.array_equal(mod._centre[k], tab[k]), k
    assert mod.A.tolist() == np.float32(tab["A"]).tolist() and float(mod.B[0, 1]) == float(np.float32(tab["B"][0, 1]))
    assert TersoffMulti.PUBLISHED["germanium"] == M.GERMANIUM and TersoffMulti.PUBLISHED["silicon"] == Tersoff.PUBLISHED["silicon"]
    sg = TersoffMulti.silicon_germanium(_cpu_system(*O.diamond_lattice(2, 5.54)), ty)
    want = M.sige()
    assert np.allclose(sg._pair["B"], want["B"], rtol=1e-14, atol=0) and abs(sg.cutoff - 3.1) < 1e-12
    one = TersoffMulti(s, np.zeros(64, dtype=int), [M.SILICON])
    assert one.n_species == 1 and tuple(one.A.shape) == (1, 1)
    # the table image: derived constants, pair entries first
    img = mod._image
    assert img.dtype == np.float32 and img.shape == (8 * 2 * 3,)
    e01 = img[8:16].astype(np.float64)
    R, D = tab["R"][0, 1], tab["D"][0, 1]
    assert np.allclose(e01, [tab["A"][0, 1], tab["B"][0, 1], tab["lam1"][0, 1], tab["lam2"][0, 1], R, R - D, R + D, 0.5 * math.pi / D],
                       rtol=1e-6)
    c1 = img[32 + 8:32 + 16].astype(np.float64)
    p = M.CARBON
    cd2 = (p["c"] / p["d"]) ** 2
    assert np.allclose(c1, [p["h"], p["beta"], p["n"], -0.5 / p["n"], p["d"] ** 2, 1.0, cd2, 2.0 * cd2 * p["d"] ** 2], rtol=1e-6)
    assert torch.equal(mod._pack_tables(mod._thetas()), torch.as_tensor(img)), "the mirror's image of untouched parameters"
    doc = TersoffMulti.__doc__
    assert "Not covered" in doc and "ties their gradients" in doc and "chi lives" in doc


def test_argument_checks_raise_value_error():
    from mdgrad_amd.interface import TersoffMulti
    from mdgrad_amd import ops
    x32, cell32, ty, tab, _ = M.gpu_cases()["sic_alloy64"]
    s = _cpu_system(x32, cell32)
    two = [M.SILICON, M.CARBON]
    for args, kw, word in (((ty[:10], two), {}, "types"), ((ty + 1, two), {}, "types"), ((-ty, two), {}, "types"),
                           ((ty.astype(np.float64), two), {}, "types"),
                           ((ty, [M.SILICON] * 5), {}, "species"), ((ty, []), {}, "species"),
                           ((ty, two), dict(chi=[[1.0, 0.9], [0.8, 1.0]]), "chi"), ((ty, two), dict(chi=[[1.1, 0.9], [0.9, 1.0]]), "chi"),
                           ((ty, two), dict(chi=[[1.0]]), "chi"),
                           ((ty, [dict(M.SILICON, lam3=1.3), M.CARBON]), {}, "lam3"), ((ty, [M.SILICON, dict(M.CARBON, m=1)]), {}, "lam3"),
                           ((ty, two), dict(index_tuple=([0], [1])), "index_tuple"), ((ty, two), dict(ex_pairs=[[0, 1]]), "ex_pairs"),
                           ((ty, [dict(M.SILICON, A=0.0), M.CARBON]), {}, "A must be positive"),
                           ((ty, [dict(M.SILICON, D=0.0), M.CARBON]), {}, "D > 0"),
                           ((ty, [M.SILICON, dict(M.CARBON, n=0.0)]), {}, "n must be positive"),
                           ((ty, [M.SILICON, dict(M.CARBON, d=0.0)]), {}, "d must not be 0"),
                           ((ty, [dict(M.SILICON, R=5.4), M.CARBON]), {}, "half the shortest cell height")):
        with pytest.raises(ValueError, match=word):
            TersoffMulti(s, *args, **kw)
    five = M.mixed([M.SILICON] * 5)
    with pytest.raises(ValueError, match="at most 4"):
        TersoffMulti.from_tables(s, ty, *M.pair_centre(five))
    pair, centre = M.pair_centre(tab)
    for bad_pair, bad_centre, word in ((dict(pair, B=-pair["B"]), centre, "B must be positive"),
                                       (dict(pair, lam2=np.zeros((2, 2))), centre, "lam2"),
                                       (dict(pair, R=pair["D"]), centre, "R > D"),
                                       (dict(pair, A=pair["A"][:1]), centre, r"pair\['A'\]"),
                                       (pair, dict(centre, beta=-centre["beta"]), "beta")):
        with pytest.raises(ValueError, match=word):
            ops.tersoff_multi_tables(bad_pair, bad_centre)


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_entry_points_validate_their_arguments():
    from mdgrad_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)                  # never dereferenced: every call below fails its checks first
    cell = _lib.make_cell([11.0, 11.0, 11.0])

    def fails(rc, word):
        msg = lib.mdg_last_error()
        assert rc == -1 and word.encode() in msg, (rc, word, msg)

    ev, C = lib.mdg_tersoff_multi_eval, ctypes.byref(cell)
    #        pos n cell col shift cnt max types S tables w  energy grad hw pth pthw partial work scale acc stream
    fails(ev(None, 8, C, p, p, p, 8, p, 2, p, None, None, p, None, None, None, None, p, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, C, p, None, p, 8, p, 2, p, None, None, p, None, None, None, None, p, 1.0, 0, None), "null buffer")
    fails(ev(p, 0, C, p, p, p, 8, p, 2, p, None, None, p, None, None, None, None, p, 1.0, 0, None), "bad sizes")
    fails(ev(p, 8, C, p, p, p, 8, p, 0, p, None, None, p, None, None, None, None, p, 1.0, 0, None), "n_species")
    fails(ev(p, 8, C, p, p, p, 8, p, 5, p, None, None, p, None, None, None, None, p, 1.0, 0, None), "n_species")
    fails(ev(p, 8, C, p, p, p, 8, None, 2, p, None, None, p, None, None, None, None, p, 1.0, 0, None), "types is null")
    fails(ev(p, 8, C, p, p, p, 8, p, 2, None, None, None, p, None, None, None, None, p, 1.0, 0, None), "tables is null")
    fails(ev(p, 8, C, p, p, p, 8, p, 2, p, None, None, p, p, None, None, None, p, 1.0, 0, None), "need w")
    fails(ev(p, 8, C, p, p, p, 8, p, 2, p, p, None, p, None, None, None, None, p, 1.0, 0, None), "without hw")
    fails(ev(p, 8, C, p, p, p, 8, p, 2, p, None, None, None, None, None, None, None, p, 1.0, 0, None), "no output")
    fails(ev(p, 8, C, p, p, p, 8, p, 2, p, None, p, None, None, None, None, None, p, 1.0, 0, None), "partial")
    fails(ev(p, 8, C, p, p, p, 8, p, 2, p, None, None, p, None, None, None, None, None, 1.0, 0, None), "bond_work")
    fails(ev(p, 8, C, p, p, p, 8, p, 2, p, p, None, None, p, None, None, None, None, 1.0, 0, None), "bond_work")
    assert lib.mdg_tersoff_multi_partial_size(64) == 4 and lib.mdg_tersoff_multi_partial_size(37) == 3
    assert lib.mdg_tersoff_multi_work_size(64, 8) == 4 * 64 * 8 and lib.mdg_tersoff_multi_work_size(1 << 20, 1 << 10) == 4 << 30
    assert [lib.mdg_tersoff_multi_table_size(s) for s in (0, 1, 2, 3, 4, 5)] == [0, 16, 48, 96, 160, 0]


# ------------------------------------------------------------------------------------------------ 5: the inputs of the GPU tests
@pytest.mark.parametrize("name", CASE_NAMES)
def test_input_conditions_of_the_gpu_configurations(name):
    """Every case: no pair separation within 0.01 A of either taper edge of either ordered pair of its species (a bond there
    would make the comparison depend on the rounding of r against the edge), and the smallest separation above 1.1 A.
    The two-species alloy cases (sic_alloy64, its skin step, tric64): at least 10 directed bonds strictly inside the taper of
    each of the four ordered species pairs and each of the 8 (centre, end, third) classes at least 10 times.  s3_64: 64 atoms
    spread over 9 ordered pairs and 27 classes do not reach those counts together with the 0.01 A gap (none of 4000 seeds did);
    every pair entry is met at least 4 times inside its taper and every class occurs.  The gases (gas37, replicas) cannot
    hold 10 C-C bonds inside 1.8 - 2.1 A at their minimum separation of 2.0 A; they keep at least 10 taper bonds in all, and
    gas37 its hub row above 16, the isolated atom, the dimer with zeta = 0 and the trimer.  traj is the start of a trajectory:
    its 192 like second-shell pairs lie at 3.083 +- 0.14 A around the Si-Si edge at 3.0 A, so no seed keeps all of them 0.01 A
    off the edge; only the smallest separation is asserted (its comparison has the trajectory tolerances, not the kernel bound).
    zb_perfect is the perfect lattice: 4 neighbours each, no bond in any taper."""
    x32, cell32, ty, tab, group = M.gpu_cases()[name]
    ty = _tile(ty, x32, group)
    c = M.census(x32, ty, tab, cell32, group=group)
    print(name, c["taper"].tolist(), "gap %.4f" % c["gap"], "rows %d..%d" % (int(c["rows"].min()), int(c["rows"].max())),
          "smallest class", int(c["classes"].min()), "rmin %.3f" % c["rmin"])
    assert c["rmin"] > 1.1
    if name != "traj":
        assert c["gap"] >= 0.01, c["gap"]
    if name in ("sic_alloy64", "skin", "tric64"):
        assert c["taper"].min() >= 10 and c["classes"].min() >= 10
    if name == "s3_64":
        assert c["taper"].shape == (3, 3) and c["taper"].min() >= 4 and c["classes"].min() >= 1
    if name in ("gas37", "replicas"):
        assert c["taper"].sum() >= 10
    if name == "gas37":
        rows = c["rows"].tolist()
        assert rows[31] == 0 and rows[32] == rows[33] == 1 and rows[34:37] == [2, 1, 1] and rows[0] > 16
        lst = M.bonds_and_triplets(x32, cell32, tab)
        _, _, zeta = M.energy(_f64(x32), ty, tab, lst, cell32, parts=True)
        pair = (lst["bc"] == 32) & (lst["be"] == 33)
        assert int(pair.sum()) == 1 and float(zeta[pair]) == 0.0, "the isolated dimer"
    if name == "zb_perfect":
        assert c["rows"].tolist() == [4] * 64 and c["taper"].sum() == 0
        assert c["classes"].tolist() == [[[0, 0], [0, 384]], [[384, 0], [0, 0]]] and 4.36 / math.sqrt(2.0) > 3.0 + 0.05
    if name == "skin":
        base = M.gpu_cases()["sic_alloy64"][0]
        assert float(np.abs(x32 - base).max()) < 0.2
