"""Multi-species Stillinger-Weber term, host side.

Tests that pin the float64 definition of tests/sw_multi_ref.py -- what the GPU tests compare the kernel with -- and need nothing
of the package: the definition against an independent loop, against the one-species definition of tests/sw_ref.py, under
relabelling, on the perfect zincblende lattice in closed form, and the input conditions of every configuration that
tests/test_gpu_sw_multi.py evaluates.  These pass whether or not the package has the term.

Tests of the package, which fail without it: StillingerWeberMulti's torch restatement against the reference, the mixing rule,
the `.sw` reader, the argument checks, the cutoff that follows sigma, the table image of ops.sw_multi_tables and the validation
of the C entry points."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sw_multi_ref as R
import sw_ref as R1

CASE_NAMES = ["ab64", "asym64", "tric64", "gas37", "s3_64", "replicas", "skin", "traj"]


def _cpu_system(pos, cell, n_rep=1):
    from mdgrad_amd.system import System
    s = System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
               masses=np.full(len(pos), 28.0855), device="cpu")
    return s.replicate(n_rep) if n_rep > 1 else s


def _f64(v):
    return torch.tensor(np.asarray(v, dtype=np.float64))


def _tile(types, x, group):
    return np.tile(types, len(x) // (group or len(x)))


def _module(x, cell, types, tab, **kw):
    from mdgrad_amd.interface import StillingerWeberMulti
    pair, triplet = R.pair_triplet(tab)
    return StillingerWeberMulti.from_tables(_cpu_system(x, cell), types, pair, triplet, **kw)


# ------------------------------------------------------------------------------------------------ 1: the definition
@pytest.mark.parametrize("name", CASE_NAMES)
def test_energy_equals_an_independent_loop(name):
    x32, cell32, ty, tab, group = R.gpu_cases()[name]
    ty = _tile(ty, x32, group)
    lst = R.pairs_and_triplets(x32, cell32, tab, group=group)
    u2, u3 = R.energy(_f64(x32), ty, tab, lst, cell32, parts=True)
    l2, l3 = R.energy_loops(x32, ty, tab, cell32, group=group)
    assert abs(float(u2) - l2) <= 1e-11 * abs(l2) and abs(float(u3) - l3) <= 1e-11 * abs(l3), (float(u2), l2, float(u3), l3)
    assert l3 > 0.0


@pytest.mark.parametrize("S", [1, 2])
def test_identical_silicon_sets_reproduce_the_one_species_definition(S):
    """U, dU/dx, H w equal those of sw_ref; the parameter gradients after the chain rule of theta_one -> tables: epsilon_one
    fills epsilon[a, b] and epsilon3[a, b, c] (a constant here, so its part is recovered from lam: K = lam epsilon3 gives
    dU/depsilon3 = lam dU/dlam / epsilon3), sigma_one fills sigma[a, b], lam_one fills lam[a, b, c]:
        dU/deps_one = sum_ab dU/deps[a, b] + lam sum_abc dU/dlam[a, b, c] / eps,
        dU/dsigma_one = sum_ab dU/dsigma[a, b],   dU/dlam_one = sum_abc dU/dlam[a, b, c]."""
    x32, cell32 = R1.jittered_diamond(2, 5.431, 0.3, 64)
    ty = R.species_split(64, S, 3)
    tab = R.mixed([R.SILICON] * S)
    k = R1.consts()
    th = np.array([R.SILICON["epsilon"], R.SILICON["sigma"], R.SILICON["lam"]], dtype=np.float64)
    w = np.random.default_rng(1).normal(0, 1, x32.shape)
    lst = R.pairs_and_triplets(x32, cell32, tab)
    assert abs(R.rc_max(tab) - k["a"] * th[1]) < 1e-12
    one = R1.evaluate(x32, th, lst, cell32, k, w=w)
    got = R.evaluate(x32, ty, tab, lst, cell32, w=w)
    for key in ("U", "grad", "hw", "A_U", "A_grad", "A_hw"):
        assert float((got[key] - one[key]).abs().max()) <= 1e-11 * float(one[key].abs().max()), key
    eps, lam = th[0], th[2]
    for key in ("dth", "dthw"):
        g = got[key]
        ge, gs, gl = g[:S * S].sum(), g[S * S:2 * S * S].sum(), g[2 * S * S:].sum()
        fold = torch.stack([ge + lam * gl / eps, gs, gl])
        assert float((fold - one[key]).abs().max()) <= 1e-10 * float(one[key].abs().max()), (key, fold, one[key])


def test_relabelling_the_species_permutes_the_tables_and_nothing_else():
    x32, cell32, ty, tab, _ = R.gpu_cases()["s3_64"]
    perm = np.array([2, 0, 1])
    w = np.random.default_rng(2).normal(0, 1, x32.shape)
    lst = R.pairs_and_triplets(x32, cell32, tab)
    a = R.evaluate(x32, ty, tab, lst, cell32, w=w)
    b = R.evaluate(x32, perm[ty], R.relabelled(tab, perm), lst, cell32, w=w)
    for key in ("U", "grad", "hw"):
        assert float((a[key] - b[key]).abs().max()) <= 1e-12 * float(a[key].abs().max()), key
    S, inv = 3, np.argsort(perm)
    for key in ("dth", "dthw"):
        for lo, shape in ((0, (S, S)), (S * S, (S, S)), (2 * S * S, (S, S, S))):
            n = int(np.prod(shape))
            A, B = a[key][lo:lo + n].reshape(shape).numpy(), b[key][lo:lo + n].reshape(shape).numpy()
            assert np.abs(A[np.ix_(*([inv] * len(shape)))] - B).max() <= 1e-12 * np.abs(A).max(), key


def zincblende_tables():
    """(table set, cubic constant): Stillinger and Weber's A, B, p = 4, q = 0, a = 1.8, cos0 = -1/3; sigma_01 = 2.0951 with the
    bond length 2^(1/6) sigma_01; sigma_00 = sigma_11 = 1.9."""
    tab = R.mixed([dict(R.SILICON), dict(R.SILICON)])
    tab["sigma"][0, 0] = tab["sigma"][1, 1] = 1.9
    return tab, 2.0 ** (1.0 / 6.0) * tab["sigma"][0, 1] * 4.0 / math.sqrt(3.0)


def test_perfect_zincblende_in_closed_form():
    tab, a0 = zincblende_tables()
    x32, cell32, ty = R.zincblende(a0)
    x = np.asarray(R1.jittered_diamond(2, a0, 0.0)[0], dtype=np.float64)
    assert a0 / math.sqrt(2.0) > 1.02 * tab["a"][0, 0] * tab["sigma"][0, 0], "the second shell lies beyond the like pairs' supports"
    assert a0 / math.sqrt(2.0) > 1.02 * tab["a"][1, 1] * tab["sigma"][1, 1]
    assert abs(a0 * math.sqrt(3) / 4 - 2.0 ** (1.0 / 6.0) * tab["sigma"][0, 1]) < 1e-12
    lst = R.pairs_and_triplets(x, cell32, tab)
    assert lst["rows"].tolist() == [4] * 64
    cen = R.census(x, ty, tab, cell32)
    assert cen["pairs"].tolist() == [[0, 128], [128, 0]], "four unlike neighbours each, no like pair inside its support"
    ev = R.evaluate(x, ty, tab, lst, cell32)
    assert abs(float(ev["U"]) / 64 + 2.0 * tab["epsilon"][0, 1]) <= 1e-8 * 2.0 * tab["epsilon"][0, 1]
    # the forces vanish: 1e-4 of one product-rule term of phi2' (float32 lattice positions)
    r, sig, eps = a0 * math.sqrt(3) / 4, tab["sigma"][0, 1], tab["epsilon"][0, 1]
    t1 = eps * R.DEFAULTS["A"] * math.exp(sig / (r - 1.8 * sig)) * 4 * R.DEFAULTS["B"] * (sig / r) ** 4 / r
    assert float(ev["grad"].abs().max()) <= 1e-4 * t1


# ------------------------------------------------------------------------------------------------ 2: the module
@pytest.mark.parametrize("name", ["asym64", "s3_64", "replicas"])
def test_torch_energy_and_its_gradients_equal_the_reference(name):
    from mdgrad_amd.interface import StillingerWeberMulti
    x32, cell32, ty, tab, group = R.gpu_cases()[name]
    pair, triplet = R.pair_triplet(tab)
    if group:
        system = _cpu_system(x32[:group], cell32, len(x32) // group)
    else:
        system = _cpu_system(x32, cell32)
    mod = StillingerWeberMulti.from_tables(system, ty, pair, triplet)
    assert mod.types.tolist() == _tile(ty, x32, group).tolist()
    tab32 = R.with_theta(tab, torch.cat([p.detach().reshape(-1) for p in (mod.epsilon, mod.sigma, mod.lam)]).double().numpy())
    lst = R.pairs_and_triplets(x32, cell32, tab32, group=group)
    ref = R.evaluate(x32, _tile(ty, x32, group), tab32, lst, cell32)
    x = _f64(x32).requires_grad_(True)
    U = mod._torch_energy(x)
    assert U.dtype == torch.float64 and abs(float(U.detach()) - float(ref["U"])) <= 1e-11 * float(ref["A_U"])
    g = torch.autograd.grad(U, (x, mod.epsilon, mod.sigma, mod.lam))
    assert float((g[0] - ref["grad"]).abs().max()) <= 1e-11 * float(ref["A_grad"].max())
    got = torch.cat([t.reshape(-1) for t in g[1:]]).double()         # (float32 parameters: their gradients arrive in float32)
    assert bool(((got - ref["dth"]).abs() <= 2.0 ** -22 * ref["A_dth"] + 1e-30).all())
    assert mod(x).dtype == torch.float64, "float64 positions take the torch restatement"
    if name == "asym64":
        # the half-and-half split over lam[a, b, c], lam[a, c, b]: equal class sums times each entry's own epsilon3
        S, gl = 2, g[3].double()
        e3 = _f64(tab["epsilon3"])
        assert abs(float(gl[0, 0, 1] / e3[0, 0, 1] - gl[0, 1, 0] / e3[0, 1, 0])) <= 1e-6 * abs(float(gl[0, 0, 1] / e3[0, 0, 1]))
        assert float(gl[0, 0, 1]) != 0.0


def test_mix_follows_the_stated_rule():
    from mdgrad_amd.interface import StillingerWeberMulti as M
    sets = [dict(M.PUBLISHED["silicon"]), dict(M.PUBLISHED["mW"], gamma=1.1, cos0=-0.3, A=7.0, B=0.61, p=5, q=1, a=1.7)]
    pair, trip = M.mix(sets)
    want = R.mixed(sets)
    for k in R.PAIR_KEYS:
        assert np.allclose(pair[k], want[k], rtol=1e-14, atol=0), k
    for k in R.TRIPLET_KEYS:
        assert np.allclose(trip[k], want[k], rtol=1e-14, atol=0), k
    e, l = [s["epsilon"] for s in sets], [s["lam"] for s in sets]
    assert abs(pair["sigma"][0, 1] - 0.5 * (2.0951 + 2.3925)) < 1e-14 and abs(pair["epsilon"][0, 1] - math.sqrt(e[0] * e[1])) < 1e-14
    assert pair["A"][1, 0] == 7.0 and pair["p"][1, 0] == 5 and pair["p"][0, 1] == 4 and trip["cos0"][1, 0, 1] == -0.3
    lab, laa = math.sqrt(l[0] * l[1]), l[0]
    assert abs(trip["lam"][0, 0, 1] * trip["epsilon3"][0, 0, 1]
               - math.sqrt(laa * pair["epsilon"][0, 0] * lab * pair["epsilon"][0, 1])) < 1e-12
    assert np.array_equal(trip["lam"], trip["lam"].transpose(0, 2, 1))
    assert M.PUBLISHED["silicon"] == dict(epsilon=2.1683, sigma=2.0951, lam=21.0) and sorted(M.PUBLISHED) == ["mW", "silicon"]
    one, _ = M.mix([M.PUBLISHED["silicon"]])
    assert one["epsilon"].shape == (1, 1) and one["a"][0, 0] == 1.8


SW_LINES = {
    ("A", "A", "A"): "2.1683 2.0951 1.80 21.0 1.20 -0.333333333333 7.049556277 0.6022245584 4.0 0.0 0.0",
    ("A", "B", "B"): "1.80 2.00 1.78 19.0 1.10 -0.25 6.80 0.62 5 1 0.0",
    ("A", "A", "B"): "1.90 0.0 0.0 18.0 0.0 -0.30 0.0 0.0 0.0 0.0 0.0",
    ("A", "B", "A"): "1.95 0.0 0.0 16.0 0.0 -0.30 0.0 0.0 0.0 0.0 0.0",
    ("B", "B", "B"): "1.50 1.90 1.75 25.0 1.00 -0.40 7.30 0.58 6 0 0.0",
    ("B", "A", "A"): "1.70 1.95 1.78 23.0 1.10 -0.35 6.90 0.60 4 0 0.0",
    ("B", "A", "B"): "1.75 0.0 0.0 20.0 0.0 -0.28 0.0 0.0 0.0 0.0 0.0",
    ("B", "B", "A"): "1.65 0.0 0.0 20.5 0.0 -0.28 0.0 0.0 0.0 0.0 0.0",
}


def _write_sw(path, lines, order=None, extra=True):
    keys = list(lines) if order is None else order
    out = ["# a test file in the LAMMPS sw format", "# e1 e2 e3 epsilon sigma a lambda gamma costheta0 A B p q tol", ""]
    for n, k in enumerate(keys):
        body = lines[k].split()
        if n % 2:                                     # an entry continued over three lines, with a trailing comment
            out += [" ".join(k) + " " + " ".join(body[:4]) + "   # continued", "    " + " ".join(body[4:9]), "  " + " ".join(body[9:])]
        else:
            out.append(" ".join(k) + "  " + "  ".join(body))
    if extra:
        out += ["C A A 1.0 1.0 1.8 1.0 1.2 -0.3 7.0 0.6 4.5 0.0 0.0   # an element that is not asked for (and a non-integer p)",
                "A C B 1.0 1.0 1.8 1.0 1.2 -0.3 7.0 0.6 4 0 0.0"]
    path.write_text("\n".join(out) + "\n")
    return str(path)


def test_from_sw_file(tmp_path):
    from mdgrad_amd.interface import StillingerWeberMulti as M
    keys = list(SW_LINES)
    shuffled = [keys[k] for k in np.random.default_rng(3).permutation(len(keys))]
    path = _write_sw(tmp_path / "ab.sw", SW_LINES, shuffled)
    pair, trip = M.read_sw_file(path, ["A", "B"])
    assert pair["sigma"].tolist() == [[2.0951, 2.00], [1.95, 1.90]] and pair["epsilon"].tolist() == [[2.1683, 1.80], [1.70, 1.50]]
    assert pair["p"].tolist() == [[4, 5], [4, 6]] and pair["q"].tolist() == [[0, 1], [0, 0]] and pair["gamma"][0, 1] == 1.10
    assert pair["a"][1, 0] == 1.78 and pair["A"][1, 1] == 7.30 and pair["B"][0, 1] == 0.62
    assert trip["lam"][0].tolist() == [[21.0, 18.0], [16.0, 19.0]] and trip["lam"][1].tolist() == [[23.0, 20.0], [20.5, 25.0]]
    assert trip["epsilon3"][0].tolist() == [[2.1683, 1.90], [1.95, 1.80]] and trip["cos0"][1, 0, 1] == trip["cos0"][1, 1, 0] == -0.28
    # the elements in the other order: the tables relabelled
    pair2, trip2 = M.read_sw_file(path, ["B", "A"])
    assert pair2["sigma"].tolist() == [[1.90, 1.95], [2.00, 2.0951]] and trip2["lam"][1, 1, 0] == 18.0
    x32, cell32, ty, _, _ = R.gpu_cases()["ab64"]
    mod = M.from_sw_file(_cpu_system(x32, cell32), ty, path, ["A", "B"])
    tab = dict(S=2, **pair, **trip)
    lst = R.pairs_and_triplets(x32, cell32, tab)
    U = float(R.energy(_f64(x32), ty, tab, lst, cell32))
    assert abs(float(mod._torch_energy(_f64(x32))) - U) <= 1e-6 * abs(U)          # (float32 parameters)
    # one species out of a two-species file
    p1, t1 = M.read_sw_file(path, ["B"])
    assert p1["sigma"].tolist() == [[1.90]] and t1["lam"].tolist() == [[[25.0]]]
    # what is rejected
    missing = {k: v for k, v in SW_LINES.items() if k != ("B", "A", "B")}
    with pytest.raises(ValueError, match="B A B"):
        M.read_sw_file(_write_sw(tmp_path / "missing.sw", missing), ["A", "B"])
    with pytest.raises(ValueError, match="non-integer"):
        M.read_sw_file(_write_sw(tmp_path / "p.sw", {**SW_LINES, ("A", "B", "B"): SW_LINES[("A", "B", "B")].replace(" 5 1 ", " 4.5 1 ")}), ["A", "B"])
    with pytest.raises(ValueError, match="non-integer"):
        M.read_sw_file(path, ["A", "B", "C"])
    asym = {**SW_LINES, ("B", "B", "A"): SW_LINES[("B", "B", "A")].replace("-0.28", "-0.27")}
    with pytest.raises(ValueError, match="cos0"):
        M.from_sw_file(_cpu_system(x32, cell32), ty, _write_sw(tmp_path / "cos0.sw", asym), ["A", "B"])
    with pytest.raises(ValueError, match="twice"):
        M.read_sw_file(_write_sw(tmp_path / "twice.sw", SW_LINES, keys + [keys[0]]), ["A", "B"])
    (tmp_path / "short.sw").write_text("A A A 1.0 2.0 1.8\n")
    with pytest.raises(ValueError, match="14-token"):
        M.read_sw_file(str(tmp_path / "short.sw"), ["A"])
    with pytest.raises(ValueError, match="distinct"):
        M.read_sw_file(path, ["A", "A"])


def test_constructor_argument_checks():
    from mdgrad_amd.interface import StillingerWeberMulti as M
    x32, cell32, ty, tab, _ = R.gpu_cases()["ab64"]
    system = _cpu_system(x32, cell32)
    pair, trip = R.pair_triplet(tab)

    for k in ("epsilon", "sigma", "a", "A"):
        p = {kk: v.copy() for kk, v in pair.items()}
        p[k][0, 1] = 0.0
        with pytest.raises(ValueError, match=k):
            M.from_tables(system, ty, p, trip)
    for k, where, v in (("gamma", (1, 0), -0.1), ("p", (0, 0), 13), ("p", (0, 1), 4.5), ("q", (1, 1), -1), ("q", (0, 0), 4)):
        p = {kk: vv.copy() for kk, vv in pair.items()}
        p[k][where] = v
        with pytest.raises(ValueError):
            M.from_tables(system, ty, p, trip)
    for k, v in (("lam", -1.0), ("epsilon3", -0.5), ("cos0", 0.1)):
        t = {kk: vv.copy() for kk, vv in trip.items()}
        t[k][0, 0, 1] = v
        with pytest.raises(ValueError, match=k):
            M.from_tables(system, ty, pair, t)
    with pytest.raises(ValueError, match="lacks"):
        M.from_tables(system, ty, {k: v for k, v in pair.items() if k != "gamma"}, trip)
    with pytest.raises(ValueError):
        M.from_tables(system, ty, dict(pair, sigma=pair["sigma"][:1]), trip)
    with pytest.raises(ValueError):
        M.from_tables(system, ty, pair, dict(trip, lam=trip["lam"][:, :, :1]))
    big = dict(pair, sigma=pair["sigma"] * 1.5)
    with pytest.raises(ValueError, match="half the shortest cell height"):
        M.from_tables(system, ty, big, trip)
    for types in (ty[:63], ty.astype(np.float64), np.where(ty == 1, 2, ty), -ty):
        with pytest.raises(ValueError, match="types"):
            M.from_tables(system, types, pair, trip)
    with pytest.raises(ValueError, match="index_tuple"):
        M.from_tables(system, ty, pair, trip, index_tuple=[[0, 1]])
    with pytest.raises(ValueError, match="ex_pairs"):
        M.from_tables(system, ty, pair, trip, ex_pairs=torch.zeros(1, 2))
    si = M.PUBLISHED["silicon"]
    with pytest.raises(ValueError, match="1 to 4"):
        M(system, ty, [si] * 5)
    with pytest.raises(ValueError, match="1 to 4"):
        M(system, ty, [])
    with pytest.raises(ValueError, match="lacks lam"):
        M(system, ty, [si, dict(epsilon=1.0, sigma=2.0)])
    with pytest.raises(ValueError, match="unknown"):
        M(system, ty, [si, dict(si, chi=1.0)])
    with pytest.raises(ValueError):
        M(system, ty, [si, dict(si, p=4.5)])
    frozen = M(system, ty, [si, si], trainable=False)
    assert list(frozen.parameters()) == [] and frozen.lam.shape == (2, 2, 2) and frozen.n_species == 2
    assert abs(frozen.cutoff - 1.02 * 1.8 * float(np.float32(2.0951))) < 1e-5


def test_a_sigma_that_outgrows_the_cell_is_rejected_when_the_cutoff_follows_it():
    from mdgrad_amd.interface import StillingerWeberMulti as M
    x32, cell32, ty, tab, _ = R.gpu_cases()["ab64"]
    mod = M.from_tables(_cpu_system(x32, cell32), ty, *R.pair_triplet(tab))
    c0, v0 = mod.cutoff, mod.static_version()
    with torch.no_grad():
        mod.sigma[0, 1] = 2.30
    mod.prepare_pass()
    assert abs(mod.cutoff - 1.02 * 1.78 * float(mod.sigma[0, 1].detach())) < 1e-5 and mod.cutoff > c0 and mod.static_version() != v0
    with torch.no_grad():
        mod.sigma[0, 1] = 3.2                      # a sigma = 5.70 A > half the cell height 5.431 A
    with pytest.raises(ValueError, match="half the shortest cell height"):
        mod.prepare_pass()
    with torch.no_grad():
        mod.sigma[0, 1] = -1.0
    with pytest.raises(ValueError, match="positive"):
        mod.prepare_pass()


def test_table_image():
    from mdgrad_amd import ops
    tab = R.asym2()
    img = ops.sw_multi_tables(*R.pair_triplet(tab))
    assert img.dtype == np.float32 and img.shape == (12 * 4 + 4 * 8,)
    P, T3 = img[:48].reshape(2, 2, 12), img[48:].reshape(2, 2, 2, 4)
    f = np.float32
    assert P[0, 1, 0] == f(1.90) and P[1, 0, 1] == f(1.95) and P[0, 1, 2] == f(1.78) * f(2.05) and P[0, 1, 3] == f(1.10) * f(2.05)
    assert P[0, 1, 7] == 5 and P[0, 1, 8] == 1 and P[1, 1, 10] == f(7.30) * f(1.50) and P[0, 0, 11] == 0
    K = 0.5 * (19.0 * 1.90 + 16.0 * 1.90)
    assert abs(T3[0, 0, 1, 0] - K) <= 1e-6 * K and T3[0, 0, 1, 0] == T3[0, 1, 0, 0] and T3[0, 0, 1, 1] == f(-0.30)
    assert T3[0, 0, 1, 2] == f(0.5) * f(1.90) and T3[0, 1, 1, 2] == f(1.70)


# ------------------------------------------------------------------------------------------------ 3: the C entry points
def test_c_entry_points_validate_their_arguments():
    from mdgrad_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)                  # never dereferenced: every call below fails its checks first
    cell = _lib.make_cell([11.0, 11.0, 11.0])

    def fails(rc, word):
        msg = lib.mdg_last_error()
        assert rc == -1 and word.encode() in msg, (rc, word, msg)

    ev, C = lib.mdg_sw_multi_eval, ctypes.byref(cell)
    #        pos n cell col shift cnt max types S tables w  energy grad hw pth pthw partial scale acc stream
    fails(ev(None, 8, C, p, p, p, 8, p, 2, p, None, None, p, None, None, None, None, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, C, p, None, p, 8, p, 2, p, None, None, p, None, None, None, None, 1.0, 0, None), "null buffer")
    fails(ev(p, 0, C, p, p, p, 8, p, 2, p, None, None, p, None, None, None, None, 1.0, 0, None), "bad sizes")
    fails(ev(p, 8, C, p, p, p, 0, p, 2, p, None, None, p, None, None, None, None, 1.0, 0, None), "bad sizes")
    fails(ev(p, 8, C, p, p, p, 8, p, 0, p, None, None, p, None, None, None, None, 1.0, 0, None), "n_species")
    fails(ev(p, 8, C, p, p, p, 8, p, 5, p, None, None, p, None, None, None, None, 1.0, 0, None), "n_species")
    fails(ev(p, 8, C, p, p, p, 8, None, 2, p, None, None, p, None, None, None, None, 1.0, 0, None), "types is null")
    fails(ev(p, 8, C, p, p, p, 8, p, 2, None, None, None, p, None, None, None, None, 1.0, 0, None), "tables is null")
    fails(ev(p, 8, C, p, p, p, 8, p, 2, p, None, None, p, p, None, None, None, 1.0, 0, None), "need w")
    fails(ev(p, 8, C, p, p, p, 8, p, 2, p, None, None, p, None, None, p, None, 1.0, 0, None), "need w")
    fails(ev(p, 8, C, p, p, p, 8, p, 2, p, p, None, p, None, None, None, None, 1.0, 0, None), "without hw")
    fails(ev(p, 8, C, p, p, p, 8, p, 2, p, None, None, None, None, None, None, None, 1.0, 0, None), "no output")
    fails(ev(p, 8, C, p, p, p, 8, p, 2, p, None, p, None, None, None, None, None, 1.0, 0, None), "partial")
    assert lib.mdg_sw_multi_partial_size(64) == 4 and lib.mdg_sw_multi_partial_size(37) == 3 and lib.mdg_sw_multi_partial_size(0) == 0
    assert [lib.mdg_sw_multi_table_size(s) for s in (0, 1, 2, 3, 4, 5)] == [0, 16, 80, 216, 448, 0]


# ------------------------------------------------------------------------------------------------ 4: the inputs of the GPU tests
@pytest.mark.parametrize("name", CASE_NAMES)
def test_input_conditions_of_the_gpu_configurations(name):
    """Every case but gas37 and traj: each ordered pair class and each (centre, {end, end}) class holds at least 20 terms inside
    its support.  gas37 keeps its row lengths instead: the hub's row above 16, the isolated atom, the dimer, the trimer, and an
    atom count that is no multiple of 16.  traj is the start of a trajectory on a jittered zincblende lattice, whose second
    shell (like atoms at 3.84 A) lies at or beyond the supports of the like pairs (3.77 and 3.33 A): the classes the lattice
    has -- the unlike pairs and the triplets with two unlike ends -- hold at least 20 terms, and nothing is asked of the rest.
    asym64: pairs with a_10 sigma_10 < r < a_01 sigma_01 exist.  skin: the move is shorter than 0.2 A.
    Every case: rounding the cutoffs a_ab sigma_ab to float32 moves no component of the float64 dU/dx by more than 8 * 2^-24 A
    (sw_multi_ref.cutoff_rounding): an eighth of the GPU tests' bound for a representation error that no float32 evaluation
    can avoid.  The configurations it excludes hold an atom whose only terms lie a few tenths of an Angstrom inside a cutoff
    (the first gas37 seed: one pair at 3.352 A under a cutoff of 3.56 A, 18 * 2^-24 A from the cutoff's rounding alone)."""
    cases = R.gpu_cases()
    x32, cell32, ty, tab, group = cases[name]
    cen = R.census(x32, _tile(ty, x32, group), tab, cell32, group=group)
    assert R.cutoff_rounding(x32, _tile(ty, x32, group), tab, cell32, group=group) <= 8.0
    rows = cen["rows"].tolist()
    if name == "gas37":
        assert rows[31] == 0 and rows[32] == rows[33] == 1 and rows[34] == 2 and rows[0] > 16 and len(rows) % 16 != 0
        assert ty[0] == ty[32] == ty[33] == 0
    elif name == "traj":
        assert cen["pairs"][0, 1] >= 20 and cen["pairs"][1, 0] >= 20 and cen["classes"][0, 1, 1] >= 20 and cen["classes"][1, 0, 0] >= 20
    else:
        assert R.populated(cen, 20), (cen["pairs"], cen["classes"])
    if name == "asym64":
        lo, hi = tab["a"][1, 0] * tab["sigma"][1, 0], tab["a"][0, 1] * tab["sigma"][0, 1]
        assert lo < hi
        unlike = cen["ti"] != cen["tj"]
        assert int((unlike & (cen["r"] > lo) & (cen["r"] < hi)).sum()) >= 5, "pairs inside one direction's support only"
        assert tab["lam"][0, 0, 1] != tab["lam"][0, 1, 0] and tab["epsilon"][0, 1] != tab["epsilon"][1, 0]
    if name == "skin":
        move = np.linalg.norm(x32.astype(np.float64) - cases["ab64"][0], axis=1)
        assert 0.0 < move.max() < 0.2
    if name == "s3_64":
        rc = np.diag(tab["a"] * tab["sigma"])
        assert len(set(np.round(rc, 6))) == 3, "three different cutoffs"
    if name == "replicas":
        assert group == 16 and len(x32) == 48
    if name == "ab64":
        flat = lambda k: [tab[k][0, 0], tab[k][0, 1], tab[k][1, 1]]
        for k in ("sigma", "epsilon", "a", "gamma", "p"):
            assert len(set(flat(k))) == 3, k
        six = lambda k: [tab[k][a, b, c] for a in range(2) for b in range(2) for c in range(b, 2)]
        assert len(set(six("cos0"))) == 6 and len(set(six("lam"))) == 6


def test_the_skin_list_carries_extra_candidates():
    """The pairs of `skin` inside rc + 0.4 A outnumber those inside rc (rc = the list cutoff 1.02 max a sigma)."""
    import coulomb_ref as C
    x32, cell32, ty, tab, _ = R.gpu_cases()["skin"]
    rc = 1.02 * R.rc_max(tab)
    n_exact = C.half_list(x32, cell32, rc)[0].numel()
    n_skin = C.half_list(x32, cell32, rc + 0.4)[0].numel()
    assert n_skin > n_exact + 20
