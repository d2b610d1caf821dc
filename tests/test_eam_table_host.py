"""Tabulated embedded-atom term, host side: tests/eam_table_ref.py -- the float64 definition the GPU tests compare the kernels
with -- against an independent loop and the properties of the interpolant; EAM's torch restatement, its constructors (Python
callables, the Sutton-Chen twin, setfl files) and argument checks; the validation of the C entry point."""
import ctypes
import io
import math

import numpy as np
import pytest
import torch

import eam_ref as SC
import eam_table_ref as R

CU = SC.PUBLISHED["copper"]
RC, RMIN = 5.2, 1.8


def _cpu_system(pos, cell):
    from mdgrad_amd.system import System
    return System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
                  masses=np.full(len(pos), 63.546), device="cpu")


def _two_species_functions():
    """Three phi, two f and two F that are all different; f_0 and f_1 differ by more than a factor of 2."""
    pair = [lambda r: 0.9 * torch.exp(-1.3 * (r - 2.5)) - 0.2, lambda r: 1.4 * torch.exp(-1.1 * (r - 2.4)) - 0.3 / r,
            lambda r: 0.6 * torch.exp(-1.7 * (r - 2.6)) + 0.05 * r]
    density = [lambda r: 1.1 * torch.exp(-0.9 * (r - 2.5)), lambda r: 3.1 * torch.exp(-1.2 * (r - 2.5))]
    embed = [lambda p: -1.2 * torch.sqrt(p + 0.5) + 0.01 * p * p, lambda p: -0.8 * torch.log(p + 1.0) + 0.03 * p]
    return pair, density, embed


def _alloy(n_r=48, n_rho=40, seed=11, dtype=torch.float64, **kw):
    from mdgrad_amd.interface import EAM
    x32, cell32 = SC.jittered_fcc(3, 3.61, 0.15, seed)
    types = np.arange(108) % 2
    pair, density, embed = _two_species_functions()
    mod = EAM.from_functions(_cpu_system(x32, cell32), types, pair, density, embed, RC, RMIN, (2.0, 60.0), n_r, n_rho, dtype=dtype, **kw)
    return mod, x32, cell32, types


# ------------------------------------------------------------------------------------------------ the interpolant
def test_interpolant_equals_an_independent_loop_and_reproduces_cubics():
    rng = np.random.default_rng(3)
    n, x0, h = 9, 1.5, 0.25
    nodes = torch.tensor(rng.normal(0, 1, (2, n, 2)))
    x = torch.tensor(np.concatenate([rng.uniform(x0 - 1.0, x0 + (n - 1) * h + 1.0, 200), x0 + h * np.arange(n)]))
    for k in range(2):
        got = R.interp(nodes, torch.full_like(x, k, dtype=torch.long), x, x0, h)
        want = R.interp_loop(nodes[k].tolist(), x.tolist(), x0, h)
        assert float((got - torch.tensor(want)).abs().max()) <= 1e-13
    # a cubic polynomial is reproduced exactly inside the grid, and continued by its end tangents outside
    c = [0.3, -1.1, 0.7, 0.45]
    poly = lambda v: c[0] + c[1] * v + c[2] * v ** 2 + c[3] * v ** 3
    dpoly = lambda v: c[1] + 2 * c[2] * v + 3 * c[3] * v ** 2
    xg = x0 + h * torch.arange(n, dtype=torch.float64)
    cub = torch.stack([poly(xg), h * dpoly(xg)], -1)[None]
    inside = x[(x >= x0) & (x <= x0 + (n - 1) * h)]
    zero = torch.zeros_like(inside, dtype=torch.long)
    assert float((R.interp(cub, zero, inside, x0, h) - poly(inside)).abs().max()) <= 1e-13
    lo, hi = torch.tensor([x0 - 0.7], dtype=torch.float64), torch.tensor([x0 + (n - 1) * h + 0.9], dtype=torch.float64)
    z1 = torch.zeros(1, dtype=torch.long)
    assert abs(float(R.interp(cub, z1, lo, x0, h)) - float(poly(xg[0]) - 0.7 * dpoly(xg[0]))) <= 1e-13
    assert abs(float(R.interp(cub, z1, hi, x0, h)) - float(poly(xg[-1]) + 0.9 * dpoly(xg[-1]))) <= 1e-13


def test_interpolant_is_c1_at_the_nodes_and_at_both_ends():
    from mdgrad_amd.interface import _hermite
    rng = np.random.default_rng(4)
    n, x0, h = 7, 0.5, 0.4
    nodes = torch.tensor(rng.normal(0, 1, (1, n, 2)))
    xg = x0 + h * torch.arange(n, dtype=torch.float64)
    eps = 1e-7
    curv = float(12 * nodes[0, :, 0].abs().max() + 6 * nodes[0, :, 1].abs().max()) / h ** 2          # >= |second derivative| of a cell
    for fn in (R.interp, _hermite):
        for side in (-eps, eps):
            x = (xg + side).requires_grad_(True)
            v = fn(nodes, torch.zeros(n, dtype=torch.long), x, x0, h)
            (dv,) = torch.autograd.grad(v.sum(), x)
            assert float((v.detach() - (nodes[0, :, 0] + side * nodes[0, :, 1] / h)).abs().max()) <= eps ** 2 * curv, "value at a node"
            assert float((dv - nodes[0, :, 1] / h).abs().max()) <= eps * curv, "slope on both sides of every node, the ends included"
    x = torch.tensor(rng.uniform(x0 - 1, x0 + n * h, 50))
    z = torch.zeros(50, dtype=torch.long)
    assert float((_hermite(nodes, z, x, x0, h) - R.interp(nodes, z, x, x0, h)).abs().max()) <= 1e-13
    # the basis derivatives the error scales use are the derivatives of the basis
    t = torch.tensor(rng.uniform(-0.5, 1.5, 40), requires_grad=True)
    for order in range(3):
        b = R.basis(t, order)
        for k in range(4):
            (d,) = torch.autograd.grad(b[:, k].sum(), t, retain_graph=True, allow_unused=True)
            d = torch.zeros_like(t) if d is None else d
            assert float((d - R.basis(t, order + 1)[:, k]).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ the Sutton-Chen twin
def test_sutton_chen_twin_converges_as_h4_to_the_analytic_term():
    from mdgrad_amd.interface import EAM
    x32, cell32 = SC.jittered_fcc(3, 3.61, 0.15, 108)
    k = SC.consts(CU[3], CU[4], RC, "force")
    lst = SC.pairs(x32, cell32, RC)
    x = torch.tensor(x32).double()
    want = float(SC.energy(x, torch.tensor(CU[:3], dtype=torch.float64), lst, cell32, k))
    _, rho = SC.density(x, CU[1], lst, cell32, k)
    rr = (0.5 * float(rho.min()), 1.5 * float(rho.max()))
    errs = []
    for n in (64, 128, 256):
        mod = EAM.from_sutton_chen(_cpu_system(x32, cell32), "copper", cutoff=RC, r_min=RMIN, n_r=n, n_rho=n, dtype=torch.float64)
        assert mod.rho_range == pytest.approx(rr, rel=1e-12), "the default rho grid is (rho_lo / 2, 3 rho_hi / 2) of the system"
        assert mod.pin_cutoff and float(mod.pair_nodes[0, -1].detach().abs().max()) == 0.0 and float(mod.density_nodes[0, -1].detach().abs().max()) == 0.0
        errs.append(abs(float(mod(x)) - want))
    print("tabulation error of U at 64, 128, 256 nodes:", errs, "U =", want)
    assert errs[0] < 1e-3 * abs(want)
    for a, b in zip(errs[:-1], errs[1:]):
        assert 12.0 <= a / b <= 20.0, "error ratio per halving of h: %.2f" % (a / b)
    with pytest.raises(ValueError, match="rho_min must be positive"):
        EAM.from_sutton_chen(_cpu_system(x32, cell32), "copper", cutoff=RC, rho_range=(0.0, 30.0))
    with pytest.raises(ValueError, match="rho_min must be positive"):
        EAM.from_sutton_chen(_cpu_system(x32, cell32), CU, cutoff=RC, rho_range=(-1.0, 30.0))
    with pytest.raises(ValueError, match="shift"):
        EAM.from_sutton_chen(_cpu_system(x32, cell32), "copper", cutoff=RC, shift="energy")
    pub = EAM.from_sutton_chen(_cpu_system(x32, cell32), "copper", cutoff=RC, shift="none", n_r=64, n_rho=64)
    assert not pub.pin_cutoff and float(pub.pair_nodes[0, -1, 0]) > 0.0, "as published the functions do not vanish at rc"


# ------------------------------------------------------------------------------------------------ the module on the host
def test_torch_energy_equals_the_float64_reference_for_two_species():
    mod, x32, cell32, types = _alloy(pin_cutoff=False)
    assert [n for n, _ in mod.named_parameters()] == ["pair_nodes", "density_nodes", "embed_nodes"] and not mod.supports_force_vjp()
    assert [tuple(p.shape) for p in mod.parameters()] == [(3, 48, 2), (2, 48, 2), (2, 40, 2)]
    g, tabs = R.grid_of(mod), R.tables_of(mod)
    lst = R.pairs(x32, cell32, RC)
    w = torch.tensor(np.random.default_rng(7).normal(0, 1, x32.shape))
    ref = R.evaluate(x32, [p.detach().double() for p in mod.parameters()], lst, cell32, types, g, w=w)
    x = torch.tensor(x32).double().requires_grad_(True)
    U = mod(x)
    assert U.dtype == torch.float64
    gs = torch.autograd.grad(U, [x] + list(mod.parameters()), create_graph=True)
    hs = torch.autograd.grad((gs[0] * w).sum(), [x] + list(mod.parameters()))
    assert abs(float(U.detach()) - float(ref["U"])) <= 1e-12 * float(ref["A_U"])
    assert float((gs[0].detach() - ref["grad"]).abs().max()) <= 1e-12 * float(ref["A_grad"].max())
    assert float((hs[0] - ref["hw"]).abs().max()) <= 1e-12 * float(ref["A_hw"].max())
    assert float((R.flat([t.detach() for t in gs[1:]]) - ref["gtab"]).abs().max()) <= 1e-12 * float(ref["A_gtab"].max())
    assert float((R.flat(hs[1:]) - ref["gtabw"]).abs().max()) <= 1e-12 * float(ref["A_gtabw"].max())
    assert bool((ref["gtab"].abs() <= ref["A_gtab"] * (1 + 1e-12)).all()) and bool((ref["gtabw"].abs() <= ref["A_gtabw"] * (1 + 1e-12)).all())
    assert bool((ref["grad"].abs() <= ref["A_grad"] * (1 + 1e-12)).all()) and bool((ref["hw"].abs() <= ref["A_hw"] * (1 + 1e-12)).all())
    # a swapped density table is a different potential
    sw = [tabs[0], tabs[1].flip(0), tabs[2]]
    assert abs(float(R.energy(x.detach(), sw, lst, cell32, types, g)) - float(ref["U"])) > 1e-3 * abs(float(ref["U"]))
    # replicas do not see each other
    from mdgrad_amd.interface import EAM
    rep = _cpu_system(x32, cell32).replicate(2)
    x2 = np.concatenate([x32, SC.jittered_fcc(3, 3.61, 0.12, 12)[0]])
    m2 = EAM(rep, types, *[p.detach() for p in mod.parameters()], RC, RMIN, (2.0, 60.0), pin_cutoff=False, trainable=False,
             dtype=torch.float64)
    assert list(m2.parameters()) == [] and set(dict(m2.named_buffers())) >= {"pair_nodes", "density_nodes", "embed_nodes"}
    lst2 = R.pairs(x2, cell32, RC, group=108)
    want = float(R.energy(torch.tensor(x2).double(), [p.double() for p in m2._nodes()], lst2, cell32,
                          np.tile(types, 2), g))
    assert abs(float(m2(torch.tensor(x2).double())) - want) <= 1e-12 * abs(want)


def test_node_gradient_equals_finite_differences_and_pinned_nodes_have_none():
    mod, x32, cell32, types = _alloy(n_r=24, n_rho=16, trainable=("density", "embed"))
    assert [n for n, _ in mod.named_parameters()] == ["density_nodes", "embed_nodes"] and mod.pin_cutoff
    assert float(mod.pair_nodes[:, -1].abs().max()) == 0.0 and float(mod.density_nodes[:, -1].abs().max()) == 0.0
    x = torch.tensor(x32).double()
    gd, ge = torch.autograd.grad(mod(x), (mod.density_nodes, mod.embed_nodes))
    assert float(gd[:, -1].abs().max()) == 0.0, "the pinned last node of every f table"
    assert float(gd[:, :-1].abs().max()) > 0.0 and float(ge.abs().max()) > 0.0
    rng = np.random.default_rng(5)
    for p, gp in ((mod.density_nodes, gd), (mod.embed_nodes, ge)):
        flat, gflat = p.data.view(-1), gp.reshape(-1)
        hot = torch.nonzero(gflat).reshape(-1)
        for k in rng.choice(hot.numel(), 6, replace=False):
            k, step = int(hot[k]), 1e-5
            old = float(flat[k])
            flat[k] = old + step
            up = float(mod(x))
            flat[k] = old - step
            dn = float(mod(x))
            flat[k] = old
            fd = (up - dn) / (2 * step)
            assert abs(fd - float(gflat[k])) <= 1e-6 * max(abs(fd), 1.0), (k, fd, float(gflat[k]))
    # an empty row: rho = 0 and F_a(0) from the table (here by the linear continuation below rho_min = 2)
    from mdgrad_amd.interface import EAM
    pos = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 4.0], [9.0, 9.0, 9.0]])
    pair, density, embed = _two_species_functions()
    lone = EAM.from_functions(_cpu_system(pos, [16.0] * 3), [0, 1, 1], pair, density, embed, 5.0, RMIN, (2.0, 60.0), 32, 32,
                              dtype=torch.float64)
    xl = torch.tensor(pos, requires_grad=True)
    U = lone(xl)
    (gx,) = torch.autograd.grad(U, xl)
    en = lone.embed_nodes.detach()
    F1_at_0 = float(en[1, 0, 0] + (0.0 - 2.0) / lone.h_rho * en[1, 0, 1])
    assert float(gx[2].abs().max()) == 0.0 and float(gx[0].abs().max()) > 0.0
    lst = R.pairs(pos, [16.0] * 3, 5.0)
    _, rho = R.density(torch.tensor(pos), R.tables_of(lone), lst, [16.0] * 3, [0, 1, 1], R.grid_of(lone))
    assert float(rho[2]) == 0.0
    parts = R.interp(en, torch.tensor([0, 1, 1]), rho, 2.0, lone.h_rho)
    assert abs(float(parts[2]) - F1_at_0) <= 1e-12 and F1_at_0 != 0.0


# ------------------------------------------------------------------------------------------------ setfl
def test_setfl_round_trip_and_five_point_slopes(tmp_path):
    from mdgrad_amd.interface import EAM
    x32, cell32 = SC.jittered_fcc(3, 3.61, 0.1, 21)
    types = np.arange(108) % 2
    s = _cpu_system(x32, cell32)
    f = [lambda r: 1.1 * np.exp(-0.9 * (r - 2.5)), lambda r: 3.1 * np.exp(-1.2 * (r - 2.5))]
    df = [lambda r: -0.9 * 1.1 * np.exp(-0.9 * (r - 2.5)), lambda r: -1.2 * 3.1 * np.exp(-1.2 * (r - 2.5))]
    F = [lambda p: -1.2 * np.sqrt(p + 8.0) + 0.01 * p * p, lambda p: -0.8 * np.log(p + 10.0) + 0.03 * p]
    dF = [lambda p: -0.6 / np.sqrt(p + 8.0) + 0.02 * p, lambda p: -0.8 / (p + 10.0) + 0.03]
    phi = [lambda r: 0.9 * np.exp(-1.3 * (r - 2.5)) - 0.2, lambda r: 1.4 * np.exp(-1.1 * (r - 2.4)) - 0.3 * r,
           lambda r: 0.6 * np.exp(-1.7 * (r - 2.6)) + 0.05 * r]
    dphi = [lambda r: -1.3 * 0.9 * np.exp(-1.3 * (r - 2.5)), lambda r: -1.1 * 1.4 * np.exp(-1.1 * (r - 2.4)) - 0.3,
            lambda r: -1.7 * 0.6 * np.exp(-1.7 * (r - 2.6)) + 0.05]
    worst = []
    for n in (101, 201):
        d_r, d_rho, cutoff = 5.0 / (n - 1), 60.0 / (n - 1), 4.99         # (the file's cutoff lies between two grid points)
        path = str(tmp_path / ("alloy%d.setfl" % n))
        wrote = R.write_setfl(path, ["Cu", "Ni"], phi, f, F, n, d_rho, n, d_r, cutoff)
        mod = EAM.from_setfl(s, types, path, dtype=torch.float64)
        gc = n - 2
        assert mod.n_species == 2 and mod.n_rho == n and mod.n_r == gc and not mod.pin_cutoff and mod.elements == ["Cu", "Ni"]
        assert mod.r_min == pytest.approx(d_r, rel=1e-15) and mod.cutoff == pytest.approx(gc * d_r, rel=1e-14) and mod.cutoff <= cutoff
        assert mod.rho_range == (0.0, pytest.approx(60.0, rel=1e-14))
        r, rho = d_r * np.arange(1, gc + 1), d_rho * np.arange(n)
        pn, dn, en = (v.detach().numpy() for v in mod._nodes())
        near = int(round(1.0 / d_r))
        assert np.array_equal(en[:, :, 0], wrote["F"]) and np.array_equal(dn[:, :, 0], wrote["f"][:, 1:gc + 1]), "node values are the file's"
        assert np.array_equal(pn[:, :, 0], wrote["z2r"][:, 1:gc + 1] / r)
        assert np.array_equal(mod.density_at_origin, wrote["f"][:, 0])
        err = max(max(np.abs(dn[a, 1:-1, 1] / d_r - df[a](r[1:-1])).max() / np.abs(df[a](r)).max() for a in range(2)),
                  max(np.abs(en[a, 2:-2, 1] / d_rho - dF[a](rho[2:-2])).max() / np.abs(dF[a](rho)).max() for a in range(2)),
                  # (phi' = ((r phi)' - phi) / r: the error of (r phi)' is divided by r, so the first points, r of a few d_r,
                  # are third order; the check starts at r = 1)
                  max(np.abs(pn[p, near:-1, 1] / d_r - dphi[p](r[near:-1])).max() / np.abs(dphi[p](r[near:])).max() for p in range(3)))
        worst.append(err)
        back = io.StringIO()
        mod.write_setfl(back)
        again = EAM.read_setfl(io.StringIO(back.getvalue()))
        first = EAM.read_setfl(path)
        assert again["elements"] == first["elements"] and (again["n_rho"], again["n_r"]) == (n, gc + 1)
        assert np.array_equal(again["F"], first["F"]) and np.array_equal(again["f"], first["f"][:, :gc + 1])
        assert float(np.abs(again["z2r"] - first["z2r"][:, :gc + 1]).max()) <= 4e-16 * float(np.abs(first["z2r"]).max())
        assert again["d_r"] == pytest.approx(d_r, rel=1e-15) and again["cutoff"] == pytest.approx(gc * d_r, rel=1e-14)
        # a species subset, re-ordered
        ni = EAM.from_setfl(s, np.zeros(108, dtype=np.int64), path, elements=["Ni"], dtype=torch.float64)
        assert ni.n_species == 1 and np.array_equal(ni.embed_nodes.detach().numpy()[0, :, 0], wrote["F"][1])
        assert np.array_equal(ni.pair_nodes.detach().numpy()[0, :, 0], wrote["z2r"][2, 1:gc + 1] / r)
    # the five-point formula is fourth order inside: its error against the analytic derivative falls ~16-fold per halving
    print("five-point slope error (relative to the largest slope) at 101, 201 points:", worst)
    assert worst[0] < 1e-5 and 10.0 <= worst[0] / worst[1] <= 20.0, worst
    with pytest.raises(ValueError, match="holds"):
        EAM.from_setfl(s, types, path, elements=["Cu", "Ag"])
    with pytest.raises(ValueError, match="setfl"):
        EAM.read_setfl(io.StringIO("one\ntwo\n"))
    with pytest.raises(ValueError, match="starts at 0"):
        _alloy()[0].write_setfl(io.StringIO())


# ------------------------------------------------------------------------------------------------ rejections
def test_argument_checks_raise_value_error():
    from mdgrad_amd.interface import EAM
    x32, cell32 = SC.jittered_fcc(3, 3.61, 0.0)
    s = _cpu_system(x32, cell32)
    ty = np.arange(108) % 2
    good = dict(types=ty, pair_nodes=np.zeros((3, 8, 2)), density_nodes=np.zeros((2, 8, 2)), embed_nodes=np.zeros((2, 6, 2)),
                cutoff=RC, r_min=RMIN, rho_range=(0.0, 10.0))
    assert EAM(s, **good).cutoff == RC
    for kw, word in ((dict(index_tuple=([0], [1])), "index_tuple"), (dict(ex_pairs=[[0, 1]]), "ex_pairs"),
                     (dict(cutoff=5.5), "half the shortest cell height"), (dict(cutoff=1.8), "r_min < cutoff"),
                     (dict(r_min=-0.1), "r_min < cutoff"), (dict(rho_range=(3.0, 3.0)), "rho_min < rho_max"),
                     (dict(rho_range=(3.0,)), "rho_range"), (dict(pair_nodes=np.zeros((2, 8, 2))), "pair_nodes is"),
                     (dict(pair_nodes=np.zeros((3, 9, 2))), "pair_nodes is"), (dict(embed_nodes=np.zeros((3, 6, 2))), "embed_nodes"),
                     (dict(embed_nodes=np.zeros((2, 6))), "nodes, 2"), (dict(embed_nodes=np.zeros((2, 3, 2))), "node counts"),
                     (dict(density_nodes=np.zeros((2, 3, 2)), pair_nodes=np.zeros((3, 3, 2))), "node counts"),
                     (dict(embed_nodes=np.zeros((2, 4097, 2))), "node counts"),
                     (dict(density_nodes=np.zeros((5, 8, 2)), pair_nodes=np.zeros((15, 8, 2)), embed_nodes=np.zeros((5, 6, 2))), "species"),
                     (dict(density_nodes=np.full((2, 8, 2), np.nan)), "finite"), (dict(types=ty[:100]), "one entry per atom"),
                     (dict(types=ty + 1), "integers in"), (dict(types=ty.astype(np.float64)), "integers in"),
                     (dict(trainable=("embed", "charge")), "trainable")):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            EAM(s, **args)
    pair, density, embed = _two_species_functions()
    with pytest.raises(ValueError, match="one function per species"):
        EAM.from_functions(s, ty, pair, density, embed[:1], RC, RMIN, (2.0, 60.0))
    with pytest.raises(ValueError, match="lacks a function"):
        EAM.from_functions(s, ty, {(0, 0): pair[0], (1, 1): pair[2]}, density, embed, RC, RMIN, (2.0, 60.0))
    with pytest.raises(ValueError, match="pair holds"):
        EAM.from_functions(s, ty, pair[:2], density, embed, RC, RMIN, (2.0, 60.0))
    by_key = EAM.from_functions(s, ty, {(0, 0): pair[0], (0, 1): pair[1], (1, 1): pair[2]}, density, embed, RC, RMIN, (2.0, 60.0), 16, 16)
    by_list = EAM.from_functions(s, ty, pair, density, embed, RC, RMIN, (2.0, 60.0), 16, 16)
    assert torch.equal(by_key.pair_nodes, by_list.pair_nodes) and by_key.pair_nodes.dtype == torch.float32
    # a supplied derivative and autograd give the same slopes
    a = EAM.tabulate(lambda r: torch.exp(-r), 1.0, 3.0, 9)
    b = EAM.tabulate((lambda r: torch.exp(-r), lambda r: -torch.exp(-r)), 1.0, 3.0, 9)
    assert float((a - b).abs().max()) <= 1e-15 and a.shape == (9, 2) and abs(float(a[0, 1]) + 0.25 * math.exp(-1.0)) <= 1e-15
    one = EAM(s, trainable=("embed",), **good)
    assert [n for n, _ in one.named_parameters()] == ["embed_nodes"] and one._select == [(2 * 5 * 8, 2 * 5 * 8 + 2 * 2 * 6)]
    assert list(EAM(s, trainable=False, **good).parameters()) == [] and len(list(EAM(s, trainable=True, **good).parameters())) == 3


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_entry_point_validates_its_arguments():
    from mdgrad_amd import _lib, ops
    lib = _lib.load()
    p = ctypes.c_void_p(64)                  # never dereferenced: every call below fails its checks first
    cell = _lib.make_cell([11.0, 11.0, 11.0])
    mk = lambda: ops.eam_table_consts(2, 64, 32, RMIN, RC, 0.5, 40.0)
    k = mk()

    def broken(**kw):
        b = mk()
        for name, v in kw.items():
            setattr(b, name, v)
        return ctypes.byref(b)

    def fails(rc, word):
        msg = lib.mdg_last_error()
        assert rc == -1 and word.encode() in msg, (rc, word, msg)

    ev, C, Kc = lib.mdg_eam_table_eval, ctypes.byref(cell), ctypes.byref(k)
    #        pos n cell col shift cnt max types consts tables w  energy grad hw gtab gtabw partial work fx
    fails(ev(None, 8, C, p, p, p, 8, p, Kc, p, None, None, p, None, None, None, None, p, None, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, None, p, p, p, 8, p, Kc, p, None, None, p, None, None, None, None, p, None, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, C, p, p, None, 8, p, Kc, p, None, None, p, None, None, None, None, p, None, 1.0, 0, None), "null buffer")
    fails(ev(p, 8, C, p, p, p, 8, None, Kc, p, None, None, p, None, None, None, None, p, None, 1.0, 0, None), "types or tables")
    fails(ev(p, 8, C, p, p, p, 8, p, Kc, None, None, None, p, None, None, None, None, p, None, 1.0, 0, None), "types or tables")
    fails(ev(p, 8, C, p, p, p, 8, p, None, p, None, None, p, None, None, None, None, p, None, 1.0, 0, None), "consts is null")
    fails(ev(p, 0, C, p, p, p, 8, p, Kc, p, None, None, p, None, None, None, None, p, None, 1.0, 0, None), "bad sizes")
    fails(ev(p, 8, C, p, p, p, 0, p, Kc, p, None, None, p, None, None, None, None, p, None, 1.0, 0, None), "bad sizes")
    for bad, word in ((dict(n_species=0), "n_species"), (dict(n_species=5), "n_species"), (dict(n_r=3), "node counts"),
                      (dict(n_r=4097), "node counts"), (dict(n_rho=3), "node counts"), (dict(n_rho=5000), "node counts"),
                      (dict(h_r=0.0), "spacings"), (dict(h_rho=-1.0), "spacings"), (dict(rc=RMIN), "r_min < rc"),
                      (dict(rc=1.0), "r_min < rc"), (dict(r_min=-1.0), "r_min < rc"), (dict(pin_cutoff=2), "pin_cutoff")):
        fails(ev(p, 8, C, p, p, p, 8, p, broken(**bad), p, None, None, p, None, None, None, None, p, None, 1.0, 0, None), word)
    fails(ev(p, 8, C, p, p, p, 8, p, Kc, p, None, None, p, p, None, None, None, p, None, 1.0, 0, None), "need w")
    fails(ev(p, 8, C, p, p, p, 8, p, Kc, p, None, None, p, None, None, p, None, p, p, 1.0, 0, None), "need w")
    fails(ev(p, 8, C, p, p, p, 8, p, Kc, p, p, None, p, None, None, None, None, p, None, 1.0, 0, None), "without hw")
    fails(ev(p, 8, C, p, p, p, 8, p, Kc, p, p, None, p, p, p, None, None, p, p, 1.0, 0, None), "gtab is the output")
    fails(ev(p, 8, C, p, p, p, 8, p, Kc, p, None, None, None, None, None, None, None, p, None, 1.0, 0, None), "no output")
    fails(ev(p, 8, C, p, p, p, 8, p, Kc, p, None, p, None, None, None, None, None, p, None, 1.0, 0, None), "partial")
    fails(ev(p, 8, C, p, p, p, 8, p, Kc, p, None, None, p, None, None, None, None, None, None, 1.0, 0, None), "atom_work is null")
    fails(ev(p, 8, C, p, p, p, 8, p, Kc, p, None, None, p, None, p, None, None, p, None, 1.0, 0, None), "fixed-point scratch")
    fails(ev(p, 8, C, p, p, p, 8, p, Kc, p, p, None, p, p, None, p, None, p, None, 1.0, 0, None), "fixed-point scratch")
    assert lib.mdg_eam_table_partial_size(64) == 4 and lib.mdg_eam_table_partial_size(37) == 3 and lib.mdg_eam_table_partial_size(0) == 0
    assert lib.mdg_eam_table_size(2, 64, 32) == 2 * (5 * 64 + 2 * 32) and lib.mdg_eam_table_fx_size(2, 64, 32) == 2 * (5 * 64 + 2 * 32) + 8
    assert lib.mdg_eam_table_size(1, 4, 4) == 24 and lib.mdg_eam_table_size(4, 4096, 4096) == 2 * 18 * 4096
    for bad in ((0, 64, 64), (5, 64, 64), (1, 3, 64), (1, 64, 4097)):
        assert lib.mdg_eam_table_size(*bad) == -1 and lib.mdg_eam_table_fx_size(*bad) == -1
    assert ctypes.sizeof(_lib.MdgEAMTableConsts) == 56
    for bad in (dict(n_species=0), dict(n_species=5), dict(n_r=3), dict(n_rho=4097), dict(cutoff=RMIN), dict(r_min=-1.0), dict(rho_max=0.5)):
        args = dict(n_species=2, n_r=64, n_rho=32, r_min=RMIN, cutoff=RC, rho_min=0.5, rho_max=40.0)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.eam_table_consts(**args)
