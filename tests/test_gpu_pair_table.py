"""The tabulated pair model (MDG_PAIR_TABLE) against a float64 restatement of its arithmetic (oracle.TableTerm).

Every user pair module (pairMLP, TpairMLP, any nn.Module phi(r), alone or stacked with built-in priors) runs on the fused
trajectory kernels as a table of c1(u) = phi'(r)/r and its slope on a uniform grid in u = r^2, evaluated by cubic Hermite
interpolation; the adjoint returns the table gradient by a fixed-point scatter.  That arithmetic is written out in
pair_eval (csrc/common.hpp: pair_ell.hip and the multi-launch kernels of traj_large.hip), in the packed loop of the
one-workgroup kernels (traj_small.hip) and in the ring kernels (traj_ring.hpp).  The tables here carry independent noise
on every node and slope, so reading the wrong cell, swapping two basis functions or losing a 1/du moves the result by the
noise, not by a smooth module's tiny node-to-node change.  The float64 reference interpolates the same float32 table on
the same float32 grid, so what is left is float32 rounding.

CPU tests pin the reference itself and the library's size rule; the others need the GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle as O
from test_gpu_parity import T, close, mk_system, liquid, DEV

gpu = pytest.mark.gpu
CUT = 2.5
EPS32 = 2.0 ** -24


def f32(x):
    return float(np.float32(x))


def noisy_lj_table(u0, du, p, seed, noise=0.04):
    """c1 = phi'(r)/r of LJ 12-6 (sigma = epsilon = 1) and du dc1/du on the nodes u0 + g du, each entry with independent
    noise of `noise` times the node's magnitude: neighbouring cells differ, and short runs stay stable."""
    rng = np.random.default_rng(seed)
    u = u0 + du * np.arange(p, dtype=np.float64)
    c1 = 24.0 * (u ** -4 - 2.0 * u ** -7)
    s = du * 24.0 * (14.0 * u ** -8 - 4.0 * u ** -5)
    mag = np.maximum(np.abs(c1), np.abs(s))
    v = c1 + noise * mag * rng.standard_normal(p)
    s = s + noise * mag * rng.standard_normal(p)
    return torch.tensor(np.stack((v, s), 1).reshape(-1), dtype=torch.float32)


# ------------------------------------------------------------------ the reference and the size rule (CPU)
def test_table_reference_interpolates_its_nodes_and_matches_a_fine_lj_table():
    """oracle.table_c1 returns the node values on the nodes, the slopes as du dc1/du there, and -- on a fine noise-free LJ
    table -- the LJ force of oracle.PairTerm; TableTerm's d(w.F)/dq is the LJ term's, and its d(w.F)/d(table) is the
    finite difference of w.F."""
    torch.manual_seed(0)
    p, u0 = 9, 0.8
    du = (CUT * CUT - u0) / (p - 1)
    tab = torch.randn(2 * p, dtype=torch.float64)
    u = (u0 + du * torch.arange(p, dtype=torch.float64)).requires_grad_(True)
    c1 = O.table_c1(tab, u0, du, u)
    assert torch.allclose(c1, tab[0::2], rtol=0, atol=1e-12)
    (g,) = torch.autograd.grad(c1.sum(), u)
    assert torch.allclose(g * du, tab[1::2], rtol=0, atol=1e-12)
    assert float(O.table_c1(tab, u0, du, torch.tensor([u0 - 0.3], dtype=torch.float64))) == float(tab[0])

    pos, cell = liquid(4, seed=3, jitter=0.05)
    q = T(pos).double()
    lj = O.PairTerm("lj", torch.tensor([1.0, 1.0], dtype=torch.float64), CUT, T(cell).double(), p=12, q=6, c=1)
    pf = 20001
    u0 = 0.64
    du = (CUT * CUT - u0) / (pf - 1)
    ug = u0 + du * torch.arange(pf, dtype=torch.float64)
    fine = torch.stack((24.0 * (ug ** -4 - 2.0 * ug ** -7), du * 24.0 * (14.0 * ug ** -8 - 4.0 * ug ** -5)), 1).reshape(-1)
    tt = O.TableTerm(fine, u0, du, CUT, T(cell).double())
    lj.reset(q)
    tt.reset(q)
    w = torch.randn_like(q)
    F1, dq1, _ = lj.force_vjp(q, w)
    F2, dq2, dth = tt.force_vjp(q, w)
    assert float((F1 - F2).abs().max()) < 1e-6 * float(F1.abs().max())
    assert float((dq1 - dq2).abs().max()) < 1e-5 * float(dq1.abs().max())
    k = int(dth.abs().argmax())
    h = 1e-6
    e = torch.zeros_like(fine)
    e[k] = h
    fd = ((w * tt._force(q, fine + e)).sum() - (w * tt._force(q, fine - e)).sum()) / (2 * h)
    assert abs(float(fd) - float(dth[k])) < 1e-6 * abs(float(dth[k]))


def test_one_workgroup_size_rule(tmp_path):
    """mdg_traj_small_fits: the adjoint's 28 state columns, the nodes and their int64 gradient words in 160 KiB of LDS less
    the kernels' own static LDS -- N <= 1 010 at 2 048 nodes, N <= 570 at 4 096; built-in forms up to FUSED_MAX_ATOMS.  The
    static LDS the rule sets aside (SMALL_STATIC_LDS, 256 bytes) must cover what every one-workgroup kernel of the gfx950
    code object declares."""
    import re
    import subprocess
    from mdgrad_amd import _lib
    from mdgrad_amd.md import FUSED_MAX_ATOMS
    fits = _lib.load().mdg_traj_small_fits
    assert fits(1010, 2048) == 1 and fits(1011, 2048) == 0 and fits(1024, 2048) == 0
    assert fits(570, 4096) == 1 and fits(571, 4096) == 0
    assert fits(108, 4096) == 1 and fits(FUSED_MAX_ATOMS, 0) == 1
    import test_ring_register_budget as rb
    if not os.path.exists(rb.READELF):
        pytest.skip("llvm-readelf of the ROCm toolchain is needed")
    out = subprocess.run([rb.READELF, "--notes", rb._gfx950_code_object(tmp_path)], capture_output=True, text=True,
                         check=True).stdout
    seen = 0
    for blk in out.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "traj_fwd_kernel" in name or "traj_adj_kernel" in name:
            seen += 1
            assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)) <= 256, name
    assert seen >= 4


# ------------------------------------------------------------------ the interpolant on pair_eval (pair_ell.hip)
def _pair_eval_vs_reference(pos, cell, table, u0, du, w):
    """pair_eval's dU/dx and H w against the float64 reference, with a per-atom tolerance from float32 rounding: the
    kernel's u carries a few ulp of u (d^2, the grid coordinate, 1/du), which moves c1 by |dc1/du| du_err and dc1/du by
    |d2c1/du2| du_err; 5x headroom."""
    from mdgrad_amd import ops, _lib
    x = T(pos, DEV)
    cs = _lib.make_cell(cell)
    p = table.numel() // 2
    term = ops.make_term(dict(kind=ops.MDG_PAIR_TABLE, p=p, a=u0, phi=du, c=1.0), CUT, 0, 2 * p, None)
    ell = ops.build_ell(x, cs, CUT)
    o = ops.pair_eval(ell, x, term, table.to(DEV), w=T(w, DEV), energy=False, theta_grads=False)
    q, w64, tab = T(pos).double(), T(w).double(), table.double()
    ref = O.TableTerm(tab, f32(u0), f32(du), CUT, T(cell).double())
    ref.reset(q)
    F, dq, _ = ref.force_vjp(q, w64)
    # per-pair rounding budget
    i, j = ref.nbr[:, 0], ref.nbr[:, 1]
    D = -O.compute_dis(q, ref.nbr, ref.off.double(), ref.cell.double())[0]
    u = D.pow(2).sum(1).requires_grad_(True)
    c1 = O.table_c1(tab, f32(u0), f32(du), u)
    (c1u,) = torch.autograd.grad(c1.sum(), u, create_graph=True)
    (c1uu,) = torch.autograd.grad(c1u.sum(), u)
    c1, c1u = c1.detach().abs(), c1u.detach().abs()
    du_err = 8 * EPS32 * CUT * CUT
    nD = D.norm(dim=1)
    wij = (w64[i] - w64[j]).norm(dim=1)
    tf = nD * (c1u * du_err + 8 * EPS32 * c1)
    th = (2 * c1uu.abs() * du_err * nD * nD * wij + c1u * du_err * wij
          + 8 * EPS32 * (2 * c1u * nD * nD * wij + c1 * wij))
    tolF, tolH = torch.zeros(len(pos), dtype=torch.float64), torch.zeros(len(pos), dtype=torch.float64)
    for tol, per in ((tolF, tf), (tolH, th)):
        tol.index_add_(0, i, per)
        tol.index_add_(0, j, per)
    for got, want, tol, nm in ((o["grad"], -F, tolF, "dU/dx"), (o["hw"], -dq, tolH, "H w")):
        err = (got.detach().cpu().double() - want).abs().max(1).values
        bad = err > 5 * tol[:] + 1e-6 * float(want.abs().max())
        assert not bool(bad.any()), "%s (p=%d): atoms %s err %s allowed %s" % (
            nm, p, bad.nonzero().reshape(-1).tolist(), err[bad].tolist(), (5 * tol[bad]).tolist())
    return ref, o


@gpu
@pytest.mark.parametrize("p", [4, 37, 2048, 4096])
def test_table_interpolant_on_pair_eval(p):
    """Four pairs far apart in a 40-wide box: on a node (the two cells that meet there must agree), mid-cell, in the first
    cell just above u0, and in the last thousandth of the last cell (p = 4: the kernels once clamped the grid coordinate
    to p - 1 - 1e-3 there, an error of ~1e-3 of the last slope); then a pair exactly at the cutoff, which is excluded.
    The table's entries are independent random numbers: every cell differs from its neighbours."""
    rng = np.random.default_rng(p)
    u0 = 0.25
    du = (CUT * CUT - u0) / (p - 1)
    table = torch.tensor(rng.uniform(-1.0, 1.0, 2 * p), dtype=torch.float32)
    cell = np.array([40.0, 40.0, 40.0], dtype=np.float32)
    g_node, g_mid = p // 2, p // 3
    # (grid coordinate of each pair, and the window it must land in once the positions are rounded to float32)
    targets = [(g_node, g_node - 0.01, g_node + 0.01), (g_mid + 0.5, g_mid + 0.49, g_mid + 0.51), (0.03, 0.0, 0.1),
               (p - 1 - 4e-4, p - 1 - 1e-3, p - 1)]
    pos = []
    for k, (tt, lo, hi) in enumerate(targets):
        base = np.array([1.0 + 6.0 * (k % 2), 1.0 + 6.0 * (k // 2), 1.5], dtype=np.float32)
        for _ in range(1000):
            n = rng.standard_normal(3)
            x = (base + np.sqrt(u0 + tt * du) * n / np.linalg.norm(n)).astype(np.float32)
            got = (((x.astype(np.float64) - base) ** 2).sum() - f32(u0)) / f32(du)
            if lo < got < hi:
                break
        else:
            raise AssertionError("could not place a pair at grid coordinate %g" % tt)
        pos += [base, x]
    pos = np.array(pos, dtype=np.float32)
    w = rng.standard_normal(pos.shape).astype(np.float32)
    _pair_eval_vs_reference(pos, cell, table, u0, du, w)
    # a pair exactly at the cutoff (excluded: topology.py's d^2 < cutoff^2) beside a mid-cell one
    pos = np.array([[10.0, 10.0, 10.0], [10.0 + CUT, 10.0, 10.0], [10.0, 10.0 + np.sqrt(u0 + (g_mid + 0.5) * du), 10.0]],
                   dtype=np.float32)
    w = rng.standard_normal(pos.shape).astype(np.float32)
    ref, o = _pair_eval_vs_reference(pos, cell, table, u0, du, w)
    assert ref.nbr.tolist() == [[0, 2]]
    assert float(o["grad"][1].abs().max()) == 0.0 and float(o["hw"][1].abs().max()) == 0.0


# ------------------------------------------------------------------ trajectories on the three kernel families
FAMILIES = ("workgroup", "ring", "ring_odd", "large")


def _integrator(system, nhc, family, nodes=2048, rmin=None):
    from mdgrad_amd import potentials as P, _lib
    from mdgrad_amd.interface import PairPotentials
    from mdgrad_amd.md import NoseHooverChain, NVE
    torch.manual_seed(0)
    mlp = P.pairMLP(n_gauss=8, r_start=0.0, r_end=CUT, n_layers=1, n_width=8, nonlinear="Tanh")
    pp = PairPotentials(system, mlp, cutoff=CUT)
    integ = (NoseHooverChain(pp, system, T=1.0, num_chains=3, Q=30.0) if nhc else NVE(pp, system)).to(DEV)
    integ.table_nodes = nodes
    if rmin is not None:
        integ.table_rmin = rmin
    if family == "large":
        integ.fused_large = True
    spec = integ.fused_spec("NH_verlet" if nhc else "verlet")
    assert spec is not None and spec.table
    if family is not None:
        assert bool(spec.large) == (family == "large")
        if not spec.large:
            spec.block = 64 if family.startswith("ring") else 256
            prm = spec.params(1, 2)
            ring = bool(_lib.load().mdg_traj_ring_taken(C.byref(prm), C.byref(spec.cell_struct), C.byref(spec.terms)))
            assert ring == family.startswith("ring")
    return integ, spec


def _loss(L):
    v, q = L[0], L[1]
    out = q[1:].pow(2).sum() / q[1:].numel() + v[-1].pow(2).sum() / v[-1].numel()
    return out + 1e-2 * L[2][-1].sum() if len(L) == 3 else out


def _run_and_compare(spec, pos, vel, mass, cell, nT, nhc, table, what, dt=0.005, table_tol=5e-4):
    """One fused forward + adjoint with `table` as theta (the returned theta gradient is dL/dtable), against the float64
    oracle: q_t, v_t (, pv_t), the adjoints of v0, q0 (, pv0) and dL/dtable entry by entry."""
    from mdgrad_amd import ops
    t = torch.tensor([dt * k for k in range(nT)], dtype=torch.float32)
    tab = table.to(DEV).requires_grad_(True)
    v0, q0 = T(vel, DEV).requires_grad_(True), T(pos, DEV).requires_grad_(True)
    pv0 = torch.zeros(3, device=DEV, requires_grad=True) if nhc else None
    out = ops.FusedTrajFn.apply(v0, q0, pv0, t.to(DEV), tab, spec)
    _loss(out).backward()

    ref = O.TableTerm(table.double(), f32(spec.u0), f32(spec.du), CUT, T(cell).double())
    model = O.ModelOracle([ref])
    m64 = T(mass).double()
    eom = O.NHCOracle(model, m64, 1.0, 30.0, 3) if nhc else O.NVEOracle(model)
    y0 = (T(vel).double(), T(pos).double()) + ((torch.zeros(3, dtype=torch.float64),) if nhc else ())
    traj = O.odeint_oracle(eom, y0, t.double())
    leaves = [x.clone().requires_grad_(True) for x in traj]
    _loss(leaves).backward()
    lam, gth = O.adjoint_oracle(eom, traj, [x.grad for x in leaves], t.double())

    close(out[1], traj[1], 0, 2e-5, "q_t (%s)" % what)
    close(out[0], traj[0], 0, 5e-4, "v_t (%s)" % what)
    if nhc:
        close(out[2], traj[2], 1e-3, 1e-5, "pv_t (%s)" % what)
    for y, l, nm in zip((v0, q0, pv0), lam, ("adj v0", "adj q0", "adj pv0")):
        close(y.grad, l, 2e-3, 5e-4 * float(l.abs().max()) + 1e-9, "%s (%s)" % (nm, what))
    assert float(gth.abs().max()) > 0
    close(tab.grad, gth, 2e-3, table_tol * float(gth.abs().max()), "dL/dtable (%s)" % what)


@gpu
@pytest.mark.parametrize("nT", [2, 6])
@pytest.mark.parametrize("ensemble", ["nhc", "nve"])
@pytest.mark.parametrize("family", FAMILIES)
def test_table_trajectory_and_adjoint_vs_float64(family, ensemble, nT):
    """One interval (T = 2) and a short run (T = 6) of a 108-atom liquid (107 for an odd ring) on each kernel family,
    NoseHooverChain and NVE, with a noisy LJ table of 2 048 nodes."""
    from conftest import load_golden
    g = load_golden("pair_mlp")
    n = 107 if family == "ring_odd" else 108
    pos, vel, mass = g["pos"][:n], g["vel"][:n], g["mass"][:n]
    system = mk_system(pos, g["cell"], vel, mass)
    nhc = ensemble == "nhc"
    _, spec = _integrator(system, nhc, family)
    table = noisy_lj_table(f32(spec.u0), f32(spec.du), spec.nodes, seed=7)
    _run_and_compare(spec, pos, vel, mass, g["cell"], nT, nhc, table, "%s %s T=%d" % (family, ensemble, nT))


@gpu
@pytest.mark.parametrize("n_atoms,nodes,large", [(1010, 2048, False), (1011, 2048, True), (1013, 2048, True),
                                                 (1024, 2048, True), (570, 4096, False), (571, 4096, True),
                                                 (573, 4096, True)])
def test_table_at_the_one_workgroup_size_limit(n_atoms, nodes, large):
    """Where the one-workgroup adjoint's LDS (state, nodes, gradient words, static LDS) runs out, fused_spec must route the
    tabulated model to the multi-launch kernels: the forward and the adjoint both complete and match the reference.  (It
    once sent every N <= 1 024 to the one-workgroup kernels, whose adjoint then refused from N = 1 013 at 2 048 nodes and
    from N = 573 at 4 096 -- and, its size check leaving out the kernels' 256 bytes of static LDS, overran the workgroup's
    LDS at N = 1 011 .. 1 012 and 571 .. 572.)  Forcing the one-workgroup kernels where they cannot hold the system gives
    the generic path."""
    side = 11 if n_atoms > 729 else 9
    pos, cell = liquid(side, seed=n_atoms, jitter=0.05)
    pos = pos[:n_atoms]
    vel = np.random.default_rng(n_atoms).normal(0, 1.0, pos.shape).astype(np.float32)
    mass = np.full(n_atoms, 1.008, dtype=np.float32)
    system = mk_system(pos, cell, vel, mass)
    integ, spec = _integrator(system, True, None, nodes=nodes)
    # (a smooth LJ table: at 1 000 atoms and 4 096 nodes a noisy one's Hessian term -- its slope noise over du -- turns the
    # float32 rounding of u into adjoint differences beyond the pins; the noisy tables are exercised at 108 atoms above)
    table = noisy_lj_table(f32(spec.u0), f32(spec.du), nodes, seed=11, noise=0.0)
    # (dL/dtable: each entry sums the contributions of thousands of pairs that largely cancel, so it carries the adjoint's
    # own float32 error of ~1e-3 of its largest entry -- the same on both kernel families; 108 atoms above pin 5e-4)
    _run_and_compare(spec, pos, vel, mass, cell, 2, True, table, "N=%d, %d nodes" % (n_atoms, nodes), table_tol=5e-3)
    assert bool(spec.large) == large, "fused_spec chose the %s kernels" % ("multi-launch" if spec.large else "one-workgroup")
    integ.fused_large = False
    assert (integ.fused_spec("NH_verlet") is None) == large


@gpu
@pytest.mark.parametrize("family", ["workgroup", "ring", "large"])
def test_pair_below_the_first_node_raises(family):
    """A pair closer than table_rmin * cutoff (the first node) has no table entry: the forward raises, naming table_rmin,
    on every kernel family (bit 2 of the per-replica flag, the ring kernels' LDS flag, the multi-launch flags).  With the
    first node 3 % below the closest pair instead, the run goes through and matches the reference."""
    from conftest import load_golden
    g = load_golden("pair_mlp")
    pos, vel, mass, cell = g["pos"], g["vel"], g["mass"], g["cell"]
    d = pos.astype(np.float64)[None] - pos.astype(np.float64)[:, None]
    d -= np.round(d / cell) * cell
    r = np.sqrt((d ** 2).sum(-1)) + np.eye(len(pos)) * 1e9
    dmin = float(r.min())
    for factor, raises in ((0.97, True), (1.03, False)):
        system = mk_system(pos, cell, vel, mass)
        _, spec = _integrator(system, False, family, rmin=dmin / (factor * CUT))
        table = noisy_lj_table(f32(spec.u0), f32(spec.du), spec.nodes, seed=5)
        if raises:
            from mdgrad_amd import ops
            t = torch.tensor([0.0, 0.005], device=DEV)
            with pytest.raises(RuntimeError, match="table_rmin"):
                ops.FusedTrajFn.apply(T(vel, DEV), T(pos, DEV), None, t, table.to(DEV), spec)
        else:
            _run_and_compare(spec, pos, vel, mass, cell, 2, False, table, "%s, closest pair 3 %% above the first node" % family)
