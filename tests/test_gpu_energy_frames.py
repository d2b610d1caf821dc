"""thermo.PotentialEnergy on the GPU (csrc/energy.hip on csrc/frame_pairs.hpp, ops.EnergyFramesFn) against the float64
reference of tests/pair_forms_ref.py.

Error measure: |kernel - ref64| over the reference's scale (U, dU/dtheta: the sum over the pairs of the absolute summands; dU/dq:
per atom and component the sum over the atom's pairs), the largest over atoms / entries.  Allowed: MARGIN x floor, MARGIN = 10,
floor = the float32 restatement of the formulas on the CPU against float64, at least 2^-24 -- nothing comes from the kernel.
With an upstream gU per frame the kernel's dL/dq[f] is compared with gU_f dU_f/dq over |gU_f| x scale, and dL/dtheta with
sum_f gU_f dU_f/dtheta over sum_f |gU_f| scale_f with the frames' floors weighted the same way.

Inputs carry no fragile pair (pair_forms_ref.fragile_pairs; for the sizes beyond its all-pairs arrays the same two criteria row
block by row block, `sparse_reference`), asserted before a kernel runs: the reference is exact on them and no case is left out.
The sizes of tests/test_gpu_pressure.py::test_sizes are built as that test builds them; of the 4 096 frames of 108 atoms five
are referenced, as there, and the others carry a zero upstream weight.

(Every case prints floor, allowed and the kernel's figure per quantity; MDG_TEST_REPORT=<file> collects them.)"""
import numpy as np
import pytest
import torch

import pair_forms_ref as PF
from test_energy_frames_host import _report, frames_108, members_of, mk_system, observable
from test_gpu_pressure import liquid as sized_liquid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 10.0


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------- reference of one LJ term, any N
def sparse_pairs(x, cell, term):
    """(i, j, fragile): the directed pairs of ONE unmasked term found row block by row block with pair_forms_ref's float32
    membership, and the number of (directed) fragile pairs by its two criteria"""
    x32 = np.asarray(x, np.float32)
    N = len(x32)
    h32, inv32, _ = PF._cell(cell, np.dtype(np.float32))
    L32, i32 = np.diag(h32), np.diag(inv32)
    rc2 = np.float32(term.cutoff) * np.float32(term.cutoff)
    rcmax2 = (term.cutoff + 1e-3) ** 2
    ii, jj, fragile = [], [], 0
    for a in range(0, N, 256):
        D = x32[None, :, :] - x32[a:a + 256, None, :]
        s = D * i32
        D = D + ((s < -0.5).astype(np.float32) - (s > 0.5).astype(np.float32)) * L32
        d2 = (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]
        m = (d2 < rc2) & (d2 > 0)
        i, j = np.nonzero(m)
        ii.append(i + a), jj.append(j)
        # (d2 - rc2 is exact in float32 this close to rc2, and so is |s| - 0.5 next to 0.5)
        fragile += int((np.abs(d2 - rc2) <= np.float32(PF.CUT_ULPS * float(np.spacing(rc2)))).sum())
        # a fractional separation within HALF_EPS of +-0.5 while either image is inside the cutoff (+ 1e-3): both images have
        # |D_c| = L_c / 2 to 1e-6, so the other components decide
        near = np.abs(np.abs(s) - np.float32(0.5)) < np.float32(PF.HALF_EPS)
        if near.any():
            r, c, k = np.nonzero(near)
            Dn = D[r, c].astype(np.float64)
            fragile += int(((Dn * Dn).sum(-1) < rcmax2 + 1e-3).sum())
    return np.concatenate(ii), np.concatenate(jj), fragile


def sparse_reference(x, cell, term, dtype, pairs=None):
    """pair_forms_ref.evaluate for ONE unmasked term without its [N, N] arrays: the pairs of sparse_pairs evaluated in `dtype`
    with the same statements.  Returns (Result, number of fragile pairs).  Checked against evaluate itself in
    test_sparse_reference_is_evaluate."""
    dt = np.dtype(dtype)
    x32 = np.asarray(x, np.float32)
    N = len(x32)
    i, j, fragile = sparse_pairs(x, cell, term) if pairs is None else pairs
    h, inv, _ = PF._cell(cell, dt)
    xd = x32.astype(dt)
    D = xd[j] - xd[i]
    s = D * np.diag(inv)
    D = D + ((s < -0.5).astype(dt) - (s > 0.5).astype(dt)) * np.diag(h)
    d2 = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
    ir = (dt.type(1) / np.sqrt(d2)).astype(dt)
    r = d2 * ir
    u, du, _, du_dth, _ = PF.phi(term, r, ir, dt)
    f = (du * ir)[:, None] * D
    F, sF = np.zeros((N, 3), dt), np.zeros((N, 3), dt)
    np.add.at(F, i, f)
    np.add.at(sF, i, np.abs(f))
    up = i < j
    res = PF.Result(u[up].sum(dtype=dt), F, None, None, [np.array([g[up].sum(dtype=dt) for g in du_dth], dt)],
                    np.abs(u[up]).sum(dtype=dt), sF, None, None, [np.array([np.abs(g[up]).sum(dtype=dt) for g in du_dth], dt)])
    return res, fragile                  # (directed pairs: each fragile pair counts twice; the callers want none)


def floors_of(ref, r32):
    return {q: max(PF.EPS, PF.error(getattr(r32, q), ref, q)) for q in ("U", "F", "dU")}


def reference_frames(xyz, cell, terms, sparse=False, found=None):
    """per frame (float64 Result, floors); no frame may carry a fragile pair (found: sparse_pairs of the frames, if at hand)"""
    out = []
    for n, x in enumerate(xyz):
        if sparse:
            pairs = sparse_pairs(x, cell, terms[0]) if found is None else found[n]
            assert pairs[2] == 0, "the fixture has %d fragile pairs at cutoff %g" % (pairs[2], terms[0].cutoff)
            ref = sparse_reference(x, cell, terms[0], np.float64, pairs)[0]
            out.append((ref, floors_of(ref, sparse_reference(x, cell, terms[0], np.float32, pairs)[0])))
        else:
            assert len(PF.fragile_pairs(x, cell, terms)) == 0, "the fixture has a fragile pair at these cutoffs"
            member = PF.membership(x, cell, terms)
            ref = PF.evaluate(x, np.zeros_like(x), cell, terms, member=member)
            out.append((ref, floors_of(ref, PF.evaluate(x, np.zeros_like(x), cell, terms, np.float32, member))))
    return out


def run_gpu(obs, mods, xyz, gU, positions=True):
    """(U, dL/dq or None, [dL/dtheta per term], route) of L = sum_f gU_f U_f through the kernels; positions=False: the frames are
    detached and the backward pass must take the parameters-only sweep"""
    from mdgrad_amd import ops
    q = T(xyz).requires_grad_(positions)
    U = obs(q)
    ps = [p for m in mods for p in m.mdg_params()]
    ops.EnergyFramesFn.last_route = None
    want = ([q] if positions else []) + ps
    if not want:
        return U.detach(), None, [np.zeros(0) for _ in mods], None
    grads = list(torch.autograd.grad((U * T(np.asarray(gU, np.float32))).sum(), want))
    gq = grads.pop(0) if positions else None
    it = iter(grads)
    gth = [np.array([float(next(it)) for _ in m.mdg_params()], np.float64) for m in mods]
    assert q.grad is None
    return U.detach(), gq, gth, ops.EnergyFramesFn.last_route


def check(what, out, refs, gU, pick=None):
    """U, dL/dq and dL/dtheta of run_gpu against the per-frame references (of the frames `pick`), each over its scale"""
    U, gq, gth, _ = out
    pick = list(range(len(refs))) if pick is None else list(pick)
    gU = np.asarray(gU, np.float64)
    figs = []
    for (ref, fl), f in zip(refs, pick):
        figs.append(("U[%d]" % f, PF.error(float(U[f]), ref, "U"), fl["U"]))
        if gq is not None and gU[f] != 0:
            figs.append(("dq[%d]" % f, PF.error(-gq[f].cpu().numpy().astype(np.float64) / gU[f], ref, "F"), fl["F"]))
    n_terms = len(refs[0][0].dU)
    for m in range(n_terms):
        want = sum(gU[f] * ref.dU[m] for (ref, _), f in zip(refs, pick))
        scale = sum(abs(gU[f]) * ref.sdU[m] for (ref, _), f in zip(refs, pick))
        floor = sum(abs(gU[f]) * ref.sdU[m] * fl["dU"] for (ref, fl), f in zip(refs, pick))        # absolute, per entry
        for k in range(len(want)):
            err = abs(gth[m][k] - want[k])
            if scale[k] > 0:
                figs.append(("dtheta[%d][%d]" % (m, k), err / scale[k], floor[k] / scale[k]))
            else:
                assert gth[m][k] == 0.0
    bad = []
    for q, v, floor in figs:
        allowed = MARGIN * floor
        _report("%-44s %-14s floor %.3e  allowed %.3e  kernel %.3e%s" % (what, q, floor, allowed, v, "" if v <= allowed else "   <-- FAILS"))
        if not v <= allowed:
            bad.append((q, v, allowed))
    assert not bad, "%s: %s" % (what, bad)


def test_sparse_reference_is_evaluate():
    fx = PF.liquid(108)
    term = PF.Term("lj", 2.5)
    for dt in (np.float64, np.float32):
        a, frag = sparse_reference(fx.x, fx.cell, term, dt)
        b = PF.evaluate(fx.x, np.zeros_like(fx.x), fx.cell, [term], dt)
        assert frag == 0
        tol = 1e-13 if dt is np.float64 else 1e-6
        assert abs(a.U - b.U) <= tol * b.sU and abs(a.sU - b.sU) <= tol * b.sU
        assert (np.abs(a.F - b.F) <= tol * b.sF).all() and (np.abs(a.dU[0] - b.dU[0]) <= tol * b.sdU[0]).all()


# ---------------------------------------------------------------------------------------------- forms, stacks, masks
GU4 = [0.7, 1.3, 0.0, -0.4]
STACKS = ["three_term", "two_cutoffs", "two_species", "excluded_pairs_lj", "two_term"]


@pytest.mark.parametrize("name", list(PF.FORMS) + STACKS)
def test_forms_and_stacks_against_the_reference(name):
    """liquid(108) and unwrapped() alternating (four frames, so a full workgroup of the wave-per-frame kernels); upstream
    weights that differ per frame, one of them zero: that frame gets exact-zero position gradients.  Both backward variants:
    full rows (positions wanted) and the once-per-pair parameters-only sweep (q detached)."""
    fx, two = frames_108()
    xyz = np.concatenate([two, two])
    members = members_of(name, 108)
    terms = PF.terms_of(members, 108)
    refs = reference_frames(two, fx.cell, terms) * 2
    obs, mods = observable(fx, members, DEV, torch.float32)
    full = run_gpu(obs, mods, xyz, GU4)
    check(name + " full rows", full, refs, GU4)
    assert full[3] == "full" and torch.equal(full[1][2], torch.zeros_like(full[1][2]))
    assert torch.equal(full[0][0], full[0][2]) and torch.equal(full[0][1], full[0][3])
    if sum(len(m.mdg_params()) for m in mods):
        only = run_gpu(obs, mods, xyz, GU4, positions=False)
        check(name + " parameters only", only, refs, GU4)
        assert only[3] == "theta" and torch.equal(only[0], full[0])
    # U of a single frame and of the frames as [R, T, N, 3]
    q = T(xyz)
    assert torch.equal(obs(q[1]), full[0][1]) and torch.equal(obs(q.reshape(2, 2, 108, 3)).reshape(-1), full[0])


@pytest.mark.parametrize("name", ["lj", "three_term", "excluded_pairs_lj", "morse_neg"])
def test_value_equals_the_model_frame_by_frame(name):
    """U[f] against PairPotentials / Stack evaluated on frame f through its neighbour list: two float32 kernels with different
    summation orders, each within MARGIN x floor of the reference, so within twice that of each other."""
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.thermo import PotentialEnergy
    fx, xyz = frames_108()
    members = members_of(name, 108)
    terms = PF.terms_of(members, 108)
    refs = reference_frames(xyz, fx.cell, terms)
    system = mk_system(fx.x, fx.cell, DEV)
    pps = {"t%d" % k: PairPotentials(system, PF.module(f, th), cutoff=rc, **(sel or {})) for k, (f, th, rc, sel) in enumerate(members)}
    model = Stack(pps) if len(pps) > 1 else pps["t0"]
    U = PotentialEnergy(system, model)(T(xyz))
    for f, (ref, fl) in enumerate(refs):
        qf = T(xyz[f])
        model._reset_topology(qf)
        Um = float(model(qf))
        err, allowed = abs(float(U[f]) - Um) / float(ref.sU), 2 * MARGIN * fl["U"]
        _report("%-44s U[%d] vs model(q[%d])  floor %.3e  allowed %.3e  figure %.3e" % (name, f, f, fl["U"], allowed, err))
        assert err <= allowed
        assert PF.error(Um, ref, "U") <= MARGIN * fl["U"]


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n,frames", [(2, 3), (3, 3), (107, 3), (1000, 2), (4096, 3), (108, 4096), (129, 2), (1024, 1), (1100, 2)])
def test_sizes(n, frames):
    """Every kernel shape and both sides of its boundaries: a wave per frame (2, 3, 107 with a partly filled workgroup of four,
    108 x 4 096 frames), a workgroup per frame (129, 1000, 1024), tiles with an odd (1100: 5) and an even (4096: 16) number of
    blocks.  Built as tests/test_gpu_pressure.py::test_sizes builds them."""
    spare = 9 if frames <= 3 else 0
    xyz, cell = sized_liquid(n, seed=n, frames=frames + spare)              # (its generator draws frame after frame)
    if n <= 3:
        cell = np.array([4.0, 4.0, 4.0], dtype=np.float32)
        xyz = (np.random.default_rng(n).uniform(1.2, 2.6, xyz.shape)).astype(np.float32)
    cutoff = min(2.5, 0.49 * float(cell[0]))
    members = [("lj", (1.0, 1.0), cutoff, None)]
    terms = PF.terms_of(members, n)
    if spare:
        # a frame with a fragile pair is passed over for the generator's next one (as rdf_ref.draw_frames redraws): of 4 096
        # atoms about every second frame holds a pair within 4 ulps of the squared cutoff, and so does the frame of 1 024
        clean, found = [], []
        for x in xyz:
            if len(clean) < frames:
                pairs = sparse_pairs(x, cell, terms[0])
                if pairs[2] == 0:
                    clean.append(x), found.append(pairs)
        assert len(clean) == frames
        xyz = np.stack(clean)
    pick = np.arange(frames) if frames <= 3 else np.array([0, 1, 2047, 4094, 4095])
    refs = reference_frames(xyz[pick], cell, terms, sparse=True, found=found if spare else None)
    obs, mods = observable(PF.Fixture("sized", xyz[0], cell, ()), members, DEV, torch.float32)
    gU = np.zeros(frames, np.float32)
    gU[pick] = np.random.default_rng(1).uniform(0.5, 1.5, frames).astype(np.float32)[pick]
    full = run_gpu(obs, mods, xyz, gU)
    check("N=%d F=%d full rows" % (n, frames), full, refs, gU, pick)
    only = run_gpu(obs, mods, xyz, gU, positions=False)
    check("N=%d F=%d parameters only" % (n, frames), only, refs, gU, pick)
    assert full[3] == "full" and only[3] == "theta" and torch.equal(only[0], full[0])
    if frames > 3:
        assert float(full[1][3].abs().max()) == 0.0 and float(full[1][2046].abs().max()) == 0.0


def test_strided_input():
    """a time slice q_t[::5] of a trajectory tensor: the value of the contiguous copy, the gradient back in q_t's layout"""
    fx, two = frames_108()
    members = members_of("lj", 108)
    obs, mods = observable(fx, members, DEV, torch.float32)
    rng = np.random.default_rng(5)
    q_t = T(np.stack([two[k % 2] + rng.normal(0, 1e-3, two[0].shape).astype(np.float32) for k in range(11)])).requires_grad_(True)
    sl = q_t[::5]
    assert not sl.is_contiguous() and sl.shape[0] == 3
    U = obs(sl)
    Uc = obs(sl.detach().contiguous())
    assert torch.equal(U.detach(), Uc)
    g = T(np.array([0.5, -1.0, 2.0], np.float32))
    (gq,) = torch.autograd.grad((U * g).sum(), q_t)
    qc = sl.detach().contiguous().requires_grad_(True)
    (gc,) = torch.autograd.grad((obs(qc) * g).sum(), qc)
    assert torch.equal(gq[::5], gc)
    rest = torch.ones(11, dtype=torch.bool)
    rest[::5] = False
    assert float(gq[rest.to(DEV)].abs().max()) == 0.0


def test_no_pair_inside_the_cutoff_gives_exact_zeros():
    xyz = np.array([[[0.5, 0.5, 0.5], [3.5, 0.6, 0.4], [0.4, 3.5, 3.6], [3.4, 3.6, 0.5]]] * 2, dtype=np.float32)
    cell = np.array([6.0, 6.0, 6.0], dtype=np.float32)
    obs, mods = observable(PF.Fixture("apart", xyz[0], cell, ()), [("buck", None, 1.5, None)], DEV, torch.float32)
    for positions in (True, False):
        U, gq, gth, _ = run_gpu(obs, mods, xyz, np.ones(2, np.float32), positions)
        assert torch.equal(U, torch.zeros_like(U)) and (gth[0] == 0).all()
        assert gq is None or torch.equal(gq, torch.zeros_like(gq))


@pytest.mark.parametrize("name,n,frames", [("lj", 108, 64), ("three_term", 108, 3), ("buck", 300, 4), ("lj", 1500, 2)])
def test_bitwise_repeatable(name, n, frames):
    """forward and both backward variants, in every kernel shape: two launches give the same bits"""
    if n == 108:
        fx, two = frames_108()
        xyz = np.stack([two[k % 2] for k in range(frames)])
    else:
        xyz, cell = sized_liquid(n, seed=7, frames=frames)
        fx = PF.Fixture("sized", xyz[0], cell, ())
    obs, mods = observable(fx, members_of(name, n), DEV, torch.float32)
    gU = np.linspace(0.5, 1.5, frames).astype(np.float32)
    for positions in (True, False):
        a, b = run_gpu(obs, mods, xyz, gU, positions), run_gpu(obs, mods, xyz, gU, positions)
        assert torch.equal(a[0], b[0]) and (positions is False or torch.equal(a[1], b[1]))
        assert all((x == y).all() for x, y in zip(a[2], b[2])) and a[3] == b[3] == ("full" if positions else "theta")


@pytest.mark.parametrize("name", ["lj", "three_term"])
def test_torch_ops_equal_the_ctypes_path(name):
    from mdgrad_amd import _torch_ops
    ns = _torch_ops.get()
    assert ns is not None
    fx, two = frames_108()
    xyz = np.concatenate([two, two[:1]])
    obs, mods = observable(fx, members_of(name, 108), DEV, torch.float32)
    gU = np.array([0.7, 1.2, 0.9], np.float32)
    q = T(xyz).requires_grad_(True)
    ps = [p for m in mods for p in m.mdg_params()]
    U = obs(q)
    grads = torch.autograd.grad((U * T(gU)).sum(), [q] + ps)
    gth = torch.cat([g.reshape(-1) for g in grads[1:]])
    (U2,) = (obs(q.detach()),)
    gth_only = torch.cat([g.reshape(-1) for g in torch.autograd.grad((U2 * T(gU)).sum(), ps)])
    theta = torch.cat([p.detach().reshape(-1) for p in ps])
    ti, tf = _torch_ops.terms_args(obs._terms)
    cell = _torch_ops.cell_args(obs._cell_struct)
    U_t = ns.energy_frames_fwd(q.detach(), cell, ti, tf, obs._masks, theta)
    gq_t, gth_t = ns.energy_frames_bwd(q.detach(), cell, ti, tf, obs._masks, theta, T(gU), True)
    none_t, gth_only_t = ns.energy_frames_bwd(q.detach(), cell, ti, tf, obs._masks, theta, T(gU), False)
    assert torch.equal(U_t, U.detach()) and torch.equal(gq_t, grads[0]) and torch.equal(gth_t, gth)
    assert none_t.numel() == 0 and torch.equal(gth_only_t, gth_only)
    with pytest.raises(RuntimeError, match="theta"):
        ns.energy_frames_fwd(q.detach(), cell, ti, tf, obs._masks, theta[:1])


def test_errors():
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, GNNPotentials, Stack
    from mdgrad_amd.nn import get_model
    from mdgrad_amd.thermo import PotentialEnergy
    fx, two = frames_108()
    system = mk_system(fx.x, fx.cell, DEV)
    pair = PairPotentials(system, P.LennardJones(1.0, 1.0), cutoff=2.5)
    gnn = GNNPotentials(system, get_model({"n_atom_basis": 16, "n_filters": 16, "n_gaussians": 8, "n_convolutions": 1,
                                           "cutoff": 2.5}), cutoff=2.5)
    with pytest.raises(NotImplementedError, match="Reweighting accepts any callable"):
        PotentialEnergy(system, Stack({"pair": pair, "gnn": gnn}))
    mlp = P.pairMLP(n_gauss=8, r_start=0.5, r_end=2.5, n_layers=1, n_width=8, nonlinear="ELU")
    with pytest.raises(NotImplementedError, match="Reweighting accepts any callable"):
        PotentialEnergy(system, PairPotentials(system, mlp, cutoff=2.5))
    tric = mk_system(fx.x, np.array([[4.8, 0, 0], [0.6, 4.8, 0], [0, 0, 4.8]]), DEV)
    with pytest.raises(ValueError, match="diagonal"):
        PotentialEnergy(tric, PairPotentials(tric, P.LennardJones(1.0, 1.0), cutoff=2.0))
    obs = PotentialEnergy(system, pair)
    with pytest.raises(ValueError, match="k \\* 108"):
        obs(torch.zeros(2, 100, 3, device=DEV))
    q = T(two).requires_grad_(True)
    (gq,) = torch.autograd.grad(obs(q).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):
        gq.pow(2).sum().backward()
    # float64 device positions take the torch restatement, not the kernels
    U64 = obs(T(two).double())
    assert U64.dtype == torch.float64 and torch.allclose(U64.float(), obs(T(two)), rtol=1e-5)
