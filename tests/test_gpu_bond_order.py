"""Bond-orientational order on the GPU (csrc/bond_order.hip, ops.BondOrderFn, observable.bond_order) against the float64
definition of tests/bond_order_ref.py (Legendre polynomials through the addition theorem, from the same float32 positions).

Tolerances are derived (bond_order_ref.bond_order64 evaluates them per atom); eps = 2^-24, every sum is bounded through the sum
of the absolute values of its terms, never through its value:

  bond vector   u = fl(x_j - x_i) - o L carries |du| <= eps (|x_j - x_i| + r), so geo = (|x_j - x_i| + r) / r is the relative error
                of u in units of eps; it moves s by geo eps and Y_l by sqrt(l (l+1)) geo eps |Y_l| (|grad_s Y_l| = sqrt(l (l+1)) |Y_l|)
  weight        |dw| <= eps (W1 r geo + 8) inside the switching zone, W1 = pi / (2 (cutoff - r_in)) >= |w'|; exact outside it
  harmonics     |Y32 - Y64|_2 <= KAPPA[l] eps |Y_l|_2 over the 2l+1 components, the recurrence's constant.  It is MEASURED, as it
                cannot be derived: numpy float32 against float64 of the same recurrences over 20 016 directions with the poles
                and the axes (bond_order_ref.measure_kappa), times 4 for the orderings the transcription does not reproduce
                (fused multiply-adds, the table applied after the sum).  Measured / table: l = 4: 23.9 / 100, l = 6: 42.0 / 176,
                l = 12: 141.3 / 576; for the tangential gradient over sqrt(l (l+1)) |Y_l|: 16.8 / 72, 29.4 / 120, 82.8 / 336.
  row sum       a chain of cnt_i terms: cnt_i eps sum_j w_j |Y_l|.  With sqrt(4 pi / (2l+1)) |Y_l(s)|_2 = 1 the scale of A_l(i) is n_i:
      efwd_l(i) = eps sum_j [w_j (KAPPA[l] + sqrt(l (l+1)) geo_j + cnt_i + 2) + W1 r_j geo_j + 8 zone_j]    >= sqrt(4 pi / (2l+1)) |dA_l(i)|_2
      en(i)     = eps sum_j [w_j cnt_i + W1 r_j geo_j + 8 zone_j]                                           >= |dn_i|
      |q_l(i) - q64| <= (efwd_l(i) + en(i)) / n_i + (2l + 8) eps          (| |A + dA| - |A| | <= |dA|: no cancellation problem at q = 0)
      |Q_l - Q64|    <= (sum_i efwd_l + sum_i en) / sum_i n_i + (N + 2l + 8) eps                          (the atom sum: N terms)
      |S_l[i,j] - S64| <= efwd_l(i) n_j + n_i efwd_l(j) + (2l + 4) eps n_i n_j
  gradient      per bond and l the terms are bounded by Gamma_l (W1 + sqrt(l (l+1)) w / r), Gamma_l = gamma_l(i) + gamma_l(j),
                gamma_l(i) = sqrt((2l+1) / (4 pi)) |dLoss/dA_l(i)|_2 (basis-free: sqrt(diag(V S V^T)) with V = dLoss/dS + transpose),
                plus (|gn_i| + |gn_j|) W1; gabs(i) is their sum over the row.  tol_g(i) adds up: the chain (cnt_i n_l + 4) eps gabs;
                per term the harmonic constants KAPPA / KAPPA_G, the geometry (one more derivative: (l + 2) geo) and the
                weight's (pi / (cutoff - r_in) r geo for w'); and the error of the cotangents themselves, which the float32
                forward result feeds: d gamma_l(i) <= 2 sum_j |V_ij| efwd_l(j) + (N + 16) eps gamma_l(i), likewise for gn.
The bounds are worst cases (every rounding aligned, and for the gradient every atom's forward error pushing the cotangents the
same way), so the observed figures sit far below them.  Every comparison prints its figure before it asserts.

Wrapped against unwrapped frames: the kernels re-image x_j - x_i themselves (they do not read the list's shifts), and
fl(x_j - x_i) differs between the two copies, so the two agree within the bounds, not bitwise.

Largest figures an MI355X showed over the cases below, as observed / allowed: q_l 4.2e-7 / 1.3e-5 (index_tuple; 0.033 of the
bound), Q_l 9.6e-8 / 1.6e-5 (fcc; 0.006), S 3.6e-7 / 9.4e-6 (switching zone; 0.038), gradient 8.7e-6 / 5.6e-3 at |g| = 4.4
(index_tuple; 0.0016), count 8.0e-10 / 1.3e-7 and its gradient 1.6e-7 / 2.3e-4; against Steinhardt's five-digit values
|q_l - table| <= 4.9e-6.  The float32 numpy transcription of the forward shows the same fractions on the CPU
(tests/test_bond_order_host.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import bond_order_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def figure(what, observed, allowed):
    print("FIGURE %-78s observed %.3e  allowed %.3e" % (what, observed, allowed))


def mk_system(pos, box, n_rep=0):
    from mdgrad_amd.system import System
    box = np.broadcast_to(np.asarray(box, dtype=np.float64), (3,))
    s = System(positions=np.asarray(pos, dtype=np.float64), cell=np.array(box), masses=np.full(len(pos), 1.008), device=DEV)
    return s.replicate(n_rep) if n_rep else s


def dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).to(DEV)


def S_of(obs, A):
    """S_l[i, j] = 4 pi / (2l+1) sum_m A_lm(i) A_lm(j) of one frame A [N, K], as elementwise float32 torch."""
    return torch.stack([4.0 * math.pi / (2 * l + 1) * (A[:, None, o0:o1] * A[None, :, o0:o1]).sum(-1)
                        for l, o0, o1 in zip(obs.ls, obs.offsets_l[:-1], obs.offsets_l[1:])])


def run(obs, x, G=None, H=None, Cm=None):
    """One frame x [N, 3]: (q [N, n_l], Q [n_l], S [n_l, N, N], A, n, g = d(sum G q + sum H Q + sum C S)/dx) through the kernels."""
    xt = dev(x).requires_grad_(True)
    A, n = obs.moments(xt[None])
    q, Q = obs._invariants(A, n)[0], obs._invariants(A.sum(-2), n.sum(-1))[0]
    S = S_of(obs, A[0])
    loss = q.sum() * 0
    if G is not None:
        loss = loss + (dev(G) * q).sum()
    if H is not None:
        loss = loss + (dev(H) * Q).sum()
    if Cm is not None:
        loss = loss + (dev(Cm) * S).sum()
    (g,) = torch.autograd.grad(loss, xt)
    return q.detach(), Q.detach(), S.detach(), A.detach()[0], n.detach()[0], g


def compare(what, ref, q, Q, S, g, grad=True):
    q, Q, S = (t.cpu().double().numpy() for t in (q, Q, S))
    assert np.isfinite(q).all() and np.isfinite(Q).all()
    for name, got, want, tol in (("q", q, ref["q"], ref["tol_q"]), ("Q", Q, ref["Q"], ref["tol_Q"]), ("S", S, ref["S"], ref["tol_S"])):
        err = np.abs(got - want)
        worst = int(np.argmax(err / (tol + 1e-300)))
        figure("%s: |%s - %s64| (worst against its bound)" % (what, name, name), err.flat[worst], tol.flat[worst])
    if grad:
        gg = g.cpu().double().numpy()
        assert np.isfinite(gg).all()
        err = np.abs(gg - ref["gx"]).max(1)
        worst = int(np.argmax(err / (ref["tol_g"] + 1e-300)))
        figure("%s: |g - g64| (worst against its bound; gabs %.2e, |g| %.2e)" % (what, ref["gabs"][worst], np.abs(ref["gx"]).max()),
               err[worst], ref["tol_g"][worst])
    assert (np.abs(q - ref["q"]) <= ref["tol_q"]).all(), what + ": q"
    assert (np.abs(Q - ref["Q"]) <= ref["tol_Q"]).all(), what + ": Q"
    assert (np.abs(S - ref["S"]) <= ref["tol_S"]).all(), what + ": S"
    if grad:
        assert (err <= ref["tol_g"]).all(), what + ": gradient"


def weights(N, nl, seed):
    """Random cotangents G [N, n_l], H [n_l], C [n_l, N, N] of comparable weight in the loss."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (N, nl)).astype(np.float32), (rng.uniform(-1, 1, nl) * N).astype(np.float32),
            (rng.uniform(-1, 1, (nl, N, N)) / N).astype(np.float32))


_refs = {}


def ref_of(key, make):
    """A float64 reference, computed once per session and never modified."""
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


# ---------------------------------------------------------------------------------------------- lattices
@pytest.mark.parametrize("name", ["sc", "fcc", "bcc8", "bcc14", "hcp", "tetrahedral"])
def test_lattice_values(name):
    """Every atom and Q_l against the reference within the bounds and against Steinhardt's values to 1e-5 (plus the bound).  sc:
    the bonds lie along +-x, +-y, +-z (the poles s_x = s_y = 0) and a third of them cross the periodic boundary."""
    from mdgrad_amd.observable import bond_order
    kind, reps, rc, ri, vals = R.LATTICES[name]
    pos, box = R.lattice(kind, reps)
    assert rc < 0.5 * box.min()
    ls = tuple(sorted(vals))
    G, H, Cm = weights(len(pos), len(ls), 5)
    ref = ref_of(("lattice", name), lambda: R.bond_order64(pos, box, rc, ri, ls, G=G, H=H, C=Cm))
    assert (ref["cnt"] == R.SHELL[name]).all()
    obs = bond_order(mk_system(pos, box), ls=ls, cutoff=rc, r_in=ri)
    q, Q, S, A, n, g = run(obs, pos, G, H, Cm)
    compare(name, ref, q, Q, S, g)
    for k, l in enumerate(ls):
        err = float((q[:, k].cpu().double() - vals[l]).abs().max())
        figure("%s: |q_%d - %.5f| over the atoms" % (name, l, vals[l]), err, 1e-5 + float(ref["tol_q"][:, k].max()))
        assert err <= 1e-5 + ref["tol_q"][:, k].max()


@pytest.mark.parametrize("name", ["sc", "fcc", "bcc8"])
def test_odd_l_vanishes_on_centrosymmetric_lattices_with_zero_gradient(name):
    from mdgrad_amd.observable import BOND_ORDER_Q_FLOOR, bond_order
    kind, reps, rc, ri, _ = R.LATTICES[name]
    pos, box = R.lattice(kind, reps)
    ls = (1, 3, 5, 11)
    G, H, _ = weights(len(pos), len(ls), 6)
    ref = ref_of(("odd", name), lambda: R.bond_order64(pos, box, rc, ri, ls, G=G, H=H))
    assert (ref["q"] <= 1e-12).all() and ref["below"].all() and ref["Below"].all() and (ref["gx"] == 0).all()
    q, Q, S, A, n, g = run(bond_order(mk_system(pos, box), ls=ls, cutoff=rc, r_in=ri), pos, G, H)
    figure("%s odd l: largest q_l" % name, float(q.max()), float(ref["tol_q"].max()))
    figure("%s odd l: largest Q_l" % name, float(Q.max()), float(ref["tol_Q"].max()))
    assert (q.cpu().double().numpy() <= ref["tol_q"]).all() and (Q.cpu().double().numpy() <= ref["tol_Q"]).all()
    assert ref["tol_q"].max() * 16 <= BOND_ORDER_Q_FLOOR
    assert (g == 0).all(), "the floor rule must give an exactly zero gradient"


# ---------------------------------------------------------------------------------------------- disordered
def _disordered_case(which):
    D = R.DISORDERED
    x = R.disordered(1)[0]
    G, H, Cm = weights(D["N"], len(D["ls"]), 7)
    kw = dict(G=G, H=H) if which == "GH" else dict(C=Cm)
    ref = ref_of(("disordered", which), lambda: R.bond_order64(x, [D["box"]] * 3, D["cutoff"], D["r_in"], D["ls"], **kw))
    return D, x, (G if which == "GH" else None), (H if which == "GH" else None), (Cm if which == "C" else None), ref


@pytest.mark.parametrize("which", ["GH", "C"])
def test_disordered_against_float64(which):
    """70 atoms (not a multiple of 64), ls = (3, 4, 6, 12).  GH: d(sum G q + sum H Q)/dx; C: d(sum C S)/dx, which pins the whole
    of A up to the basis and drives the backward with a generic gA.  No atom is left out by the floor rule (Q_3 is: Q_l of an odd
    l vanishes identically, every bond being counted in both directions -- and its gradient is zero on both sides)."""
    from mdgrad_amd.observable import bond_order
    D, x, G, H, Cm, ref = _disordered_case(which)
    assert not ref["below"].any(), "an atom of the disordered configuration sits at or below the floor: pick another seed"
    obs = bond_order(mk_system(x, D["box"]), ls=D["ls"], cutoff=D["cutoff"], r_in=D["r_in"])
    q, Q, S, A, n, g = run(obs, x, G, H, Cm)
    compare("disordered " + which, ref, q, Q, S, g)
    assert float(g.abs().max()) > 0


# ---------------------------------------------------------------------------------------------- edge cases
def test_atoms_without_neighbours():
    from mdgrad_amd.observable import bond_order, bond_order_distribution
    P, x = R.SPARSE, R.sparse9()
    G, H, _ = weights(9, 2, 8)
    ref = ref_of("sparse", lambda: R.bond_order64(x, [P["box"]] * 3, P["cutoff"], P["r_in"], P["ls"], G=G, H=H))
    lonely = ref["n"] == 0
    assert lonely.sum() == 2
    system = mk_system(x, P["box"])
    q, Q, S, A, n, g = run(bond_order(system, ls=P["ls"], cutoff=P["cutoff"], r_in=P["r_in"]), x, G, H)
    compare("9 atoms in a box of 10", ref, q, Q, S, g)
    lone = torch.as_tensor(lonely).to(DEV)
    assert (q[lone] == 0).all() and (n[lone] == 0).all() and (g[lone] == 0).all() and torch.isfinite(g).all()
    # the histogram leaves them out: a centre at q = 0 receives nothing although two atoms have q = 0
    dist = bond_order_distribution(system, 6, 3, (0.0, 1.0), P["cutoff"], r_in=P["r_in"], width=0.01)
    bins, count, qq = dist(dev(x)[None])
    assert float(count[0]) == 0.0 and abs(float(count.sum()) - 1.0) <= 4 * R.EPS and qq.shape == (1, 9)


def test_switching_zone_and_the_cutoff_edge():
    from mdgrad_amd.observable import bond_order
    P, x = R.SWITCHING, R.switching()
    G, H, Cm = weights(6, 2, 9)
    ref = ref_of("switching", lambda: R.bond_order64(x, [P["box"]] * 3, P["cutoff"], P["r_in"], P["ls"], G=G, H=H, C=Cm))
    assert ref["cnt"][0] == 4                                    # the atom at r = cutoff exactly is no neighbour
    assert abs(ref["n"][0] - 3.5) < 1e-12                        # three full bonds and w(1.375) = 1/2 half-way through the zone
    q, Q, S, A, n, g = run(bond_order(mk_system(x, P["box"]), ls=P["ls"], cutoff=P["cutoff"], r_in=P["r_in"]), x, G, H, Cm)
    compare("switching zone", ref, q, Q, S, g)
    figure("switching zone: |n_0 - 3.5|", abs(float(n[0]) - 3.5), 16 * R.EPS)
    assert abs(float(n[0]) - 3.5) <= 16 * R.EPS


def test_rows_longer_than_a_wave():
    from mdgrad_amd.observable import bond_order
    P, x = R.DENSE, R.dense()
    G, H, Cm = weights(P["N"], 2, 10)
    ref = ref_of("dense", lambda: R.bond_order64(x, [P["box"]] * 3, P["cutoff"], P["r_in"], P["ls"], G=G, H=H, C=Cm))
    assert ref["cnt"].max() == 69 > 64
    q, Q, S, A, n, g = run(bond_order(mk_system(x, P["box"]), ls=P["ls"], cutoff=P["cutoff"], r_in=P["r_in"]), x, G, H, Cm)
    compare("rows of 69", ref, q, Q, S, g)


def test_index_tuple():
    from mdgrad_amd import ops
    from mdgrad_amd.observable import bond_order
    D = R.DISORDERED
    x = R.disordered(1)[0]
    it = (list(range(0, 30)), list(range(20, 70)))
    mask = ops.build_mask(D["N"], it, None, "cpu").numpy()
    ls = (4, 6)
    G, H, _ = weights(D["N"], 2, 11)
    ref = ref_of("index_tuple", lambda: R.bond_order64(x, [D["box"]] * 3, D["cutoff"], D["r_in"], ls, mask=mask, G=G, H=H))
    full = _disordered_case("GH")[-1]
    assert ref["cnt"].sum() < full["cnt"].sum()
    obs = bond_order(mk_system(x, D["box"]), ls=ls, cutoff=D["cutoff"], r_in=D["r_in"], index_tuple=it)
    q, Q, S, A, n, g = run(obs, x, G, H)
    compare("index_tuple", ref, q, Q, S, g)


def test_replicas_equal_separate_runs_bitwise():
    from mdgrad_amd.observable import bond_order
    D = R.DISORDERED
    xs = R.disordered(3, seed=21)                                               # [3, N, 3]: three different configurations
    kw = dict(ls=D["ls"], cutoff=D["cutoff"], r_in=D["r_in"])
    one, stk = bond_order(mk_system(xs[0], D["box"]), **kw), bond_order(mk_system(xs[0], D["box"], 3), **kw)
    stacked = dev(xs.reshape(1, 3 * D["N"], 3)).requires_grad_(True)
    q, Q = stk.per_atom(stacked), stk.per_frame(stacked)
    assert q.shape == (1, 3, D["N"], 4) and Q.shape == (1, 3, 4) and stk(stacked).shape == (4,)
    G, H, _ = weights(D["N"], 4, 12)
    (g,) = torch.autograd.grad((q * dev(G)).sum() + (Q * dev(H)).sum(), stacked)
    for r in range(3):
        xr = dev(xs[r])[None].requires_grad_(True)
        qr, Qr = one.per_atom(xr), one.per_frame(xr)
        assert qr.shape == (1, D["N"], 4) and Qr.shape == (1, 4)
        (gr,) = torch.autograd.grad((qr * dev(G)).sum() + (Qr * dev(H)).sum(), xr)
        assert torch.equal(qr[0], q[0, r]) and torch.equal(Qr[0], Q[0, r])
        assert torch.equal(gr[0], g[0, r * D["N"]:(r + 1) * D["N"]])
    assert torch.equal(stk(stacked), Q.reshape(-1, 4).mean(0))


def test_wrapped_and_unwrapped_frames_agree_within_the_bounds():
    from mdgrad_amd.observable import bond_order
    D, x, G, H, _, ref = _disordered_case("GH")
    shift = np.random.default_rng(13).integers(0, 2, x.shape) * (x < 0.5 * D["box"])             # some atoms one cell further out
    xu = (x + np.float32(D["box"]) * shift).astype(np.float32)
    assert shift.any() and np.abs(xu[:, None] - xu[None]).max() < 1.5 * D["box"]
    refu = ref_of("unwrapped", lambda: R.bond_order64(xu, [D["box"]] * 3, D["cutoff"], D["r_in"], D["ls"], G=G, H=H))
    assert np.abs(refu["q"] - ref["q"]).max() < 1e-5            # the same frame up to the float32 rounding of x + L
    obs = bond_order(mk_system(x, D["box"]), ls=D["ls"], cutoff=D["cutoff"], r_in=D["r_in"])
    q, Q, S, A, n, g = run(obs, xu, G, H)
    compare("unwrapped copy", refu, q, Q, S, g)


def test_frame_chunks_and_launches_are_bitwise_equal():
    from mdgrad_amd import ops
    from mdgrad_amd.observable import bond_order, bond_order_distribution
    D = R.DISORDERED
    xs = dev(R.disordered(5, seed=31))
    kw = dict(cutoff=D["cutoff"], r_in=D["r_in"])
    obs = bond_order(mk_system(xs[0].cpu().numpy(), D["box"]), ls=D["ls"], **kw)
    dist = bond_order_distribution(mk_system(xs[0].cpu().numpy(), D["box"]), 6, 24, (0.0, 1.0), D["cutoff"], r_in=D["r_in"])
    Gq = dev(np.random.default_rng(14).uniform(-1, 1, (5, D["N"], 4)))

    def once():
        xt = xs.clone().requires_grad_(True)
        A, n = obs.moments(xt)
        q = obs.per_atom(xt)
        (g,) = torch.autograd.grad((q * Gq).sum() + obs(xt).sum(), xt)
        return A.detach().clone(), n.detach().clone(), q.detach(), g, dist(xt)[1].detach()

    a, b = once(), once()
    assert all(torch.equal(p, r) for p, r in zip(a, b)), "two launches differ"
    assert ops.BOND_ORDER_CHUNK_FRAMES is None
    ops.BOND_ORDER_CHUNK_FRAMES = 2                             # 5 frames: chunks of 2, 2 and 1
    try:
        c = once()
    finally:
        ops.BOND_ORDER_CHUNK_FRAMES = None
    assert all(torch.equal(p, r) for p, r in zip(a, c)), "several frame chunks differ from one"
    figure("histogram sum - 1 (chunked)", abs(float(c[4].sum()) - 1.0), 24 * R.EPS)
    assert abs(float(c[4].sum()) - 1.0) <= 24 * R.EPS           # a float32 sum of 24 non-negative terms


def test_torch_ops_equal_the_ctypes_path():
    """ops.BondOrderFn goes through torch.ops.mdgrad.bond_order_fwd / _bwd when the op library is loaded; the C ABI called
    through ctypes gives the same bits."""
    from mdgrad_amd import _lib, _torch_ops, ops
    ns = _torch_ops.get()
    assert ns is not None and hasattr(ns, "bond_order_fwd") and hasattr(ns, "bond_order_bwd")
    D = R.DISORDERED
    x = dev(R.disordered(2, seed=41))
    F, N, ls = 2, D["N"], list(D["ls"])
    K = sum(2 * l + 1 for l in ls)
    cs = _lib.make_cell(torch.tensor([D["box"]] * 3))
    flat = x.reshape(-1, 3)
    ell = ops.build_ell(flat, cs, D["cutoff"], None, group=N)
    A, n = ns.bond_order_fwd(flat, F, N, _torch_ops.cell_args(cs), D["cutoff"], D["r_in"], ell.col, ell.cnt, ls)
    assert A.shape == (K, F * N) and n.shape == (F * N,)
    gA, gn = torch.randn(F * N, K, device=DEV), torch.randn(F * N, device=DEV)
    g = ns.bond_order_bwd(flat, F, N, _torch_ops.cell_args(cs), D["cutoff"], D["r_in"], ell.col, ell.cnt, ls, gA, gn)
    lib = _lib.load()
    A2, n2, g2 = torch.empty_like(A), torch.empty_like(n), torch.empty_like(g)
    ls_c = (C.c_int32 * len(ls))(*ls)
    st = _lib.stream_ptr(x.device)
    args = (_lib.ptr(flat), F, N, C.byref(cs), D["cutoff"], D["r_in"], _lib.ptr(ell.col), _lib.ptr(ell.cnt), ell.max_nbr, ls_c, len(ls))
    _lib.check(lib.mdg_bond_order_fwd(*args, _lib.ptr(A2), _lib.ptr(n2), st), "mdg_bond_order_fwd")
    _lib.check(lib.mdg_bond_order_bwd(*args, _lib.ptr(gA), _lib.ptr(gn), _lib.ptr(g2), st), "mdg_bond_order_bwd")
    assert torch.equal(A, A2) and torch.equal(n, n2) and torch.equal(g, g2)
    Af, nf = ops.BondOrderFn.apply(x, tuple(ls), D["cutoff"], D["r_in"], cs, None)
    assert torch.equal(Af, A.view(K, F, N).permute(1, 2, 0)) and torch.equal(nf, n.view(F, N))
    with pytest.raises(RuntimeError, match="distinct"):
        ns.bond_order_fwd(flat, F, N, _torch_ops.cell_args(cs), D["cutoff"], D["r_in"], ell.col, ell.cnt, [4, 4])
    xg = x.clone().requires_grad_(True)
    Ag, ng = ops.BondOrderFn.apply(xg, tuple(ls), D["cutoff"], D["r_in"], cs, None)
    (gg,) = torch.autograd.grad((Ag * gA.view(F, N, K)).sum() + (ng * gn.view(F, N)).sum(), xg, create_graph=True)
    assert torch.equal(gg.reshape(-1, 3), g)
    with pytest.raises(RuntimeError):
        gg.sum().backward()                                     # differentiable once


def test_distribution_against_float64():
    """count and d(sum c count)/dx of bond_order_distribution on two disordered frames against bond_order64 composed with
    float64 Gaussian smearing.  Bounds: raw_b = sum_i e_ib with |d e_ib| <= |d e_ib / dq| tol_q(i) + 8 eps e_ib, a float32 sum of
    F N terms, count = raw / sum raw; for the gradient the cotangent dLoss/dq is itself in error by |Hessian| tol_q + 32 eps
    sum_b |c_b| |d count_b / dq_i|, which reaches x through at most gabs of that error (the gradient is linear in the cotangent)."""
    from mdgrad_amd.observable import bond_order_distribution
    D = R.DISORDERED
    xs = R.disordered(2, seed=51)
    l, nbins, F, N = 6, 16, 2, D["N"]
    dist = bond_order_distribution(mk_system(xs[0], D["box"]), l, nbins, (0.1, 0.8), D["cutoff"], r_in=D["r_in"])
    xt = dev(xs).requires_grad_(True)
    bins, count, q = dist(xt)
    cw = np.random.default_rng(15).uniform(-1, 1, nbins).astype(np.float32)
    (g,) = torch.autograd.grad((count * dev(cw)).sum(), xt)
    assert bins.shape == (nbins + 1,) and count.shape == (nbins,) and q.shape == (F, N)
    figure("distribution: |sum count - 1|", abs(float(count.detach().sum()) - 1.0), nbins * R.EPS)
    assert abs(float(count.detach().sum()) - 1.0) <= nbins * R.EPS
    none = bond_order_distribution(mk_system(xs[0], D["box"]), l, nbins, (0.1, 0.8), D["cutoff"], r_in=D["r_in"], keep_values=False)
    assert none(xt)[2] is None and torch.equal(none(xt)[1], count)
    box = [D["box"]] * 3
    plain = [R.bond_order64(xs[f], box, D["cutoff"], D["r_in"], (l,)) for f in range(F)]
    q64 = torch.tensor(np.concatenate([p["q"][:, 0] for p in plain]), requires_grad=True)
    tq = torch.tensor(np.concatenate([p["tol_q"][:, 0] for p in plain]))
    offsets, width = dist.smear.offsets.cpu().double(), float(dist.smear.width[0])
    ones, cw64 = torch.ones(F * N, dtype=torch.float64), torch.tensor(cw).double()
    loss_of = lambda v: (R.smear64(v, ones, offsets, width) * cw64).sum()
    c64 = R.smear64(q64, ones, offsets, width)
    (G64,) = torch.autograd.grad(loss_of(q64), q64)
    with torch.no_grad():
        e = torch.exp(-0.5 / width ** 2 * (q64[:, None] - offsets[None, :]) ** 2)
        de = (q64[:, None] - offsets[None, :]).abs() / width ** 2 * e
        d_raw = (de * tq[:, None] + 8 * R.EPS * e).sum(0) + F * N * R.EPS * e.sum(0)
        tol_c = (d_raw + c64 * d_raw.sum()) / e.sum() + 4 * R.EPS * c64
        Hess = torch.autograd.functional.hessian(loss_of, q64.detach())
        dcount = de / e.sum() + c64[None, :] * de.sum(1, keepdim=True) / e.sum()             # >= |d count_b / d q_i|
        dG = Hess.abs() @ tq + 32 * R.EPS * (dcount * cw64.abs()[None, :]).sum(1)
    err = (count.detach().cpu().double() - c64.detach()).abs()
    worst = int(torch.argmax(err / tol_c))
    figure("distribution: |count - count64| (worst against its bound)", float(err[worst]), float(tol_c[worst]))
    assert (err <= tol_c).all()
    for f in range(F):
        sl = slice(f * N, (f + 1) * N)
        ref = R.bond_order64(xs[f], box, D["cutoff"], D["r_in"], (l,), G=G64[sl].numpy()[:, None])
        extra = R.bond_order64(xs[f], box, D["cutoff"], D["r_in"], (l,), G=(dG[sl] + R.EPS * G64[sl].abs()).numpy()[:, None])["gabs"]
        gerr = np.abs(g[f].cpu().double().numpy() - ref["gx"]).max(1)
        tol = ref["tol_g"] + extra
        worst = int(np.argmax(gerr / (tol + 1e-300)))
        figure("distribution frame %d: |g - g64| (worst against its bound, |g| %.2e)" % (f, np.abs(ref["gx"]).max()), gerr[worst], tol[worst])
        assert (gerr <= tol).all() and np.abs(ref["gx"]).max() > 0


def test_non_finite_positions_give_nan():
    from mdgrad_amd.observable import bond_order
    D = R.DISORDERED
    x = R.disordered(1)[0].copy()
    x[17] = np.nan
    x[40, 1] = np.inf
    obs = bond_order(mk_system(R.disordered(1)[0], D["box"]), ls=(4, 6), cutoff=D["cutoff"], r_in=D["r_in"])
    xt = dev(x)[None].requires_grad_(True)
    q, Q = obs.per_atom(xt), obs.per_frame(xt)
    bad = torch.zeros(D["N"], dtype=torch.bool, device=DEV)
    bad[[17, 40]] = True
    assert torch.isnan(q[0, bad]).all() and torch.isfinite(q[0, ~bad]).all() and torch.isnan(Q).all()
    (g,) = torch.autograd.grad(q[0, ~bad].sum(), xt)
    assert torch.isnan(g[0, bad]).all()
    allnan = torch.full((1, D["N"], 3), float("nan"), device=DEV)
    assert torch.isnan(obs.per_atom(allnan)).all()
    torch.cuda.synchronize()
