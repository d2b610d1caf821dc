"""The Ewald correction for excluded and scaled pairs on the host, in float64 (no GPU): the explicit pair sums of
tests/ewald_excl_ref.py against autograd of its energy, the identity that makes an excluded pair's 1/r vanish from the Ewald
sum, the independence of the total of the splitting parameter, s = 1 against the real-space psi, EwaldExclusions / ewald on CPU
positions (the torch restatement) with their argument checks, and topology.exclusions_from_bonds."""
import numpy as np
import pytest
import torch

import coulomb_ref as R
import ewald_ref as E
import ewald_excl_ref as X


def _system(pos, cell, dim=3):
    from mdgrad_amd.system import System
    return System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
                  masses=np.full(len(pos), 1.008), device="cpu", dim=dim)


def _parts(x32, cell32, q32, pairs, rc, alpha, kc, scale=None):
    """(U_real with the mask, U_real without it, U_rec, U_excl) in float64, conversion 1."""
    x, q = torch.tensor(x32).double(), torch.tensor(q32).double()
    k = R.consts(rc, alpha, "none", 1.0)
    masked = R.energy(x, q, R.half_list(x32, cell32, rc, ex_pairs=pairs), cell32, k)
    plain = R.energy(x, q, R.half_list(x32, cell32, rc), cell32, k)
    n, _ = E.vectors(cell32.astype(np.float64), kc)
    rec = E.energy(x, q, n, cell32.astype(np.float64), alpha)
    excl = X.energy(x, q, pairs, scale, cell32.astype(np.float64), alpha)
    return float(masked), float(plain), float(rec), float(excl)


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("group", [None, 9], ids=["one_replica", "two_replicas"])
def test_explicit_pair_sums_equal_autograd_of_the_energy(group):
    """grad, H.w, dU/dq and d(w.dU/dx)/dq of ewald_excl_ref.evaluate against autograd of its energy on 18 atoms with 9 pairs
    (one across the box boundary, one coincident, scales 0 / 0.5 / 1), to 1e-10 of the largest entry."""
    rng = np.random.default_rng(9)
    L = np.array([5.0, 6.0, 7.0])
    x = rng.uniform(0, 1, (18, 3)) * L
    x[1] = np.mod(x[0] + np.array([0.4, 0.0, 0.0]), L)
    x[0, 0], x[1, 0] = 0.1, 4.8                                  # pair (0, 1) across the boundary
    x[5] = x[4]                                                  # pair (4, 5) coincident
    g = 18 if group is None else group
    pairs = np.array([[0, 1], [2, 3], [4, 5], [6, 7], [1, 2], [8, 0], [3, 5], [7, 8], [6, 2]])
    pairs = pairs if group is not None else np.concatenate([pairs, pairs[:4] + 9])
    scale = np.resize(np.array([0.0, 0.5, 1.0]), len(pairs))
    x = torch.tensor(x, requires_grad=True)
    q = torch.tensor(rng.normal(0, 1, 18) + 0.2, requires_grad=True)
    w = torch.tensor(rng.normal(0, 1, (18, 3)))
    alpha, conv = 0.8, 1.7
    U = X.energy(x, q, pairs, scale, L, alpha, conv, group=g)
    gx, gq = torch.autograd.grad(U, (x, q), create_graph=True)
    hx, hq = torch.autograd.grad((gx * w).sum(), (x, q))
    ref = X.evaluate(x.detach(), q.detach(), pairs, scale, L, alpha, conv, w=w, group=g)

    def same(a, b, what):
        assert float((a - b).abs().max()) <= 1e-10 * float(b.abs().max()), what
    same(ref["U"].reshape(1), U.detach().reshape(1), "U")
    same(ref["grad"], gx.detach(), "dU/dx")
    same(conv * ref["pot"], gq.detach(), "dU/dq")
    same(conv * ref["potw"], hq, "d(w.dU/dx)/dq")
    # the Hessian of a coincident pair is the limit, which autograd of the guarded energy does not see: compare elsewhere,
    # and the coincident pair against the limit of a pair 1e-5 apart
    rest = torch.ones(18, dtype=torch.bool)
    rest[[4, 5]] = False
    same(ref["hw"][rest], hx[rest], "H.w")
    x2 = x.detach().clone()
    x2[5, 0] += 1e-5
    only = np.array([[4, 5]])
    near = X.evaluate(x2, q.detach(), only, None, L, alpha, conv, w=w, group=g)
    at = X.evaluate(x.detach(), q.detach(), only, None, L, alpha, conv, w=w, group=g)
    assert float(at["hw"][4].abs().max()) > 0 and float(at["grad"][4:6].abs().max()) == 0.0 and float(at["potw"][4:6].abs().max()) == 0.0
    assert float((near["hw"][4:6] - at["hw"][4:6]).abs().max()) <= 1e-4 * float(at["hw"][4:6].abs().max())
    assert float((near["U"] - at["U"]).abs()) <= 1e-8 * float(at["A_U"]) and float(at["U"]) != 0.0
    for key in ("grad", "pot", "hw", "potw"):
        assert bool((ref[key].abs() <= ref["A_" + key] * (1 + 1e-12)).all()), "A_%s bounds |%s|" % (key, key)


# ------------------------------------------------------------------------------------------------ (b)
def test_identity_an_excluded_pair_loses_its_whole_coulomb_interaction():
    """water27, rc = 4.5, conversion 1:  U_real(masked) + U_rec + U_excl(s = 0) == U_real(unmasked) + U_rec - sum_P q_i q_j / r_ij
    to 1e-10 (both sides -0.05235053)."""
    x32, cell32, q32, _, pairs, _, _ = X.water27()
    alpha, kc = 0.7540, 5.117
    masked, plain, rec, excl = _parts(x32, cell32, q32, pairs, 4.5, alpha, kc)
    x, q = torch.tensor(x32).double(), torch.tensor(q32).double()
    d = X.reimage(x[pairs[:, 0]] - x[pairs[:, 1]], cell32.astype(np.float64))
    bare = float((q[pairs[:, 0]] * q[pairs[:, 1]] / d.pow(2).sum(-1).sqrt()).sum())
    lhs, rhs = masked + rec + excl, plain + rec - bare
    print("identity: %.8f %.8f   parts: real %.5f  recip %.5f  excl %.5f" % (lhs, rhs, masked, rec, excl))
    assert abs(lhs - rhs) <= 1e-10
    assert abs(lhs + 0.05235053) <= 5e-8, "the figure of the issue"


def test_total_with_exclusions_is_independent_of_alpha():
    """The totals at (alpha, k_cutoff) = (0.7540, 5.117) and (0.8445, 6.419) differ by at most 1e-5 (observed -0.05235053 and
    -0.05234792: 2.6e-6) while the three parts are of order +-11."""
    x32, cell32, q32, _, pairs, _, _ = X.water27()
    tot = []
    for alpha, kc in ((0.7540, 5.117), (0.8445, 6.419)):
        masked, _, rec, excl = _parts(x32, cell32, q32, pairs, 4.5, alpha, kc)
        tot.append(masked + rec + excl)
        assert max(abs(masked), abs(rec), abs(excl)) > 5.0
    print("totals", tot)
    assert abs(tot[0] - tot[1]) <= 1e-5


# ------------------------------------------------------------------------------------------------ (c)
def test_scale_one_is_the_real_space_psi_pair_by_pair():
    r = torch.tensor(np.geomspace(1e-3, 6.0, 50))
    for alpha in (0.4, 0.754, 1.3):
        got = X.chi(r, torch.ones_like(r), alpha)
        want = R.psi(r, R.consts(10.0, alpha, "none"))
        # (1 - erf carries the rounding of 1: the agreement is relative to the s part 1/r, 1/r^2, 2/r^3)
        for a, b, sc, nm in zip(got, want, (1 / r, 1 / r ** 2, 2 / r ** 3), ("chi", "chi'", "chi''")):
            assert float(((a - b).abs() / sc).max()) <= 1e-14, nm


# ------------------------------------------------------------------------------------------------ (d)
def test_class_on_cpu_float64_equals_the_reference_energy():
    from mdgrad_amd.interface import CoulombPotentials, EwaldExclusions, EwaldReciprocal
    x32, cell32, q32, types, pairs, _, _ = X.water27()
    system = _system(x32, cell32)
    real = CoulombPotentials(system, q32, 4.5, alpha=0.754, shift="none", conversion=2.5, ex_pairs=pairs)
    scale = np.resize(np.array([0.0, 0.5, 1.0]), len(pairs))
    for sc in (None, 0.5, scale):
        ex = EwaldExclusions(system, real, scale=sc)
        assert ex.alpha == 0.754 and ex.conversion == 2.5 and ex.charges is real.charges and not ex.supports_force_vjp()
        # unwrapped positions (whole boxes added) give the same value: the bond-vector re-imaging
        shift = np.random.default_rng(1).integers(-1, 2, (27, 1, 3)).repeat(3, 1).reshape(81, 3) * cell32.astype(np.float64)
        vals = []
        for xs in (x32.astype(np.float64), x32.astype(np.float64) + shift):
            x = torch.tensor(xs).requires_grad_(True)
            want = X.energy(x, torch.tensor(q32).double(), pairs, sc, cell32.astype(np.float64), 0.754, 2.5)
            got = ex(x)
            assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))
            (g,) = torch.autograd.grad(got, x)
            (gw,) = torch.autograd.grad(want, x)
            assert float((g - gw).abs().max()) <= 1e-11 * float(gw.abs().max())
            vals.append(float(got))
        assert abs(vals[0] - vals[1]) <= 1e-9 * abs(vals[0])
    rec = EwaldReciprocal(system, real, k_cutoff=5.117, exclusions=EwaldExclusions(system, real))
    assert rec.charges is real.charges
    # three replicas of per-type charges, the pairs of one replica serve all
    sys3 = _system(x32, cell32).replicate(3)
    real3 = CoulombPotentials(sys3, [-0.8, 0.4], 4.5, alpha=0.754, shift="none", conversion=1.0, types=types, ex_pairs=pairs,
                              trainable=True)
    ex3 = EwaldExclusions(sys3, real3, scale=0.5)
    x3 = torch.tensor(np.concatenate([x32, x32 + 0.1, x32 - 0.2])).double()
    c64 = torch.tensor([-0.8, 0.4], dtype=torch.float32).double().requires_grad_(True)
    want3 = X.energy(x3, c64[torch.as_tensor(types)].repeat(3), pairs, 0.5, cell32.astype(np.float64), 0.754, 1.0, group=81)
    got3 = ex3(x3)
    assert abs(float(got3) - float(want3)) <= 1e-12 * abs(float(want3))
    (gc,) = torch.autograd.grad(got3, ex3.charges)
    (gcw,) = torch.autograd.grad(want3, c64)
    assert float((gc.double() - gcw).abs().max()) <= 1e-6 * float(gcw.abs().max())
    # a coincident pair: the limit, finite, zero gradient there
    xc = x32.astype(np.float64).copy()
    xc[1] = xc[0]
    x = torch.tensor(xc).requires_grad_(True)
    ex0 = EwaldExclusions(system, real)
    got = ex0(x)
    want = X.evaluate(xc, q32, pairs, None, cell32.astype(np.float64), 0.754, 2.5)
    assert abs(float(got) - float(want["U"])) <= 1e-12 * float(want["A_U"])
    (g,) = torch.autograd.grad(got, x)
    assert bool(torch.isfinite(g).all()) and float((g - want["grad"]).abs().max()) <= 1e-11 * float(want["A_grad"].max())


def test_ewald_with_ex_pairs_returns_three_members_sharing_one_charges_tensor():
    from mdgrad_amd.interface import CoulombPotentials, EwaldExclusions, EwaldReciprocal, Stack, ewald
    x32, cell32, q32, types, pairs, _, _ = X.water27()
    system = _system(x32, cell32)
    terms = ewald(system, [-0.82, 0.41], 4.5, accuracy=1e-4, types=types, conversion=1.0, trainable=True, ex_pairs=pairs, scale=0.5)
    assert list(terms) == ["coulomb_real", "coulomb_recip", "coulomb_excl"]
    a, b, c = terms.values()
    assert isinstance(a, CoulombPotentials) and isinstance(b, EwaldReciprocal) and isinstance(c, EwaldExclusions)
    assert isinstance(a.charges, torch.nn.Parameter) and b.charges is a.charges and c.charges is a.charges
    assert len(list(Stack(terms).parameters())) == 1
    assert a.ex_pairs is pairs and float(c.scale.min()) == float(c.scale.max()) == 0.5 and c.alpha == a.alpha
    two = ewald(system, [-0.82, 0.41], 4.5, accuracy=1e-4, types=types, conversion=1.0)
    assert list(two) == ["coulomb_real", "coulomb_recip"], "without ex_pairs: exactly the two members"
    with pytest.raises(ValueError, match="scale"):
        ewald(system, q32, 4.5, scale=0.5)


# ------------------------------------------------------------------------------------------------ (e)
def test_classes_reject_what_the_sum_does_not_cover():
    from mdgrad_amd.interface import CoulombPotentials, EwaldExclusions, EwaldReciprocal
    x32, cell32, q32, _, pairs, _, _ = X.water27()
    system = _system(x32, cell32)

    def real(sysm=system, **kw):
        args = dict(alpha=0.754, shift="none", conversion=1.0, ex_pairs=pairs)
        args.update(kw)
        return CoulombPotentials(sysm, q32, 4.5, **args)
    for what, r, sysm in [("no ex_pairs", real(ex_pairs=None), system), ("shift", real(shift="force"), system),
                          ("shift", real(shift="potential"), system), ("alpha = 0", real(alpha=0.0), system),
                          ("self_energy", real(self_energy=False), system),
                          ("index_tuple", real(index_tuple=(list(range(10)), list(range(10, 81)))), system),
                          ("system.dim", real(), _system(x32, cell32, dim=2)),
                          ("i == j", real(ex_pairs=np.array([[0, 1], [3, 3]])), system),
                          ("twice", real(ex_pairs=np.array([[0, 1], [2, 3], [0, 1]])), system),
                          ("twice", real(ex_pairs=np.array([[0, 1], [2, 3], [1, 0]])), system)]:
        with pytest.raises(ValueError, match=what):
            EwaldExclusions(sysm, r)
    sys3 = _system(x32, cell32).replicate(3)
    outside = CoulombPotentials(sys3, q32, 4.5, alpha=0.754, shift="none", ex_pairs=np.array([[0, 1]]))
    outside.ex_pairs = np.array([[0, 81]])                      # (inside the system, outside the replica)
    with pytest.raises(ValueError, match="outside the replica"):
        EwaldExclusions(sys3, outside)
    outside.ex_pairs = np.array([[-1, 2]])
    with pytest.raises(ValueError, match="outside the replica"):
        EwaldExclusions(sys3, outside)
    for bad in (-0.1, 1.5, np.full(81, 2.0)):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            EwaldExclusions(system, real(), scale=bad)
    with pytest.raises(ValueError, match="one number per excluded pair"):
        EwaldExclusions(system, real(), scale=np.zeros(5))
    tric = _system(x32, np.array([[9.3, 0, 0], [1.0, 9.3, 0], [0, 0, 9.3]]))
    with pytest.raises(ValueError, match="diagonal"):
        EwaldExclusions(tric, real(tric))
    with pytest.raises(ValueError, match="CoulombPotentials"):
        EwaldExclusions(system, object())
    # EwaldReciprocal: refused as before without `exclusions`, with a pointer; lifted by the term built on the same `real`
    r1, r2 = real(), real()
    with pytest.raises(ValueError, match=r"ex_pairs.*exclusions="):
        EwaldReciprocal(system, r1)
    with pytest.raises(ValueError, match="same real-space term"):
        EwaldReciprocal(system, r1, exclusions=EwaldExclusions(system, r2))
    with pytest.raises(ValueError, match="same real-space term"):
        EwaldReciprocal(system, r1, exclusions=object())
    assert EwaldReciprocal(system, r1, k_cutoff=5.0, exclusions=EwaldExclusions(system, r1)).n_vectors > 100
    it = real(index_tuple=(list(range(10)), list(range(10, 81))))
    with pytest.raises(ValueError, match="index_tuple"):
        EwaldReciprocal(system, it)


# ------------------------------------------------------------------------------------------------ (f)
def test_exclusions_from_bonds_on_a_chain_a_branched_molecule_and_a_three_ring():
    from mdgrad_amd.topology import exclusions_from_bonds
    chain = [[0, 1], [1, 2], [2, 3], [3, 4]]
    p = exclusions_from_bonds(chain)
    assert p.dtype == torch.long and p.tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3], [2, 4], [3, 4]]
    p, sep = exclusions_from_bonds(chain, n_bonds=3, return_separation=True)
    assert p.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [1, 4], [2, 3], [2, 4], [3, 4]]
    assert sep.tolist() == [1, 2, 3, 1, 2, 3, 1, 2, 1]
    assert exclusions_from_bonds(chain, n_bonds=1).tolist() == [[0, 1], [1, 2], [2, 3], [3, 4]]
    # isobutane-like: centre 1 bonded to 0, 2, 3; 3 bonded to 4 (listed in mixed orientation, one bond twice, a self-bond)
    branched = torch.tensor([[1, 0], [1, 2], [3, 1], [3, 4], [0, 1], [2, 2]])
    p, sep = exclusions_from_bonds(branched, n_bonds=3, return_separation=True)
    assert p.tolist() == [[0, 1], [0, 2], [0, 3], [0, 4], [1, 2], [1, 3], [1, 4], [2, 3], [2, 4], [3, 4]]
    assert sep.tolist() == [1, 2, 2, 3, 1, 1, 2, 2, 3, 1]
    assert exclusions_from_bonds(branched).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [1, 4], [2, 3], [3, 4]]
    # three-ring with a tail: the shortest path counts (0-2 is one bond, not two)
    ring = [[0, 1], [1, 2], [2, 0], [2, 3]]
    p, sep = exclusions_from_bonds(ring, n_bonds=2, return_separation=True)
    assert p.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]] and sep.tolist() == [1, 1, 2, 1, 2, 1]
    assert exclusions_from_bonds(np.zeros((0, 2), dtype=np.int64)).shape == (0, 2)
    with pytest.raises(ValueError):
        exclusions_from_bonds(chain, n_bonds=0)
    # water: the 81 intramolecular pairs of water27 from its 54 bonds
    _, _, _, _, pairs, bonds, _ = X.water27()
    assert np.array_equal(exclusions_from_bonds(bonds).numpy(), pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))])
