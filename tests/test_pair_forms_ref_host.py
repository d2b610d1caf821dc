"""CPU checks of tests/pair_forms_ref.py, the float64 reference that tests/test_gpu_pair_forms_ref.py holds the trajectory
kernels and pair_ell to: its derivatives against central differences of its own energy, against float64 autograd of the torch
modules of mdgrad_amd/potentials.py over compute_dis-style distances, and against oracle.PairTerm.force_vjp in float64; the
fixtures (no fragile pair but the two placed ones, which land on the intended side of the cutoff); masks; and the float32
floors of every fixture, form and quantity, printed once (the GPU file's table quotes them)."""
import numpy as np
import pytest
import torch

import oracle as O
import pair_forms_ref as R

FORMS = list(R.FORMS)
ORACLE_KIND = {"lj": "lj", "morse": "morse", "buck": "buck", "yukawa": "yukawa"}


def _half_list(fx, term):
    """(i, j, offsets) of the selected pairs i < j with x_i - x_j - offsets . h the minimum-image vector (compute_dis)"""
    m = R.membership(fx.x, fx.cell, [term])[0]
    i, j = np.nonzero(np.triu(m, 1))
    D, _, _ = R._images(fx.x, fx.cell, np.dtype(np.float64))
    h = R._cell(fx.cell, np.dtype(np.float64))[0]
    x = fx.x.astype(np.float64)
    off = np.rint(((x[i] - x[j]) + D[i, j]) @ np.linalg.inv(h))             # x_i - x_j - off . h = -D
    return i, j, off, h


@pytest.mark.parametrize("form", FORMS)
def test_force_and_hessian_product_are_central_differences_of_the_energy(form):
    fx = R.liquid(31)
    term = R.Term(form)
    w = R.direction(31)
    member = R.membership(fx.x, fx.cell, [term])
    x0 = fx.x.astype(np.float64)
    ref = R.evaluate(x0, w, fx.cell, [term], member=member)

    def U(x):
        return float(R.evaluate(x, w, fx.cell, [term], member=member).U)

    h = 1e-4
    w64 = w.astype(np.float64)
    F, dq = np.zeros_like(x0), np.zeros_like(x0)
    for a in range(31):
        for c in range(3):
            e = np.zeros_like(x0)
            e[a, c] = h
            F[a, c] = -(U(x0 + e) - U(x0 - e)) / (2 * h)
            # d(w.F)/dx_ac = -d/dx_ac (w . grad U): the mixed second difference of U along e_ac and w
            dq[a, c] = -(U(x0 + e + h * w64) - U(x0 + e - h * w64) - U(x0 - e + h * w64) + U(x0 - e - h * w64)) / (4 * h * h)
    assert np.abs(F - ref.F).max() <= 1e-6 * ref.sF.max(), np.abs(F - ref.F).max() / ref.sF.max()
    assert np.abs(dq - ref.dq).max() <= 2e-5 * ref.sdq.max(), np.abs(dq - ref.dq).max() / ref.sdq.max()


@pytest.mark.parametrize("fixture", ["liquid108", "triclinic"])
@pytest.mark.parametrize("form", FORMS)
def test_every_derivative_is_float64_autograd_of_the_torch_module(form, fixture):
    fx = R.liquid(108) if fixture == "liquid108" else R.triclinic()
    term = R.Term(form)
    w = R.direction(108)
    ref = R.evaluate(fx.x, w, fx.cell, [term])
    i, j, off, h = _half_list(fx, term)
    mod = R.module(form).double()
    params = list(mod.parameters())
    x = torch.tensor(fx.x.astype(np.float64), requires_grad=True)
    d = x[i] - x[j] - torch.tensor(off @ h)
    r = d.pow(2).sum(1).sqrt()
    assert float(r.detach().max()) < 2.5
    U = mod(r[:, None]).sum()
    assert abs(float(U) - float(ref.U)) <= 1e-12 * float(ref.sU)
    (g,) = torch.autograd.grad(U, x, create_graph=True)
    wF = (torch.tensor(w.astype(np.float64)) * -g).sum()
    assert np.abs(-g.detach().numpy() - ref.F).max() <= 1e-12 * ref.sF.max()
    grads = torch.autograd.grad(wF, [x] + params, retain_graph=True)
    assert np.abs(grads[0].numpy() - ref.dq).max() <= 1e-12 * ref.sdq.max()
    if params:
        dth = np.array([float(v) for v in grads[1:]])
        dU = np.array([float(v) for v in torch.autograd.grad(U, params)])
        # (the modules' parameter order is the kernels': mdg_params())
        order = [k for p in mod.mdg_params() for k, q in enumerate(params) if q is p]
        assert np.abs(dth[order] - ref.dth[0]).max() <= 1e-12 * ref.sdth[0].max()
        assert np.abs(dU[order] - ref.dU[0]).max() <= 1e-12 * ref.sdU[0].max()
    else:
        assert ref.dth[0].size == 0 and ref.dU[0].size == 0


@pytest.mark.parametrize("sel", [None, "two_species", "excluded_pairs"])
@pytest.mark.parametrize("form", FORMS)
def test_reference_matches_the_oracle_pair_term_in_float64(form, sel):
    fx = R.liquid(107)
    n = 107
    kw = {} if sel is None else R.stack(sel, n)[0][3]
    term = R.Term(form, 2.5, None if sel is None else R.select_mask(n, **kw))
    w = R.direction(n)
    ref = R.evaluate(fx.x, w, fx.cell, [term])
    kind, consts, _ = R.FORMS[form]
    ot = O.PairTerm(ORACLE_KIND[kind], torch.tensor(term.theta, dtype=torch.float64), 2.5,
                    torch.tensor(fx.cell.astype(np.float64)), **kw, **consts)
    q = torch.tensor(fx.x.astype(np.float64))
    ot.reset(q)
    assert len(ot.nbr) == int(np.triu(R.membership(fx.x, fx.cell, [term])[0], 1).sum())
    F, dq, dth = ot.force_vjp(q, torch.tensor(w.astype(np.float64)))
    assert abs(float(ot.energy(q)) - float(ref.U)) <= 1e-12 * float(ref.sU)
    assert np.abs(F.numpy() - ref.F).max() <= 1e-12 * ref.sF.max()
    assert np.abs(dq.numpy() - ref.dq).max() <= 1e-12 * ref.sdq.max()
    if term.n_theta:
        assert np.abs(dth.numpy() - ref.dth[0]).max() <= 1e-12 * ref.sdth[0].max()


def _all_fixtures():
    return ([R.liquid(n) for n in (2, 3, 31, 54, 107, 108, 130, 131, 256, 1000)] +
            [R.liquid(108, 6.4), R.contact(), R.cutoff_pair(), R.unwrapped(), R.triclinic()])


def test_fixtures_carry_no_fragile_pair_but_the_two_placed_ones():
    for fx in _all_fixtures():
        terms = [R.Term("lj", 2.5)] + ([] if fx.name == "cutoff_pair" else [R.Term("lj", 1.8)])
        got = R.fragile_pairs(fx.x, fx.cell, terms).tolist()
        assert got == sorted(map(list, fx.placed)), (fx.name, got)
        # ... so the float32 pair set is the float64 one (placed pairs apart), under every cutoff used
        _, _, d64 = R._images(fx.x, fx.cell, np.dtype(np.float64))
        for t, m in zip(terms, R.membership(fx.x, fx.cell, terms)):
            m64 = (d64 < float(np.float32(t.cutoff)) ** 2) & (d64 > 0)
            diff = np.argwhere(np.triu(m != m64, 1)).tolist()
            assert all(tuple(p) in fx.placed for p in diff), (fx.name, diff)
        assert np.abs(fx.x).min() >= 0.25, fx.name
        inside = fx.x.min() > -0.24 * fx.cell.max() and (fx.x / np.diag(fx.cell) if fx.cell.ndim == 2 else fx.x / fx.cell).max() < 1.24
        assert inside == (fx.name not in ("unwrapped", "triclinic108")), fx.name


def test_cutoff_fixture_places_its_two_pairs_on_the_intended_side():
    fx = R.cutoff_pair()
    (a, b), (c, d) = R.CUTOFF_PAIR_IN, R.CUTOFF_PAIR_OUT
    assert np.float32(fx.x[b, 0] - fx.x[a, 0]) == np.nextafter(np.float32(2.5), np.float32(0))
    assert float(fx.x[b, 0]) - float(fx.x[a, 0]) == float(np.nextafter(np.float32(2.5), np.float32(0)))
    assert np.float32(fx.x[d, 1] - fx.x[c, 1]) == np.float32(2.5)
    m = R.membership(fx.x, fx.cell, [R.Term("lj", 2.5)])[0]
    assert m[a, b] and m[b, a] and m[a].sum() == 1 and m[b].sum() == 1
    assert not m[c].any() and not m[d].any() and not m[:, c].any() and not m[:, d].any()
    ref = R.evaluate(fx.x, R.direction(32), fx.cell, [R.Term("lj", 2.5)])
    assert (ref.sF[[c, d]] == 0).all() and (ref.F[[c, d]] == 0).all() and (ref.dq[[c, d]] == 0).all()
    assert ref.sF[a, 0] > 0 and ref.F[a, 0] == -ref.F[b, 0] and ref.F[a, 0] > 0           # (attractive at 2.5)
    assert R.error(np.zeros((32, 3)), ref, "F") > 0 and R.error(ref.F, ref, "F") == 0
    bad = ref.F.copy()
    bad[c, 1] = 1e-30
    assert R.error(bad, ref, "F") == np.inf                     # (an atom with scale 0 must hold exact zeros)


def test_masks_are_honoured_in_both_orientations():
    fx = R.liquid(108)
    n, w = 108, R.direction(108)
    full = R.evaluate(fx.x, w, fx.cell, [R.Term("lj")])
    m = R.membership(fx.x, fx.cell, [R.Term("lj")])[0]
    a, b = map(int, np.argwhere(np.triu(m, 1))[17])
    one = R.evaluate(fx.x, w, fx.cell, [R.Term("lj", 2.5, R.select_mask(n, ex_pairs=[[a, b]]))])
    only = R.evaluate(fx.x, w, fx.cell, [R.Term("lj", 2.5, ~R.select_mask(n, ex_pairs=[[b, a]]))])
    for q in ("F", "dq"):
        d = getattr(full, q) - getattr(one, q)
        assert np.abs(d[[a, b]]).min() > 0 and np.abs(np.delete(d, [a, b], 0)).max() == 0
        assert np.abs(d - getattr(only, q)).max() <= 1e-12 * np.abs(getattr(full, q)).max()
        assert np.abs(d[a] + d[b]).max() <= 1e-12 * np.abs(d).max() or q == "dq"
    assert abs((full.U - one.U) - only.U) <= 1e-12 * abs(full.U)
    with pytest.raises(AssertionError):
        one_sided = np.ones((n, n), bool)
        one_sided[a, b] = False
        R.Term("lj", 2.5, one_sided)
    # a one-sided mask (no supported input; it lets a GPU test catch a transposed read): atom a loses the pair, atom b keeps it
    half = R.evaluate(fx.x, w, fx.cell, [R.Term("lj", 2.5, one_sided, one_sided=True)])
    assert np.array_equal(half.F[a], one.F[a]) and np.array_equal(half.F[b], full.F[b]) and np.abs(one.F[b] - full.F[b]).max() > 0
    assert np.array_equal(half.dq[a], one.dq[a]) and np.array_equal(half.dq[b], full.dq[b])
    m1 = R.one_sided_mask(n)
    assert (m1 != m1.T).sum() == 2 * len(R.excluded_list(n)) and not m1[0, 1] and m1[1, 0]
    # species selections: A-B pairs only; A-A + B-B + A-B with one form is the unmasked term
    A, B = R.species(n)
    parts = [R.evaluate(fx.x, w, fx.cell, [R.Term("lj", 2.5, R.select_mask(n, index_tuple=s))]) for s in ((A, A), (B, B), (A, B))]
    assert np.abs(sum(p.F for p in parts) - full.F).max() <= 1e-12 * full.sF.max()
    assert np.abs(sum(p.dth[0] for p in parts) - full.dth[0]).max() <= 1e-12 * full.sdth[0].max()


def test_two_cutoffs_select_per_term():
    fx = R.liquid(108)
    terms = R.terms_of(R.stack("two_cutoffs", 108), 108)
    m = R.membership(fx.x, fx.cell, terms)
    _, _, d2 = R._images(fx.x, fx.cell, np.dtype(np.float64))
    assert d2[m[0]].max() > 1.8 ** 2 and d2[m[1]].max() < 1.8 ** 2 and m[1].sum() > 0
    both = R.evaluate(fx.x, R.direction(108), fx.cell, terms)
    sep = [R.evaluate(fx.x, R.direction(108), fx.cell, [t]) for t in terms]
    assert np.abs(both.F - sep[0].F - sep[1].F).max() <= 1e-12 * both.sF.max()
    assert np.allclose(both.dth[1], sep[1].dth[0], rtol=1e-12, atol=0)


def test_a_supercell_of_exact_copies_has_the_tiled_reference():
    """pair_forms_ref.supercell: the dense evaluation of two copies (1 000 atoms) is the 500-atom result tiled -- the same
    pair counts, the same float64 sums to rounding, and the float32 floor of the copies is the original's to summation order"""
    base = R.base500()
    assert (base.x * 2.0 ** 18 == np.rint(base.x * 2.0 ** 18)).all() and np.abs(base.x).min() >= 0.25
    fx = R.supercell((2, 1, 1))
    assert fx.x.shape == (1000, 3) and fx.cell.tolist() == [16.0, 8.0, 8.0] and (fx.x[500:] == fx.x[:500] + [8.0, 0, 0]).all()
    assert R.fragile_pairs(fx.x, fx.cell, [R.Term("lj", 2.5), R.Term("lj", 1.8)]).size == 0
    w = R.direction(500)
    for form in ("lj", "morse_neg", "yukawa"):
        terms = [R.Term(form)]
        ref, fl, member = R.reference(base, terms, w)
        big, flb, mb = R.reference(fx, terms, np.tile(w, (2, 1)))
        assert mb[0].sum(1).tolist() == np.tile(member[0].sum(1), 2).tolist()
        want = R.tile(ref, 2)
        for q in R.QUANTITIES:
            assert R.error(getattr(big, q), want, q) <= 1e-13, (form, q)
            assert R._flat(getattr(big, "s" + q)) == pytest.approx(R._flat(getattr(want, "s" + q)), rel=1e-13)
            assert 0.5 * fl[q] <= flb[q] <= 2.0 * fl[q] or max(fl[q], flb[q]) <= 2.0 ** -23, (form, q, fl[q], flb[q])
    for reps, n in (((2, 2, 3), 6000), ((3, 3, 2), 9000), ((3, 3, 4), 18000)):
        big = R.supercell(reps)
        assert big.x.shape == (n, 3) and big.x.max() < 32.0 and len(np.unique(big.x, axis=0)) == n


def test_print_the_float32_floors():
    """floor per fixture, form and quantity (largest over atoms; at least 2^-24)"""
    print()
    print("%-14s %-10s" % ("fixture", "form") + "".join("%10s" % q for q in R.QUANTITIES))
    for fx in [R.liquid(n) for n in (2, 3, 31, 107, 108, 131, 256, 1000)] + [R.contact(), R.cutoff_pair(), R.unwrapped(),
                                                                            R.base500(),
                                                                            R.triclinic()]:
        for form in FORMS:
            if fx.name == "liquid1000" and form not in ("lj", "morse_neg", "yukawa"):
                continue
            _, fl, _ = R.reference(fx, [R.Term(form)], R.direction(len(fx.x)))
            assert all(2.0 ** -24 <= v < 1e-4 for v in fl.values()), (fx.name, form, fl)
            print("%-14s %-10s" % (fx.name, form) + "".join("%10.2e" % fl[q] for q in R.QUANTITIES))
