"""The neighbour-list references of tests/nbr_ref.py, pinned on the CPU before they judge a kernel (tests/test_gpu_nbr_ref.py),
and the cell list's bin arithmetic (csrc/nbr.hip make_bins / bin_coord) ported to numpy:

  * full_list32_diag (the float32 emulation of pair_test<true>) agrees with full_list64 on every decided pair of every
    orthorhombic input of the GPU tests, codes included;
  * every random input has at most UNDECIDED_CAP = 5 undecided ordered pairs besides the ties its case places on purpose
    (the seeds in nbr_ref.py were chosen for that; the placed ties are checked to be undecided, i.e. really on a boundary);
  * the placed pairs of case C come out of both references as its docstring says;
  * with floor(L / cutoff) bins the 27-bin stencil misses pairs the float32 pair test accepts -- the construction first
    reported (rc 1.6618019, L 6.6472077, bins 3 and 1 of 4) and the family around it, binned with make_cell's inverse, with
    and without the fused multiply-add the device code compiles bin_coord to -- and with the margin of make_bins it misses
    none of them, nor any pair of the other inputs;
  * the library's bin count (mdg_nbr_cell_bins) is the port's, ops._use_cell_list follows it, and the boxes of the timed
    configurations keep the bin counts they had.
"""
import ctypes

import numpy as np
import pytest

import nbr_ref as R
from conftest import load_golden


def _names(diag_only=False):
    return [n for n, c in R.cases().items() if c.diag or not diag_only]


@pytest.mark.parametrize("name", _names(diag_only=True))
def test_float32_emulation_agrees_with_float64_on_every_decided_pair(name):
    c = R.cases()[name]
    r64, r32 = c.ref64(), c.ref32()
    assert R.compare64(r64, r32) == []
    assert R.invariants(r32) == [] and R.invariants(R.Full(r64.keep, r64.code, None, None, 0.0)) == []


@pytest.mark.parametrize("name", R.RANDOM)
def test_undecided_pairs_of_the_random_inputs_are_capped(name):
    c = R.cases()[name]
    und = c.undecided_outside_ties()
    print("%s: %d undecided ordered pairs outside the placed ties, delta %.3g" % (name, len(und), c.ref64().delta))
    assert len(und) <= R.UNDECIDED_CAP, und
    for i, j in c.ties:
        assert c.ref64().und[i, j] and c.ref64().und[j, i], "placed tie (%d, %d) is not on a decision boundary" % (i, j)
    assert c.ref64().keep.sum() > 0 or len(c.pos) < 3


def test_triclinic_reference_against_a_search_over_125_images():
    """Case B: every pair of the one-image rule is a pair of the true minimum image (searched over 5 x 5 x 5 images), and in
    this cell -- every height above two cutoffs -- the two agree; the float64 list obeys the symmetry rules."""
    c = R.cases()["B triclinic"]
    r = c.ref64()
    x, h = c.pos.astype(np.float64), c.cell.astype(np.float64)
    D = x[None] - x[:, None]
    best = np.full(D.shape[:2], np.inf)
    for ox in (-2, -1, 0, 1, 2):
        for oy in (-2, -1, 0, 1, 2):
            for oz in (-2, -1, 0, 1, 2):
                v = D + np.array([ox, oy, oz], np.float64) @ h
                best = np.minimum(best, np.where((v * v).sum(-1) > 0, (v * v).sum(-1), np.inf))
    true_min = (best < 2.5 ** 2) & ~np.eye(len(x), dtype=bool)
    assert np.array_equal(true_min, r.keep)
    assert r.keep.sum() > 1000 and len(np.unique(r.code[r.keep])) >= 15, "the case must use many image codes"
    assert R.invariants(R.Full(r.keep, r.code, None, None, 0.0)) == []


def test_case_c_placed_pairs():
    c = R.cases()["C box under two cutoffs"]
    for r in (c.ref32(), R.Full(c.ref64().keep, c.ref64().code, None, None, 0.0)):
        assert r.keep[0, 1] and r.keep[1, 0] and r.code[0, 1] == 13 and r.code[1, 0] == 13      # s = 0.5: no shift
        assert r.keep[2, 3] and r.code[2, 3] == 12 and r.code[3, 2] == 14                       # the image at d = 1.5
        assert not r.keep[4, 5] and not r.keep[5, 4]                                              # d = rc exactly
        assert not r.keep[8, 9] and not r.keep[9, 8]                                              # coincident
    assert c.ref32().keep[6, 7] and c.ref32().keep[7, 6] and c.ref32().code[6, 7] == 13           # d^2 one float below rc^2
    assert c.ref32().keep.sum(1).max() >= 25                                                      # rows nearly N - 1 long


def test_half_list_is_the_upper_triangle_in_row_order():
    c = R.cases()["D 65 atoms"]
    nbr, off = R.half_list(c.ref32())
    assert (nbr[:, 0] < nbr[:, 1]).all() and len(nbr) * 2 == c.ref32().keep.sum()
    key = nbr[:, 0] * len(c.pos) + nbr[:, 1]
    assert (np.diff(key) > 0).all()
    assert np.array_equal(R.code_of(off), c.ref32().code[nbr[:, 0], nbr[:, 1]])
    assert off.dtype == np.float32 and set(np.unique(off)) <= {-1.0, 0.0, 1.0}


# ----------------------------------------------------------------------------------------------- the bins of the cell list
def test_reported_construction_is_missed_with_bins_of_exactly_the_cutoff():
    f32 = np.float32
    rc, L = f32(1.6618019), f32(6.6472077)
    pos = np.array([[4.9854054, 1, 1], [3.3236036, 1, 1]], f32)
    Ls = np.full(3, L, f32)
    inv = R.cell_inv(Ls)
    assert inv[0] == f32(1) / L, "make_cell's inverse of a diagonal cell is the rounded reciprocal"
    full = R.full_list32_diag(pos, Ls, rc, inv)
    assert full.keep[0, 1] and full.keep[1, 0]
    assert list(R.make_bins(Ls, rc, guarded=False)) == [4, 4, 4]
    for coord in (R.bin_coord, R.bin_coord_plain):
        assert list(coord(pos[:, 0], inv[0], 4)) == [3, 1]
        assert len(R.stencil_misses(full, pos, Ls, inv, [4, 4, 4], coord)[0]) == 2
    nb = R.make_bins(Ls, rc)
    assert list(nb) == [3, 3, 3]
    assert len(R.stencil_misses(full, pos, Ls, inv, nb)[0]) == 0


def test_search_finds_the_family_and_the_margin_removes_it():
    """1 000 boxes of the family (seed 11; the fixture came from seed 7): some are missed with floor(L / rc) bins -- a
    prediction for the GPU, confirmed by tests/test_gpu_nbr_ref.py case F on the unguarded builder -- none with the margin."""
    found = R.search_bin_edge(1000, 11)
    boxes = {(float(r[0]), float(r[1])) for r in found}
    print("%d constructions in %d of 1000 boxes" % (len(found), len(boxes)))
    assert len(found) >= 5
    for rc, L, n, k, xa, xb in found:
        Ls = np.full(3, L, np.float32)
        pos = np.array([[xa, 1, 1], [xb, 1, 1]], np.float32)
        inv = R.cell_inv(Ls)
        full = R.full_list32_diag(pos, Ls, rc, inv)
        nb = R.make_bins(Ls, rc)
        assert nb[0] == n - 1
        for coord in (R.bin_coord, R.bin_coord_plain):
            assert len(R.stencil_misses(full, pos, Ls, inv, nb, coord)[0]) == 0


@pytest.mark.parametrize("n", [3, 4, 8, 16, 40])
def test_margin_holds_at_the_narrowest_bins_the_builder_takes(n):
    """The tightest boxes make_bins still gives n bins: L the first float32 with floor(L / (rc + 2^-18 L)) = n, bins wider than
    the cutoff by just the margin.  Atoms within 5 ulps of every pair of bin edges one bin apart, inside the box and one cell
    outside it (where the binning error is largest): whatever lands two bins apart, the float32 pair test rejects."""
    f32 = np.float32
    rng = np.random.default_rng(100 + n)
    checked = 0
    for _ in range(40):
        rc = f32(rng.uniform(1.0, 3.0))
        L = f32(float(rc) * n * (1.0 + n * R.BIN_MARGIN))
        while int(R.make_bins([L], rc)[0]) < n:
            L = np.nextafter(L, f32(np.inf))
        assert int(R.make_bins([np.nextafter(L, f32(0))], rc)[0]) == n - 1
        inv = R.cell_inv(np.full(3, L, f32))[0]
        for k in range(1, n + 1):
            xb = R._around(f32(np.float64(L) * (k - 1) / n))                # around the lower edge of bin k - 1 ... its upper edge
            xb = np.concatenate([xb, R._around(f32(np.float64(L) * k / n))])
            xa = R._around(f32(np.float64(L) * (k + 1) / n))                # around the lower edge of bin k + 1
            xa, xb = np.concatenate([xa, xa + L, xa - L]), np.concatenate([xb, xb + L, xb - L])
            d = xa[:, None] - xb[None, :]
            o = -np.clip(np.rint(d * inv), f32(-1), f32(1))
            dm = (o.astype(np.float64) * np.float64(L) + d.astype(np.float64)).astype(f32)
            d2 = dm * dm
            accepted = (d2 < f32(rc * rc)) & (d2 != 0)
            for coord in (R.bin_coord, R.bin_coord_plain):
                diff = np.abs(coord(xa, inv, n)[:, None] - coord(xb, inv, n)[None, :])
                apart = np.minimum(diff, n - diff) > 1
                assert not (apart & accepted).any(), (float(rc), float(L), k)
                checked += int(apart.sum())
    assert checked > 1000 or n == 3


def test_fixture_constructions_are_missed_without_the_margin_only():
    g = load_golden("nbr_bin_edge")
    assert g["pos"].dtype == np.float32 and g["lengths"].dtype == np.float32 and g["cutoff"].dtype == np.float32
    assert len(g["cutoff"]) >= 6 and set(g["axis"].tolist()) == {0, 1, 2}
    for name, c in R.cases().items():
        if not name.startswith("F "):
            continue
        inv = R.cell_inv(c.cell)
        old, new = R.make_bins(c.cell, c.cutoff, guarded=False), R.make_bins(c.cell, c.cutoff)
        assert (old >= 3).all() and (new >= 3).all(), "both bin counts must leave the cell list applicable"
        for coord in (R.bin_coord, R.bin_coord_plain):
            ii, jj = R.stencil_misses(c.ref32(), c.pos, c.cell, inv, old, coord)
            assert sorted(zip(ii.tolist(), jj.tolist())) == [(0, 1), (1, 0)]
            assert len(R.stencil_misses(c.ref32(), c.pos, c.cell, inv, new, coord)[0]) == 0


@pytest.mark.parametrize("name", [n for n, c in R.cases().items() if "cell" in c.methods and not n.startswith("F ")])
def test_stencil_holds_every_pair_of_the_cell_list_inputs(name):
    c = R.cases()[name]
    inv = R.cell_inv(c.cell)
    nb = R.make_bins(c.cell, c.cutoff)
    assert (nb >= 3).all()
    for coord in (R.bin_coord, R.bin_coord_plain):
        assert len(R.stencil_misses(c.ref32(), c.pos, c.cell, inv, nb, coord)[0]) == 0


def test_case_e_bin_grids():
    want = {"E bins 333": [3, 3, 3], "E bins 444": [4, 4, 4], "E bins 345": [3, 4, 5], "E dilute": [5, 5, 5], "E droplet": [4, 4, 4],
            "D groups index_tuple": [3, 3, 3], "D groups ex_pairs": [3, 3, 3]}
    for name, nb in want.items():
        c = R.cases()[name]
        assert list(R.make_bins(c.cell, c.cutoff)) == nb, name
    # the droplet: more than 64 candidates in one stencil range (three consecutive z-bins of one column)
    c = R.cases()["E droplet"]
    inv = R.cell_inv(c.cell)
    b = np.stack([R.bin_coord(c.pos[:, k], inv[k], 4) for k in range(3)], 1)
    col, cnt = np.unique(b[:, 0] * 4 + b[:, 1], return_counts=True)
    assert cnt.max() > 64 + 40
    # the dilute box: most bins empty
    c = R.cases()["E dilute"]
    inv = R.cell_inv(c.cell)
    b = np.stack([R.bin_coord(c.pos[:, k], inv[k], 5) for k in range(3)], 1)
    assert len(np.unique((b[:, 0] * 5 + b[:, 1]) * 5 + b[:, 2])) < 125 // 2


def _lib_bins(lengths, cutoff):
    from mdgrad_amd import _lib
    lib = _lib.load()
    cs = _lib.make_cell(np.asarray(lengths, np.float32))
    nb = (ctypes.c_int32 * 3)()
    ok = lib.mdg_nbr_cell_bins(ctypes.byref(cs), float(cutoff), nb)
    return list(nb), ok, cs


def test_library_bin_count_is_the_port_and_use_cell_list_follows_it():
    from mdgrad_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(5)
    boxes = [(rng.uniform(2.0, 40.0, 3), rng.uniform(0.8, 6.0)) for _ in range(200)]
    boxes += [(np.full(3, np.float32(rc) * np.float32(n)), rc) for rc in (2.5, 1.1, 6.0, 2.75) for n in (1, 2, 3, 4, 7, 16)]
    boxes += [(c.cell, c.cutoff) for c in R.cases().values() if c.diag]
    for Ls, rc in boxes:
        nb, ok, cs = _lib_bins(Ls, rc)
        assert nb == list(R.make_bins(Ls, rc)), (Ls, rc)
        assert ok == int(min(nb) >= 3)
        assert ops._use_cell_list(512, cs, rc) == bool(ok) and not ops._use_cell_list(511, cs, rc)
        ncell = nb[0] * nb[1] * nb[2]
        assert lib.mdg_nbr_cell_scratch_groups(130, 65, ctypes.byref(cs), float(rc)) == 2 * 130 + 3 * (ncell * 2 + 1) + 8
    # exactly three cutoffs per side: two guarded bins, the dense builder takes over
    nb, ok, cs = _lib_bins(np.full(3, 7.5, np.float32), 2.5)
    assert nb == [2, 2, 2] and ok == 0 and not ops._use_cell_list(4096, cs, 2.5)
    tri = _lib.make_cell(np.array([[9.0, 0, 0], [1.0, 9.0, 0], [0, 0, 9.0]], np.float32))
    assert lib.mdg_nbr_cell_bins(ctypes.byref(tri), 2.5, None) == 0


def test_timed_configurations_keep_their_bin_counts():
    """The boxes bench.py builds its cell-list workloads in (LJ liquids at rho 0.845 with cutoff 2.5, coarse-grained water
    on a diamond lattice with cutoff 6; also with the skins of the stored lists, 0.02 and 0.12 of the cutoff): none is within the margin of a whole
    number of cutoffs, so the margin changes no bin count there."""
    from mdgrad_amd import units
    boxes = []
    for n_side in (8, 10, 16):
        L = (n_side ** 3 / 0.845) ** (1 / 3)
        boxes += [(L, rc) for rc in (2.5, 2.5 * 1.02, 2.5 * 1.12, 2.6, 2.62, 3.0)]
    a = units.get_unit_len(0.997, 18.01528, 8)
    for size in (2, 4, 8):
        boxes += [(a * size, rc) for rc in (5.0, 5.0 * 1.02, 6.0, 6.0 * 1.02, 6.0 * 1.12, 6.5)]
    for L, rc in boxes:
        Ls = np.full(3, L, np.float32)
        assert list(R.make_bins(Ls, rc)) == list(R.make_bins(Ls, rc, guarded=False)), (L, rc)
