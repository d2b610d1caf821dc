"""The neighbour-list builders of csrc/nbr.hip (K1: nbr_dense_kernel, the cell list, the half list) against the plain
references of tests/nbr_ref.py -- float64 with the reference's one-image rule (decided pairs exactly, undecided pairs either
way) and, for orthorhombic cells, the bit-exact float32 emulation of the pair test (ties included) -- at the shapes where a
compaction, rank-sort or stencil kernel goes wrong.  The inputs (nbr_ref.cases(), pinned on the CPU by
tests/test_nbr_ref_host.py):

  A  orthorhombic, non-cubic (7.3, 8.1, 9.4), 200 atoms, atoms one cell outside, coordinates at -1e-9 and at L
  B  triclinic, 150 atoms (dense builder, float64 reference)
  C  box of 4.0 < 2 cutoffs: one image only, rows up to N - 1 long; placed pairs at s = 0.5, d = rc, d^2 one float below
     rc^2, coincident atoms
  D  1, 2, 63, 64, 65, 129 atoms (wave tails of the ordered compaction); three groups of 65 with a [65, 65] mask from
     index_tuple / ex_pairs, both builders
  E  cell-list geometry: bin grids (3,3,3), (4,4,4), (3,4,5) with about 600 atoms, a dilute 5 x 5 x 5 grid with 40 atoms, a
     droplet that puts more than 100 candidates into one stencil range; the cell list also against the dense list
  F  the bin-edge constructions of tests/golden/nbr_bin_edge.npz: boxes of a whole number of cutoffs per side with a pair at
     the cutoff two bins apart.  The cell list with floor(L / cutoff) bins misses these pairs (each F case failed with
     "2 missing: (0,1), (1,0)" on the builder before make_bins asked for a margin; the dense builder lists them)
  G  overflow protocol of the C entry points and of build_ell's fixed-capacity mode
  H  half list, edge_id map, fixed-capacity half list above and below the pair count
  I  on every list: j in row i <=> i in row j, the two codes add up to 26, rows strictly ascending (nbr_ref.as_full)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import nbr_ref as R
from test_gpu_parity import T, DEV

pytestmark = pytest.mark.gpu

_BUILT = {}


def _mask(case):
    from mdgrad_amd import ops
    return ops.build_mask(case.group or len(case.pos), index_tuple=case.index_tuple, ex_pairs=case.ex_pairs, device=DEV)


def _build(name, method):
    """(EllList, its list as nbr_ref.Full) of one case through ops.build_ell, built once per (case, builder)."""
    if (name, method) not in _BUILT:
        from mdgrad_amd import ops, _lib
        c = R.cases()[name]
        ell = ops.build_ell(T(c.pos, DEV), _lib.make_cell(c.cell), c.cutoff, mask=_mask(c), method=method, group=c.group)
        torch.cuda.synchronize()
        _BUILT[(name, method)] = (ell, R.as_full(ell.cnt.cpu().numpy(), ell.col.cpu().numpy(), ell.shift.cpu().numpy()))
    return _BUILT[(name, method)]


PAIRS = [(n, m) for n, c in R.cases().items() for m in c.methods]


@pytest.mark.parametrize("name,method", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_builder_against_the_references(name, method):
    c = R.cases()[name]
    ell, got = _build(name, method)                       # (as_full: rows strictly ascending, indices and codes in range)
    assert ell.n_atoms == len(c.pos) and ell.max_nbr >= int(ell.cnt.max())
    assert R.invariants(got) == []
    assert R.compare64(c.ref64(), got) == []
    if c.diag:
        assert R.compare_exact(c.ref32(), got) == []
        assert np.array_equal(ell.cnt.cpu().numpy(), c.ref32().keep.sum(1))
    if method == "cell":
        assert R.compare_exact(_build(name, "dense")[1], got) == []


def test_case_c_placed_pairs_on_the_device():
    _, got = _build("C box under two cutoffs", "dense")
    assert got.keep[0, 1] and got.code[0, 1] == 13 and got.keep[1, 0] and got.code[1, 0] == 13       # s = 0.5: no shift
    assert got.keep[2, 3] and got.code[2, 3] == 12 and got.code[3, 2] == 14                          # one image: d = 1.5
    assert not got.keep[4, 5] and not got.keep[5, 4]                                                   # d = rc exactly
    assert got.keep[6, 7] and got.keep[7, 6]                                                           # d^2 one float below rc^2
    assert not got.keep[8, 9] and not got.keep[9, 8]                                                   # coincident
    assert got.keep.sum(1).max() >= 25


def test_no_pair_crosses_a_group():
    for name in ("D groups index_tuple", "D groups ex_pairs"):
        for method in ("dense", "cell"):
            _, got = _build(name, method)
            i, j = np.nonzero(got.keep)
            assert len(i) and (i // 65 == j // 65).all()


# ----------------------------------------------------------------------------------------------- G: overflow protocol
SENTINEL = -7


def _raw_build(c, method, max_nbr):
    from mdgrad_amd import _lib
    from mdgrad_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    n, g = len(c.pos), c.group or len(c.pos)
    cs = _lib.make_cell(c.cell)
    x = T(c.pos, DEV)
    col = torch.full((n, max_nbr), SENTINEL, dtype=torch.int32, device=DEV)
    shift = torch.full((n, max_nbr), SENTINEL, dtype=torch.int32, device=DEV)
    cnt = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    overflow = torch.zeros(1, dtype=torch.int32, device=DEV)
    mask = _mask(c)
    st = stream_ptr(x.device)
    if method == "cell":
        ns = int(lib.mdg_nbr_cell_scratch_groups(n, g, C.byref(cs), c.cutoff))
        assert ns > 0
        scratch = torch.empty(ns, dtype=torch.int32, device=DEV)
        check(lib.mdg_nbr_build_cell_groups(ptr(x), n, g, C.byref(cs), c.cutoff, ptr(mask), ptr(col), ptr(shift), ptr(cnt),
                                            max_nbr, ptr(overflow), ptr(scratch), st), "mdg_nbr_build_cell_groups")
    else:
        check(lib.mdg_nbr_build_dense_groups(ptr(x), n, g, C.byref(cs), c.cutoff, ptr(mask), ptr(col), ptr(shift), ptr(cnt),
                                             max_nbr, ptr(overflow), st), "mdg_nbr_build_dense_groups")
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), col.cpu().numpy(), shift.cpu().numpy(), int(overflow.item())


G_CASES = [("E bins 345", "dense"), ("E bins 345", "cell"), ("E droplet", "cell"), ("D 129 atoms", "dense"),
           ("D groups ex_pairs", "cell")]


@pytest.mark.parametrize("name,method", G_CASES, ids=["%s-%s" % p for p in G_CASES])
def test_overflow_clamps_rows_and_reports_the_longest(name, method):
    c = R.cases()[name]
    ref_cnt, rows = R.rows_of(c.ref32())
    longest = int(ref_cnt.max())
    max_nbr = max(1, min(int(np.median(ref_cnt)), longest // 2))
    assert max_nbr < longest
    cnt, col, shift, overflow = _raw_build(c, method, max_nbr)
    assert np.array_equal(cnt, np.minimum(ref_cnt, max_nbr))
    assert overflow == longest
    for i, (j, code) in enumerate(rows):
        assert np.array_equal(col[i, :cnt[i]], j[:max_nbr]) and np.array_equal(shift[i, :cnt[i]], code[:max_nbr]), i
        assert (col[i, cnt[i]:] == SENTINEL).all() and (shift[i, cnt[i]:] == SENTINEL).all(), "row %d written past its count" % i
    # a capacity that fits: the overflow word stays untouched
    cnt, col, shift, overflow = _raw_build(c, method, longest)
    assert overflow == 0 and np.array_equal(cnt, ref_cnt)


@pytest.mark.parametrize("method", ["dense", "cell"])
def test_fixed_capacity_mode_leaves_the_longest_row_in_need(method):
    from mdgrad_amd import ops, _lib
    c = R.cases()["E bins 444"]
    ref_cnt = c.ref32().keep.sum(1)
    need = torch.zeros(2, dtype=torch.int32, device=DEV)
    cap = int(ref_cnt.max()) - 9
    ell = ops.build_ell(T(c.pos, DEV), _lib.make_cell(c.cell), c.cutoff, method=method, max_nbr=cap, need=need)
    assert ell.max_nbr == cap and need.cpu().tolist() == [int(ref_cnt.max()), 0]
    assert np.array_equal(ell.cnt.cpu().numpy(), np.minimum(ref_cnt, cap))
    need.zero_()
    ell = ops.build_ell(T(c.pos, DEV), _lib.make_cell(c.cell), c.cutoff, method=method, max_nbr=int(ref_cnt.max()), need=need)
    assert need.cpu().tolist() == [0, 0] and np.array_equal(ell.cnt.cpu().numpy(), ref_cnt)


# ----------------------------------------------------------------------------------------------- H: half list
H_CASES = [("E bins 345", "cell"), ("C box under two cutoffs", "dense"), ("D 65 atoms", "dense"), ("D groups index_tuple", "dense")]


def _check_edge_id(ell, nbr, eid, capacity=None):
    cnt, col = ell.cnt.cpu().numpy(), ell.col.cpu().numpy()
    nbr, eid = nbr.cpu().numpy(), eid.cpu().numpy()
    filled = np.arange(col.shape[1])[None, :] < cnt[:, None]
    i = np.broadcast_to(np.arange(len(cnt))[:, None], col.shape)[filled]
    j, e = col[filled], eid[filled]
    assert (e >= 0).all() and (e < (len(nbr) if capacity is None else capacity)).all()
    if capacity is None:
        lo, hi = np.minimum(i, j), np.maximum(i, j)
        assert np.array_equal(nbr[e, 0], lo) and np.array_equal(nbr[e, 1], hi)
        assert np.array_equal(np.sort(np.bincount(e, minlength=len(nbr))), np.full(len(nbr), 2))      # both slots of a pair


@pytest.mark.parametrize("name,method", H_CASES, ids=["%s-%s" % p for p in H_CASES])
def test_half_list_and_edge_ids(name, method):
    c = R.cases()[name]
    ell, got = _build(name, method)
    want_nbr, want_off = R.half_list(c.ref32())
    assert R.compare_exact(c.ref32(), got) == []
    P = len(want_nbr)
    nbr, off, eid = ell.half_list(with_edge_id=True)
    assert nbr.dtype == torch.int64 and off.dtype == torch.float32 and eid.dtype == torch.int32
    assert np.array_equal(nbr.cpu().numpy(), want_nbr)
    assert np.array_equal(off.cpu().numpy(), want_off)                       # the codes of the (i, j > i) slots
    _check_edge_id(ell, nbr, eid)
    # fixed capacity above the pair count
    pad = 1.0e4
    need = torch.zeros(2, dtype=torch.int32, device=DEV)
    cap = P + 37
    nbr, off, eid, n_valid = ell.half_list_padded(cap, pad, need)
    torch.cuda.synchronize()
    assert int(n_valid) == P and need.cpu().tolist() == [0, 0]
    assert np.array_equal(nbr[:P].cpu().numpy(), want_nbr) and np.array_equal(off[:P].cpu().numpy(), want_off)
    assert (nbr[P:] == -1).all()
    assert np.array_equal(off[P:].cpu().numpy(), np.tile(np.array([pad, 0, 0], np.float32), (37, 1)))
    _check_edge_id(ell, nbr[:P], eid)
    # ... and below it
    cap = P - min(100, P // 2)
    nbr, off, eid, n_valid = ell.half_list_padded(cap, pad, need)
    torch.cuda.synchronize()
    assert int(n_valid) == cap and need.cpu().tolist() == [0, P]
    assert np.array_equal(nbr.cpu().numpy(), want_nbr[:cap]) and np.array_equal(off.cpu().numpy(), want_off[:cap])
    _check_edge_id(ell, nbr, eid, capacity=cap)
