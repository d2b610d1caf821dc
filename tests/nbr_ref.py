"""Plain references of the neighbour-list builders (csrc/nbr.hip, K1) in numpy, CPU only, from exactly what a builder
receives: float32 positions [N, 3], the cell (three float32 lengths or a 3x3 float32 matrix), the float32 cutoff, an optional
group size (pairs stay inside groups of consecutive atoms) and an optional [group, group] selection mask.

    full_list64       float64 throughout, the reference's ONE-IMAGE rule (torchmd/topology.py:59-64, not the true minimum
                      image): D = x_j - x_i, s = D . inv, o = -[s > .5] + [s < -.5] per component, D += o . h, kept iff
                      0 < d^2 < rc^2.  Image code (ox+1) + 3 (oy+1) + 9 (oz+1) as in include/mdgrad_hip.h K1.  The kernels do
                      this arithmetic in float32, so the float64 verdict binds them only away from its decision boundaries:
                      a pair is UNDECIDED when |d - rc| <= delta, delta = 2^-21 (max |coordinate| + longest cell edge) --
                      one rounding of each coordinate difference, one of the image add and three of the square sum, each
                      2^-24 of its operands, with a factor of about two in hand -- or when some |s_k| lies within 2^-21 of
                      0.5 or 1.5 (the image of that component may then flip).
    full_list32_diag  bit-exact emulation of pair_test<true> (orthorhombic cells) in numpy float32: d = fl(x_j - x_i),
                      s = fl(d inv), o = -clip(rint(s), -1, 1), d = fma(o, h, d) (the float64 sum rounded once: exact,
                      o is -1, 0 or 1), d^2 = fl(fl(fl(dx^2) + fl(dy^2)) + fl(dz^2)) < fl(rc rc).  No undecided set: the
                      orthorhombic builders must equal it, ties included.  inv comes from _lib.make_cell (cell_inv).
    half_list         the reference's lexicographic i < j half list with float offsets (topology.py:68-73).

    compare_exact / compare64    a builder's (cnt, col, shift) against the two references; invariants() the symmetry rules.
    make_bins / bin_coord / cell_bins   numpy port of the cell list's binning, as compiled (see bin_coord).
    CASES             the inputs of tests/test_gpu_nbr_ref.py; tests/test_nbr_ref_host.py pins the references on them.
"""
import collections
import os

import numpy as np

S_EPS = 2.0 ** -21
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# keep [N, N] bool, code [N, N] int8 (valid where keep); und [N, N] bool and ok_code [N, N, 27] bool (the codes an
# undecided pair may carry when listed) for full_list64 only, None otherwise.
Full = collections.namedtuple("Full", "keep code und ok_code delta")


def _matrix(cell, dt):
    h = np.asarray(cell, np.float32).astype(dt)
    return np.diag(h) if h.ndim == 1 else h


def _selection(n_atoms, group, mask):
    """bool [N, N]: i != j, same group, and selected by the [group, group] mask."""
    g = n_atoms if group is None else int(group)
    assert n_atoms % g == 0
    gid = np.arange(n_atoms) // g
    sel = (gid[:, None] == gid[None, :]) & ~np.eye(n_atoms, dtype=bool)
    if mask is not None:
        m = np.asarray(mask).astype(bool)
        assert m.shape == (g, g)
        sel &= np.tile(m, (n_atoms // g, n_atoms // g))
    return sel


def code_of(o):
    o = np.asarray(o).astype(np.int64)
    return ((o[..., 0] + 1) + 3 * (o[..., 1] + 1) + 9 * (o[..., 2] + 1)).astype(np.int8)


def offsets_of(code):
    c = np.asarray(code).astype(np.int64)
    return np.stack([c % 3 - 1, (c // 3) % 3 - 1, c // 9 - 1], -1)


def full_list64(pos, cell3x3, cutoff, group=None, mask=None):
    x = np.asarray(pos)
    assert x.dtype == np.float32, "the positions are the float32 values a builder receives"
    x = x.astype(np.float64)
    n = x.shape[0]
    h = _matrix(cell3x3, np.float64)
    inv = np.linalg.inv(h)
    rc = float(np.float32(cutoff))
    sel = _selection(n, group, mask)
    D = x[None, :, :] - x[:, None, :]                                  # D[i, j] = x_j - x_i
    s = D @ inv
    o = (s < -0.5).astype(np.float64) - (s > 0.5).astype(np.float64)
    Dm = D + o @ h
    d2 = (Dm * Dm).sum(-1)
    keep = sel & (d2 < rc * rc) & (d2 > 0)
    code = code_of(o)
    delta = S_EPS * (float(np.abs(x).max()) + float(np.sqrt((h * h).sum(1)).max()))
    a = np.abs(s)
    near = (np.abs(a - 0.5) <= S_EPS) | (np.abs(a - 1.5) <= S_EPS)      # [N, N, 3]
    und = sel & (d2 > 0) & ((np.abs(np.sqrt(d2) - rc) <= delta) | near.any(-1))
    # codes a listed undecided pair may carry: every component either the float64 choice or, where |s_k| is near 0.5 or
    # 1.5, the other candidate; and the float64 distance under that image within delta of being inside the cutoff
    ok_code = np.zeros((n, n, 27), bool)
    for i, j in zip(*np.nonzero(und)):
        cands = []
        for k in range(3):
            c = {int(o[i, j, k])}
            if near[i, j, k]:
                sg = 1 if s[i, j, k] > 0 else -1
                c |= ({0, -sg} if a[i, j, k] < 1.0 else {-sg, -2 * sg})
            cands.append(sorted(c))
        for ox in cands[0]:
            for oy in cands[1]:
                for oz in cands[2]:
                    if max(abs(ox), abs(oy), abs(oz)) > 1:
                        continue                                        # (no code for it: the clamp keeps |o| <= 1)
                    v = D[i, j] + np.array([ox, oy, oz], np.float64) @ h
                    dd = float(np.sqrt((v * v).sum()))
                    if 0 < dd < rc + delta:
                        ok_code[i, j, int(code_of([ox, oy, oz]))] = True
    return Full(keep, code, und, ok_code, delta)


def cell_inv(lengths):
    """The three float32 reciprocals a builder receives: the diagonal of _lib.make_cell's inverse (torch, float32, CPU)."""
    from mdgrad_amd import _lib
    cs = _lib.make_cell(np.asarray(lengths, np.float32))
    assert cs.diag
    return np.array([cs.inv[0], cs.inv[4], cs.inv[8]], np.float32)


def full_list32_diag(pos, lengths, cutoff, inv=None, group=None, mask=None):
    x = np.asarray(pos)
    assert x.dtype == np.float32
    n = x.shape[0]
    h = np.asarray(lengths, np.float32)
    assert h.shape == (3,)
    inv = cell_inv(h) if inv is None else np.asarray(inv, np.float32)
    rc = np.float32(cutoff)
    rc2 = np.float32(rc * rc)
    d = x[None, :, :] - x[:, None, :]                                   # float32, one rounding
    s = d * inv[None, None, :]                                          # float32, one rounding
    o = -np.clip(np.rint(s), np.float32(-1), np.float32(1))
    dm = (o.astype(np.float64) * h.astype(np.float64) + d.astype(np.float64)).astype(np.float32)      # fmaf(o, h, d)
    sq = dm * dm
    d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    assert d2.dtype == np.float32
    keep = _selection(n, group, mask) & (d2 < rc2) & (d2 != 0)
    return Full(keep, code_of(o), None, None, 0.0)


def rows_of(full):
    """(cnt [N], list of (j ascending, code) per row)."""
    rows = []
    for i in range(full.keep.shape[0]):
        j = np.nonzero(full.keep[i])[0]
        rows.append((j, full.code[i, j]))
    return full.keep.sum(1), rows


def half_list(full):
    """(nbr int64 [P, 2], offsets float32 [P, 3]): the pairs i < j of the full list in lexicographic order."""
    i, j = np.nonzero(np.triu(full.keep, 1))
    return np.stack([i, j], 1).astype(np.int64), offsets_of(full.code[i, j]).astype(np.float32)


# ----------------------------------------------------------------------------------------------- judging a builder
def as_full(cnt, col, shift):
    """A builder's output as matrices; raises AssertionError for rows that are not strictly ascending, indices out of
    range or codes outside 0..26.  Only the first cnt[i] entries of a row are read."""
    cnt, col, shift = (np.asarray(a) for a in (cnt, col, shift))
    n = cnt.shape[0]
    assert (cnt >= 0).all() and (cnt <= col.shape[1]).all(), "cnt outside [0, max_nbr]"
    keep = np.zeros((n, n), bool)
    code = np.zeros((n, n), np.int8)
    for i in range(n):
        j, c = col[i, :cnt[i]].astype(np.int64), shift[i, :cnt[i]]
        assert ((j >= 0) & (j < n)).all(), "row %d: neighbour index out of range" % i
        assert (np.diff(j) > 0).all(), "row %d is not strictly ascending: %s" % (i, j)
        assert ((c >= 0) & (c < 27)).all(), "row %d: image code out of range" % i
        keep[i, j] = True
        code[i, j] = c
    return Full(keep, code, None, None, 0.0)


def _fmt(kind, ii, jj, limit=6):
    return "%d %s: %s" % (len(ii), kind, ", ".join("(%d,%d)" % p for p in list(zip(ii, jj))[:limit]))


def compare_exact(ref, got):
    """Differences of two full lists (pairs and codes) as a list of strings; empty when they are equal."""
    out = []
    miss, extra = np.nonzero(ref.keep & ~got.keep), np.nonzero(got.keep & ~ref.keep)
    both = ref.keep & got.keep
    wrong = np.nonzero(both & (ref.code != got.code))
    for kind, (ii, jj) in (("missing", miss), ("extra", extra), ("with another image code", wrong)):
        if len(ii):
            out.append(_fmt(kind, ii, jj))
    return out


def compare64(ref, got):
    """A builder's list against full_list64: decided pairs present or absent exactly with the exact code; undecided pairs
    either way, a listed one with a code of ref.ok_code."""
    dec = ~ref.und
    out = compare_exact(Full(ref.keep & dec, ref.code, None, None, 0.0), Full(got.keep & dec, got.code, None, None, 0.0))
    ii, jj = np.nonzero(got.keep & ref.und)
    bad = ~ref.ok_code[ii, jj, got.code[ii, jj].astype(np.int64)]
    if bad.any():
        out.append(_fmt("undecided pairs listed under an image outside the cutoff", ii[bad], jj[bad]))
    return out


def invariants(got):
    """j in row i <=> i in row j, and the two image codes add up to 26 (opposite shifts)."""
    out = []
    ii, jj = np.nonzero(got.keep & ~got.keep.T)
    if len(ii):
        out.append(_fmt("one-way pairs", ii, jj))
    ii, jj = np.nonzero(got.keep & got.keep.T & (got.code.astype(np.int64) + got.code.T.astype(np.int64) != 26))
    if len(ii):
        out.append(_fmt("pairs whose two codes do not add up to 26", ii, jj))
    return out


# ----------------------------------------------------------------------------------------------- the cell list's bins
BIN_MARGIN = 2.0 ** -18


def make_bins(lengths, cutoff, guarded=True):
    """csrc/nbr.hip make_bins: bins per side.  guarded=False: floor(L / cutoff) in float32, what the builder took before a
    bin had to be wider than the cutoff by BIN_MARGIN of the box."""
    L = np.asarray(lengths, np.float32)
    rc = np.float32(cutoff)
    if not guarded:
        return np.maximum(np.floor(L / rc).astype(np.int64), 1)
    L64 = L.astype(np.float64)
    return np.maximum(np.floor(L64 / (float(rc) + BIN_MARGIN * L64)).astype(np.int64), 1)


def bin_coord(x, inv, nb):
    """csrc/nbr.hip bin_coord as the compiler emits it for gfx950 (device code contracts a * b - c):
        p = fl(x inv); fr = fma(x, inv, -floor(p)); b = (int) fl(fr nb), clamped to [0, nb - 1].
    x inv is exact in float64 (24 x 24 bits), and so is the difference with the integer: one rounding to float32."""
    x = np.asarray(x, np.float32)
    inv = np.float32(inv)
    p = x * inv
    fr = (x.astype(np.float64) * np.float64(inv) - np.floor(p).astype(np.float64)).astype(np.float32)
    b = (fr * np.float32(nb)).astype(np.int64)                          # (int): truncation toward zero
    return np.clip(b, 0, int(nb) - 1)


def bin_coord_plain(x, inv, nb):
    """The same without the contraction: fr = fl(p - floor(p))."""
    x = np.asarray(x, np.float32)
    p = x * np.float32(inv)
    fr = p - np.floor(p)
    return np.clip((fr * np.float32(nb)).astype(np.int64), 0, int(nb) - 1)


def stencil_misses(full, pos, lengths, inv, nb, coord=bin_coord):
    """Ordered pairs of `full` that a 27-bin stencil over `nb` bins per side never tests: some component's bins differ by
    more than one (cyclically)."""
    b = np.stack([coord(np.asarray(pos, np.float32)[:, k], inv[k], nb[k]) for k in range(3)], 1)
    out = np.zeros_like(full.keep)
    for k in range(3):
        diff = np.abs(b[:, None, k] - b[None, :, k])
        out |= np.minimum(diff, int(nb[k]) - diff) > 1
    return np.nonzero(out & full.keep)


def _around(x0, k=5):
    """x0 and its k float32 neighbours on either side."""
    up, dn = [np.float32(x0)], [np.float32(x0)]
    for _ in range(k):
        up.append(np.nextafter(up[-1], np.float32(np.inf)))
        dn.append(np.nextafter(dn[-1], np.float32(-np.inf)))
    return np.array(dn[:0:-1] + up, np.float32)


def search_bin_edge(n_boxes, seed, n_range=(4, 9)):
    """Boxes whose side is a whole number of cutoffs to within one float32 (L = fl(rc n) or the next float above,
    n_range[0] <= n < n_range[1], rc uniform in [1, 3)) with floor(L / rc) = n bins of the cutoff, and in each the pairs
    (x_A, x_B) along one axis, x_A within 5 ulps above-or-below the lower edge of bin k + 1 and x_B around the upper edge
    of bin k - 1 (k + 1 = n: across the periodic face, x_A = 0 .. 5 ulp(L)), that
        * bin_coord AND bin_coord_plain put two bins apart with the real inverse (cell_inv), and
        * the float32 pair test accepts: fl(d^2) < fl(rc^2).
    Returns rows (rc, L, n, k, x_A, x_B) as float32/ints in a list, in the order found (deterministic in seed)."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    out = []
    for _ in range(n_boxes):
        rc = f32(rng.uniform(1.0, 3.0))
        n = int(rng.integers(*n_range))
        L = f32(rc * f32(n))
        if rng.integers(2):
            L = np.nextafter(L, f32(np.inf))
        k = int(rng.integers(1, n))                       # B under the edge k w, A over the edge (k + 1) w
        if int(make_bins([L], rc, guarded=False)[0]) != n:
            continue
        inv = cell_inv(np.full(3, L, f32))[0]
        xb = _around(f32(np.float64(L) * k / n))
        xa = _around(f32(np.float64(L) * (k + 1) / n)) if k + 1 < n else np.arange(6).astype(f32) * np.spacing(L)
        ok = np.ones((len(xa), len(xb)), bool)
        for coord in (bin_coord, bin_coord_plain):
            gap = (coord(xa, inv, n)[:, None] - coord(xb, inv, n)[None, :]) % n
            ok &= gap == 2
        d = xa[:, None] - xb[None, :]
        o = -np.clip(np.rint(d * inv), f32(-1), f32(1))
        dm = (o.astype(np.float64) * np.float64(L) + d.astype(np.float64)).astype(f32)
        d2 = dm * dm
        ok &= (d2 < f32(rc * rc)) & (d2 != 0)
        for ia, ib in zip(*np.nonzero(ok)):
            out.append((rc, L, n, k, xa[ia], xb[ib]))
    return out


# ----------------------------------------------------------------------------------------------- inputs of the GPU tests
def _unwrap(pos, lengths):
    """Every 7th atom one cell further along x, every 11th one cell back along y (float32 adds, as a caller would)."""
    pos = pos.copy()
    L = np.asarray(lengths, np.float32)
    pos[::7, 0] += L[0]
    pos[::11, 1] -= L[1]
    return pos


def _uniform(n, lengths, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0, 1, (n, 3)) * np.asarray(lengths, np.float64)).astype(np.float32)


class Case:
    """One input: pos float32 [N, 3], cell (float32 [3] or [3, 3]), cutoff, group, mask arguments for ops.build_mask,
    the builders that apply, and `ties`: the unordered pairs put on a decision boundary on purpose (undecided for
    full_list64 by construction; the cap on undecided pairs counts the others)."""

    def __init__(self, name, pos, cell, cutoff, methods, group=None, index_tuple=None, ex_pairs=None, ties=()):
        self.name, self.pos, self.cell, self.cutoff = name, np.ascontiguousarray(pos, np.float32), np.asarray(cell, np.float32), cutoff
        self.methods, self.group, self.index_tuple, self.ex_pairs, self.ties = methods, group, index_tuple, ex_pairs, tuple(ties)
        self._refs = {}

    diag = property(lambda self: self.cell.ndim == 1)

    def mask(self):
        if self.index_tuple is None and self.ex_pairs is None:
            return None
        g = self.group or len(self.pos)
        keep = np.ones((g, g), bool)
        if self.index_tuple is not None:
            sel = np.zeros((g, g), bool)
            sel[np.asarray(self.index_tuple[0])[:, None], np.asarray(self.index_tuple[1])[None, :]] = True
            keep &= sel | sel.T
        if self.ex_pairs is not None:
            ex = np.asarray(self.ex_pairs).reshape(-1, 2)
            keep[ex[:, 0], ex[:, 1]] = False
            keep[ex[:, 1], ex[:, 0]] = False
        return keep

    def ref64(self):
        if "r64" not in self._refs:
            self._refs["r64"] = full_list64(self.pos, self.cell, self.cutoff, self.group, self.mask())
        return self._refs["r64"]

    def ref32(self):
        if "r32" not in self._refs:
            self._refs["r32"] = full_list32_diag(self.pos, self.cell, self.cutoff, None, self.group, self.mask())
        return self._refs["r32"]

    def undecided_outside_ties(self):
        ii, jj = np.nonzero(self.ref64().und)
        t = {frozenset(p) for p in self.ties}
        return [(int(i), int(j)) for i, j in zip(ii, jj) if frozenset((int(i), int(j))) not in t]


def _case_a():
    L = np.array([7.3, 8.1, 9.4], np.float32)
    pos = _unwrap(_uniform(200, L, 101), L)
    pos[3, 0] = pos[50, 1] = pos[120, 2] = np.float32(-1e-9)
    pos[5, 0], pos[60, 1], pos[130, 2] = L[0], L[1], L[2]
    return Case("A orthorhombic", pos, L, 2.5, ("dense",))


def _case_b():
    h = np.array([[7.5, 0, 0], [1.5, 8.0, 0], [-1.0, 2.0, 8.5]], np.float32)
    fr = np.random.default_rng(202).uniform(0, 1, (150, 3))
    return Case("B triclinic", (fr @ h.astype(np.float64)).astype(np.float32), h, 2.5, ("dense",))


def _case_c():
    """A box shorter than two cutoffs: one image only, rows nearly N - 1 long.  Atoms 0..9 are placed:
      (0, 1)  dx = 2.0 = L / 2 exactly: s = 0.5 is a tie, no shift, listed at d = 2.0 with the centre code 13
      (2, 3)  (1, 1, 1) and (3.5, 1, 1): s = 0.625, the one image is dx - L = -1.5: listed at d = 1.5 (codes 12 / 14)
      (4, 5)  D = (0, 1.5, 2.0): d^2 = 6.25 = rc^2 exactly in float32 and float64 (dz = L / 2 takes no shift): excluded
      (6, 7)  D = (0, 1.5, nextbelow(2.0)): d^2 = 6.25 - 2^-21, the float32 number below rc^2: included
      (8, 9)  coincide: excluded both ways."""
    L = np.full(3, 4.0, np.float32)
    pos = _uniform(30, L, 303)
    pos[0], pos[1] = (0.40625, 3.28125, 3.09375), (2.40625, 3.28125, 3.09375)
    pos[2], pos[3] = (1.0, 1.0, 1.0), (3.5, 1.0, 1.0)
    pos[4], pos[5] = (2.71875, 0.53125, 0.15625), (2.71875, 2.03125, 2.15625)
    pos[6], pos[7] = (1.84375, 0.5, 0.0), (1.84375, 2.0, np.nextafter(np.float32(2.0), np.float32(0)))
    pos[8] = pos[9] = (3.21875, 1.34375, 2.65625)
    return Case("C box under two cutoffs", pos, L, 2.5, ("dense",), ties=((0, 1), (4, 5), (6, 7)))


D_SIZES = (1, 2, 63, 64, 65, 129)


def _case_d(n):
    L = np.full(3, 5.5, np.float32)
    return Case("D %d atoms" % n, _uniform(129, L, 404)[:n], L, 2.5, ("dense",))


def _case_d_groups(kind):
    L = np.full(3, 8.0, np.float32)                       # three bins per side: both builders
    pos = _uniform(195, L, 405 if kind == "index_tuple" else 406)
    if kind == "index_tuple":
        return Case("D groups index_tuple", pos, L, 2.5, ("dense", "cell"), group=65, index_tuple=(list(range(0, 27)), list(range(27, 65))))
    return Case("D groups ex_pairs", pos, L, 2.5, ("dense", "cell"), group=65, ex_pairs=[[0, 1], [7, 64], [10, 11], [63, 64], [0, 64]])


def _case_e(name):
    both = ("dense", "cell")
    if name in ("333", "444", "345"):
        L = {"333": (7.6, 7.6, 7.6), "444": (10.5, 10.5, 10.5), "345": (8.0, 10.4, 12.9)}[name]
        n = {"333": 601, "444": 600, "345": 599}[name]
        seed = {"333": 501, "444": 502, "345": 503}[name]
        L = np.array(L, np.float32)
        return Case("E bins " + name, _unwrap(_uniform(n, L, seed), L), L, 2.5, both)
    if name == "dilute":
        L = np.full(3, 13.0, np.float32)
        return Case("E dilute", _uniform(40, L, 504), L, 2.5, both)
    assert name == "droplet"
    L = np.full(3, 12.0, np.float32)
    rng = np.random.default_rng(505)
    drop = np.array([6.6, 1.2, 11.0]) + rng.normal(0, 0.45, (150, 3))   # one bin of the 4 x 4 x 4 grid, on two faces
    pos = np.concatenate([rng.uniform(0, 12.0, (70, 3)), drop]).astype(np.float32)
    return Case("E droplet", pos, L, 2.5, both)


E_NAMES = ("333", "444", "345", "dilute", "droplet")


def _case_f():
    """The bin-edge constructions of tests/golden/nbr_bin_edge.npz, one case per construction: the two atoms of the pair
    plus filler atoms far from both."""
    g = dict(np.load(os.path.join(GOLDEN, "nbr_bin_edge.npz"), allow_pickle=False))
    out = []
    for k in range(len(g["cutoff"])):
        L, ax = g["lengths"][k], int(g["axis"][k])
        fill = np.full((4, 3), 0.77)                      # the pair sits at 0.3 of the other two sides: far from these
        fill[:, ax] = (0.1, 0.13, 0.55, 0.58)
        pos = np.concatenate([g["pos"][k], (fill * L.astype(np.float64)).astype(np.float32)])
        out.append(Case("F construction %d" % k, pos, L, float(g["cutoff"][k]), ("dense", "cell"), ties=((0, 1),)))
    return out


_CACHE = {}


def cases():
    """{name: Case} of every input of tests/test_gpu_nbr_ref.py, built once."""
    if not _CACHE:
        cs = [_case_a(), _case_b(), _case_c()] + [_case_d(n) for n in D_SIZES]
        cs += [_case_d_groups("index_tuple"), _case_d_groups("ex_pairs")] + [_case_e(n) for n in E_NAMES] + _case_f()
        _CACHE.update({c.name: c for c in cs})
    return _CACHE


RANDOM = ("A orthorhombic", "B triclinic", "C box under two cutoffs", "D 129 atoms", "D groups index_tuple", "D groups ex_pairs",
          "E bins 333", "E bins 444", "E bins 345", "E dilute", "E droplet")
UNDECIDED_CAP = 5
