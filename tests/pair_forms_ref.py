"""Reference of the built-in pair forms (LJ family with arbitrary powers, excluded volume, modified Morse with phi of either
sign, Buckingham, Yukawa) as the trajectory kernels and pair_ell evaluate them: numpy, CPU only, all pairs, no lists.

    U       = sum_terms sum_{i<j selected, 0 < d^2 < rc^2} phi(r)
    F_i     = -dU/dx_i            = sum_j c1 D,             D = x_j - x_i (minimum image), c1 = phi'/r
    dq_i    = d(w.F)/dx_i         = -sum_j [kk (w_ij.D) D + c1 w_ij],   w_ij = w_i - w_j, kk = (phi'' - phi'/r) / r^2
    dth_k   = d(w.F)/dtheta_k     = sum_{i<j} (d phi'/d theta_k) / r (w_ij.D)      per term and parameter
    dU_k    = dU/dtheta_k         = sum_{i<j} d phi/d theta_k

The forms are written from their energies (mdgrad_amd/potentials.py, oracle.pair_phi's docstring) and differentiated by hand;
tests/test_pair_forms_ref_host.py pins every derivative to float64 autograd of the torch modules, to central differences of U
and to oracle.PairTerm in float64.  Minimum image: topology.py:59-64 (one image: s = D . inv, shift by -1 where s > 0.5 and by
+1 where s < -0.5).

Every quantity comes with its SCALE: per atom (and component) the sum over the atom's pairs of the absolute values of the
summands -- for the theta sums and U over all pairs.  Errors are measured over that scale, so an atom whose forces cancel is
judged by what was added up, not by what is left.

`dtype=np.float32` restates the same formulas in float32 with the kernels' association where it matters: d^2 = (x^2 + y^2) +
z^2 (norm2_ref), 1/r = rsqrt(d^2), r = d^2 rsqrt(d^2), integer powers by repeated squaring, float32 sums.  `floors()` is
|float32 - float64| / scale, the largest over atoms (per entry for theta), at least 2^-24: the rounding floor of the formula
itself, CPU only, never compared with a kernel's bits.

Pair membership is decided by the float32 d^2 (numpy, un-contracted) against the float32 rc^2 -- for a fixture free of fragile
pairs that is the float64 set; `fragile_pairs` lists the pairs whose float32 d^2 lies within 4 ulps of some term's rc^2 or whose
fractional separation lies within 1e-6 of +-0.5 while either image is inside the largest cutoff.  Every fixture is free of them
except the two pairs `cutoff_pair` places on purpose (one at pred(rc), included; one at exactly rc, excluded).

Selection masks are symmetric [N, N] boolean arrays (what ops.build_mask makes of index_tuple / ex_pairs); the kernels read a
pair's bit from whichever side evaluates it, so a one-sided mask has no defined meaning and `Term` refuses it -- unless asked
(`one_sided=True`, `one_sided_mask`): the kernels that give every atom a row of its own (workgroup, large path, pair_ell) read
mask[i, j] for the sums of atom i, so with a bit cleared on one side only F_i and dq_i lose the pair while F_j and dq_j keep it.
That is no supported input; it exists so that a transposed read of the mask, which no symmetric mask can show, fails a test.
(U and the theta sums run over i < j and are not defined for it.)"""
import collections
import math

import numpy as np

F32 = np.float32
EPS = 2.0 ** -24
HALF_EPS, CUT_ULPS = 1e-6, 4
TRICLINIC = ((6.0, 0.0, 0.0), (1.2, 5.5, 0.0), (0.7, -0.9, 6.3))          # the cell of tests/golden/nbr_tric64.npz

# name -> (kind, constants, theta): the form() values of tests/test_gpu_parity.py and its Yukawa
FORMS = collections.OrderedDict([
    ("lj", ("lj", dict(p=12, q=6, c=1.0), (1.05, 0.9))),
    ("ljfam_8_4", ("lj", dict(p=8, q=4, c=1.0), (0.95, 1.1))),
    ("lj69", ("lj", dict(p=9, q=6, c=1.0), (1.0, 1.2))),
    ("exvol12", ("lj", dict(p=12, q=0, c=0.0), (1.0, 1.0))),
    ("exvol10", ("lj", dict(p=10, q=0, c=0.0), (1.1, 0.7))),
    ("morse_pos", ("morse", dict(a=3.0, phi=1.5), ())),
    ("morse_neg", ("morse", dict(a=2.5, phi=-1.2), ())),
    ("buck", ("buck", {}, (1000.0, 3.5, 5.0))),
    ("yukawa", ("yukawa", {}, (1.3, 0.8))),
])


class Term:
    """One pair term: a form of FORMS (or kind / consts / theta given directly), its cutoff and an optional symmetric mask."""

    def __init__(self, form, cutoff=2.5, mask=None, theta=None, one_sided=False):
        self.form = form
        self.kind, self.consts, th = FORMS[form]
        self.theta = tuple(float(F32(v)) for v in (th if theta is None else theta))      # the float32 values a kernel receives
        self.cutoff = float(cutoff)
        self.mask = None if mask is None else np.asarray(mask).astype(bool)
        if self.mask is not None and not one_sided:
            assert (self.mask == self.mask.T).all(), "selection masks are symmetric"

    @property
    def n_theta(self):
        return len(self.theta)


def module(form, theta=None):
    """the torch module of mdgrad_amd.potentials for a form of FORMS"""
    from mdgrad_amd import potentials as P
    kind, c, th = FORMS[form]
    th = th if theta is None else theta
    if kind == "lj":
        if c["c"] == 0.0:
            return P.ExcludedVolume(sigma=th[0], epsilon=th[1], power=c["p"])
        return P.LJFamily(sigma=th[0], epsilon=th[1], attr_pow=c["q"], rep_pow=c["p"])
    if kind == "morse":
        return P.ModifiedMorse(a=c["a"], phi=c["phi"])
    if kind == "buck":
        return P.Buck(A=th[0], B=th[1], C=th[2])
    return P.Yukawa(epsilon=th[0], kappa=th[1])


# ------------------------------------------------------------------------------------------------ the forms
def _ipow(x, n):
    """x^n by repeated squaring (csrc/common.hpp ipow) -- in float64 the same value as x ** n to rounding"""
    r = np.ones_like(x)
    while n > 0:
        if n & 1:
            r = r * x
        x = x * x
        n >>= 1
    return r


def phi(term, r, ir, dt):
    """(u, u', u'', [du/dtheta_k], [du'/dtheta_k]) at distances r with ir = 1/r, every operation in dtype dt."""
    c = dt.type
    k, cs, th = term.kind, term.consts, [c(v) for v in term.theta]
    if k == "lj":
        p, q, cc = cs["p"], cs["q"], c(cs["c"])
        sig, eps = th
        s = sig * ir
        sp = _ipow(s, p)
        sq = _ipow(s, q) * cc
        fp, fq = c(p), c(q)
        e4 = c(4) * eps
        u = e4 * (sp - sq)
        du = -e4 * (fp * sp - fq * sq) * ir
        d2u = e4 * (fp * (fp + c(1)) * sp - fq * (fq + c(1)) * sq) * ir * ir
        du_dth = [e4 * (fp * sp - fq * sq) / sig, c(4) * (sp - sq)]
        ddu_dth = [-e4 * (fp * fp * sp - fq * fq * sq) * ir / sig, -c(4) * (fp * sp - fq * sq) * ir]
        return u, du, d2u, du_dth, ddu_dth
    if k == "morse":
        a, ph = c(cs["a"]), c(cs["phi"])
        A = c(0.0) if cs["phi"] >= 0 else c(math.exp(2 * cs["a"] / cs["phi"]) - 2 * math.exp(cs["a"] / cs["phi"]))
        n = c(1) / (c(1) + A)
        rp = np.power(r, ph)
        x = a * (c(1) - rp) / ph
        e1 = np.exp(x)
        e2 = e1 * e1
        x1 = -a * rp * ir                                   # x'
        x2 = -a * (ph - c(1)) * rp * ir * ir                # x''
        ux = (c(2) * e2 - c(2) * e1) * n
        uxx = (c(4) * e2 - c(2) * e1) * n
        return (e2 - c(2) * e1 - A) * n, ux * x1, uxx * x1 * x1 + ux * x2, [], []
    if k == "buck":
        A, B, C = th
        e = np.exp(-B * r)
        ir2 = ir * ir
        ir6 = ir2 * ir2 * ir2
        u = A * e - C * ir6
        du = -A * B * e + c(6) * C * ir6 * ir
        d2u = A * B * B * e - c(42) * C * ir6 * ir2
        return u, du, d2u, [e, -A * r * e, -ir6], [-B * e, A * e * (B * r - c(1)), c(6) * ir6 * ir]
    if k == "yukawa":
        eps, kap = th
        e = np.exp(-kap * r)
        kr = kap * r
        u = eps * e * ir
        du = -eps * e * (kr + c(1)) * ir * ir
        d2u = eps * e * (kr * kr + c(2) * kr + c(2)) * ir * ir * ir
        return u, du, d2u, [e * ir, -eps * e], [-e * (kr + c(1)) * ir * ir, eps * e * kap]
    raise ValueError(k)


# ------------------------------------------------------------------------------------------------ geometry
def _cell(cell, dt):
    h = np.asarray(cell, F32)
    if h.ndim == 1:
        h = np.diag(h)
    inv = np.linalg.inv(h.astype(np.float64)).astype(F32)            # (the float32 inverse a kernel receives)
    return h.astype(dt), inv.astype(dt), bool((h == np.diag(np.diag(h))).all())


def _images(x, cell, dt):
    """D[i, j] = x_j - x_i with the one-image minimum image, the fractional separations s, and d^2 = (x^2 + y^2) + z^2"""
    h, inv, diag = _cell(cell, dt)
    x = np.asarray(x).astype(dt)                                     # (float32 values; float64 for finite differences)
    D = x[None, :, :] - x[:, None, :]
    s = D * np.diag(inv) if diag else D @ inv
    o = (s < -0.5).astype(dt) - (s > 0.5).astype(dt)
    D = D + (o * np.diag(h) if diag else o @ h)
    d2 = (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]
    return D, s, d2


def membership(x, cell, terms):
    """per term: bool [N, N] of the directed pairs it evaluates -- the float32 d^2 against the float32 rc^2, and its mask"""
    _, _, d2 = _images(x, cell, np.dtype(F32))
    out = []
    for t in terms:
        rc2 = F32(t.cutoff) * F32(t.cutoff)
        m = (d2 < rc2) & (d2 > 0)
        out.append(m & t.mask if t.mask is not None else m)
    return out


def fragile_pairs(x, cell, terms):
    """sorted rows (i, j), i < j: the float32 d^2 within CUT_ULPS ulps of some term's float32 rc^2, or a fractional separation
    within HALF_EPS of +-0.5 while the pair, under either image, is inside the largest cutoff."""
    _, _, d2 = _images(x, cell, np.dtype(F32))
    D, s, d64 = _images(x, cell, np.dtype(np.float64))
    h = _cell(cell, np.dtype(np.float64))[0]
    n = len(d2)
    hit = np.zeros((n, n), bool)
    rcmax = max(t.cutoff for t in terms)
    for t in terms:
        rc2 = F32(t.cutoff) * F32(t.cutoff)
        hit |= np.abs(d2.astype(np.float64) - float(rc2)) <= CUT_ULPS * float(np.spacing(rc2))
    for c in range(3):
        i, j = np.nonzero(np.abs(np.abs(s[..., c]) - 0.5) < HALF_EPS)
        for a, b in zip(i, j):
            alt = [D[a, b], D[a, b] + h[c], D[a, b] - h[c]]
            if min(float((v * v).sum()) for v in alt) < (rcmax + 1e-3) ** 2:
                hit[a, b] = True
    hit |= hit.T
    i, j = np.nonzero(np.triu(hit, 1))
    return np.stack([i, j], 1)


# ------------------------------------------------------------------------------------------------ the evaluation
Result = collections.namedtuple("Result", "U F dq dth dU sU sF sdq sdth sdU")


def evaluate(x, w, cell, terms, dtype=np.float64, member=None):
    """Result for positions x [N, 3] (float32 values), direction w, the cell and the terms, every operation in `dtype`.
    dth / dU / their scales: one array per term."""
    dt = np.dtype(dtype)
    member = membership(x, cell, terms) if member is None else member
    D, _, d2 = _images(x, cell, dt)
    w = np.asarray(w).astype(dt)
    n = len(d2)
    z = lambda *s: np.zeros(s, dt)                                   # noqa: E731
    U, sU, F, sF, dq, sdq = z(), z(), z(n, 3), z(n, 3), z(n, 3), z(n, 3)
    dth, dU, sdth, sdU = [], [], [], []
    for t, m in zip(terms, member):
        i, j = np.nonzero(m)                                         # directed pairs
        Dp, d2p = D[i, j], d2[i, j]
        ir = (dt.type(1) / np.sqrt(d2p)).astype(dt)                  # rsqrt(d^2)
        r = d2p * ir
        u, du, d2u, du_dth, ddu_dth = phi(t, r, ir, dt)
        c1 = du * ir
        kk = (d2u - c1) * ir * ir
        wij = w[i] - w[j]
        b = (wij[:, 0] * Dp[:, 0] + wij[:, 1] * Dp[:, 1]) + wij[:, 2] * Dp[:, 2]
        f = c1[:, None] * Dp
        h1, h2 = (kk * b)[:, None] * Dp, c1[:, None] * wij
        np.add.at(F, i, f)
        np.add.at(sF, i, np.abs(f))
        np.add.at(dq, i, -(h1 + h2))
        np.add.at(sdq, i, np.abs(h1) + np.abs(h2))
        up = i < j                                                   # each pair once
        U, sU = U + u[up].sum(dtype=dt), sU + np.abs(u[up]).sum(dtype=dt)
        tb = [(g * ir * b)[up] for g in ddu_dth]
        dth.append(np.array([v.sum(dtype=dt) for v in tb], dt))
        sdth.append(np.array([np.abs(v).sum(dtype=dt) for v in tb], dt))
        dU.append(np.array([g[up].sum(dtype=dt) for g in du_dth], dt))
        sdU.append(np.array([np.abs(g[up]).sum(dtype=dt) for g in du_dth], dt))
    return Result(U, F, dq, dth, dU, sU, sF, sdq, sdth, sdU)


QUANTITIES = ("U", "F", "dq", "dth", "dU")


def _flat(v):
    return np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in v]) if isinstance(v, list) else np.asarray(v, np.float64)


def error(got, ref, q, slack=None):
    """largest |got - ref64| / scale of quantity q over atoms and components (entries for dth / dU); where the scale is zero
    `got` must be an exact zero (inf otherwise).  `slack`: an absolute error of the MEASUREMENT (not of the kernel) per entry,
    taken off |got - ref64| first -- the trajectory adjoint hands d(w.F)/dq out as w + dq / 2 rounded to float32."""
    g, r, s = _flat(got), _flat(getattr(ref, q)), _flat(getattr(ref, "s" + q))
    assert g.shape == r.shape, (q, g.shape, r.shape)
    d = np.abs(g - r)
    if slack is not None:
        d = np.maximum(d - _flat(slack), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(s > 0, d / s, np.where(g == 0, 0.0, np.inf))
    return float(e.max()) if e.size else 0.0


def floors(x, w, cell, terms, ref=None, member=None):
    """{quantity: floor}: the float32 restatement against float64, at least 2^-24"""
    member = membership(x, cell, terms) if member is None else member
    ref = evaluate(x, w, cell, terms, member=member) if ref is None else ref
    r32 = evaluate(x, w, cell, terms, np.float32, member)
    return {q: max(EPS, error(getattr(r32, q), ref, q)) for q in QUANTITIES}


# ------------------------------------------------------------------------------------------------ fixtures
Fixture = collections.namedtuple("Fixture", "name x cell placed")      # placed: the fragile pairs put there on purpose
_FCC = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])


def _fcc(side, n):
    """the first n sites of a side^3 fcc box with lattice constant 1.6 (the headline's 4.8 cell at side 3), from 0.4 up"""
    c = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    return ((c + _FCC[None]).reshape(-1, 3) + 0.25)[:n] * 1.6


def _clean(name, make, cell, terms, placed=()):
    """the first seed whose fixture has no fragile pair beyond the placed ones (for the cutoffs 2.5 and 1.8 used here)"""
    for seed in range(50):
        x = make(np.random.default_rng(1000 + seed)).astype(F32)
        if fragile_pairs(x, cell, terms).tolist() == sorted(map(list, placed)):
            return Fixture(name, x, np.asarray(cell, F32), tuple(placed))
    raise AssertionError("no seed gives a fixture without fragile pairs: " + name)


_GUARD = None


def _guard_terms():
    global _GUARD
    if _GUARD is None:
        _GUARD = [Term("lj", 2.5), Term("lj", 1.8)]
    return _GUARD


_CACHE = {}


def _cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def liquid(n, cell_len=None):
    """n atoms of a jittered fcc lattice: 4.8 cell (side 3) up to 108 atoms, 6.4 (side 4) up to 256, 11.2 (side 7) beyond;
    `cell_len` rescales the 108-atom lattice to another cell.  Every coordinate is at least 0.25."""
    side = 3 if n <= 108 else (4 if n <= 256 else 7)
    L = 1.6 * side if cell_len is None else float(cell_len)
    scale = L / (1.6 * side)

    def make(rng):
        x = _fcc(side, n) * scale + rng.normal(0, 0.05, (n, 3))
        assert x.min() >= 0.25 and x.max() < L
        return x
    return _cached(("liquid", n, L), lambda: _clean("liquid%d%s" % (n, "" if cell_len is None else "@%g" % L), make,
                                                    [L, L, L], _guard_terms()))


def contact():
    """liquid(108) with four atoms pushed to 0.84 .. 0.89 of a neighbour (0.80 .. 0.85 sigma of the LJ form; above the
    turnover of the Buckingham form at 0.75): the twelfth power dominates"""
    def make(rng):
        x = _fcc(3, 108) + rng.normal(0, 0.05, (108, 3))
        for k, (a, b) in enumerate(((0, 1), (20, 21), (50, 53), (106, 107))):
            d = x[b] - x[a]
            x[b] = x[a] + d / np.linalg.norm(d) * (0.84 + 0.05 * k / 3.0)
        assert x.min() >= 0.25
        return x
    return _cached("contact", lambda: _clean("contact", make, [4.8] * 3, _guard_terms()))


CUTOFF_PAIR_IN, CUTOFF_PAIR_OUT = (28, 29), (30, 31)


def cutoff_pair():
    """32 atoms in a 9.6 cell: a jittered cluster of 28, one pair along x at pred(2.5) (atoms 28, 29: included, each other's
    only neighbour) and one along y at exactly 2.5 (atoms 30, 31: excluded, no neighbour at all -- exact zeros)."""
    def make(rng):
        x = np.zeros((32, 3))
        x[:28] = _fcc(3, 28) + rng.normal(0, 0.05, (28, 3))
        x[28] = (1.0, 7.0, 7.0)
        x[29] = (float(F32(1.0) + np.nextafter(F32(2.5), F32(0))), 7.0, 7.0)
        x[30] = (7.0, 2.0, 8.0)
        x[31] = (7.0, 4.5, 8.0)
        return x
    fx = _cached("cutoff_pair", lambda: _clean("cutoff_pair", make, [9.6] * 3, [Term("lj", 2.5)],
                                               (CUTOFF_PAIR_IN, CUTOFF_PAIR_OUT)))
    return fx


def unwrapped():
    """liquid(108) with every third atom shifted by a whole cell (+x, -y, +z in turn): outside the [-0.24, 1.24] window, so
    the clamped image runs"""
    def make(rng):
        x = (_fcc(3, 108) + rng.normal(0, 0.05, (108, 3))).astype(F32)
        for k, a in enumerate(range(0, 108, 3)):
            x[a, k % 3] += F32(4.8) * (F32(-1) if k % 3 == 1 else F32(1))
        assert np.abs(x).min() >= 0.25
        return x
    return _cached("unwrapped", lambda: _clean("unwrapped", make, [4.8] * 3, _guard_terms()))


def triclinic(n=108):
    """n atoms of the jittered fcc lattice in fractional coordinates of the TRICLINIC cell, moved so every coordinate >= 0.25"""
    h = np.asarray(TRICLINIC)

    def make(rng):
        x = (_fcc(3, n) / 4.8) @ h + rng.normal(0, 0.05, (n, 3)) + np.array([0.5, 1.5, 0.5])
        assert x.min() >= 0.25
        return x
    return _cached(("triclinic", n), lambda: _clean("triclinic%d" % n, make, h, _guard_terms()))


def base500():
    """500 atoms of the jittered fcc lattice (side 5) in an 8.0 cell, every coordinate a multiple of 2^-18"""
    def make(rng):
        x = np.round((_fcc(5, 500) + rng.normal(0, 0.05, (500, 3))) * 2.0 ** 18) / 2.0 ** 18
        assert x.min() >= 0.25 and x.max() < 8.0
        return x
    return _cached("base500", lambda: _clean("base500", make, [8.0] * 3, _guard_terms()))


def supercell(reps):
    """base500 repeated reps = (rx, ry, rz) times along the axes, copy after copy, in the cell (8 rx, 8 ry, 8 rz).  The
    coordinates are multiples of 2^-18 below 32 and the shifts multiples of 8, so every copy is exact in float32 and every
    minimum-image vector is, bit for bit, the one of base500 (whose half cell, 4, exceeds the cutoffs): each atom sees what
    its original sees.  A system of 6 000 to 18 000 atoms whose reference is the 500-atom one, tiled (`tile`)."""
    fx = base500()
    sh = np.stack(np.meshgrid(*[np.arange(r) for r in reps], indexing="ij"), -1).reshape(-1, 1, 3) * 8.0
    x64 = (fx.x.astype(np.float64)[None] + sh).reshape(-1, 3)
    x = x64.astype(F32)
    assert (x.astype(np.float64) == x64).all() and x.max() < 32.0
    return Fixture("base500x%dx%dx%d" % tuple(reps), x, np.asarray([8.0 * r for r in reps], F32), ())


def tile(res, k):
    """the Result of k exact copies of a system with the Result `res`: per-atom rows repeated, sums over pairs times k"""
    rows = lambda a: np.tile(a, (k, 1))                                # noqa: E731
    return Result(res.U * k, rows(res.F), rows(res.dq), [a * k for a in res.dth], [a * k for a in res.dU],
                  res.sU * k, rows(res.sF), rows(res.sdq), [a * k for a in res.sdth], [a * k for a in res.sdU])


def direction(n, seed=11):
    return np.random.default_rng(seed).standard_normal((n, 3)).astype(F32)


# masks (as test_ring_kernels_with_a_selection_mask_vs_oracle / ..._several_masked_terms...): index_tuple / ex_pairs selections
def species(n):
    return list(range(0, n, 2)), list(range(1, n, 2))


def excluded_list(n):
    return [[i, i + 1] for i in range(0, n - 1, 3)] + ([[0, 5], [7, 100]] if n > 100 else [])


def select_mask(n, index_tuple=None, ex_pairs=None):
    """the symmetric selection of ops.build_mask, as a bool array"""
    keep = np.ones((n, n), bool)
    if index_tuple is not None:
        sel = np.zeros((n, n), bool)
        sel[np.asarray(index_tuple[0])[:, None], np.asarray(index_tuple[1])[None, :]] = True
        keep &= sel | sel.T
    if ex_pairs is not None:
        ex = np.asarray(ex_pairs).reshape(-1, 2)
        keep[ex[:, 0], ex[:, 1]] = False
        keep[ex[:, 1], ex[:, 0]] = False
    return keep


def one_sided_mask(n):
    """all ones but mask[a, b] = 0 for the pairs (a, b) of excluded_list, a < b, on that side only"""
    m = np.ones((n, n), bool)
    for a, b in excluded_list(n):
        m[a, b] = False
    return m


# term stacks: (form, theta or None, cutoff, selection keyword or None) per member
def stack(name, n):
    A, B = species(n)
    return {
        "two_species": [("lj", None, 2.5, dict(index_tuple=(A, B)))],
        "excluded_pairs": [("ljfam_8_4", None, 2.5, dict(ex_pairs=excluded_list(n)))],
        "excluded_pairs_lj": [("lj", None, 2.5, dict(ex_pairs=excluded_list(n)))],
        "three_term": [("lj", (1.0, 1.0), 2.5, dict(index_tuple=(A, A))), ("lj", (0.9, 0.8), 2.5, dict(index_tuple=(B, B))),
                       ("lj", (0.95, 1.2), 2.5, dict(index_tuple=(A, B)))],
        "three_term_ljfam": [("ljfam_8_4", (1.0, 1.0), 2.5, dict(index_tuple=(A, A))),
                             ("ljfam_8_4", (0.9, 0.8), 2.5, dict(index_tuple=(B, B))),
                             ("ljfam_8_4", (0.95, 1.2), 2.5, dict(index_tuple=(A, B)))],
        "two_term": [("ljfam_8_4", (0.9, 0.6), 2.5, dict(index_tuple=(A, B))), ("ljfam_8_4", (1.0, 0.4), 2.5, None)],
        "two_cutoffs": [("lj", (1.0, 1.0), 2.5, dict(index_tuple=(A, B))), ("lj", (0.9, 0.8), 1.8, None)],
    }[name]


def terms_of(members, n):
    return [Term(f, rc, None if sel is None else select_mask(n, **sel), th) for f, th, rc, sel in members]


def reference(fx, terms, w):
    """(Result in float64, floors, membership) of a fixture"""
    member = membership(fx.x, fx.cell, terms)
    ref = evaluate(fx.x, w, fx.cell, terms, member=member)
    return ref, floors(fx.x, w, fx.cell, terms, ref, member), member
