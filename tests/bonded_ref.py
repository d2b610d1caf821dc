"""The float64 definitions behind the bonded-term tests, as CPU torch (differentiable; pass float64 tensors -- or float32 ones:
the same formulas evaluated in float32 are the error floor the GPU tests scale their tolerances from).

    bond  (i, j)     b  = image(x_i - x_j)                              U = 1/2 k (|b|^2 - ro)^2      (SQUARED length against ro)
    angle (i, j, k)  b1 = image(x_i - x_j),  b2 = image(x_k - x_j)      U = 1/2 k (theta - theta0)^2
                     theta = atan2(|b1 x b2|, b1.b2)   in [0, pi]

image(b) = b + (-[b >= L/2] + [b < -L/2]) L per component: the single flag of topology.get_offsets, NON-strict on the upper side;
it is piecewise constant and carries no derivative.  L is the diagonal of the cell.

An angle term with |b1 x b2|^2 <= eps^2 |b1|^2 |b2|^2, eps = 2^-20 (three collinear atoms, or a bond vector of length zero), keeps
its energy -- theta is 0 or pi there -- and contributes zero gradient and zero H w: theta has a kink at both ends, zero is its
symmetric subgradient (the convention of csrc/adf.hip and csrc/dihedral.hip).

A term's energy is booked on its role-0 atom (column 0 of its row), like the kernel's per-atom energies."""
import numpy as np
import torch

BOND, ANGLE = 0, 1
EPS = 2.0 ** -20


def cell_lengths(cell):
    """The diagonal of a [3, 3] cell, or the [3] lengths themselves, as float32 numbers (what both classes keep)."""
    c = np.asarray(cell, dtype=np.float32)
    return np.diag(c).copy() if c.ndim == 2 else c


def _image(b, L):
    L = torch.as_tensor(np.asarray(L, dtype=np.float32)).to(b)
    return b + (-(b >= 0.5 * L).to(b) + (b < -0.5 * L).to(b)) * L


def _rows(top, width, n_atoms):
    t = torch.as_tensor(np.asarray(top), dtype=torch.long).reshape(-1, width)
    return torch.where(t < 0, t + n_atoms, t)


def bond_vectors(x, top, L):
    t = _rows(top, 2, x.shape[0])
    return _image(x[t[:, 0]] - x[t[:, 1]], L)


def angle_geometry(x, top, L):
    """(b1, b2, theta, regular) of every row: theta [n] carries no gradient where `regular` is False."""
    t = _rows(top, 3, x.shape[0])
    b1 = _image(x[t[:, 0]] - x[t[:, 1]], L)
    b2 = _image(x[t[:, 2]] - x[t[:, 1]], L)
    c = torch.cross(b1, b2, dim=-1)
    C, dot = c.pow(2).sum(-1), (b1 * b2).sum(-1)
    regular = C > EPS * EPS * b1.pow(2).sum(-1) * b2.pow(2).sum(-1)
    one = torch.ones_like(C)
    th = torch.atan2(torch.where(regular, C, one).sqrt(), torch.where(regular, dot, one))
    flat = torch.atan2(C.detach().sqrt(), dot.detach())                 # 0 or pi (to within eps), a constant
    return b1, b2, torch.where(regular, th, flat), regular


def term_energies(x, kind, top, k, x0, L):
    """U of every term [n_terms]."""
    if kind == BOND:
        return 0.5 * k * (bond_vectors(x, top, L).pow(2).sum(-1) - x0).pow(2)
    return 0.5 * k * (angle_geometry(x, top, L)[2] - x0).pow(2)


def energy(x, kind, top, k, x0, L):
    return term_energies(x, kind, top, k, x0, L).sum()


def per_atom_energy(x, kind, top, k, x0, L):
    t = _rows(top, 2 if kind == BOND else 3, x.shape[0])
    return torch.zeros(x.shape[0], dtype=x.dtype).index_add(0, t[:, 0], term_energies(x, kind, top, k, x0, L))


def _grad(y, x, create_graph=False):
    if not y.requires_grad:
        return torch.zeros_like(x)
    (g,) = torch.autograd.grad(y, x, create_graph=create_graph, allow_unused=True)
    return torch.zeros_like(x) if g is None else g


def grad(x, kind, top, k, x0, L):
    """dU/dx [N, 3] by autograd, in the dtype of x."""
    with torch.enable_grad():
        q = x.detach().requires_grad_(True)
        return _grad(energy(q, kind, top, k, x0, L), q).detach()


def hvp(x, w, kind, top, k, x0, L):
    """H w = d(w . dU/dx)/dx [N, 3] by double autograd, in the dtype of x."""
    with torch.enable_grad():
        q = x.detach().requires_grad_(True)
        g = _grad(energy(q, kind, top, k, x0, L), q, create_graph=True)
        return _grad((g * w.detach().to(q)).sum(), q).detach()


def evaluate(x, kind, top, k, x0, L, w=None):
    """dict(energy, e_atom, grad, hw) in the dtype of x (hw only with w)."""
    out = dict(energy=energy(x, kind, top, k, x0, L).detach(), e_atom=per_atom_energy(x, kind, top, k, x0, L).detach(),
               grad=grad(x, kind, top, k, x0, L))
    if w is not None:
        out["hw"] = hvp(x, w, kind, top, k, x0, L)
    return out


def scale(x, kind, top, k, x0, L):
    """The error scales of the GPU tests, float64: dict(energy, e_atom [N], grad [N], hw [N], sin [N]).  A per-atom scale is the sum,
    over the terms the atom takes part in, of the magnitude of the term's factors -- not of their (possibly cancelling) result:

        bond   grad  2 k max(|b|^2, ro) |b|                hw  2 k max(|b|^2, ro) + 4 k |b|^2     (H = 2k(|b|^2 - ro) 1 + 4k b b^T)
        angle  grad  k |theta - theta0| (1/|b1| + 1/|b2|)  hw  k (|theta - theta0| + 1) (1/|b1| + 1/|b2|)
        energy sum of |U_term|
        e_atom sum over the terms booked on the atom of 1/2 k max(|b|^2, ro)^2, resp. 1/2 k max(theta, theta0)^2: a single term's
               U = 1/2 k (difference)^2 cancels where the term sits at its minimum, its error follows the operands

    Terms that contribute no gradient by the collinearity rule contribute no scale either.  `sin` is the smallest sin(theta) over
    an atom's regular angle terms (1 for bonds, and for atoms in none): the near-collinear tests bound err * sin."""
    x = x.detach().double()
    N = x.shape[0]
    u = term_energies(x, kind, top, k, x0, L).abs()
    t = _rows(top, 2 if kind == BOND else 3, N)
    sin = torch.ones(N, dtype=torch.float64)
    if kind == BOND:
        s = bond_vectors(x, top, L).pow(2).sum(-1)
        sg = 2.0 * k * torch.clamp(s, min=float(x0)) * s.sqrt()
        sh = 2.0 * k * torch.clamp(s, min=float(x0)) + 4.0 * k * s
        se = 0.5 * k * torch.clamp(s, min=float(x0)).pow(2)
    else:
        b1, b2, th, regular = angle_geometry(x, top, L)
        inv = torch.where(regular, 1.0 / torch.where(regular, b1.norm(dim=-1), torch.ones_like(th))
                          + 1.0 / torch.where(regular, b2.norm(dim=-1), torch.ones_like(th)), torch.zeros_like(th))
        sg = k * (th - x0).abs() * inv
        sh = k * ((th - x0).abs() + 1.0) * inv
        se = 0.5 * k * torch.clamp(th, min=float(x0)).pow(2)
        st = torch.where(regular, th.sin().abs(), torch.ones_like(th))
        for r in range(3):
            sin = sin.scatter_reduce(0, t[:, r], st, "amin")
    g, h = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    for r in range(t.shape[1]):
        g = g.index_add(0, t[:, r], sg)
        h = h.index_add(0, t[:, r], sh)
    return dict(energy=u.sum(), e_atom=torch.zeros(N, dtype=torch.float64).index_add(0, t[:, 0], se), grad=g, hw=h, sin=sin)


def ratio(got, ref, sc, weight=None):
    """max over atoms and components of |got - ref| (* weight) / scale; an entry of scale 0 must be met exactly."""
    got = torch.as_tensor(got).detach().cpu().double()
    ref = torch.as_tensor(ref).detach().double()
    sc = torch.as_tensor(sc).double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    if weight is not None:
        err = err * (weight[:, None] if err.dim() == 2 else weight)
    if err.dim() == 2 and sc.dim() == 1:
        sc = sc[:, None].expand_as(err)
    if err.numel() == 0:
        return 0.0
    r = torch.where(sc > 0, err / torch.where(sc > 0, sc, torch.ones_like(sc)),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
# Every case holds float32 inputs; the reference sees the same float32 values, cast up.  The constants are float32 numbers too.
K_BOND, RO, K_ANGLE = 3.0, 1.0, 2.0                    # (chains step by 1.1: |b|^2 = 1.21, stretched against ro = 1)
TH0, PI32 = float(np.float32(1.9)), float(np.float32(np.pi))
F32 = np.float32


class Case:
    def __init__(self, name, kind, pos, top, L, k=None, x0=None, seed=0):
        self.name, self.kind = name, kind
        self.pos = np.ascontiguousarray(pos, dtype=F32)
        self.top = np.asarray(top, dtype=np.int64).reshape(-1, 2 if kind == BOND else 3)
        self.L = cell_lengths(L)
        self.k = (K_BOND if kind == BOND else K_ANGLE) if k is None else float(k)
        self.x0 = (RO if kind == BOND else TH0) if x0 is None else float(x0)
        self.w = np.random.default_rng(1000 + seed).normal(0, 1, self.pos.shape).astype(F32)
        self._cache = None

    @property
    def n_atoms(self):
        return self.pos.shape[0]

    def args(self):
        return self.kind, self.top, self.k, self.x0, self.L

    def reference(self):
        """(ref64, scale, ref32): the float64 reference of the float32 inputs, its error scales, and the same formulas in
        float32 -- whose distance from ref64, in units of the scales, is the floor.  Computed once."""
        if self._cache is None:
            x, w = torch.tensor(self.pos), torch.tensor(self.w)
            self._cache = (evaluate(x.double(), *self.args(), w=w.double()), scale(x.double(), *self.args()),
                           evaluate(x, *self.args(), w=w))
        return self._cache


    def energy_floor(self):
        """sum_t |U_t in float32 - U_t| / sum_t |U_t|: the float32 error of the energy without the luck of cancelling roundings
        (one scalar's error is no floor)."""
        x = torch.tensor(self.pos)
        u64 = term_energies(x.double(), *self.args())
        u32 = term_energies(x, *self.args()).double()
        return float((u32 - u64).abs().sum() / u64.abs().sum()) if float(u64.abs().sum()) > 0 else 0.0


QUANTITIES = ("energy", "e_atom", "grad", "hw")


def ratios(out, ref, sc, sin_weighted=False):
    """{quantity: max |out - ref| / scale} over the quantities `out` holds; grad and hw times sin(theta) when asked."""
    r = {}
    for q in QUANTITIES:
        if out.get(q) is None:
            continue
        if q == "energy":
            r[q] = ratio(torch.as_tensor(out[q]).reshape(1), ref[q].reshape(1), sc[q].reshape(1))
        else:
            r[q] = ratio(out[q], ref[q], sc[q], sc["sin"] if (sin_weighted and q in ("grad", "hw")) else None)
    return r


def random_chain(n, seed, step=1.1, min_sin=0.35, start=(2.5, 2.5, 2.5)):
    """float64 [n, 3]: a random walk of fixed step whose consecutive bonds make an angle with sine >= min_sin."""
    rng = np.random.default_rng(seed)
    x = [np.asarray(start, dtype=np.float64)]
    prev = None
    while len(x) < n:
        s = rng.normal(0, 1, 3)
        s *= step / np.linalg.norm(s)
        if prev is not None and np.linalg.norm(np.cross(prev, s)) < min_sin * step * step:
            continue
        x.append(x[-1] + s)
        prev = s
    return np.array(x)


def chain_rows(kind, n, start=0):
    w = 2 if kind == BOND else 3
    return np.array([[start + i + r for r in range(w)] for i in range(max(0, n - w + 1))], dtype=np.int64).reshape(-1, w)


def chain_case(kind, n, free=0, extras=False, L=(6.0, 6.0, 6.0)):
    """A chain of n atoms wrapped into the cell, `free` more atoms in no term; extras: the first five rows again, rows 5..9 in
    the other direction, and one row in negative indices."""
    rng = np.random.default_rng(n)
    pos = np.concatenate([random_chain(n, 10 + n), rng.uniform(0, 6, (free, 3))])
    top = chain_rows(kind, n)
    if extras:
        neg = (top[-1] - (n + free))[None, ::-1]
        top = np.concatenate([top, top[:5], top[5:10, ::-1], neg])
    return Case("%s chain %d+%d%s" % ("bond" if kind == BOND else "angle", n, free, " extras" if extras else ""), kind,
                np.mod(pos, np.asarray(L)), top, L, seed=n)


def star_case(kind, n, hub_last):
    """A hub with 64 leaves among n atoms (the rest in no term), the hub at index 0 or n - 1.  Bonds: hub-leaf, in alternating
    direction.  Angles: the hub as centre of 63 rows (leaf, hub, next leaf), as first end of 63 (hub, leaf, next leaf) and as
    last end of 63 (next leaf, leaf, hub): 64 bonds or 189 angle entries in its incidence list."""
    rng = np.random.default_rng(64 + n + int(hub_last))
    dirs = random_chain(65, 7 + n + int(hub_last), step=1.0)                       # consecutive steps: sine >= 0.35
    d = np.diff(dirs, axis=0) * rng.uniform(0.9, 1.3, (64, 1))
    pos = rng.uniform(0, 12, (n, 3))
    hub = n - 1 if hub_last else 0
    leaves = np.arange(64) + (0 if hub_last else 1)
    pos[hub] = (6.0, 6.0, 6.0)
    pos[leaves] = pos[hub] + d
    if kind == BOND:
        top = np.array([[hub, l] if i % 2 == 0 else [l, hub] for i, l in enumerate(leaves)])
    else:
        a, b = leaves[:-1], leaves[1:]
        h = np.full(63, hub)
        top = np.concatenate([np.stack([a, h, b], 1), np.stack([h, a, b], 1), np.stack([b, a, h], 1)])
    return Case("%s star %d hub %d" % ("bond" if kind == BOND else "angle", n, hub), kind, pos, top, (12.0, 12.0, 12.0), seed=n + hub)


def empty_case(kind, n):
    return Case("%s empty %d" % ("bond" if kind == BOND else "angle", n), kind, np.random.default_rng(n).uniform(0, 6, (n, 3)),
                np.zeros((0, 2 if kind == BOND else 3)), (6.0, 6.0, 6.0), seed=n)


ANISO = (3.0, 4.5, 7.0)


def image_case(kind, n=48):
    """Cell (3.0, 4.5, 7.0): a chain of n atoms (step 1.1 < L/2) wrapped into the cell and then unwrapped at random by up to one
    cell, onto [-L/4, 5L/4), so that raw bond components reach beyond +-0.9 L; and, per axis, four terms over dyadic coordinates
    whose first bond vector has a raw component of exactly +L/2, -L/2, +3L/2 and -3L/2 (the single flag leaves the last two at
    +L/2 and -L/2: it folds once)."""
    rng = np.random.default_rng(48 + kind)
    L = np.asarray(ANISO)
    x = np.mod(random_chain(n, 101, start=(1.0, 2.0, 3.0)), L)
    flip = rng.random(x.shape) < 0.5
    x = np.where(flip & (x < 0.25 * L), x + L, np.where(flip & (x >= 0.75 * L), x - L, x))
    top = [chain_rows(kind, n)]
    edge = []
    for a in range(3):
        for half in (0.5, -0.5, 1.5, -1.5):
            q = np.array([0.5, 0.75, 1.25]) + 0.125 * a
            p = q.copy()
            p[a] += half * L[a]
            p[(a + 1) % 3] += 0.25
            r = q + np.array([0.5, -0.75, 0.625])
            m = n + len(edge)
            edge += [p, q, r]
            top.append(np.array([[m, m + 1]] if kind == BOND else [[m, m + 1, m + 2]]))
    return Case("%s images" % ("bond" if kind == BOND else "angle"), kind, np.concatenate([x, np.array(edge)]),
                np.concatenate(top), ANISO, seed=48)


def sweep_case(delta, at_pi, theta0, n=64):
    """n isolated triplets of angle delta (or pi - delta) in random orientations, |b| in [0.8, 1.4], centres in [-1/2, 1/2)^3."""
    rng = np.random.default_rng(int(round(-1000 * np.log10(delta))) + 7 * int(at_pi))
    th = (np.pi - delta) if at_pi else delta
    Q = np.linalg.qr(rng.normal(0, 1, (n, 3, 3)))[0]
    r1, r2 = rng.uniform(0.8, 1.4, (n, 1)), rng.uniform(0.8, 1.4, (n, 1))
    c = rng.uniform(-0.5, 0.5, (n, 3))
    b1 = Q[:, :, 0] * r1
    b2 = (Q[:, :, 0] * np.cos(th) + Q[:, :, 1] * np.sin(th)) * r2
    pos = np.stack([c + b1, c, c + b2], 1).reshape(3 * n, 3)
    return Case("angle %s%g theta0 %.4f" % ("pi-" if at_pi else "", delta, theta0), ANGLE, pos, np.arange(3 * n).reshape(n, 3),
                (16.0, 16.0, 16.0), x0=theta0, seed=n)


SWEEP = (1.0, 0.3, 0.1, 0.03, 0.01, 0.003, 0.001, 3e-4, 1e-4, 1e-5)


def collinear_case(theta0):
    """Five angle rows over dyadic coordinates: b2 = -2 b1 (theta = pi), b2 = b1 / 2 (theta = 0), a right angle, a zero-length
    b1, and a bent row that shares its centre with the first."""
    pos = np.array([[1.0, 1.0, 1.0], [1.5, 1.25, 0.75], [2.5, 1.75, 0.25],            # 0 1 2: b1 = -(.5, .25, -.25), b2 = -2 b1
                    [4.0, 4.0, 4.0], [4.5, 4.5, 4.25], [4.25, 4.25, 4.125],           # 4 3 5: b1 = (.5, .5, .25), b2 = b1 / 2
                    [6.0, 1.0, 1.0], [6.0, 2.0, 1.0], [7.0, 1.0, 1.0],                # 7 6 8: right angle
                    [2.0, 6.0, 6.0], [2.0, 6.0, 6.0], [3.0, 6.0, 6.0],                # 9 10 11: x_9 = x_10
                    [1.5, 2.25, 1.0]])                                                # 12 1 2: bent, centre 1
    top = np.array([[0, 1, 2], [4, 3, 5], [7, 6, 8], [9, 10, 11], [12, 1, 2]])
    return Case("angle collinear theta0 %.4f" % theta0, ANGLE, pos, top, (16.0, 16.0, 16.0), x0=theta0, seed=13)


COLLINEAR_ONLY = [0, 3, 4, 5, 9, 10, 11]          # the atoms of collinear_case whose every term is collinear


def rod_case(dy):
    """16 atoms along x, one apart, alternate atoms displaced by dy in y; theta0 = pi (a stiff chain as it is initialised)."""
    pos = np.zeros((16, 3))
    pos[:, 0] = 1.0 + np.arange(16)
    pos[:, 1] = 4.0 + dy * (np.arange(16) % 2)
    pos[:, 2] = 4.0
    return Case("angle rod dy %g" % dy, ANGLE, pos, chain_rows(ANGLE, 16), (32.0, 32.0, 32.0), x0=PI32, seed=16)
