"""The float64 definitions behind the tests of the Ewald correction for excluded and scaled pairs, as CPU torch (pass float64
tensors; differentiable where stated).

For a list of pairs p = (i, j) of one replica, each with a scale s_p in [0, 1], the splitting parameter alpha,
E1(r) = erf(alpha r) and G(r) = (2 alpha / sqrt(pi)) exp(-alpha^2 r^2):

    chi(r)   = (s - E1) / r
    chi'(r)  = -(s - E1) / r^2 - G / r
    chi''(r) = 2 (s - E1) / r^3 + 2 G / r^2 + 2 alpha^2 G

    U_excl = conversion * sum_{p, every replica} q_i q_j chi_{s_p}(r_ij)

r_ij is the length of d = x_i - x_j re-imaged on the diagonal cell like a bond vector (topology.get_offsets:
d += (-[d >= L/2] + [d < -L/2]) L per component, piecewise constant).  s = 0 removes the erf(alpha r)/r the reciprocal sum
holds for the pair, s = 1 gives the real-space psi of coulomb_ref with shift = "none".  A coincident pair (r == 0) contributes
the limits of the erf part -- chi -> -2 alpha / sqrt(pi), zero gradient, Hessian (4 alpha^3 / (3 sqrt(pi))) times the unit
matrix -- and its s / r part is dropped.  With `group`, the rows of x are replicas of `group` atoms and the pairs index one
replica.

Everything but `energy` is written out as explicit pair sums (no autograd), so that chi' and chi'' are checked against
autograd of `energy` by tests/test_ewald_excl_host.py rather than assumed."""
import math

import numpy as np
import torch

SQRT_PI = math.sqrt(math.pi)


def chi(r, s, alpha):
    """(chi, chi', chi'') at the distances r > 0 for the scales s."""
    E1 = torch.erf(alpha * r)
    G = (2 * alpha / SQRT_PI) * torch.exp(-(alpha * r) ** 2)
    return (s - E1) / r, -(s - E1) / r ** 2 - G / r, 2 * (s - E1) / r ** 3 + 2 * G / r ** 2 + 2 * alpha * alpha * G


def reimage(d, lengths):
    L = torch.as_tensor(np.asarray(lengths, dtype=np.float64)).to(d)
    return d + (-(d.detach() >= 0.5 * L).to(d) + (d.detach() < -0.5 * L).to(d)) * L


def _expand(pairs, scale, N, group):
    """pairs / scales of one replica -> those of all N // group replicas."""
    p = torch.as_tensor(np.asarray(pairs, dtype=np.int64)).reshape(-1, 2)
    g = N if group is None else int(group)
    assert N % g == 0 and (p.numel() == 0 or int(p.max()) < g)
    s = torch.zeros(len(p), dtype=torch.float64) if scale is None else torch.as_tensor(np.asarray(scale, dtype=np.float64)).reshape(-1)
    if s.numel() == 1:
        s = s.expand(len(p))
    R = N // g
    off = (torch.arange(R) * g)[:, None]
    return (p[:, 0][None, :] + off).reshape(-1), (p[:, 1][None, :] + off).reshape(-1), s.repeat(R)


def energy(x, q, pairs, scale, lengths, alpha, conversion=1.0, group=None):
    """U_excl (differentiable in x and q)."""
    i, j, s = _expand(pairs, scale, x.shape[0], group)
    d = reimage(x[i] - x[j], lengths)
    d2 = d.pow(2).sum(-1)
    apart = d2 != 0
    r = torch.where(apart, d2, torch.ones_like(d2)).sqrt()
    c = torch.where(apart, chi(r, s.to(x), alpha)[0], torch.full_like(r, -2 * alpha / SQRT_PI))
    return conversion * (q[i] * q[j] * c).sum()


def evaluate(x, q, pairs, scale, lengths, alpha, conversion=1.0, w=None, group=None):
    """Explicit pair sums in float64: U, grad = dU/dx, pot_i = sum_j q_j chi, and with w: hw = H w, potw_i = sum_j q_j chi'
    rhat_ij.(w_i - w_j); plus the absolute sums A_* of the pair contributions per output component, built from |chi|, |chi'|
    and |chi''| of the pair (not from their cancelling s and erf parts): a float32 evaluation carries a relative error of a few
    ulp on each of the three radial functions, so a pair's error in H w is proportional to
    |q_i q_j| (|chi''| |rhat.a| |rhat_c| + |chi'| / r |a_c - (rhat.a) rhat_c|)."""
    x, q = torch.as_tensor(x).double(), torch.as_tensor(q).double()
    N, cv = x.shape[0], float(conversion)
    i, j, s = _expand(pairs, scale, N, group)
    d = reimage(x[i] - x[j], lengths)
    r = d.pow(2).sum(-1).sqrt()
    zero = r == 0
    rs = torch.where(zero, torch.ones_like(r), r)
    rh = d / rs[:, None]                                                       # (zero for a coincident pair)
    c0, c1, c2 = chi(rs, s, alpha)
    g0 = 2 * alpha / SQRT_PI
    c0 = torch.where(zero, torch.full_like(r, -g0), c0)
    c1 = torch.where(zero, torch.zeros_like(r), c1)
    c1r = torch.where(zero, torch.full_like(r, 4 * alpha ** 3 / (3 * SQRT_PI)), c1 / rs)     # the limit of chi'/r and of chi''
    c2 = torch.where(zero, c1r, c2)
    qq = cv * q[i] * q[j]

    def both(vi, vj, shape):
        out = torch.zeros(shape, dtype=torch.float64)
        out.index_add_(0, i, vi)
        out.index_add_(0, j, vj)
        return out
    out = dict(U=(qq * c0).sum(), A_U=(qq * c0).abs().sum())
    t = (qq * c1)[:, None] * rh
    out["grad"], out["A_grad"] = both(t, -t, (N, 3)), both(t.abs(), t.abs(), (N, 3))
    out["pot"], out["A_pot"] = both(q[j] * c0, q[i] * c0, (N,)), both((q[j] * c0).abs(), (q[i] * c0).abs(), (N,))
    if w is not None:
        w = torch.as_tensor(w).double()
        wij = w[i] - w[j]
        a = (rh * wij).sum(1)
        par, perp = a[:, None] * rh, wij - a[:, None] * rh
        hv = (qq * c2)[:, None] * par + (qq * c1r)[:, None] * perp
        ah = (qq * c2).abs()[:, None] * par.abs() + (qq * c1r).abs()[:, None] * perp.abs()
        out["hw"], out["A_hw"] = both(hv, -hv, (N, 3)), both(ah, ah, (N, 3))
        out["potw"] = both(q[j] * c1 * a, q[i] * c1 * a, (N,))
        out["A_potw"] = both((q[j] * c1 * a).abs(), (q[i] * c1 * a).abs(), (N,))
    return out


class ExclTerm:
    """The correction with the oracle's term protocol (n_theta, reset, energy, force, force_vjp by autograd, like
    ewald_ref.EwaldTerm), with the charges ([n] or [n_types] with `types`) as its parameters."""

    def __init__(self, charges, cell, alpha, pairs, scale=None, types=None, conversion=1.0):
        self.theta = torch.as_tensor(np.asarray(charges, dtype=np.float32)).reshape(-1)
        self.lengths = np.asarray(cell, dtype=np.float32).astype(np.float64).reshape(3)
        self.alpha, self.conversion, self.types = float(alpha), float(conversion), types
        self.pairs, self.scale = np.asarray(pairs, dtype=np.int64).reshape(-1, 2), scale

    @property
    def n_theta(self):
        return self.theta.numel()

    def reset(self, q):
        pass

    def energy(self, q, theta=None):
        th = self.theta.to(q) if theta is None else theta
        qa = th if self.types is None else th[torch.as_tensor(np.asarray(self.types), dtype=torch.long)]
        if q.dtype == torch.float64:
            return energy(q, qa, self.pairs, self.scale, self.lengths, self.alpha, self.conversion)
        return energy(q.double(), qa.double(), self.pairs, self.scale, self.lengths, self.alpha, self.conversion).to(q.dtype)

    def force(self, q):
        with torch.enable_grad():
            x = q.detach().requires_grad_(True)
            (g,) = torch.autograd.grad(self.energy(x), x)
        return -g

    def force_vjp(self, q, w):
        with torch.enable_grad():
            x = q.detach().requires_grad_(True)
            th = self.theta.to(q).detach().requires_grad_(True)
            (g,) = torch.autograd.grad(self.energy(x, th), x, create_graph=True)
            dq, dth = torch.autograd.grad((w.detach() * (-g)).sum(), (x, th))
        return (-g).detach(), dq.detach(), dth.detach()


# ------------------------------------------------------------------------------------------------ test systems
def water27(seed=27, L=9.3, jitter=0.05):
    """(x float32 [81, 3], cell float32 [3], q float32 [81], types int64 [81], pairs int64 [81, 2], bonds [54, 2], angles
    [27, 3]): 27 three-site molecules on a 3 x 3 x 3 grid of spacing L / 3, centred at (n + 0.5) L / 3.  Template: O at the
    origin, H at (1, 0, 0) and (cos 109.47, sin 109.47, 0), each molecule rotated by the Q factor of a QR of a
    default_rng(seed) normal 3 x 3 matrix; normal jitter, positions wrapped into the box and cast to float32.  Charges
    -0.82 / +0.41; the 81 intramolecular pairs (O-H, O-H, H-H) are the excluded ones.  81 atoms: no multiple of the wave."""
    rng = np.random.default_rng(seed)
    th = math.radians(109.47)
    tmpl = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [math.cos(th), math.sin(th), 0.0]])
    pos = []
    for n in np.ndindex(3, 3, 3):
        Q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
        pos.append((np.asarray(n) + 0.5) * (L / 3) + tmpl @ Q.T + rng.normal(0, jitter, (3, 3)))   # (drawn molecule by molecule)
    pos = np.mod(np.concatenate(pos), L).astype(np.float32)
    o = 3 * np.arange(27)
    pairs = np.stack([np.stack([o, o + 1], 1), np.stack([o, o + 2], 1), np.stack([o + 1, o + 2], 1)], 1).reshape(-1, 2)
    bonds = np.stack([np.stack([o, o + 1], 1), np.stack([o, o + 2], 1)], 1).reshape(-1, 2)
    angles = np.stack([o + 1, o, o + 2], 1)
    types = np.tile(np.array([0, 1, 1], dtype=np.int64), 27)
    q = np.where(types == 0, -0.82, 0.41).astype(np.float32)
    return pos, np.array([L, L, L], dtype=np.float32), q, types, pairs.astype(np.int64), bonds.astype(np.int64), angles.astype(np.int64)
