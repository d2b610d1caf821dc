"""The float64 definitions behind the Ewald reciprocal-space tests, as CPU torch (pass float64 tensors; differentiable where
stated).

For one replica on a diagonal cell L = (Lx, Ly, Lz), V = Lx Ly Lz, charges q_i, splitting parameter alpha and the wave
vectors k(n) = 2 pi (nx / Lx, ny / Ly, nz / Lz), integer n != 0 with |k| <= k_cutoff, of the half space of
observable.sk_vectors (nx > 0, or nx = 0 and ny > 0, or nx = ny = 0 and nz > 0; k and -k contribute equally):

    rho(k) = A + iB = sum_j q_j exp(i k.x_j)
    c(k)   = (4 pi / V) exp(-k^2 / (4 alpha^2)) / k^2
    U_rec  = conversion * [ sum_k c(k) |rho(k)|^2  -  pi (sum_j q_j)^2 / (2 V alpha^2) ]

The second term is the neutralising background.  The self term -alpha / sqrt(pi) sum q_i^2 belongs to the real-space sum
(coulomb_ref.consts with shift = "none" and self energy): the two together are the Ewald energy.  With `group`, the rows of x
are replicas of `group` atoms; every replica has its own modes and the energies add.

Everything but `energy` is written out as explicit mode sums (no autograd), so that the derivative formulas of the kernel
are checked against autograd of `energy` by tests/test_ewald_host.py rather than assumed."""
import math

import numpy as np
import torch

MAX_INDEX = 1024


def vectors(lengths, k_cutoff):
    """(n int64 [M, 3], |k|^2 float64 [M]) of the half space with |k| <= k_cutoff, sorted by |k|^2 and then by (nx, ny, nz)."""
    L = np.asarray(lengths, dtype=np.float64).reshape(3)
    nmax = np.floor(float(k_cutoff) * L / (2 * np.pi)).astype(np.int64)
    ax = [np.arange(0, nmax[0] + 1), np.arange(-nmax[1], nmax[1] + 1), np.arange(-nmax[2], nmax[2] + 1)]
    n = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    half = (n[:, 0] > 0) | ((n[:, 0] == 0) & ((n[:, 1] > 0) | ((n[:, 1] == 0) & (n[:, 2] > 0))))
    n = n[half]
    k2 = ((2 * np.pi * n / L) ** 2).sum(1)
    keep = k2 <= float(k_cutoff) ** 2
    n, k2 = n[keep], k2[keep]
    order = np.lexsort((n[:, 2], n[:, 1], n[:, 0], k2))
    return n[order], k2[order]


def coef(k2, volume, alpha):
    k2 = torch.as_tensor(k2, dtype=torch.float64)
    return (4 * math.pi / volume) * torch.exp(-k2 / (4 * alpha * alpha)) / k2


def _modes(x, n, lengths):
    L = torch.as_tensor(np.asarray(lengths, dtype=np.float64))
    k = 2 * math.pi * torch.as_tensor(np.asarray(n), dtype=torch.float64) / L            # [M, 3]
    ph = x.matmul(k.t())                                                                  # [N, M]
    return k, torch.cos(ph), torch.sin(ph)


def energy(x, q, n, lengths, alpha, conversion=1.0, group=None, background=True):
    """U_rec (differentiable in x and q)."""
    N = x.shape[0]
    g = N if group is None else int(group)
    V = float(np.prod(np.asarray(lengths, dtype=np.float64)))
    k, c, s = _modes(x, n, lengths)
    cf = coef((k * k).sum(1), V, alpha)
    A = (q[:, None] * c).reshape(N // g, g, -1).sum(1)
    B = (q[:, None] * s).reshape(N // g, g, -1).sum(1)
    U = (cf * (A * A + B * B)).sum()
    if background:
        U = U - math.pi * q.reshape(N // g, g).sum(1).pow(2).sum() / (2 * V * alpha * alpha)
    return conversion * U


def evaluate(x, q, n, lengths, alpha, conversion=1.0, w=None, group=None):
    """Explicit mode sums in float64: U, grad = dU/dx, pot_i = sum_k 2 c (A c_i + B s_i), dq = dU/dq_i =
    conversion (pot_i - pi Q / (V alpha^2)), and with w: hw = H w, potw_i = d(w.dU/dx)/dq_i / conversion; plus the scales
    A_* per output component: the same sums with every product replaced by its absolute value and the mode amplitudes
    |rho|, |sigma| by the absolute sums S = sum_j |q_j|, Sw(k) = sum_j |q_j| |k.w_j| -- a float32 mode sum errs in proportion to
    the absolute sum, not to |rho|."""
    x, q = torch.as_tensor(x).double(), torch.as_tensor(q).double()
    N, cv = x.shape[0], float(conversion)
    g = N if group is None else int(group)
    R = N // g
    V = float(np.prod(np.asarray(lengths, dtype=np.float64)))
    k, c, s = _modes(x, n, lengths)
    cf = coef((k * k).sum(1), V, alpha)                                                   # [M]
    ac, as_ = c.abs(), s.abs()

    def per_rep(v):                     # [N, M] -> the replica's sum, back on every atom of it
        return v.reshape(R, g, -1).sum(1).repeat_interleave(g, 0)
    A, B = per_rep(q[:, None] * c), per_rep(q[:, None] * s)
    S = per_rep(q.abs()[:, None].expand(N, 1))                                            # [N, 1]
    Q = per_rep(q[:, None].expand(N, 1))
    bg = math.pi / (V * alpha * alpha)
    out = dict(U=cv * ((cf * (A * A + B * B)).sum() / g - 0.5 * bg * (Q * Q).sum() / g),
               A_U=cv * ((cf * (S * S)).sum() / g + 0.5 * bg * (S * S).sum() / g))
    P, Qm = A * c + B * s, B * c - A * s
    aP = S * (ac + as_)
    t = (2 * cv) * q[:, None] * cf * Qm
    out["grad"] = t.matmul(k)
    out["A_grad"] = ((2 * cv) * q.abs()[:, None] * cf * aP).matmul(k.abs())
    out["pot"], out["A_pot"] = (2 * cf * P).sum(1), (2 * cf * aP).sum(1)
    out["dq"] = cv * (out["pot"] - bg * Q[:, 0])
    out["A_dq"] = cv * (out["A_pot"] + bg * S[:, 0])
    if w is not None:
        w = torch.as_tensor(w).double()
        kw = w.matmul(k.t())                                                              # [N, M]
        Sr, Si = per_rep(q[:, None] * kw * c), per_rep(q[:, None] * kw * s)
        Sw = per_rep(q.abs()[:, None] * kw.abs())
        T = Sr * c + Si * s - kw * P
        aT = Sw * (ac + as_) + kw.abs() * aP
        out["hw"] = ((2 * cv) * q[:, None] * cf * T).matmul(k)
        out["A_hw"] = ((2 * cv) * q.abs()[:, None] * cf * aT).matmul(k.abs())
        out["potw"] = (2 * cf * (kw * Qm + Sr * s - Si * c)).sum(1)
        out["A_potw"] = (2 * cf * aT).sum(1)
    return out


class EwaldTerm:
    """The reciprocal term with the oracle's term protocol (n_theta, reset, energy, force, force_vjp by autograd, like
    coulomb_ref.CoulombTerm), with the charges ([n] or [n_types] with `types`) as its parameters."""

    def __init__(self, charges, cell, alpha, k_cutoff, types=None, conversion=1.0):
        self.theta = torch.as_tensor(np.asarray(charges, dtype=np.float32)).reshape(-1)
        self.lengths = np.asarray(cell, dtype=np.float32).astype(np.float64).reshape(3)
        self.alpha, self.conversion, self.types = float(alpha), float(conversion), types
        self.n = vectors(self.lengths, k_cutoff)[0]

    @property
    def n_theta(self):
        return self.theta.numel()

    def reset(self, q):
        pass

    def energy(self, q, theta=None):
        th = self.theta.to(q) if theta is None else theta
        qa = th if self.types is None else th[torch.as_tensor(np.asarray(self.types), dtype=torch.long)]
        if q.dtype == torch.float64:
            return energy(q, qa, self.n, self.lengths, self.alpha, self.conversion)
        return energy(q.double(), qa.double(), self.n, self.lengths, self.alpha, self.conversion).to(q.dtype)

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
def jittered_nacl64(seed=64, sigma=0.25):
    """(x float32 [64, 3], cell float32 [3], q float32 [64]): the recipe of test_gpu_coulomb._jittered_nacl64."""
    import coulomb_ref as R
    pos, q, L = R.nacl(2)
    rng = np.random.default_rng(seed)
    x32 = np.mod(pos + rng.normal(0, sigma, pos.shape), L).astype(np.float32)
    return x32, np.array([L, L, L], dtype=np.float32), q.astype(np.float32)


def gas37(zero=True):
    """(x float32 [37, 3], box float32 [3], q float32 [37]): positions and charges of test_gpu_coulomb._gas37 -- 37 seeded
    atoms in a 7 x 8 x 9 box with normal charges, net charge -1.30; zero: charge 5 set to zero as there (net -1.17)."""
    import coulomb_ref as R
    box = np.array([7.0, 8.0, 9.0], dtype=np.float32)
    x32 = R.seeded_gas(37, box, 0.8, seed=37).astype(np.float32)
    q32 = np.random.default_rng(370).normal(0, 1, 37).astype(np.float32)
    if zero:
        q32[5] = 0.0
    return x32, box, q32
