"""The float64 definition behind the Sutton-Chen tests, as CPU torch (pass float64 tensors; differentiable where stated).

For one species with theta = (epsilon, a, c) and the constants k = (n, m, rc, shift):

    U      = sum_i [ 1/2 sum_{j != i} phi(r_ij) - epsilon c sqrt(rho_i) ],   rho_i = sum_{j != i} f(r_ij)
    phi(r) = epsilon S_n(r),   f(r) = S_m(r)
    S_k(r) = (a/r)^k - (a/rc)^k + k (r - rc) (a/rc)^k / rc     r < rc, else 0     (shift = "force")
    S_k(r) = (a/r)^k                                            r < rc, else 0     (shift = "none")

An atom with rho_i = 0 has no embedding energy and F'(rho_i) = F''(rho_i) = 0 (F = -epsilon c sqrt(rho)).  The pairs are those
of coulomb_ref.half_list (generate_nbr_list, torchmd/topology.py:30-73) at the cutoff rc.

`energy` is the definition; `evaluate` differentiates it with float64 autograd.  The error scales A_* that `evaluate` returns
are the float64 sums of the absolute values of what a float32 evaluation adds up, in closed form:

  * S_k is three pieces, (a/r)^k, -(a/rc)^k and k (r - rc) (a/rc)^k / rc, that cancel towards the cutoff; each carries its own
    rounding, so a pair counts with the sum of their absolute values (one piece for shift = "none"), and S_k' = -k (a/r)^k / r
    + k (a/rc)^k / rc with both of its pieces.
  * The embedding contributions are conditioned through rho_i.  The float32 error of rho_i is a few ulp of
    A_rho_i = sum_j (|(a/r)^m| + |(a/rc)^m| + |m (r - rc) (a/rc)^m / rc|), relative to rho_i an amplification
    kappa_i = A_rho_i / rho_i >= 1 (exactly 1 for shift = "none").  F, F' and F'' are powers of rho_i, so their relative error
    is that of rho_i times 1/2, 1/2 and 3/2: every embedding contribution's scale is multiplied by kappa of the atom whose
    F' (F, F'') it carries.
  * d rho_i = sum_j S_m'(r_ij) e_ij.(w_j - w_i) (the directional derivative of rho_i along w) is a sum of either sign; it counts
    with A_drho_i = sum_j (|pieces of S_m'|) |e_ij.(w_j - w_i)|, and F''(rho_i) d rho_i with |F''| kappa_i A_drho_i.

With these the kernel tolerance is the project's 64 * 2^-24 * A."""
import numpy as np
import torch

import coulomb_ref as C

# (epsilon / eV, a / Angstrom, c, n, m) of Sutton and Chen 1990
PUBLISHED = {"copper": (1.2382e-2, 3.61, 39.432, 9, 6), "nickel": (1.5707e-2, 3.52, 39.432, 9, 6),
             "silver": (2.5415e-3, 4.09, 144.41, 12, 6), "gold": (1.2793e-2, 4.08, 34.408, 10, 8)}


def consts(n, m, rc, shift="force"):
    assert shift in ("force", "none")
    return dict(n=int(n), m=int(m), rc=float(rc), shift=shift)


def pairs(x, cell, rc, group=None):
    """dict(i, j, off: the half list at rc; rows: the row lengths; margin: see coulomb_ref.half_list)."""
    i, j, off, margin = C.half_list(x, cell, rc, group=group)
    N = int(torch.as_tensor(x).shape[0])
    rows = torch.bincount(torch.cat([i, j]), minlength=N)
    return dict(i=i, j=j, off=off, rows=rows, margin=margin)


def shape(r, a, kk, k):
    """S_kk(r) for r inside the support (the list holds no other pair)."""
    s = (a / r) ** kk
    if k["shift"] == "none":
        return s
    q = (a / k["rc"]) ** kk
    return s - q + kk * (r - k["rc"]) * q / k["rc"]


def _root(rho):
    """sqrt(rho) with the rho = 0 rule: exactly 0 there, with zero derivatives."""
    dense = rho > 0
    return torch.where(dense, rho, torch.ones_like(rho)).sqrt() * dense.to(rho)


def density(x, a, lst, cell, k):
    d = x[lst["i"]] - x[lst["j"]] - lst["off"].to(x).matmul(C.cell_matrix(cell).to(x))
    r = d.pow(2).sum(-1).sqrt()
    f = shape(r, a, k["m"], k)
    rho = x.new_zeros(x.shape[0]).index_add(0, torch.cat([lst["i"], lst["j"]]), torch.cat([f, f]))
    return r, rho


def energy(x, theta, lst, cell, k, parts=False):
    """U (differentiable in x and theta = (epsilon, a, c)) on lst = pairs(...)."""
    eps, a, c = theta[0], theta[1], theta[2]
    r, rho = density(x, a, lst, cell, k)
    up, ue = eps * shape(r, a, k["n"], k).sum(), -eps * c * _root(rho).sum()
    return (up, ue) if parts else up + ue


def _scales(x, theta, lst, cell, k, w):
    """The A_* of the module docstring, in closed form over the directed entries (i <- j) of every row."""
    eps, a, c = (float(t) for t in theta)
    n, m, rc, shifted = k["n"], k["m"], k["rc"], k["shift"] == "force"
    N = x.shape[0]
    h = C.cell_matrix(cell).double()
    d = x[lst["i"]] - x[lst["j"]] - lst["off"].double().matmul(h)                   # x_i - x_j
    I, J = torch.cat([lst["i"], lst["j"]]), torch.cat([lst["j"], lst["i"]])
    u = torch.cat([-d, d])                                                           # centre I -> end J
    r = u.pow(2).sum(-1).sqrt()
    e = u / r[:, None]

    def pieces(kk):
        s, q = (a / r) ** kk, (a / rc) ** kk if shifted else 0.0
        aS = s + q + (kk * (rc - r) * q / rc if shifted else 0.0)                   # |pieces of S|
        aD = kk * s / r + kk * q / rc                                                # |pieces of S'|
        aH = kk * (kk + 1) * s / r ** 2                                              # |S''|
        S = s - q + (kk * (r - rc) * q / rc if shifted else 0.0)
        return S, aS, aD, aH
    Sn, aSn, aDn, aHn = pieces(n)
    Sm, aSm, aDm, aHm = pieces(m)
    zeros = lambda *sh: torch.zeros(*sh, dtype=torch.float64)
    per_atom = lambda v: zeros(N).index_add(0, I, v)
    rho, A_rho = per_atom(Sm), per_atom(aSm)
    dense = rho > 0
    safe = torch.where(dense, rho, torch.ones_like(rho))
    kappa = torch.where(dense, A_rho / safe, torch.ones_like(rho))
    root = safe.sqrt() * dense
    aF = eps * c * root * kappa                                                      # |F| kappa
    aF1 = eps * c / (2 * safe.sqrt()) * dense * kappa                                # |F'| kappa
    aF2 = eps * c / (4 * safe ** 1.5) * dense * kappa                                # |F''| kappa
    sumSn = per_atom(aSn)
    out = dict(kappa=kappa, rho=rho)
    out["A_U"] = (0.5 * eps * sumSn + aF).sum()
    lin = eps * aDn + (aF1[I] + aF1[J]) * aDm                                        # |dU/dr| of an entry, piece by piece
    out["A_grad"] = zeros(N, 3).index_add(0, I, lin[:, None] * e.abs())
    out["A_dth"] = torch.stack([out["A_U"] / eps, (0.5 * n * eps * sumSn + m * rho * aF1).sum() / a, (eps * root * kappa).sum()])
    if w is not None:
        dw = w[J] - w[I]
        rdot = (e * dw).sum(-1)
        edot = (dw - e * rdot[:, None]) / r[:, None]
        A_drho = per_atom(aDm * rdot.abs())
        curv = eps * aHn + (aF1[I] + aF1[J]) * aHm
        emb2 = (aF2[I] * A_drho[I] + aF2[J] * A_drho[J]) * aDm
        out["A_hw"] = zeros(N, 3).index_add(0, I, (curv * rdot.abs() + emb2)[:, None] * e.abs() + lin[:, None] * edot.abs())
        pair_w = per_atom(aDn * rdot.abs())                                          # sum_j |pieces of S_n'| |rdot|
        out["A_dthw"] = torch.stack([(0.5 * eps * pair_w + aF1 * A_drho).sum() / eps,
                                     (0.5 * n * eps * pair_w + 1.5 * m * aF1 * A_drho).sum() / a,
                                     (eps / (2 * safe.sqrt()) * dense * kappa * A_drho).sum()])
    return out


def evaluate(x, theta, lst, cell, k, w=None):
    """float64 autograd of `energy`: U, grad = dU/dx, dth = dU/dtheta, and with w: hw = H w, dthw = d(w.dU/dx)/dtheta; plus
    A_U, A_grad, A_dth, A_hw, A_dthw (module docstring), and kappa, rho per atom."""
    x = torch.as_tensor(x).detach().double()
    theta = (theta.detach() if torch.is_tensor(theta) else torch.tensor(np.asarray(theta, dtype=np.float64))).double().reshape(3)
    xg, tg = x.clone().requires_grad_(True), theta.clone().requires_grad_(True)
    U = energy(xg, tg, lst, cell, k)
    g, gt = torch.autograd.grad(U, (xg, tg), create_graph=w is not None)
    out = dict(U=U.detach(), grad=g.detach(), dth=gt.detach())
    if w is not None:
        w = torch.as_tensor(w).detach().double()
        hw, hth = torch.autograd.grad((g * w).sum(), (xg, tg))
        out["hw"], out["dthw"] = hw, hth
    out.update(_scales(x, theta, lst, cell, k, w))
    return out


def energy_loops(x, theta, cell, k, group=None):
    """The same energy as plain Python loops over every ordered pair with the minimum image taken per vector -- written
    separately from everything above.  Returns (pair part, embedding part)."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(cell, dtype=np.float64)
    h = np.diag(h) if h.ndim == 1 else h
    hinv = np.linalg.inv(h)
    eps, a, c = (float(t) for t in theta)
    rc, n, m = k["rc"], k["n"], k["m"]
    N = x.shape[0]
    g = N if group is None else group

    def S(r, kk):
        v = (a / r) ** kk
        if k["shift"] == "force":
            v += -(a / rc) ** kk + kk * (r - rc) * (a / rc) ** kk / rc
        return v
    up = ue = 0.0
    for i in range(N):
        lo = (i // g) * g
        rho = 0.0
        for j in range(lo, lo + g):
            if j == i:
                continue
            v = x[j] - x[i]
            s = v @ hinv
            v = v + (-(s > 0.5).astype(float) + (s < -0.5).astype(float)) @ h
            r = float(np.sqrt((v ** 2).sum()))
            if r < rc and r != 0.0:
                up += 0.5 * eps * S(r, n)
                rho += S(r, m)
        if rho > 0.0:
            ue -= eps * c * np.sqrt(rho)
    return up, ue


def fcc_sums(n, m, a0=1.0, a=1.0, rc=None, reach=40.0):
    """(S_n, S_m, number of sites) with S_k = sum over the fcc lattice (cube edge a0) of (a/r)^k: truncated at rc when given, otherwise summed to
    `reach` a0 with the integral tail 4 pi rho_N a^k R^(3-k) / (k - 3), rho_N = 4 / a0^3."""
    R = reach * a0 if rc is None else rc
    M = int(np.ceil(R / a0)) + 1
    g = np.arange(-M, M + 1, dtype=np.float64)
    base = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    out, r2s = [], []
    for b in ([0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]):
        r2 = ((base + np.array(b)) ** 2).sum(1) * a0 * a0
        r2s.append(r2[(r2 > 1e-12) & ((r2 < R * R) if rc is not None else (r2 <= R * R))])
    r = np.sqrt(np.sort(np.concatenate(r2s)))
    for kk in (n, m):
        s = float(((a / r[::-1]) ** kk).sum())                   # (small terms first)
        if rc is None:
            s += 4 * np.pi * (4.0 / a0 ** 3) * a ** kk * R ** (3 - kk) / (kk - 3)
        out.append(s)
    return out[0], out[1], r.size


def jittered_fcc(cells=3, a0=3.61, jit=0.15, seed=108):
    """(float32 positions, float32 cell) of an fcc lattice of cells^3 conventional cells jittered by jit."""
    import oracle as O
    pos, cell = O.fcc_lattice(cells, a0)
    rng = np.random.default_rng(seed)
    x = np.mod(pos + rng.normal(0, jit, pos.shape), cell) if jit else pos
    return x.astype(np.float32), np.asarray(cell).astype(np.float32)


class SCTerm:
    """The Sutton-Chen term with the oracle's term protocol (n_theta, reset, energy, force, force_vjp by autograd, like
    sw_ref.SWTerm) and theta = (epsilon, a, c): force_vjp's third output is d(w.F)/dtheta.  The pairs are those of the last
    reset(q), searched at rc."""

    def __init__(self, epsilon, a, c, n, m, rc, cell, shift="force", group=None):
        self.theta = torch.tensor([epsilon, a, c], dtype=torch.float32)
        self.k = consts(n, m, rc, shift)
        self.cell = np.asarray(cell, dtype=np.float32)
        self.group = group
        self.lst = None

    @property
    def n_theta(self):
        return 3

    def reset(self, q):
        self.lst = pairs(q.detach(), self.cell, self.k["rc"], group=self.group)

    def energy(self, q, theta=None):
        return energy(q, self.theta.to(q) if theta is None else theta, self.lst, self.cell, self.k)

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
