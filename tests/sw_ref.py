"""The float64 definition behind the Stillinger-Weber tests, as CPU torch (pass float64 tensors; differentiable where stated).

For one species with theta = (epsilon, sigma, lam) and the constants k = (a, gamma, cos0, A, B, p, q), rc = a sigma:

    U    = sum_{i<j} phi2(r_ij) + sum_i sum_{j<k in row(i)} phi3(r_ij, r_ik, cos theta_jik)
    phi2 = A eps [B (sigma/r)^p - (sigma/r)^q] exp(sigma / (r - a sigma))                    r < a sigma, else 0
    phi3 = lam eps (cos theta - cos0)^2 exp(gamma sigma/(r_ij - a sigma)) exp(gamma sigma/(r_ik - a sigma))

The pairs are those of coulomb_ref.half_list (generate_nbr_list, torchmd/topology.py:30-73) at the cutoff rc; row(i) holds
every pair that atom i is part of, and the triplets are the unordered pairs of entries of one row.

`energy` is the definition.  `evaluate` differentiates it with float64 autograd and, for the error scales, evaluates every
pair and every triplet on its own gathered copies of the positions and parameters: the derivative with respect to such a
copy is that one term's contribution, and the scales are the explicit sums of their absolute values."""
import numpy as np
import torch

import coulomb_ref as C

SILICON = dict(epsilon=2.1683, sigma=2.0951, lam=21.0)
KCAL_PER_MOL = 4184.0 / (1.602176634e-19 * 6.02214076e23)          # eV
MW = dict(epsilon=6.189 * KCAL_PER_MOL, sigma=2.3925, lam=23.15)


def consts(a=1.80, gamma=1.20, cos0=-1.0 / 3.0, A=7.049556277, B=0.6022245584, p=4, q=0):
    return dict(a=float(a), gamma=float(gamma), cos0=float(cos0), A=float(A), B=float(B), p=int(p), q=int(q))


def pairs_and_triplets(x, cell, rc, group=None):
    """dict(i, j, off: the half list at rc; tc, ta, tb, oa, ob: centre, the two end atoms and the image offsets of
    x_end - x_centre of every triplet; rows: the row lengths; margin: see coulomb_ref.half_list)."""
    i, j, off, margin = C.half_list(x, cell, rc, group=group)
    N = int(torch.as_tensor(x).shape[0])
    rows = [[] for _ in range(N)]
    for p in range(i.numel()):
        a, b = int(i[p]), int(j[p])
        rows[a].append((b, off[p]))                 # d = x_i - x_j - off.h  =>  x_j - x_i + off.h points from i to j
        rows[b].append((a, -off[p]))
    tc, ta, tb, oa, ob = [], [], [], [], []
    for c, row in enumerate(rows):
        for m in range(len(row)):
            for n in range(m + 1, len(row)):
                tc.append(c), ta.append(row[m][0]), tb.append(row[n][0]), oa.append(row[m][1]), ob.append(row[n][1])
    idx = lambda v: torch.tensor(v, dtype=torch.long)
    offs = lambda v: torch.stack(v) if v else torch.zeros(0, 3, dtype=torch.float64)
    return dict(i=i, j=j, off=off, tc=idx(tc), ta=idx(ta), tb=idx(tb), oa=offs(oa), ob=offs(ob),
                rows=torch.tensor([len(r) for r in rows]), margin=margin)


def _cut(r, rc):
    """(inside, r - rc made safe outside the support)."""
    inside = r < rc
    return inside, torch.where(inside, r - rc, -torch.ones_like(r))


def phi2(d, eps, sig, k):
    """Pair energies for the separation vectors d [P, 3]; eps, sig scalars or [P]."""
    r = d.pow(2).sum(-1).sqrt()
    inside, dr = _cut(r, k["a"] * sig)
    s = sig / r
    v = k["A"] * eps * (k["B"] * s ** k["p"] - s ** k["q"]) * torch.exp(sig / dr)
    return torch.where(inside, v, torch.zeros_like(v))


def phi3(ua, ub, eps, sig, lam, k):
    """Triplet energies for the vectors centre -> end ua, ub [T, 3]."""
    ra, rb = ua.pow(2).sum(-1).sqrt(), ub.pow(2).sum(-1).sqrt()
    ia, da = _cut(ra, k["a"] * sig)
    ib, db = _cut(rb, k["a"] * sig)
    c = (ua * ub).sum(-1) / (ra * rb)
    v = lam * eps * (c - k["cos0"]) ** 2 * torch.exp(k["gamma"] * sig / da) * torch.exp(k["gamma"] * sig / db)
    return torch.where(ia & ib, v, torch.zeros_like(v))


def _vectors(x, lst, cell):
    h = C.cell_matrix(cell).to(x)
    d = x[lst["i"]] - x[lst["j"]] - lst["off"].to(x).matmul(h)
    ua = x[lst["ta"]] - x[lst["tc"]] + lst["oa"].to(x).matmul(h)
    ub = x[lst["tb"]] - x[lst["tc"]] + lst["ob"].to(x).matmul(h)
    return d, ua, ub


def energy(x, theta, lst, cell, k, parts=False):
    """U (differentiable in x and theta = (epsilon, sigma, lam)) on lst = pairs_and_triplets(...)."""
    eps, sig, lam = theta[0], theta[1], theta[2]
    d, ua, ub = _vectors(x, lst, cell)
    u2, u3 = phi2(d, eps, sig, k).sum(), phi3(ua, ub, eps, sig, lam, k).sum()
    return (u2, u3) if parts else u2 + u3


def evaluate(x, theta, lst, cell, k, w=None):
    """float64 autograd of `energy`: U, grad = dU/dx, dth = dU/dtheta, and with w: hw = H w, dthw = d(w.dU/dx)/dtheta; plus
    A_U, A_grad, A_dth, A_hw, A_dthw, the sums of the absolute pair and triplet contributions to every component."""
    x = torch.as_tensor(x).detach().double()
    theta = torch.as_tensor(theta).detach().double().reshape(3)
    N = x.shape[0]
    xg, tg = x.clone().requires_grad_(True), theta.clone().requires_grad_(True)
    U = energy(xg, tg, lst, cell, k)
    g, gt = torch.autograd.grad(U, (xg, tg), create_graph=w is not None)
    out = dict(U=U.detach(), grad=g.detach(), dth=gt.detach())
    if w is not None:
        w = torch.as_tensor(w).detach().double()
        hw, hth = torch.autograd.grad((g * w).sum(), (xg, tg))
        out["hw"], out["dthw"] = hw, hth
    # ---- scales: every term on its own copies of its atoms' positions and of theta
    h = C.cell_matrix(cell).double()
    P, Tn = lst["i"].numel(), lst["tc"].numel()
    A_grad, A_hw = torch.zeros(N, 3, dtype=torch.float64), torch.zeros(N, 3, dtype=torch.float64)
    A_dth, A_dthw, A_U = torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    groups = [((lst["i"], lst["j"]), P), ((lst["tc"], lst["ta"], lst["tb"]), Tn)]
    for kind, (atoms, n) in enumerate(groups):
        if n == 0:
            continue
        X = [x[a].clone().requires_grad_(True) for a in atoms]
        th = theta[None, :].repeat(n, 1).requires_grad_(True)
        if kind == 0:
            v = phi2(X[0] - X[1] - lst["off"].double().matmul(h), th[:, 0], th[:, 1], k)
        else:
            v = phi3(X[1] - X[0] + lst["oa"].double().matmul(h), X[2] - X[0] + lst["ob"].double().matmul(h),
                     th[:, 0], th[:, 1], th[:, 2], k)
        A_U = A_U + v.detach().abs().sum()
        gs = torch.autograd.grad(v.sum(), X + [th], create_graph=w is not None, allow_unused=True)
        for a, ga in zip(atoms, gs[:-1]):
            A_grad.index_add_(0, a, ga.detach().abs())
        gth = gs[-1] if gs[-1] is not None else torch.zeros_like(th)
        A_dth += gth.detach().abs().sum(0)
        if w is not None:
            s = sum((ga * w[a]).sum() for a, ga in zip(atoms, gs[:-1]))
            hs = torch.autograd.grad(s, X + [th], allow_unused=True)
            for a, ha in zip(atoms, hs[:-1]):
                A_hw.index_add_(0, a, ha.abs())
            if hs[-1] is not None:
                A_dthw += hs[-1].abs().sum(0)
    out.update(A_U=A_U, A_grad=A_grad, A_dth=A_dth)
    if w is not None:
        out.update(A_hw=A_hw, A_dthw=A_dthw)
    return out


def energy_loops(x, theta, cell, k, group=None):
    """The same energy as plain numpy loops over every pair and every ordered (centre; j < k) triple with the minimum image
    taken per vector -- written separately from everything above."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(cell, dtype=np.float64)
    h = np.diag(h) if h.ndim == 1 else h
    hinv = np.linalg.inv(h)
    eps, sig, lam = (float(t) for t in theta)
    rc = k["a"] * sig
    N = x.shape[0]
    n = N if group is None else group

    def image(v):
        s = v @ hinv
        return v + (-(s > 0.5).astype(float) + (s < -0.5).astype(float)) @ h
    U2 = U3 = 0.0
    for c in range(N):
        lo = (c // n) * n
        vec = []
        for e in range(lo, lo + n):
            if e == c:
                continue
            v = image(x[e] - x[c])
            r = float(np.sqrt((v ** 2).sum()))
            if r < rc and r != 0.0:
                vec.append((v, r))
                if e > c:
                    s = sig / r
                    U2 += k["A"] * eps * (k["B"] * s ** k["p"] - s ** k["q"]) * np.exp(sig / (r - rc))
        for m in range(len(vec)):
            for o in range(m + 1, len(vec)):
                (va, ra), (vb, rb) = vec[m], vec[o]
                c_ = float(va @ vb) / (ra * rb)
                U3 += lam * eps * (c_ - k["cos0"]) ** 2 * np.exp(k["gamma"] * sig / (ra - rc)) * np.exp(k["gamma"] * sig / (rb - rc))
    return U2, U3


def jittered_diamond(cells=2, a0=5.431, sigma_jit=0.3, seed=64):
    """(float32 positions, float32 cell) of a diamond lattice of cells^3 conventional cells jittered by sigma_jit."""
    import oracle as O
    pos, cell = O.diamond_lattice(cells, a0)
    rng = np.random.default_rng(seed)
    x = np.mod(pos + rng.normal(0, sigma_jit, pos.shape), cell) if sigma_jit else pos
    return x.astype(np.float32), cell.astype(np.float32)


class SWTerm:
    """The Stillinger-Weber term with the oracle's term protocol (n_theta, reset, energy, force, force_vjp by autograd, like
    coulomb_ref.CoulombTerm) and theta = (epsilon, sigma, lam): force_vjp's third output is d(w.F)/dtheta.  The pairs and
    triplets are those of the last reset(q), searched at a sigma."""

    def __init__(self, epsilon, sigma, lam, cell, group=None, **k):
        self.theta = torch.tensor([epsilon, sigma, lam], dtype=torch.float32)
        self.k = consts(**k)
        self.cell = np.asarray(cell, dtype=np.float32)
        self.group = group
        self.lst = None

    @property
    def n_theta(self):
        return 3

    def reset(self, q):
        self.lst = pairs_and_triplets(q.detach(), self.cell, self.k["a"] * float(self.theta[1]), group=self.group)

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
