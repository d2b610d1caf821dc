"""The float64 definitions behind the Coulomb tests, as CPU torch (pass float64 tensors; differentiable where stated).

For charges q_i, cutoff rc, damping alpha >= 0, E(r) = erfc(alpha r), G(r) = (2 alpha / sqrt(pi)) exp(-alpha^2 r^2):

    psi(r)   = E(r)/r - c0 + c1 (r - rc)
    psi'(r)  = -E/r^2 - G/r + c1
    psi''(r) = 2E/r^3 + 2G/r^2 + 2 alpha^2 G

    shift = "none":       c0 = 0,         c1 = 0
    shift = "potential":  c0 = E(rc)/rc,  c1 = 0
    shift = "force":      c0 = E(rc)/rc,  c1 = E(rc)/rc^2 + G(rc)/rc

    U = conversion * [ sum_{pairs i<j} q_i q_j psi(r_ij)  -  s sum_i q_i^2 ],   s = c0/2 + alpha/sqrt(pi)  (0 without self energy)

The pairs are those of generate_nbr_list (torchmd/topology.py:30-73), restated here: D = x_j - x_i, zeroed where the
index_tuple / ex_pairs selection drops the pair, s = D h^-1, image o = -(s > 1/2) + (s < -1/2), D += o h, kept when
(|D|^2 < rc^2) & (|D|^2 != 0); with `group`, pairs stay inside blocks of `group` consecutive atoms.

Everything but `energy` is written out as explicit pair sums (no autograd), so that psi' and psi'' are checked against autograd
of `energy` by tests/test_coulomb_host.py rather than assumed."""
import math

import numpy as np
import torch

SHIFTS = ("none", "potential", "force")
KE = 8.987551787e9 * 6.241509125883258e+18 ** -2 * (1 / 1.60210e-19) * 1e10      # the reference's unit expression (eV A / e^2)


def consts(rc, alpha=0.0, shift="force", conversion=1.0, self_energy=True):
    assert shift in SHIFTS and alpha >= 0
    g0 = 2.0 * alpha / math.sqrt(math.pi)
    E, G = math.erfc(alpha * rc), g0 * math.exp(-(alpha * rc) ** 2)
    c0 = E / rc if shift != "none" else 0.0
    c1 = E / rc ** 2 + G / rc if shift == "force" else 0.0
    s = 0.5 * c0 + alpha / math.sqrt(math.pi) if self_energy else 0.0
    return dict(rc=float(rc), alpha=float(alpha), g0=g0, c0=c0, c1=c1, s=s, conversion=float(conversion))


def psi(r, k):
    """(psi, psi', psi'') at the distances r."""
    a = k["alpha"]
    E = torch.erfc(a * r)
    G = k["g0"] * torch.exp(-(a * r) ** 2)
    return (E / r - k["c0"] + k["c1"] * (r - k["rc"]), -E / r ** 2 - G / r + k["c1"],
            2 * E / r ** 3 + 2 * G / r ** 2 + 2 * a * a * G)


def cell_matrix(cell):
    c = torch.as_tensor(np.asarray(cell, dtype=np.float64))
    return torch.diag(c) if c.dim() == 1 else c


def keep_matrix(n, index_tuple=None, ex_pairs=None):
    keep = torch.ones(n, n, dtype=torch.bool)
    if index_tuple is not None:
        a, b = torch.as_tensor(list(index_tuple[0])), torch.as_tensor(list(index_tuple[1]))
        sel = torch.zeros(n, n, dtype=torch.bool)
        sel[a[:, None], b[None, :]] = True
        keep &= sel | sel.t()
    if ex_pairs is not None:
        ex = torch.as_tensor(np.asarray(ex_pairs, dtype=np.int64)).reshape(-1, 2)
        keep[ex[:, 0], ex[:, 1]] = False
        keep[ex[:, 1], ex[:, 0]] = False
    return keep


def half_list(x, cell, rc, index_tuple=None, ex_pairs=None, group=None):
    """(i, j, offsets o) of the kept pairs i < j, and the smallest | |D| - rc | over all candidate pairs (how far the
    selection is from flipping under float32 rounding of the kernel's own test)."""
    x = torch.as_tensor(x).detach().double()
    h = cell_matrix(cell)
    N = x.shape[0]
    n = N if group is None else int(group)
    assert N % n == 0
    iu = torch.triu_indices(n, n, offset=1)
    sel = keep_matrix(n, index_tuple, ex_pairs)[iu[0], iu[1]]
    I, J, Off, margin = [], [], [], float("inf")
    for b in range(N // n):
        xb = x[b * n:(b + 1) * n]
        D = (xb[iu[1]] - xb[iu[0]]) * sel[:, None].double()
        s = D.matmul(h.inverse())
        o = -(s > 0.5).double() + (s < -0.5).double()
        D = D + o.matmul(h)
        d2 = D.pow(2).sum(-1)
        m = (d2 < rc ** 2) & (d2 != 0)
        if bool(sel.any()):
            margin = min(margin, float((d2[sel].sqrt() - rc).abs().min()))
        I.append(iu[0][m] + b * n), J.append(iu[1][m] + b * n), Off.append(o[m])
    return torch.cat(I), torch.cat(J), torch.cat(Off), margin


def _geom(x, i, j, off, cell):
    d = x[i] - x[j] - off.to(x).matmul(cell_matrix(cell).to(x))              # compute_dis, topology.py:9-10
    r = d.pow(2).sum(-1).sqrt()
    return d, r


def energy(x, q, lst, cell, k):
    """U (differentiable in x and q) on the half list lst = (i, j, offsets)."""
    i, j, off = lst[:3]
    _, r = _geom(x, i, j, off, cell)
    return k["conversion"] * ((q[i] * q[j] * psi(r, k)[0]).sum() - k["s"] * q.pow(2).sum())


def evaluate(x, q, lst, cell, k, w=None):
    """Explicit pair sums in float64: U, grad = dU/dx, pot_i = sum_j q_j psi, and with w: hw = H w,
    potw_i = sum_j q_j psi' rhat_ij.(w_i - w_j); plus the absolute sums A_* of the pair contributions per output component
    (A_U also holds the self terms)."""
    x, q = torch.as_tensor(x).double(), torch.as_tensor(q).double()
    i, j, off = lst[:3]
    N, cv = x.shape[0], k["conversion"]
    d, r = _geom(x, i, j, off, cell)
    rh = d / r[:, None]
    p0, p1, p2 = psi(r, k)
    qq = cv * q[i] * q[j]

    def both(vi, vj, shape):
        out = torch.zeros(shape, dtype=torch.float64)
        out.index_add_(0, i, vi)
        out.index_add_(0, j, vj)
        return out
    self_terms = cv * k["s"] * q.pow(2)
    out = dict(U=(qq * p0).sum() - self_terms.sum(), A_U=(qq * p0).abs().sum() + self_terms.abs().sum())
    t = (qq * p1)[:, None] * rh
    out["grad"], out["A_grad"] = both(t, -t, (N, 3)), both(t.abs(), t.abs(), (N, 3))
    out["pot"], out["A_pot"] = both(q[j] * p0, q[i] * p0, (N,)), both((q[j] * p0).abs(), (q[i] * p0).abs(), (N,))
    if w is not None:
        w = torch.as_tensor(w).double()
        wij = w[i] - w[j]
        a = (rh * wij).sum(1)
        hv = (qq * p2 * a)[:, None] * rh + (qq * p1 / r)[:, None] * (wij - a[:, None] * rh)
        out["hw"], out["A_hw"] = both(hv, -hv, (N, 3)), both(hv.abs(), hv.abs(), (N, 3))
        out["potw"] = both(q[j] * p1 * a, q[i] * p1 * a, (N,))
        out["A_potw"] = both((q[j] * p1 * a).abs(), (q[i] * p1 * a).abs(), (N,))
    return out


def expand(charges, types=None, n_rep=1):
    """[n] or [n_types] charges -> one charge per atom of the (replica-stacked) system."""
    qa = charges if types is None else charges[torch.as_tensor(np.asarray(types), dtype=torch.long)]
    return qa.repeat(n_rep) if n_rep > 1 else qa


class CoulombTerm:
    """The Coulomb term with the oracle's term protocol (n_theta, reset, energy, force, force_vjp by autograd, like
    dihedral_ref.DihedralTerm), with the charges ([n] or [n_types] with `types`) as its parameters: force_vjp's third output
    is d(w.F)/dcharges.  The pair list is the one of the last reset(q), as in oracle.PairTerm."""

    def __init__(self, charges, cutoff, cell, alpha=0.0, shift="force", types=None, index_tuple=None, ex_pairs=None,
                 conversion=KE, self_energy=True):
        self.theta = torch.as_tensor(np.asarray(charges, dtype=np.float32)).reshape(-1)
        self.k = consts(cutoff, alpha, shift, conversion, self_energy)
        self.cell = np.asarray(cell, dtype=np.float32)
        self.types, self.index_tuple, self.ex_pairs = types, index_tuple, ex_pairs
        self.lst = None

    @property
    def n_theta(self):
        return self.theta.numel()

    def reset(self, q):
        self.lst = half_list(q.detach(), self.cell, self.k["rc"], self.index_tuple, self.ex_pairs)

    def energy(self, q, theta=None):
        th = self.theta.to(q) if theta is None else theta
        return energy(q, expand(th, self.types), self.lst, self.cell, self.k)

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


def nacl(cells, a=5.64):
    """(positions [8 cells^3, 3], charges +-1, box length) of a perfect rock-salt lattice of cells^3 conventional cells:
    nearest distance a / 2, simple cubic sites with alternating charge."""
    m = 2 * cells
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)
    return g * (0.5 * a), np.where(g.sum(1) % 2 == 0, 1.0, -1.0), cells * a


MADELUNG_NACL = 1.747565


def madelung(U, n_ions, nearest, conversion):
    """The Madelung constant a lattice energy U of n_ions unit charges implies."""
    return -2.0 * nearest * float(U) / (n_ions * conversion)


def seeded_gas(n, box, min_sep, seed):
    """float64 [n, 3]: uniformly drawn positions in an orthorhombic box with every minimum-image distance >= min_sep."""
    rng = np.random.default_rng(seed)
    box = np.asarray(box, dtype=np.float64)
    pts = []
    while len(pts) < n:
        p = rng.uniform(0, 1, 3) * box
        if pts:
            d = np.array(pts) - p
            d -= box * np.round(d / box)
            if np.sqrt((d ** 2).sum(1)).min() < min_sep:
                continue
        pts.append(p)
    return np.array(pts)
