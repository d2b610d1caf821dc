"""The float64 definition behind the Tersoff tests, as CPU torch (pass float64 tensors; differentiable where stated).

For one species with theta = (A, B, h) and the constants k = (lam1, lam2, beta, n, c, d, R, D, lam3, m, gamma), rc = R + D:

    U       = 1/2 sum_i sum_{j != i} fc(r_ij) [ A exp(-lam1 r_ij) - b_ij B exp(-lam2 r_ij) ]
    b_ij    = (1 + (beta zeta_ij)^n)^(-1/(2n)),  exactly 1 with zero derivatives where zeta_ij = 0
    zeta_ij = sum_{k != i, j} fc(r_ik) g(cos theta_jik) exp[ (lam3 (r_ij - r_ik))^m ]
    g(x)    = gamma (1 + c^2/d^2 - c^2/(d^2 + (h - x)^2))                                  (the published form)
    fc(r)   = 1 for r <= R - D;  1/2 - 1/2 sin(pi (r - R) / (2 D)) for R - D < r < R + D;  0 for r >= R + D

The pairs are those of coulomb_ref.half_list (generate_nbr_list, torchmd/topology.py:30-73) at the cutoff rc; every pair is two
directed bonds (centre -> end), and the triplets of a bond are the other entries of its centre's row.

`energy` is the definition.  `evaluate` differentiates it with float64 autograd and, for the error scales, evaluates it once
more with every piece that a float32 evaluation adds up on its own gathered copies of the positions and parameters: the
repulsive half 1/2 fc A exp(-lam1 r) of every bond, its attractive half -1/2 fc b B exp(-lam2 r) (the two cancel near the
equilibrium bond length, and each carries its own rounding), and every triplet term of zeta.  The derivative with respect to
such a copy is that one piece's contribution -- for a triplet the chain through dU/dzeta of its bond -- and the scales A_* are
the explicit sums of their absolute values per component.  zeta is a sum of non-negative terms, so it is itself well
conditioned and needs no further factor."""
import math

import numpy as np
import torch

import coulomb_ref as C

# the published sets (energies in eV, lengths in Angstrom): Tersoff 1988 Si(C), Tersoff 1989 carbon
SILICON = dict(A=1830.8, B=471.18, lam1=2.4799, lam2=1.7322, beta=1.1e-6, n=0.78734, c=1.0039e5, d=16.217, h=-0.59825,
               R=2.85, D=0.15)
CARBON = dict(A=1393.6, B=346.74, lam1=3.4879, lam2=2.2119, beta=1.5724e-7, n=0.72751, c=38049.0, d=4.3484, h=-0.57058,
              R=1.95, D=0.15)


def consts(lam1, lam2, beta, n, c, d, R, D, lam3=0.0, m=3, gamma=1.0, **_theta):
    """The constants as a dict; A, B, h of a full parameter set are ignored (they are theta)."""
    assert int(m) in (1, 3)
    return dict(lam1=float(lam1), lam2=float(lam2), beta=float(beta), n=float(n), c=float(c), d=float(d), R=float(R),
                D=float(D), lam3=float(lam3), m=int(m), gamma=float(gamma), rc=float(R) + float(D))


def theta_of(p):
    return [p["A"], p["B"], p["h"]]


def bonds_and_triplets(x, cell, rc, group=None):
    """dict(i, j, off: the half list at rc; bc, be, bo: centre, end and image offset of x_end - x_centre of every directed
    bond; tb, tk, to: the bond, the third atom and the image offset of x_third - x_centre of every triplet term; rows: the row
    lengths; margin: see coulomb_ref.half_list)."""
    i, j, off, margin = C.half_list(x, cell, rc, group=group)
    N = int(torch.as_tensor(x).shape[0])
    rows = [[] for _ in range(N)]
    for p in range(i.numel()):
        a, b = int(i[p]), int(j[p])
        rows[a].append((b, off[p]))                 # d = x_i - x_j - off.h  =>  x_j - x_i + off.h points from i to j
        rows[b].append((a, -off[p]))
    bc, be, bo, tb, tk, to = [], [], [], [], [], []
    for c, row in enumerate(rows):
        for m in range(len(row)):
            b = len(bc)
            bc.append(c), be.append(row[m][0]), bo.append(row[m][1])
            for n in range(len(row)):
                if n != m:
                    tb.append(b), tk.append(row[n][0]), to.append(row[n][1])
    idx = lambda v: torch.tensor(v, dtype=torch.long)
    offs = lambda v: torch.stack(v).double() if v else torch.zeros(0, 3, dtype=torch.float64)
    return dict(i=i, j=j, off=off, bc=idx(bc), be=idx(be), bo=offs(bo), tb=idx(tb), tk=idx(tk), to=offs(to),
                rows=torch.tensor([len(r) for r in rows]), margin=margin)


def fc(r, k):
    taper = 0.5 - 0.5 * torch.sin((0.5 * math.pi / k["D"]) * (r - k["R"]))
    return torch.where(r <= k["R"] - k["D"], torch.ones_like(r), torch.where(r < k["R"] + k["D"], taper, torch.zeros_like(r)))


def g_angle(cos, h, k):
    return k["gamma"] * (1.0 + k["c"] ** 2 / k["d"] ** 2 - k["c"] ** 2 / (k["d"] ** 2 + (h - cos) ** 2))


def zeta_terms(dj, dk, h, k):
    """The terms fc(r_k) g(cos) exp[(lam3 (r_j - r_k))^m] for the vectors centre -> end dj and centre -> third atom dk [T, 3]."""
    rj, rk = dj.pow(2).sum(-1).sqrt(), dk.pow(2).sum(-1).sqrt()
    cos = (dj * dk).sum(-1) / (rj * rk)
    t = fc(rk, k) * g_angle(cos, h, k)
    if k["lam3"] != 0.0:
        t = t * torch.exp((k["lam3"] * (rj - rk)) ** k["m"])
    return t


def bond_order(zeta, k):
    bonded = zeta > 0
    z = torch.where(bonded, zeta, torch.ones_like(zeta))
    return torch.where(bonded, (1.0 + (k["beta"] * z) ** k["n"]) ** (-0.5 / k["n"]), torch.ones_like(zeta))


def _pieces(XR, XA, XT, thR, thA, thT, lst, h, k):
    """(repulsive halves [nb], attractive halves [nb], zeta [nb]) with the repulsive half of every bond on the positions XR =
    (centre, end) and the parameters thR [nb, 3], the attractive half on XA and thA, every triplet term on XT = (centre, end,
    third atom) and thT [nt, 3]."""
    bo, to, tb = lst["bo"].to(h).matmul(h), lst["to"].to(h).matmul(h), lst["tb"]
    rR = (XR[1] - XR[0] + bo).pow(2).sum(-1).sqrt()
    rA = (XA[1] - XA[0] + bo).pow(2).sum(-1).sqrt()
    t = zeta_terms(XT[1] - XT[0] + bo[tb], XT[2] - XT[0] + to, thT[:, 2], k)
    zeta = torch.zeros_like(rA).index_add(0, tb, t)
    vR = 0.5 * fc(rR, k) * thR[:, 0] * torch.exp(-k["lam1"] * rR)
    vA = -0.5 * fc(rA, k) * bond_order(zeta, k) * thA[:, 1] * torch.exp(-k["lam2"] * rA)
    return vR, vA, zeta


def _gathered(x, theta, lst):
    bc, be, tb, tk = lst["bc"], lst["be"], lst["tb"], lst["tk"]
    XR, XA, XT = [x[bc], x[be]], [x[bc], x[be]], [x[bc[tb]], x[be[tb]], x[tk]]
    ths = [theta[None, :].expand(bc.numel(), 3), theta[None, :].expand(bc.numel(), 3), theta[None, :].expand(tb.numel(), 3)]
    atoms = [bc, be, bc, be, bc[tb], be[tb], tk]
    return XR, XA, XT, ths, atoms


def energy(x, theta, lst, cell, k, parts=False):
    """U (differentiable in x and theta = (A, B, h)) on lst = bonds_and_triplets(...); parts: (repulsive, attractive, zeta)."""
    XR, XA, XT, ths, _ = _gathered(x, theta, lst)
    vR, vA, zeta = _pieces(XR, XA, XT, ths[0], ths[1], ths[2], lst, C.cell_matrix(cell).to(x), k)
    return (vR.sum(), vA.sum(), zeta) if parts else vR.sum() + vA.sum()


def evaluate(x, theta, lst, cell, k, w=None):
    """float64 autograd of `energy`: U, grad = dU/dx, dth = dU/dtheta, and with w: hw = H w, dthw = d(w.dU/dx)/dtheta; plus
    A_U, A_grad, A_dth, A_hw, A_dthw, the sums of the absolute contributions of the bond halves and the triplet terms to every
    component (module docstring); zeta per directed bond."""
    x = torch.as_tensor(x).detach().double()
    theta = torch.as_tensor(np.asarray(theta, dtype=np.float64)).reshape(3)
    N = x.shape[0]
    xg, tg = x.clone().requires_grad_(True), theta.clone().requires_grad_(True)
    U = energy(xg, tg, lst, cell, k)
    g, gt = torch.autograd.grad(U, (xg, tg), create_graph=w is not None)
    out = dict(U=U.detach(), grad=g.detach(), dth=gt.detach())
    if w is not None:
        w = torch.as_tensor(w).detach().double()
        hw, hth = torch.autograd.grad((g * w).sum(), (xg, tg))
        out["hw"], out["dthw"] = hw, hth
    # ---- scales: every piece on its own copies of its atoms' positions and of theta
    XR, XA, XT, ths, atoms = _gathered(x, theta, lst)
    X = [t.clone().requires_grad_(True) for t in XR + XA + XT]
    TH = [t.clone().requires_grad_(True) for t in ths]
    vR, vA, zeta = _pieces(X[0:2], X[2:4], X[4:7], TH[0], TH[1], TH[2], lst, C.cell_matrix(cell).double(), k)
    out["zeta"] = zeta.detach()
    out["A_U"] = vR.detach().abs().sum() + vA.detach().abs().sum()
    zeros = lambda *s: torch.zeros(*s, dtype=torch.float64)
    fill = lambda gs, like: [zeros(*l.shape) if v is None else v for v, l in zip(gs, like)]
    gs = fill(torch.autograd.grad(vR.sum() + vA.sum(), X + TH, create_graph=w is not None, allow_unused=True), X + TH)
    A_grad, A_dth = zeros(N, 3), zeros(3)
    for a, ga in zip(atoms, gs[:7]):
        A_grad.index_add_(0, a, ga.detach().abs())
    for gth in gs[7:]:
        A_dth += gth.detach().abs().sum(0)
    out.update(A_grad=A_grad, A_dth=A_dth)
    if w is not None:
        s = sum((ga * w[a]).sum() for a, ga in zip(atoms, gs[:7]))
        A_hw, A_dthw = zeros(N, 3), zeros(3)
        if s.requires_grad:
            hs = fill(torch.autograd.grad(s, X + TH, allow_unused=True), X + TH)
            for a, ha in zip(atoms, hs[:7]):
                A_hw.index_add_(0, a, ha.abs())
            for hth in hs[7:]:
                A_dthw += hth.abs().sum(0)
        out.update(A_hw=A_hw, A_dthw=A_dthw)
    return out


def energy_loops(x, theta, cell, k, group=None):
    """The same energy as plain numpy loops over every ordered pair and every third atom with the minimum image taken per
    vector -- written separately from everything above.  Returns (repulsive part, attractive part)."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(cell, dtype=np.float64)
    h = np.diag(h) if h.ndim == 1 else h
    hinv = np.linalg.inv(h)
    A, B, hh = (float(t) for t in theta)
    R, D, rc = k["R"], k["D"], k["R"] + k["D"]
    N = x.shape[0]
    n = N if group is None else group

    def image(v):
        s = v @ hinv
        return v + (-(s > 0.5).astype(float) + (s < -0.5).astype(float)) @ h

    def cut(r):
        if r <= R - D:
            return 1.0
        return 0.5 - 0.5 * math.sin(0.5 * math.pi * (r - R) / D) if r < rc else 0.0
    UR = UA = 0.0
    for c in range(N):
        lo = (c // n) * n
        vec = []
        for e in range(lo, lo + n):
            if e != c:
                v = image(x[e] - x[c])
                r = float(np.sqrt((v ** 2).sum()))
                if r < rc and r != 0.0:
                    vec.append((v, r))
        for a, (va, ra) in enumerate(vec):
            zeta = 0.0
            for b, (vb, rb) in enumerate(vec):
                if b != a:
                    cos = float(va @ vb) / (ra * rb)
                    gg = k["gamma"] * (1.0 + k["c"] ** 2 / k["d"] ** 2 - k["c"] ** 2 / (k["d"] ** 2 + (hh - cos) ** 2))
                    zeta += cut(rb) * gg * math.exp((k["lam3"] * (ra - rb)) ** k["m"])
            bo = (1.0 + (k["beta"] * zeta) ** k["n"]) ** (-0.5 / k["n"]) if zeta > 0.0 else 1.0
            UR += 0.5 * cut(ra) * A * math.exp(-k["lam1"] * ra)
            UA -= 0.5 * cut(ra) * bo * B * math.exp(-k["lam2"] * ra)
    return UR, UA


def diamond_closed_form(p, a):
    """(U / N, zeta, b) of the perfect diamond lattice with the cubic constant a, lam3 = 0: four neighbours at a sqrt(3) / 4
    inside R - D, the second shell at a / sqrt(2) beyond R + D, so zeta = 3 g(-1/3)."""
    r0 = a * math.sqrt(3.0) / 4.0
    assert r0 < p["R"] - p["D"] and a / math.sqrt(2.0) > p["R"] + p["D"]
    gamma = p.get("gamma", 1.0)
    zeta = 3.0 * gamma * (1.0 + p["c"] ** 2 / p["d"] ** 2 - p["c"] ** 2 / (p["d"] ** 2 + (p["h"] + 1.0 / 3.0) ** 2))
    b = (1.0 + (p["beta"] * zeta) ** p["n"]) ** (-0.5 / p["n"])
    return 2.0 * (p["A"] * math.exp(-p["lam1"] * r0) - b * p["B"] * math.exp(-p["lam2"] * r0)), zeta, b


def jittered_diamond(cells=2, a0=5.432, sigma_jit=0.3, seed=64):
    """(float32 positions, float32 cell) of a diamond lattice of cells^3 conventional cells, every coordinate jittered by a
    normal deviate of width sigma_jit."""
    import oracle as O
    pos, cell = O.diamond_lattice(cells, a0)
    rng = np.random.default_rng(seed)
    x = np.mod(pos + rng.normal(0, sigma_jit, pos.shape), cell) if sigma_jit else pos
    return x.astype(np.float32), cell.astype(np.float32)


def taper_census(x, cell, k, group=None):
    """(number of directed bonds strictly inside the taper (R - D, R + D), the smallest distance of any pair separation below
    rc + 0.05 from R - D or R + D) -- the input conditions of the GPU tests."""
    i, j, off, _ = C.half_list(x, cell, k["rc"] + 0.05, group=group)
    X = torch.as_tensor(x).double()
    r = (X[i] - X[j] - off.double().matmul(C.cell_matrix(cell).double())).pow(2).sum(-1).sqrt()
    inside = 2 * int(((r > k["R"] - k["D"]) & (r < k["R"] + k["D"])).sum())
    gap = float(torch.minimum((r - (k["R"] - k["D"])).abs(), (r - (k["R"] + k["D"])).abs()).min()) if r.numel() else math.inf
    return inside, gap


class TersoffTerm:
    """The Tersoff term with the oracle's term protocol (n_theta, reset, energy, force, force_vjp by autograd, like
    sw_ref.SWTerm) and theta = (A, B, h): force_vjp's third output is d(w.F)/dtheta.  The bonds and triplets are those of the
    last reset(q), searched at R + D."""

    def __init__(self, params, cell, group=None):
        self.theta = torch.tensor(theta_of(params), dtype=torch.float32)
        self.k = consts(**params)
        self.cell = np.asarray(cell, dtype=np.float32)
        self.group = group
        self.lst = None

    @property
    def n_theta(self):
        return 3

    def reset(self, q):
        self.lst = bonds_and_triplets(q.detach(), self.cell, self.k["rc"], group=self.group)

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


# ---------------------------------------------------------------------------------------------- the inputs of the GPU tests
# Every configuration below is checked on the CPU by tests/test_tersoff_host.py: at least 10 directed bonds strictly inside the
# taper, no pair separation within 0.01 A of R - D or R + D, and a bond with zeta = 0 where a test speaks of one.  The seeds
# are the first for which this holds.
LAM3 = dict(SILICON, lam3=1.3258, m=3)
SEEDS = dict(si64=6, c64=257, gas37=2, tric64=33, replicas=20, traj=2, skin=79)


def sheared_diamond(cells=2, a0=5.432, sigma_jit=0.3, seed=0):
    """(float32 positions, float32 [3, 3] cell) of the jittered diamond lattice in a triclinic cell: the cubic cell sheared."""
    import oracle as O
    pos, cell = O.diamond_lattice(cells, a0)
    L = float(np.asarray(cell).reshape(-1)[0])
    h = L * np.array([[1.0, 0.0, 0.0], [0.2, 1.0, 0.0], [0.1, -0.15, 1.0]])
    rng = np.random.default_rng(seed)
    frac = np.mod(pos / L + rng.normal(0, sigma_jit, pos.shape) @ np.linalg.inv(h), 1.0)
    return (frac @ h).astype(np.float32), h.astype(np.float32)


def gas37(seed=0):
    """37 atoms in a 14 x 15 x 16 box: a hub with 18 neighbours on a shell of 2.45 A around it (0 - 18: a row longer than the
    lanes of an atom), 12 atoms drawn around them with a minimum separation of 2.0 A (19 - 30), an atom far from everything
    (31), two atoms that only see each other (32, 33: zeta = 0) and a bent trimer on its own (34 centre, 35, 36)."""
    rng = np.random.default_rng(seed)
    hub = np.array([5.0, 5.0, 5.0])
    n = 18
    kk = np.arange(n) + 0.5
    phi, z = np.pi * (1 + 5 ** 0.5) * kk, 1 - 2 * kk / n
    shell = 2.45 * np.stack([np.cos(phi) * np.sqrt(1 - z * z), np.sin(phi) * np.sqrt(1 - z * z), z], 1)
    pts = [hub] + list(hub + shell + rng.normal(0, 0.08, shell.shape))
    while len(pts) < 31:
        p = rng.uniform(1.0, 9.0, 3)
        if all(np.linalg.norm(p - q) >= 2.0 for q in pts):
            pts.append(p)
    c = np.array([5.0, 12.0, 12.5])
    ang = np.deg2rad(100.0)
    pts += [np.array([11.5, 12.0, 13.0]), np.array([11.5, 4.0, 11.0]), np.array([11.5, 4.0, 13.35]),
            c, c + 2.3 * np.array([1.0, 0.0, 0.0]), c + 2.4 * np.array([np.cos(ang), np.sin(ang), 0.0])]
    return np.array(pts).astype(np.float32), np.array([14.0, 15.0, 16.0], dtype=np.float32)


def replicas16(seed=0):
    """(the 16 base positions, the box, float32 positions of three jittered copies): three replicas of a 16-atom gas."""
    box = np.array([8.0, 8.0, 8.5], dtype=np.float32)
    base = C.seeded_gas(16, box, 2.0, seed=16 + seed)
    rng = np.random.default_rng(240 + seed)
    x32 = np.concatenate([np.mod(base + rng.normal(0, 0.1, base.shape), box) for _ in range(3)]).astype(np.float32)
    return base, box, x32


def skin_step(x32, seed=0):
    """The positions after a move of less than 0.18 A per atom (inside half a skin of 0.4 A)."""
    rng = np.random.default_rng(670 + seed)
    step = rng.normal(0, 1, x32.shape)
    step = 0.18 * step / np.linalg.norm(step, axis=1)[:, None] * rng.uniform(0.3, 1.0, (x32.shape[0], 1))
    return (x32 + step).astype(np.float32)


def gpu_cases():
    """name -> (float32 positions, float32 cell, parameter set, group): every configuration the GPU tests evaluate."""
    si = jittered_diamond(2, 5.432, 0.3, SEEDS["si64"])
    base, box, x3 = replicas16(SEEDS["replicas"])
    return {"si64": si + (SILICON, None),
            "c64": jittered_diamond(2, 3.566, 0.15, SEEDS["c64"]) + (CARBON, None),
            "gas37": gas37(SEEDS["gas37"]) + (SILICON, None),
            "tric64": sheared_diamond(2, 5.432, 0.3, SEEDS["tric64"]) + (SILICON, None),
            "lam3": si + (LAM3, None),
            "replicas": (x3, box, SILICON, 16),
            "skin": (skin_step(si[0], SEEDS["skin"]), si[1], SILICON, None),
            "traj": jittered_diamond(2, 5.432, 0.2, SEEDS["traj"]) + (SILICON, None)}
