"""The float64 definition behind the multi-species Tersoff tests, as CPU torch (pass float64 tensors; differentiable where
stated).  Atom i has the species t_i in [0, S); with a = t_i, b = t_j, c = t_k (Tersoff 1989, the LAMMPS convention, lam3 = 0):

    U       = 1/2 sum_i sum_{j != i} fc_ab(r_ij) [ A_ab exp(-lam1_ab r_ij) - b_ij B_ab exp(-lam2_ab r_ij) ]
    b_ij    = (1 + (beta_a zeta_ij)^n_a)^(-1/(2 n_a)),  exactly 1 with zero derivatives where zeta_ij = 0
    zeta_ij = sum_{k != i, j} fc_ac(r_ik) g_a(cos theta_jik)
    g_a(x)  = gamma_a (1 + c_a^2/d_a^2 - c_a^2/(d_a^2 + (h_a - x)^2))                         (the published form)
    fc_ab   = 1 for r <= R_ab - D_ab;  1/2 - 1/2 sin(pi (r - R_ab) / (2 D_ab)) inside;  0 for r >= R_ab + D_ab

A table set `tab` is a dict: S; the [S, S] float64 arrays A, B, lam1, lam2, R, D (row = centre species, column = end species);
the [S] arrays beta, n, c, d, h, gamma.  theta = (A.flat, B.flat, h), 2 S^2 + S numbers.

The pairs are those of coulomb_ref.half_list at the cutoff max_ab (R_ab + D_ab); every pair is two directed bonds (centre ->
end) and the triplets of a bond are the other entries of its centre's row (tersoff_ref.bonds_and_triplets).  An entry beyond
the cutoff of its own pair of species has fc = 0 and so adds nothing, as a bond or as a third atom.

`energy` is the definition.  `evaluate` differentiates it with float64 autograd and forms the error scales A_* exactly as
tersoff_ref.evaluate does: the repulsive half of every bond, its attractive half and every triplet term each on its own
gathered copies of the positions and of theta; the scales are the sums of the absolute derivatives with respect to the copies."""
import math

import numpy as np
import torch

import coulomb_ref as C
import tersoff_ref as R1

SILICON, CARBON = R1.SILICON, R1.CARBON
GERMANIUM = dict(A=1769.0, B=419.23, lam1=2.4451, lam2=1.7047, beta=9.0166e-7, n=0.75627, c=1.0643e5, d=15.652, h=-0.43884,
                 R=2.95, D=0.15)
CHI_SIC, CHI_SIGE = 0.9776, 1.00061
PAIR_KEYS = ("A", "B", "lam1", "lam2", "R", "D")
CENTRE_KEYS = ("beta", "n", "c", "d", "h", "gamma")


# ---------------------------------------------------------------------------------------------- tables
def mixed(species, chi=None):
    """The table set of S one-species sets under Tersoff's mixing rules, element by element: A_ab = sqrt(A_a A_b), B_ab =
    chi_ab sqrt(B_a B_b), lam_ab = (lam_a + lam_b) / 2, the inner radius R - D and the outer radius R + D each as the geometric
    mean of the two species', R_ab and D_ab from those."""
    S = len(species)
    tab = dict(S=S, **{k: np.zeros((S, S)) for k in PAIR_KEYS}, **{k: np.zeros(S) for k in CENTRE_KEYS})
    for a, p in enumerate(species):
        for k in CENTRE_KEYS:
            tab[k][a] = float(p.get(k, 1.0)) if k == "gamma" else float(p[k])
        for b, q in enumerate(species):
            x = 1.0 if a == b or chi is None else float(chi[a][b])
            tab["A"][a, b] = math.sqrt(p["A"] * q["A"])
            tab["B"][a, b] = x * math.sqrt(p["B"] * q["B"])
            tab["lam1"][a, b] = 0.5 * (p["lam1"] + q["lam1"])
            tab["lam2"][a, b] = 0.5 * (p["lam2"] + q["lam2"])
            rin = math.sqrt((p["R"] - p["D"]) * (q["R"] - q["D"]))
            rout = math.sqrt((p["R"] + p["D"]) * (q["R"] + q["D"]))
            tab["R"][a, b], tab["D"][a, b] = 0.5 * (rin + rout), 0.5 * (rout - rin)
    return tab


def sic():
    return mixed([SILICON, CARBON], [[1.0, CHI_SIC], [CHI_SIC, 1.0]])


def sige():
    return mixed([SILICON, GERMANIUM], [[1.0, CHI_SIGE], [CHI_SIGE, 1.0]])


def sicge():
    """Three species; no chi is published for C-Ge, 1 is taken."""
    return mixed([SILICON, CARBON, GERMANIUM], [[1.0, CHI_SIC, CHI_SIGE], [CHI_SIC, 1.0, 1.0], [CHI_SIGE, 1.0, 1.0]])


def pair_centre(tab):
    """(pair, centre) as TersoffMulti.from_tables takes them."""
    return {k: tab[k] for k in PAIR_KEYS}, {k: tab[k] for k in CENTRE_KEYS}


def theta_of(tab):
    return np.concatenate([tab["A"].reshape(-1), tab["B"].reshape(-1), tab["h"].reshape(-1)])


def n_theta(tab):
    return 2 * tab["S"] ** 2 + tab["S"]


def rc_max(tab):
    return float((tab["R"] + tab["D"]).max())


def relabelled(tab, perm):
    """The table set with species a renamed perm[a]."""
    inv = np.argsort(np.asarray(perm))
    out = dict(S=tab["S"])
    for k in PAIR_KEYS:
        out[k] = tab[k][np.ix_(inv, inv)].copy()
    for k in CENTRE_KEYS:
        out[k] = tab[k][inv].copy()
    return out


# ---------------------------------------------------------------------------------------------- the definition
def bonds_and_triplets(x, cell, tab, group=None):
    return R1.bonds_and_triplets(x, cell, rc_max(tab), group=group)


def fc(r, Rab, Dab):
    taper = 0.5 - 0.5 * torch.sin((0.5 * math.pi / Dab) * (r - Rab))
    return torch.where(r <= Rab - Dab, torch.ones_like(r), torch.where(r < Rab + Dab, taper, torch.zeros_like(r)))


def bond_order(zeta, beta, n):
    bonded = zeta > 0
    z = torch.where(bonded, zeta, torch.ones_like(zeta))
    return torch.where(bonded, (1.0 + (beta * z) ** n) ** (-0.5 / n), torch.ones_like(zeta))


def _pieces(XR, XA, XT, thR, thA, thT, lst, types, h, tab):
    """(repulsive halves [nb], attractive halves [nb], zeta [nb]): the repulsive half of every bond on the positions XR =
    (centre, end) and the parameters thR [nb, P], the attractive half on XA and thA, every triplet term on XT = (centre, end,
    third atom) and thT [nt, P]; every constant gathered by the species of the atoms involved."""
    S = tab["S"]
    t64 = lambda k: torch.as_tensor(tab[k], dtype=h.dtype)
    bo, to, tb = lst["bo"].to(h).matmul(h), lst["to"].to(h).matmul(h), lst["tb"]
    ta, te = types[lst["bc"]], types[lst["be"]]                  # centre and end species of every bond
    tc = types[lst["tk"]]                                        # third-atom species of every triplet term
    nb, nt = ta.numel(), tb.numel()
    rR = (XR[1] - XR[0] + bo).pow(2).sum(-1).sqrt()
    rA = (XA[1] - XA[0] + bo).pow(2).sum(-1).sqrt()
    dj, dk = XT[1] - XT[0] + bo[tb], XT[2] - XT[0] + to
    rj, rk = dj.pow(2).sum(-1).sqrt(), dk.pow(2).sum(-1).sqrt()
    cos = (dj * dk).sum(-1) / (rj * rk)
    a3 = ta[tb]                                                  # the centre's species, per triplet term
    hh = thT[torch.arange(nt), 2 * S * S + a3]
    c2, d2 = t64("c")[a3] ** 2, t64("d")[a3] ** 2
    g = t64("gamma")[a3] * (1.0 + c2 / d2 - c2 / (d2 + (hh - cos) ** 2))
    t = fc(rk, t64("R")[a3, tc], t64("D")[a3, tc]) * g
    zeta = torch.zeros_like(rA).index_add(0, tb, t)
    Ab = thR[torch.arange(nb), ta * S + te]
    Bb = thA[torch.arange(nb), S * S + ta * S + te]
    Rb, Db = t64("R")[ta, te], t64("D")[ta, te]
    vR = 0.5 * fc(rR, Rb, Db) * Ab * torch.exp(-t64("lam1")[ta, te] * rR)
    vA = -0.5 * fc(rA, Rb, Db) * bond_order(zeta, t64("beta")[ta], t64("n")[ta]) * Bb * torch.exp(-t64("lam2")[ta, te] * rA)
    return vR, vA, zeta


def _gathered(x, theta, lst):
    bc, be, tb, tk = lst["bc"], lst["be"], lst["tb"], lst["tk"]
    P = theta.numel()
    XR, XA, XT = [x[bc], x[be]], [x[bc], x[be]], [x[bc[tb]], x[be[tb]], x[tk]]
    ths = [theta[None, :].expand(bc.numel(), P), theta[None, :].expand(bc.numel(), P), theta[None, :].expand(tb.numel(), P)]
    atoms = [bc, be, bc, be, bc[tb], be[tb], tk]
    return XR, XA, XT, ths, atoms


def _types(types):
    return torch.as_tensor(np.asarray(types)).long()


def energy(x, types, tab, lst, cell, theta=None, parts=False):
    """U (differentiable in x and in theta [2 S^2 + S], which defaults to the tables' own A, B, h); parts: (repulsive,
    attractive, zeta)."""
    theta = torch.as_tensor(theta_of(tab)).to(x) if theta is None else theta
    XR, XA, XT, ths, _ = _gathered(x, theta, lst)
    vR, vA, zeta = _pieces(XR, XA, XT, ths[0], ths[1], ths[2], lst, _types(types), C.cell_matrix(cell).to(x), tab)
    return (vR.sum(), vA.sum(), zeta) if parts else vR.sum() + vA.sum()


def evaluate(x, types, tab, lst, cell, w=None, theta=None):
    """float64 autograd of `energy`: U, grad = dU/dx, dth = dU/dtheta [2 S^2 + S], and with w: hw = H w, dthw =
    d(w.dU/dx)/dtheta; plus A_U, A_grad, A_dth, A_hw, A_dthw (module docstring); zeta per directed bond."""
    x = torch.as_tensor(x).detach().double()
    theta = torch.as_tensor(np.asarray(theta_of(tab) if theta is None else theta, dtype=np.float64)).reshape(-1)
    ty = _types(types)
    N, P = x.shape[0], theta.numel()
    xg, tg = x.clone().requires_grad_(True), theta.clone().requires_grad_(True)
    U = energy(xg, ty, tab, lst, cell, theta=tg)
    g, gt = torch.autograd.grad(U, (xg, tg), create_graph=w is not None)
    out = dict(U=U.detach(), grad=g.detach(), dth=gt.detach())
    if w is not None:
        w = torch.as_tensor(w).detach().double()
        hw, hth = torch.autograd.grad((g * w).sum(), (xg, tg))
        out["hw"], out["dthw"] = hw, hth
    XR, XA, XT, ths, atoms = _gathered(x, theta, lst)
    X = [t.clone().requires_grad_(True) for t in XR + XA + XT]
    TH = [t.clone().requires_grad_(True) for t in ths]
    vR, vA, zeta = _pieces(X[0:2], X[2:4], X[4:7], TH[0], TH[1], TH[2], lst, ty, C.cell_matrix(cell).double(), tab)
    out["zeta"] = zeta.detach()
    out["A_U"] = vR.detach().abs().sum() + vA.detach().abs().sum()
    zeros = lambda *s: torch.zeros(*s, dtype=torch.float64)
    fill = lambda gs, like: [zeros(*l.shape) if v is None else v for v, l in zip(gs, like)]
    gs = fill(torch.autograd.grad(vR.sum() + vA.sum(), X + TH, create_graph=w is not None, allow_unused=True), X + TH)
    A_grad, A_dth = zeros(N, 3), zeros(P)
    for a, ga in zip(atoms, gs[:7]):
        A_grad.index_add_(0, a, ga.detach().abs())
    for gth in gs[7:]:
        A_dth += gth.detach().abs().sum(0)
    out.update(A_grad=A_grad, A_dth=A_dth)
    if w is not None:
        s = sum((ga * w[a]).sum() for a, ga in zip(atoms, gs[:7]))
        A_hw, A_dthw = zeros(N, 3), zeros(P)
        if s.requires_grad:
            hs = fill(torch.autograd.grad(s, X + TH, allow_unused=True), X + TH)
            for a, ha in zip(atoms, hs[:7]):
                A_hw.index_add_(0, a, ha.abs())
            for hth in hs[7:]:
                A_dthw += hth.abs().sum(0)
        out.update(A_hw=A_hw, A_dthw=A_dthw)
    return out


def energy_loops(x, types, tab, cell, group=None):
    """The same energy as plain numpy loops over every ordered pair and every third atom with the minimum image taken per
    vector -- written separately from everything above.  Returns (repulsive part, attractive part)."""
    x = np.asarray(x, dtype=np.float64)
    ty = np.asarray(types).astype(int)
    h = np.asarray(cell, dtype=np.float64)
    h = np.diag(h) if h.ndim == 1 else h
    hinv = np.linalg.inv(h)
    N = x.shape[0]
    n = N if group is None else group

    def image(v):
        s = v @ hinv
        return v + (-(s > 0.5).astype(float) + (s < -0.5).astype(float)) @ h

    def cut(r, a, b):
        Rab, Dab = tab["R"][a, b], tab["D"][a, b]
        if r <= Rab - Dab:
            return 1.0
        return 0.5 - 0.5 * math.sin(0.5 * math.pi * (r - Rab) / Dab) if r < Rab + Dab else 0.0
    UR = UA = 0.0
    for c in range(N):
        lo = (c // n) * n
        a = ty[c]
        vec = []
        for e in range(lo, lo + n):
            if e != c:
                v = image(x[e] - x[c])
                r = float(np.sqrt((v ** 2).sum()))
                if r != 0.0 and r < tab["R"][a, ty[e]] + tab["D"][a, ty[e]]:
                    vec.append((v, r, ty[e]))
        for m, (vj, rj, b) in enumerate(vec):
            zeta = 0.0
            for q, (vk, rk, cc) in enumerate(vec):
                if q != m:
                    cos = float(vj @ vk) / (rj * rk)
                    gg = tab["gamma"][a] * (1.0 + tab["c"][a] ** 2 / tab["d"][a] ** 2
                                            - tab["c"][a] ** 2 / (tab["d"][a] ** 2 + (tab["h"][a] - cos) ** 2))
                    zeta += cut(rk, a, cc) * gg
            bo = (1.0 + (tab["beta"][a] * zeta) ** tab["n"][a]) ** (-0.5 / tab["n"][a]) if zeta > 0.0 else 1.0
            UR += 0.5 * cut(rj, a, b) * tab["A"][a, b] * math.exp(-tab["lam1"][a, b] * rj)
            UA -= 0.5 * cut(rj, a, b) * bo * tab["B"][a, b] * math.exp(-tab["lam2"][a, b] * rj)
    return UR, UA


def zincblende_closed_form(tab, a, s0=0, s1=1):
    """(U / N, b of the bonds centred on s0, b of those centred on s1) of the perfect zincblende lattice (diamond when s0 = s1)
    with the cubic constant a: four unlike neighbours at a sqrt(3) / 4 inside R - D of the unlike pair, the second shell (like
    atoms) at a / sqrt(2) beyond R + D of both like pairs, so zeta = 3 g(-1/3) with the centre's constants."""
    r0 = a * math.sqrt(3.0) / 4.0
    u, bs = 0.0, []
    for p, q in ((s0, s1), (s1, s0)):
        assert r0 < tab["R"][p, q] - tab["D"][p, q] and a / math.sqrt(2.0) > tab["R"][p, p] + tab["D"][p, p]
        zeta = 3.0 * tab["gamma"][p] * (1.0 + tab["c"][p] ** 2 / tab["d"][p] ** 2
                                        - tab["c"][p] ** 2 / (tab["d"][p] ** 2 + (tab["h"][p] + 1.0 / 3.0) ** 2))
        b = (1.0 + (tab["beta"][p] * zeta) ** tab["n"][p]) ** (-0.5 / tab["n"][p])
        u += 0.5 * 2.0 * (tab["A"][p, q] * math.exp(-tab["lam1"][p, q] * r0) - b * tab["B"][p, q] * math.exp(-tab["lam2"][p, q] * r0))
        bs.append(b)
    return u, bs[0], bs[1]


def closed_form_minimum(tab, a0, s0=0, s1=1):
    """(a, U / N) at the minimum of zincblende_closed_form near a0, by golden-section search."""
    lo, hi = a0 - 0.05, a0 + 0.05
    f = lambda s: zincblende_closed_form(tab, s, s0, s1)[0]
    gr = (math.sqrt(5.0) - 1.0) / 2.0
    for _ in range(80):
        c, d = hi - gr * (hi - lo), lo + gr * (hi - lo)
        lo, hi = (lo, d) if f(c) < f(d) else (c, hi)
    return 0.5 * (lo + hi), f(0.5 * (lo + hi))


def census(x, types, tab, cell, group=None):
    """The input conditions of a configuration: taper[a][b] = the number of directed bonds a -> b strictly inside the taper of
    (a, b); gap = the smallest distance of any pair separation from either taper edge of either ordered pair of its species;
    classes[a][b][c] = the number of triplet terms with centre a, end b, third atom c and both entries inside their supports;
    rmin = the smallest pair separation."""
    S = tab["S"]
    ty = _types(types)
    i, j, off, _ = C.half_list(x, cell, rc_max(tab) + 0.05, group=group)
    X = torch.as_tensor(x).double()
    r = (X[i] - X[j] - off.double().matmul(C.cell_matrix(cell).double())).pow(2).sum(-1).sqrt()
    taper = np.zeros((S, S), dtype=int)
    gap = math.inf
    for a, b in ((ty[i], ty[j]), (ty[j], ty[i])):
        Rab, Dab = torch.as_tensor(tab["R"])[a, b], torch.as_tensor(tab["D"])[a, b]
        inside = (r > Rab - Dab) & (r < Rab + Dab)
        np.add.at(taper, (a[inside].numpy(), b[inside].numpy()), 1)
        if r.numel():
            gap = min(gap, float(torch.minimum((r - (Rab - Dab)).abs(), (r - (Rab + Dab)).abs()).min()))
    lst = bonds_and_triplets(x, cell, tab, group=group)
    hm = C.cell_matrix(cell).double()
    bc, be, tb, tk = lst["bc"], lst["be"], lst["tb"], lst["tk"]
    rb = (X[be] - X[bc] + lst["bo"].matmul(hm)).pow(2).sum(-1).sqrt()
    rt = (X[tk] - X[bc[tb]] + lst["to"].matmul(hm)).pow(2).sum(-1).sqrt()
    rcs = torch.as_tensor(tab["R"] + tab["D"])
    a3, b3, c3 = ty[bc[tb]], ty[be[tb]], ty[tk]
    live = (rb[tb] < rcs[a3, b3]) & (rt < rcs[a3, c3])
    classes = np.zeros((S, S, S), dtype=int)
    np.add.at(classes, (a3[live].numpy(), b3[live].numpy(), c3[live].numpy()), 1)
    return dict(taper=taper, gap=gap, classes=classes, rmin=float(r.min()) if r.numel() else math.inf, rows=lst["rows"])


class TersoffMultiTerm:
    """The term with the oracle's term protocol (n_theta, reset, energy, force, force_vjp by autograd, like
    tersoff_ref.TersoffTerm) and theta = (A.flat, B.flat, h): force_vjp's third output is d(w.F)/dtheta [2 S^2 + S].  The
    bonds and triplets are those of the last reset(q), searched at max (R + D)."""

    def __init__(self, tab, types, cell, group=None):
        self.tab = tab
        self.types = _types(types)
        self.theta = torch.tensor(theta_of(tab), dtype=torch.float32)
        self.cell = np.asarray(cell, dtype=np.float32)
        self.group = group
        self.lst = None

    @property
    def n_theta(self):
        return n_theta(self.tab)

    def reset(self, q):
        self.lst = bonds_and_triplets(q.detach(), self.cell, self.tab, group=self.group)

    def energy(self, q, theta=None):
        return energy(q, self.types, self.tab, self.lst, self.cell, theta=self.theta.to(q) if theta is None else theta)

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
# Every configuration below is checked on the CPU by tests/test_tersoff_multi_host.py (test_input_conditions_...); the seeds are
# the first for which its conditions hold.
SEEDS = dict(sic_alloy64=188, tric64=1870, gas37=12, s3_64=39, replicas=17, skin=85, traj=0)


def species_split(n, S, seed):
    """n species labels, as equal a number of each of the S as n allows, in an order drawn from `seed`."""
    return np.random.default_rng(1000 + seed).permutation(np.arange(n) % S).astype(np.int32)


def alloy64(seed, S=2, a0=4.6, sigma_jit=0.25):
    """(float32 positions, float32 cell, types): a 2 x 2 x 2 diamond lattice with the species assigned by a seeded permutation and
    every coordinate jittered by a normal deviate of width sigma_jit."""
    x, cell = R1.jittered_diamond(2, a0, sigma_jit, seed)
    return x, cell, species_split(64, S, seed)


def sheared_alloy64(seed, a0=4.6, sigma_jit=0.25):
    x, cell = R1.sheared_diamond(2, a0, sigma_jit, seed)
    return x, cell, species_split(64, 2, seed)


def gas37(seed):
    """tersoff_ref.gas37 with random species; the hub (0), the dimer (32, 33) and the trimer (34 - 36) are silicon, so that the
    hub's row of 18 is inside its cutoff and the dimer and the trimer are bonded."""
    x, cell = R1.gas37(seed)
    ty = species_split(37, 2, seed)
    ty[[0, 32, 33, 34, 35, 36]] = 0
    return x, cell, ty


def replicas16(seed):
    """(the 16 base positions, the box, float32 positions of three jittered copies, the 16 species of a replica)."""
    base, box, x3 = R1.replicas16(seed)
    return base, box, x3, species_split(16, 2, seed)


def zincblende(a, sigma_jit=0.0, seed=0):
    """(float32 positions, float32 cell, types) of 2 x 2 x 2 zincblende cells: species 0 on the fcc sites, 1 on the others."""
    x, cell = R1.jittered_diamond(2, a, sigma_jit, seed)
    return x, cell, (np.arange(64) % 8 >= 4).astype(np.int32)


def gpu_cases():
    """name -> (float32 positions, float32 cell, types of a replica, table set, group)."""
    alloy = alloy64(SEEDS["sic_alloy64"])
    base, box, x3, ty16 = replicas16(SEEDS["replicas"])
    out = {"sic_alloy64": alloy + (sic(), None),
           "tric64": sheared_alloy64(SEEDS["tric64"]) + (sic(), None),
           "gas37": gas37(SEEDS["gas37"]) + (sic(), None),
           "s3_64": alloy64(SEEDS["s3_64"], S=3, a0=4.9) + (sicge(), None),
           "replicas": (x3, box, ty16, sic(), 16),
           "skin": (R1.skin_step(alloy[0], SEEDS["skin"]), alloy[1], alloy[2], sic(), None),
           "traj": zincblende(4.36, 0.1, SEEDS["traj"]) + (sic(), None),
           "zb_perfect": zincblende(4.36) + (sic(), None)}
    return out
