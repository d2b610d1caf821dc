"""The float64 definition behind the multi-species Stillinger-Weber tests, as CPU torch (pass float64 tensors; differentiable
where stated).  Atom i has the species t_i in [0, S); with a = t_i (the centre), b = t_j, c = t_k (LAMMPS `pair_style sw`):

    U        = 1/2 sum_i sum_{j != i} phi2_ab(r_ij) + sum_i sum_{j<k in row(i)} phi3_abc(r_ij, r_ik, cos theta_jik)
    phi2_ab  = A_ab eps_ab [B_ab (sigma_ab/r)^p_ab - (sigma_ab/r)^q_ab] exp(sigma_ab / (r - a_ab sigma_ab))   r < a_ab sigma_ab, else 0
    g_ab     = exp(gamma_ab sigma_ab / (r - a_ab sigma_ab))                                                   r < a_ab sigma_ab, else 0
    phi3_abc = K_a{bc} (cos theta - cos0_abc)^2 g_ab(r_ij) g_ac(r_ik),   K_a{bc} = (lam_abc eps3_abc + lam_acb eps3_acb) / 2

A table set `tab` is a dict: S; the [S, S] float64 arrays epsilon, sigma, a, gamma, A, B, p, q (row = centre species, column =
end species); the [S, S, S] arrays lam, epsilon3, cos0.  theta = (epsilon.flat, sigma.flat, lam.flat), 2 S^2 + S^3 numbers.

The pairs are those of coulomb_ref.half_list at the cutoff max_ab a_ab sigma_ab; every pair is two halves, phi2_ab / 2 seen
from i and phi2_ba / 2 seen from j; row(i) holds every pair atom i is part of and the triplets are the unordered pairs of
entries of one row (sw_ref.pairs_and_triplets).  An entry beyond the support of its own pair of species adds nothing.

`energy` is the definition.  `evaluate` differentiates it with float64 autograd and, for the error scales, evaluates every
pair half and every triplet on its own gathered copies of the positions and of theta: the derivative with respect to such a
copy is that one term's contribution, and the scales A_* are the explicit sums of their absolute values."""
import math

import numpy as np
import torch

import coulomb_ref as C
import sw_ref as R1
import tersoff_ref as RT

PAIR_KEYS = ("epsilon", "sigma", "a", "gamma", "A", "B", "p", "q")
TRIPLET_KEYS = ("lam", "epsilon3", "cos0")
DEFAULTS = dict(a=1.80, gamma=1.20, cos0=-1.0 / 3.0, A=7.049556277, B=0.6022245584, p=4, q=0)
SILICON, MW = R1.SILICON, R1.MW


# ---------------------------------------------------------------------------------------------- tables
def mixed(species):
    """The table set of S one-species sets under the mixing rule of StillingerWeberMulti, element by element: sigma, a, gamma
    arithmetic means, epsilon the geometric mean, A, B, p, q, cos0 of the centre, lam_ab = sqrt(lam_a lam_b), lam_abc =
    sqrt(lam_ab lam_ac), epsilon3_abc = sqrt(epsilon_ab epsilon_ac)."""
    S = len(species)
    sp = [dict(DEFAULTS, **s) for s in species]
    tab = dict(S=S, **{k: np.zeros((S, S)) for k in PAIR_KEYS}, **{k: np.zeros((S, S, S)) for k in TRIPLET_KEYS})
    for a, p in enumerate(sp):
        for b, q in enumerate(sp):
            tab["epsilon"][a, b] = math.sqrt(p["epsilon"] * q["epsilon"])
            for k in ("sigma", "a", "gamma"):
                tab[k][a, b] = 0.5 * (p[k] + q[k])
            for k in ("A", "B", "p", "q"):
                tab[k][a, b] = p[k]
            for c, r in enumerate(sp):
                lab, lac = math.sqrt(p["lam"] * q["lam"]), math.sqrt(p["lam"] * r["lam"])
                eab, eac = math.sqrt(p["epsilon"] * q["epsilon"]), math.sqrt(p["epsilon"] * r["epsilon"])
                tab["lam"][a, b, c] = math.sqrt(lab * lac)
                tab["epsilon3"][a, b, c] = math.sqrt(eab * eac)
                tab["cos0"][a, b, c] = p["cos0"]
    return tab


def unlike2():
    """Two species whose tables differ in every entry between (0,0), (0,1) = (1,0), (1,1), with cos0, lam and epsilon3
    different in each of the six (centre, {end, end}) classes; symmetric in the pair and in the ends."""
    sym = lambda x, y, z: np.array([[x, y], [y, z]], dtype=np.float64)
    tab = dict(S=2, epsilon=sym(2.1683, 1.80, 1.50), sigma=sym(2.0951, 2.00, 1.90), a=sym(1.80, 1.78, 1.75),
               gamma=sym(1.20, 1.10, 1.00), A=sym(7.049556277, 6.80, 7.30), B=sym(0.6022245584, 0.62, 0.58),
               p=sym(4, 5, 6), q=sym(0, 1, 0))
    tab["lam"] = np.stack([sym(21.0, 19.0, 17.0), sym(23.0, 20.0, 25.0)])
    tab["epsilon3"] = np.stack([sym(2.1683, 1.90, 1.70), sym(1.60, 1.75, 1.50)])
    tab["cos0"] = np.stack([sym(-1.0 / 3.0, -0.30, -0.25), sym(-0.35, -0.28, -0.40)])
    return tab


def asym2():
    """unlike2 with asymmetric pair entries and an asymmetric lam: sigma[0,1] != sigma[1,0], epsilon[0,1] != epsilon[1,0],
    lam[0,0,1] != lam[0,1,0]."""
    tab = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in unlike2().items()}
    tab["sigma"][0, 1], tab["sigma"][1, 0] = 2.05, 1.95
    tab["epsilon"][0, 1], tab["epsilon"][1, 0] = 1.90, 1.70
    tab["lam"][0, 0, 1], tab["lam"][0, 1, 0] = 19.0, 16.0
    return tab


def three():
    """Three species with three different cutoffs (a sigma = 3.77, 3.42, 3.96 for the like pairs), mixed."""
    return mixed([dict(SILICON), dict(epsilon=1.7, sigma=1.90, lam=26.0, gamma=1.1, cos0=-0.30, p=5, q=1),
                  dict(epsilon=2.5, sigma=2.20, lam=18.0, A=6.9, B=0.61)])


def pair_triplet(tab):
    """(pair, triplet) as StillingerWeberMulti.from_tables takes them."""
    return {k: tab[k] for k in PAIR_KEYS}, {k: tab[k] for k in TRIPLET_KEYS}


def theta_of(tab):
    return np.concatenate([tab["epsilon"].reshape(-1), tab["sigma"].reshape(-1), tab["lam"].reshape(-1)])


def with_theta(tab, theta):
    """The table set with (epsilon, sigma, lam) taken from the flat theta."""
    S = tab["S"]
    th = np.asarray(theta, dtype=np.float64).reshape(-1)
    out = dict(tab)
    out["epsilon"], out["sigma"] = th[:S * S].reshape(S, S).copy(), th[S * S:2 * S * S].reshape(S, S).copy()
    out["lam"] = th[2 * S * S:].reshape(S, S, S).copy()
    return out


def n_theta(tab):
    return 2 * tab["S"] ** 2 + tab["S"] ** 3


def rc_max(tab):
    return float((tab["a"] * tab["sigma"]).max())


def relabelled(tab, perm):
    """The table set with species a renamed perm[a]."""
    inv = np.argsort(np.asarray(perm))
    out = dict(S=tab["S"])
    for k in PAIR_KEYS:
        out[k] = tab[k][np.ix_(inv, inv)].copy()
    for k in TRIPLET_KEYS:
        out[k] = tab[k][np.ix_(inv, inv, inv)].copy()
    return out


# ---------------------------------------------------------------------------------------------- the definition
def pairs_and_triplets(x, cell, tab, group=None, rc=None):
    return R1.pairs_and_triplets(x, cell, rc_max(tab) if rc is None else rc, group=group)


def _types(types):
    return torch.as_tensor(np.asarray(types)).long()


def _cut(r, rc):
    inside = r < rc
    return inside, torch.where(inside, r - rc, -torch.ones_like(r))


def phi2_half(d, a, b, th, tab):
    """phi2_ab / 2 for the separation vectors d [n, 3], the species a (centre), b (end) and the parameter rows th [n, P]."""
    S = tab["S"]
    t64 = lambda k: torch.as_tensor(tab[k], dtype=d.dtype)[a, b]
    n = torch.arange(a.numel())
    eps, sig = th[n, a * S + b], th[n, S * S + a * S + b]
    r = d.pow(2).sum(-1).sqrt()
    inside, dr = _cut(r, t64("a") * sig)
    s = sig / r
    v = 0.5 * t64("A") * eps * (t64("B") * s ** t64("p") - s ** t64("q")) * torch.exp(sig / dr)
    return torch.where(inside, v, torch.zeros_like(v))


def phi3(ua, ub, a, b, c, th, tab):
    """Triplet energies for the vectors centre -> end ua, ub [n, 3] with the species a (centre), b, c (ends)."""
    S = tab["S"]
    t64 = lambda k: torch.as_tensor(tab[k], dtype=ua.dtype)
    n = torch.arange(a.numel())
    sab, sac = th[n, S * S + a * S + b], th[n, S * S + a * S + c]
    labc, lacb = th[n, 2 * S * S + (a * S + b) * S + c], th[n, 2 * S * S + (a * S + c) * S + b]
    K = 0.5 * (labc * t64("epsilon3")[a, b, c] + lacb * t64("epsilon3")[a, c, b])
    ra, rb = ua.pow(2).sum(-1).sqrt(), ub.pow(2).sum(-1).sqrt()
    ia, da = _cut(ra, t64("a")[a, b] * sab)
    ib, db = _cut(rb, t64("a")[a, c] * sac)
    cth = (ua * ub).sum(-1) / (ra * rb)
    v = K * (cth - t64("cos0")[a, b, c]) ** 2 * torch.exp(t64("gamma")[a, b] * sab / da) * torch.exp(t64("gamma")[a, c] * sac / db)
    return torch.where(ia & ib, v, torch.zeros_like(v))


def _pieces(X, TH, lst, ty, h, tab):
    """(halves seen from i, halves seen from j, triplets) on the positions X = [x_i, x_j, x_j', x_i', x_c, x_a, x_b] and the
    parameter rows TH = [for the first halves, the second halves, the triplets]."""
    ti, tj = ty[lst["i"]], ty[lst["j"]]
    off = lst["off"].to(h).matmul(h)
    v1 = phi2_half(X[0] - X[1] - off, ti, tj, TH[0], tab)
    v2 = phi2_half(X[3] - X[2] - off, tj, ti, TH[1], tab)
    ua = X[5] - X[4] + lst["oa"].to(h).matmul(h)
    ub = X[6] - X[4] + lst["ob"].to(h).matmul(h)
    v3 = phi3(ua, ub, ty[lst["tc"]], ty[lst["ta"]], ty[lst["tb"]], TH[2], tab)
    return v1, v2, v3


def _gathered(x, theta, lst):
    i, j, tc, ta, tb = lst["i"], lst["j"], lst["tc"], lst["ta"], lst["tb"]
    P = theta.numel()
    X = [x[i], x[j], x[j], x[i], x[tc], x[ta], x[tb]]
    TH = [theta[None, :].expand(i.numel(), P), theta[None, :].expand(i.numel(), P), theta[None, :].expand(tc.numel(), P)]
    return X, TH, [i, j, j, i, tc, ta, tb]


def energy(x, types, tab, lst, cell, theta=None, parts=False):
    """U (differentiable in x and in theta [2 S^2 + S^3], which defaults to the tables' own epsilon, sigma, lam); parts:
    (pair part, triplet part)."""
    theta = torch.as_tensor(theta_of(tab)).to(x) if theta is None else theta
    X, TH, _ = _gathered(x, theta, lst)
    v1, v2, v3 = _pieces(X, TH, lst, _types(types), C.cell_matrix(cell).to(x), tab)
    return (v1.sum() + v2.sum(), v3.sum()) if parts else v1.sum() + v2.sum() + v3.sum()


def evaluate(x, types, tab, lst, cell, w=None, theta=None):
    """float64 autograd of `energy`: U, grad = dU/dx, dth = dU/dtheta [2 S^2 + S^3], and with w: hw = H w, dthw =
    d(w.dU/dx)/dtheta; plus A_U, A_grad, A_dth, A_hw, A_dthw (module docstring)."""
    x = torch.as_tensor(x).detach().double()
    theta = torch.as_tensor(np.asarray(theta_of(tab) if theta is None else theta, dtype=np.float64)).reshape(-1)
    ty = _types(types)
    N, P = x.shape[0], theta.numel()
    xg, tg = x.clone().requires_grad_(True), theta.clone().requires_grad_(True)
    U = energy(xg, ty, tab, lst, cell, theta=tg)
    g, gt = torch.autograd.grad(U, (xg, tg), create_graph=w is not None, allow_unused=True)
    zeros = lambda *s: torch.zeros(*s, dtype=torch.float64)
    if g is None:
        g, gt = zeros(N, 3), zeros(P)
    out = dict(U=U.detach(), grad=g.detach(), dth=gt.detach())
    if w is not None:
        w = torch.as_tensor(w).detach().double()
        if g.requires_grad:
            hw, hth = torch.autograd.grad((g * w).sum(), (xg, tg), allow_unused=True)
            hth = zeros(P) if hth is None else hth
        else:
            hw, hth = zeros(N, 3), zeros(P)
        out["hw"], out["dthw"] = hw, hth
    Xs, THs, atoms = _gathered(x, theta, lst)
    X = [t.clone().requires_grad_(True) for t in Xs]
    TH = [t.clone().requires_grad_(True) for t in THs]
    v1, v2, v3 = _pieces(X, TH, lst, ty, C.cell_matrix(cell).double(), tab)
    out["A_U"] = v1.detach().abs().sum() + v2.detach().abs().sum() + v3.detach().abs().sum()
    fill = lambda gs, like: [zeros(*l.shape) if v is None else v for v, l in zip(gs, like)]
    A_grad, A_dth, A_hw, A_dthw = zeros(N, 3), zeros(P), zeros(N, 3), zeros(P)
    tot = v1.sum() + v2.sum() + v3.sum()
    if tot.requires_grad and lst["i"].numel():
        gs = fill(torch.autograd.grad(tot, X + TH, create_graph=w is not None, allow_unused=True), X + TH)
        for a, ga in zip(atoms, gs[:7]):
            A_grad.index_add_(0, a, ga.detach().abs())
        for gth in gs[7:]:
            A_dth += gth.detach().abs().sum(0)
        if w is not None:
            s = sum((ga * w[a]).sum() for a, ga in zip(atoms, gs[:7]))
            if s.requires_grad:
                hs = fill(torch.autograd.grad(s, X + TH, allow_unused=True), X + TH)
                for a, ha in zip(atoms, hs[:7]):
                    A_hw.index_add_(0, a, ha.abs())
                for hth in hs[7:]:
                    A_dthw += hth.abs().sum(0)
    out.update(A_grad=A_grad, A_dth=A_dth)
    if w is not None:
        out.update(A_hw=A_hw, A_dthw=A_dthw)
    return out


def energy_loops(x, types, tab, cell, group=None):
    """The same energy as plain numpy loops over every ordered pair and every (centre; j < k) triple with the minimum image
    taken per vector -- written separately from everything above.  Returns (pair part, triplet part)."""
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
    U2 = U3 = 0.0
    for c in range(N):
        lo = (c // n) * n
        a = ty[c]
        vec = []
        for e in range(lo, lo + n):
            if e == c:
                continue
            b = ty[e]
            v = image(x[e] - x[c])
            r = float(np.sqrt((v ** 2).sum()))
            sig = tab["sigma"][a, b]
            rc = tab["a"][a, b] * sig
            if r < rc and r != 0.0:
                vec.append((v, r, b, math.exp(tab["gamma"][a, b] * sig / (r - rc))))
                s = sig / r
                U2 += 0.5 * tab["A"][a, b] * tab["epsilon"][a, b] * (tab["B"][a, b] * s ** int(tab["p"][a, b])
                                                                      - s ** int(tab["q"][a, b])) * math.exp(sig / (r - rc))
        for m in range(len(vec)):
            for o in range(m + 1, len(vec)):
                (va, ra, b, ga), (vb, rb, cc, gb) = vec[m], vec[o]
                K = 0.5 * (tab["lam"][a, b, cc] * tab["epsilon3"][a, b, cc] + tab["lam"][a, cc, b] * tab["epsilon3"][a, cc, b])
                U3 += K * (float(va @ vb) / (ra * rb) - tab["cos0"][a, b, cc]) ** 2 * ga * gb
    return U2, U3


def census(x, types, tab, cell, group=None):
    """The input conditions of a configuration: pairs[a][b] = the number of directed bonds a -> b inside the support of
    (a, b); classes[a][b][c] (b <= c) = the number of triplets with the centre a and the ends {b, c}, both entries inside their
    supports; rows = the row lengths at the largest cutoff."""
    S = tab["S"]
    ty = _types(types)
    lst = pairs_and_triplets(x, cell, tab, group=group)
    X = torch.as_tensor(x).double()
    hm = C.cell_matrix(cell).double()
    rcs = torch.as_tensor(tab["a"] * tab["sigma"])
    r = (X[lst["i"]] - X[lst["j"]] - lst["off"].double().matmul(hm)).pow(2).sum(-1).sqrt()
    pairs = np.zeros((S, S), dtype=int)
    for a, b in ((ty[lst["i"]], ty[lst["j"]]), (ty[lst["j"]], ty[lst["i"]])):
        live = r < rcs[a, b]
        np.add.at(pairs, (a[live].numpy(), b[live].numpy()), 1)
    a3, b3, c3 = ty[lst["tc"]], ty[lst["ta"]], ty[lst["tb"]]
    ra = (X[lst["ta"]] - X[lst["tc"]] + lst["oa"].double().matmul(hm)).pow(2).sum(-1).sqrt()
    rb = (X[lst["tb"]] - X[lst["tc"]] + lst["ob"].double().matmul(hm)).pow(2).sum(-1).sqrt()
    live = (ra < rcs[a3, b3]) & (rb < rcs[a3, c3])
    classes = np.zeros((S, S, S), dtype=int)
    lo, hi = torch.minimum(b3, c3), torch.maximum(b3, c3)
    np.add.at(classes, (a3[live].numpy(), lo[live].numpy(), hi[live].numpy()), 1)
    return dict(pairs=pairs, classes=classes, rows=lst["rows"], r=r, ti=ty[lst["i"]], tj=ty[lst["j"]])


def cutoff_rounding(x, types, tab, cell, group=None):
    """How ill-conditioned a configuration is at float32, measured without any kernel: the largest change of a component of
    the float64 dU/dx, in units of 2^-24 A_grad, when every cutoff a_ab sigma_ab is rounded to float32 (which any float32
    evaluation must do; r itself is rounded by as much again).  exp(sigma / (r - rc)) and g have the relative slope
    sigma / (r - rc)^2 in rc: 46 / A at 0.2 A inside the cutoff, so half an ulp of rc = 3.56 (1.2e-7) moves such a term by
    5e-6 = 90 * 2^-24 of itself.  An atom whose only terms are of that kind has A as small as they are, and its error ratio
    measures this slope, not the evaluation."""
    tab = with_theta(tab, theta_of(tab).astype(np.float32).astype(np.float64))
    rounded = dict(tab)
    rounded["a"] = (tab["a"] * tab["sigma"]).astype(np.float32).astype(np.float64) / tab["sigma"]
    lst = pairs_and_triplets(x, cell, tab, group=group, rc=rc_max(tab) + 1e-3)
    a, b = evaluate(x, types, tab, lst, cell), evaluate(x, types, rounded, lst, cell)
    live = a["A_grad"] > 0
    return float(((a["grad"] - b["grad"]).abs()[live] / (2.0 ** -24 * a["A_grad"][live])).max())


def populated(cen, least=20):
    """Whether every ordered pair class and every (centre, {end, end}) class of census() holds at least `least` terms."""
    S = cen["pairs"].shape[0]
    return bool((cen["pairs"] >= least).all()) and all(cen["classes"][a, b, c] >= least
                                                        for a in range(S) for b in range(S) for c in range(b, S))


class SWMultiTerm:
    """The term with the oracle's term protocol (n_theta, reset, energy, force, force_vjp by autograd, like sw_ref.SWTerm) and
    theta = (epsilon.flat, sigma.flat, lam.flat): force_vjp's third output is d(w.F)/dtheta [2 S^2 + S^3].  The pairs and
    triplets are those of the last reset(q), searched at max a sigma."""

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
        self.lst = pairs_and_triplets(q.detach(), self.cell, self.tab, group=self.group)

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
# Every configuration below is checked on the CPU by tests/test_sw_multi_host.py (test_input_conditions_...); the seeds are
# the first for which its conditions hold.
SEEDS = dict(ab64=0, tric64=0, gas37=1, s3_64=0, replicas=3, skin=0, traj=0)
A0 = 5.431


def species_split(n, S, seed):
    """n species labels, as equal a number of each of the S as n allows, in an order drawn from `seed`."""
    return np.random.default_rng(1000 + seed).permutation(np.arange(n) % S).astype(np.int32)


def alloy64(seed, S=2, a0=A0, sigma_jit=0.3):
    """(float32 positions, float32 cell, types): a 2 x 2 x 2 diamond lattice with the species in a seeded random order and
    every coordinate jittered by a normal deviate of width sigma_jit."""
    x, cell = R1.jittered_diamond(2, a0, sigma_jit, seed)
    return x, cell, species_split(64, S, seed)


def sheared_alloy64(seed, a0=A0, sigma_jit=0.3):
    x, cell = RT.sheared_diamond(2, a0, sigma_jit, seed)
    return x, cell, species_split(64, 2, seed)


def gas37(seed):
    """tersoff_ref.gas37 (a hub with a row of 18, an isolated atom 31, a dimer 32-33, a bent trimer 34-36) with random species;
    the hub, the dimer and the trimer are species 0.  The dimer is 2.30 A long, as in the gas case of tests/test_gpu_sw.py,
    not tersoff_ref's 2.35 A: that is the minimum of phi2_00 (2^(1/6) sigma_00), where the two product-rule terms of phi2'
    cancel (4.7 eV/A each against a net 0.01 eV/A) and the net contribution A no longer scales the rounding of either --
    the perfect-lattice tests cover that point with the scale that belongs to it."""
    x, cell = RT.gas37(seed)
    x[33, 2] = x[32, 2] + np.float32(2.30)
    ty = species_split(37, 2, seed)
    ty[[0, 32, 33, 34, 35, 36]] = 0
    return x, cell, ty


def replicas16(seed):
    """(the 16 base positions, the box, float32 positions of three jittered copies, the 16 species of a replica)."""
    base, box, x3 = RT.replicas16(seed)
    return base, box, x3, species_split(16, 2, seed)


def zincblende(a, sigma_jit=0.0, seed=0):
    """(float32 positions, float32 cell, types) of 2 x 2 x 2 zincblende cells: species 0 on the fcc sites, 1 on the others."""
    x, cell = R1.jittered_diamond(2, a, sigma_jit, seed)
    return x, cell, (np.arange(64) % 8 >= 4).astype(np.int32)


def gpu_cases():
    """name -> (float32 positions, float32 cell, types of a replica, table set, group)."""
    ab = alloy64(SEEDS["ab64"])
    base, box, x3, ty16 = replicas16(SEEDS["replicas"])
    return {"ab64": ab + (unlike2(), None),
            "asym64": ab + (asym2(), None),
            "tric64": sheared_alloy64(SEEDS["tric64"]) + (unlike2(), None),
            "gas37": gas37(SEEDS["gas37"]) + (unlike2(), None),
            "s3_64": alloy64(SEEDS["s3_64"], S=3) + (three(), None),
            "replicas": (x3, box, ty16, unlike2(), 16),
            "skin": (RT.skin_step(ab[0], SEEDS["skin"]), ab[1], ab[2], unlike2(), None),
            "traj": zincblende(A0, 0.1, SEEDS["traj"]) + (unlike2(), None)}
