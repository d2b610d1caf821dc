"""The float64 definition of observable.bond_order for the tests, in CPU torch, built on the addition theorem

    4 pi / (2l+1) sum_m A_lm(i) A_lm(j) = S_l[i, j] = sum_{b in row(i)} sum_{b' in row(j)} w_b w_b' P_l(s_b . s_b')

with Legendre polynomials only -- no spherical harmonics, so it is independent of the kernels' basis:

    q_l(i) = sqrt(S_l[i, i]) / n_i        Q_l = sqrt(sum_ij S_l[i, j]) / sum_i n_i        n_i = sum_b w_b

bond_order64 takes the float32 positions the kernels see, cast to float64, with the kernels' neighbour rule (u = x_j - x_i
re-imaged by u - L clamp(rint(u / L), -1, 1), r < cutoff, i != j, the mask), the same w(r) and the same floor rule (q <= q_floor:
a constant), and returns values, the gradient of  sum G q + sum H Q + sum C S  from float64 autograd, and the error bounds a
float32 evaluation is allowed (derived in tests/test_gpu_bond_order.py's docstring).

harmonics() is something else: a transcription of the recurrences of csrc/bond_order.hip in numpy, in float32 or float64.  The
tests use it only to MEASURE the rounding constants of those recurrences (float32 against float64 of the same formula) and to
rehearse the bounds without a GPU; the float64 run is itself checked against the addition theorem."""
import math

import numpy as np
import torch

EPS = 2.0 ** -24
# Rounding constants of the harmonic recurrences in units of 2^-24: KAPPA[l] bounds |Y32 - Y64|_2 / |Y_l|_2 over the 2l+1
# components of one bond, KAPPA_G[l] bounds the Frobenius error of the tangential gradient over sqrt(l (l+1)) |Y_l|_2.  Four times
# the largest figure of measure_kappa() (tests/test_bond_order_host.py asserts that and prints the measured figures).
KAPPA = {1: 12, 2: 32, 3: 64, 4: 100, 5: 140, 6: 176, 7: 224, 8: 288, 9: 352, 10: 416, 11: 496, 12: 576}
KAPPA_G = {1: 16, 2: 28, 3: 48, 4: 72, 5: 88, 6: 120, 7: 144, 8: 176, 9: 208, 10: 240, 11: 272, 12: 336}


# ---------------------------------------------------------------------------------------------- the definition
def legendre(lmax, t):
    """[P_0(t), ..., P_lmax(t)] by Bonnet's recurrence."""
    out = [torch.ones_like(t), t]
    for k in range(2, lmax + 1):
        out.append(((2 * k - 1) * t * out[-1] - (k - 1) * out[-2]) / k)
    return out[:lmax + 1]


def switch(r, r_in, cutoff):
    t = (r - r_in) / (cutoff - r_in)
    w = 0.5 * (1.0 + torch.cos(math.pi * t))
    return torch.where(r <= r_in, torch.ones_like(r), torch.where(r < cutoff, w, torch.zeros_like(r)))


def rows(x, L, cutoff, mask=None):
    """The padded neighbour rows of one frame x [N, 3] (float64 tensor): idx [N, M], valid [N, M], raw |x_j - x_i| [N, M]."""
    with torch.no_grad():
        N = x.shape[0]
        d = x[None, :, :] - x[:, None, :]
        raw = d.norm(dim=-1)
        d = d - L * torch.clamp(torch.round(d / L), -1, 1)
        nb = (d.norm(dim=-1) < cutoff) & ~torch.eye(N, dtype=torch.bool)
        if mask is not None:
            nb &= torch.as_tensor(np.asarray(mask)).bool()
        cnt = nb.sum(1)
        M = max(int(cnt.max()), 1)
        idx = torch.argsort((~nb).to(torch.int8), dim=1, stable=True)[:, :M]
        valid = torch.arange(M)[None, :] < cnt[:, None]
    return idx, valid, torch.gather(raw, 1, idx)


def bonds(x, L, cutoff, r_in, idx, valid):
    """s [N, M, 3], r [N, M], w [N, M] of the padded rows (differentiable in x); padding entries have w = 0, s = e_x."""
    u = x[idx] - x[:, None, :]
    u = u - L * torch.clamp(torch.round(u.detach() / L), -1, 1)
    u = torch.where(valid[..., None], u, torch.tensor([1.0, 0.0, 0.0], dtype=x.dtype))
    r = u.norm(dim=-1)
    return u / r[..., None], r, switch(r, r_in, cutoff) * valid


def _chunks(N, M):
    step = max(1, 400000 // max(1, M * N * M))
    return [(a, min(N, a + step)) for a in range(0, N, step)]


def bond_order64(x, L, cutoff, r_in, ls, mask=None, G=None, H=None, C=None, q_floor=None):
    """One frame (one replica) x [N, 3].  Returns a dict of numpy float64 arrays:
      q [N, n_l], Q [n_l], n [N], S [n_l, N, N], cnt [N]
      gx [N, 3]    d(sum G q + sum H Q + sum C S)/dx   (G [N, n_l], H [n_l], C [n_l, N, N]; missing ones are zero)
      below [N, n_l], Below [n_l]   where the floor rule made q_l(i), Q_l a constant
      tol_q [N, n_l], tol_Q [n_l], tol_S [n_l, N, N], tol_g [N]   the float32 error bounds;  gabs [N] the absolute-value sum of
      the gradient terms of an atom (the scale tol_g is built on)."""
    if q_floor is None:
        from mdgrad_amd.observable import BOND_ORDER_Q_FLOOR as q_floor
    ls = [int(l) for l in ls]
    nl, lmax = len(ls), max(ls)
    x32 = np.asarray(x, dtype=np.float32)
    N = x32.shape[0]
    Lt = torch.as_tensor(np.asarray(L, dtype=np.float32).astype(np.float64)).reshape(3)
    cutoff, r_in = float(np.float32(cutoff)), float(np.float32(r_in))
    xq = torch.tensor(x32, dtype=torch.float64, requires_grad=True)
    idx, valid, raw = rows(xq.detach(), Lt, cutoff, mask)
    M = idx.shape[1]
    cnt = valid.sum(1)

    def S_rows(a, b, s, w):
        t = torch.einsum("imc,jnc->imjn", s[a:b], s)
        P = legendre(lmax, t)
        return torch.stack([torch.einsum("im,imjn,jn->ij", w[a:b], P[l], w) for l in ls])        # [n_l, b - a, N]

    # pass 1: the values
    with torch.no_grad():
        s0, r0, w0 = bonds(xq, Lt, cutoff, r_in, idx, valid)
        S = torch.cat([S_rows(a, b, s0, w0) for a, b in _chunks(N, M)], 1)
        n = w0.sum(1)
    # the small graph: (q, Q, loss) as functions of (S, n)
    Sl, nl_ = S.clone().requires_grad_(True), n.clone().requires_grad_(True)

    def floored(num2, den):
        """sqrt(num2) / den: 0 where den = 0; at or below the floor a constant, and the sqrt never sees the 0 it cannot differentiate"""
        with torch.no_grad():
            has = den > 0
            val = torch.where(has, num2.clamp_min(0.0).sqrt() / torch.where(has, den, torch.ones_like(den)), torch.zeros_like(num2))
            live = val > q_floor
        return torch.where(live, torch.where(live, num2, torch.ones_like(num2)).sqrt() / torch.where(live, den, torch.ones_like(den)), val), ~live

    q, below = floored(torch.diagonal(Sl, dim1=1, dim2=2).t(), nl_[:, None].expand(N, nl))            # [N, n_l]
    Q, Below = floored(Sl.sum((1, 2)), nl_.sum().expand(nl))
    Gt = torch.zeros(N, nl, dtype=torch.float64) if G is None else torch.as_tensor(np.asarray(G, dtype=np.float32)).double()
    Ht = torch.zeros(nl, dtype=torch.float64) if H is None else torch.as_tensor(np.asarray(H, dtype=np.float32)).double()
    Ct = torch.zeros(nl, N, N, dtype=torch.float64) if C is None else torch.as_tensor(np.asarray(C, dtype=np.float32)).double()
    loss = (Gt * q).sum() + (Ht * Q).sum() + (Ct * Sl).sum()
    if loss.requires_grad:
        W, dn = torch.autograd.grad(loss, (Sl, nl_), allow_unused=True)
        W = torch.zeros_like(S) if W is None else W
        dn = torch.zeros_like(n) if dn is None else dn
    else:
        W, dn = torch.zeros_like(S), torch.zeros_like(n)
    # pass 2: the chain rule through S and n, a chunk of rows at a time
    for a, b in _chunks(N, M):
        s, r, w = bonds(xq, Lt, cutoff, r_in, idx, valid)
        ((S_rows(a, b, s, w) * W[:, a:b]).sum() + (w[a:b].sum(1) * dn[a:b]).sum()).backward()
    gx = xq.grad if xq.grad is not None else torch.zeros_like(xq)

    # ------------------------------------------------------------------ the float32 error bounds (see test_gpu_bond_order.py)
    with torch.no_grad():
        zone = ((r0 > r_in) & (r0 < cutoff) & valid).double()
        dr = cutoff - r_in
        W1 = zone * (0.5 * math.pi / dr)
        geo = (raw + r0) / r0 * valid                                    # |delta u| / r in units of 2^-24
        dw = EPS * (W1 * r0 * geo + 8.0 * zone)                          # |delta w| of a bond
        cn = cnt.double()[:, None]
        en = (EPS * w0 * cn + dw).sum(1)
        efwd = torch.stack([(EPS * w0 * (KAPPA[l] + math.sqrt(l * (l + 1)) * geo + cn + 2.0) + dw).sum(1) for l in ls], 1)   # [N, n_l]
        nsafe = torch.where(n > 0, n, torch.ones_like(n))
        l_t = torch.tensor(ls, dtype=torch.float64)
        tol_q = (efwd + en[:, None]) / nsafe[:, None] + EPS * (2 * l_t + 8)[None, :]
        tol_Q = (efwd.sum(0) + en.sum()) / max(float(n.sum()), 1e-300) + EPS * (N + 2 * l_t + 8)
        tol_S = (efwd.t()[:, :, None] * n[None, None, :] + n[None, :, None] * efwd.t()[:, None, :]
                 + EPS * (2 * l_t + 4)[:, None, None] * n[None, :, None] * n[None, None, :]) * 1.001
        # cotangents: gamma_l(i) = sqrt((2l+1)/(4 pi)) |dLoss/dA_l(i)|_2 = sqrt(diag(V S V^T)), V = W + W^T
        V = W + W.transpose(1, 2)
        gamma = torch.einsum("lij,ljk,lik->li", V, S, V).clamp_min(0.0).sqrt()                       # [n_l, N]
        dgamma = 2.0 * torch.einsum("lij,jl->li", V.abs(), efwd) + gamma * EPS * (N + 16)
        Ga, Ha = Gt.abs() * (~below), Ht.abs() * (~Below)
        dgn = 2.0 * ((Ga * tol_q).sum(1) / nsafe + (Ha * tol_Q).sum() / max(float(n.sum()), 1e-300)) + 8 * EPS * dn.abs()
        gabs = torch.zeros(N, dtype=torch.float64)
        tol_g = torch.zeros(N, dtype=torch.float64)
        gj = lambda v: v[idx] * valid                                   # a per-atom quantity at the row's neighbours
        wr = w0 / r0
        gnc, dgnc = dn.abs()[:, None] + gj(dn.abs()), dgn[:, None] + gj(dgn)
        gabs += (gnc * W1).sum(1)
        tol_g += (dgnc * W1 + EPS * gnc * W1 * (8.0 + math.pi / dr * r0 * geo)).sum(1)
        for k, l in enumerate(ls):
            ll = math.sqrt(l * (l + 1))
            Gm, dGm = gamma[k][:, None] + gj(gamma[k]), dgamma[k][:, None] + gj(dgamma[k])
            base = W1 + wr * ll
            gabs += (Gm * base).sum(1)
            tol_g += (dGm * base + EPS * Gm * (W1 * (KAPPA[l] + ll * geo + 8.0 + math.pi / dr * r0 * geo)
                                               + wr * ll * (KAPPA_G[l] + (l + 2) * geo + 8.0)) + Gm * ll / r0 * dw).sum(1)
        tol_g += EPS * (cn[:, 0] * nl + 4.0) * gabs
    out = dict(q=q, Q=Q, n=n, S=S, cnt=cnt, gx=gx, below=below, Below=Below, tol_q=tol_q, tol_Q=tol_Q, tol_S=tol_S, tol_g=tol_g,
               gabs=gabs)
    return {k: v.detach().numpy() for k, v in out.items()}


def smear64(values, weights, offsets, width):
    """GaussianSmearing(values).sum(0) with per-value weights, normalised: float64 torch, differentiable."""
    coeff = -0.5 / width ** 2
    raw = (weights[:, None] * torch.exp(coeff * (values[:, None] - offsets[None, :]) ** 2)).sum(0)
    return raw / raw.sum()


# ---------------------------------------------------------------------------------------------- the kernels' recurrences
def _tables(l):
    """(na [l+1], nz [l+1]) of csrc/bond_order.hip in float64: (m ? sqrt2 : 1) N_lm (2m-1)!! and the same times (2m+1)."""
    na, nz, df = [], [], 1.0
    for m in range(l + 1):
        if m:
            df *= 2 * m - 1
        nlm = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - m) / math.factorial(l + m)) * (math.sqrt(2.0) if m else 1.0)
        na.append(nlm * df)
        nz.append(nlm * df * (2 * m + 1))
    return na, nz


def harmonics(u, l, dtype):
    """(Y [n, 2l+1], r dY/du [n, 2l+1, 3]) of the bond vectors u [n, 3] as csrc/bond_order.hip evaluates them, in `dtype`
    arithmetic (numpy; no fused multiply-adds): s = u / |u|, the q_l^m recurrences, C_m / S_m, and the tangential projection.
    Component order: index l - m holds S_m, l holds m = 0, l + m holds C_m."""
    f = dtype
    u = np.asarray(u, dtype=f)
    r = np.sqrt(u[:, 2] * u[:, 2] + (u[:, 1] * u[:, 1] + u[:, 0] * u[:, 0]))
    inv = f(1.0) / r
    x, y, c = u[:, 0] * inv, u[:, 1] * inv, u[:, 2] * inv
    na, nz = _tables(l)
    n = len(u)
    qs = []
    for m in range(l + 1):
        p2, p1 = np.ones(n, f), (np.ones(n, f) if l == m else f(2 * m + 1) * c)
        for k in range(m + 2, l + 1):
            p2, p1 = p1, (f((2.0 * k - 1.0) / (k - m)) * c) * p1 - f((k + m - 1.0) / (k - m)) * p2
        qs.append(p1)
    Cs, Ss = [np.ones(n, f)], [np.zeros(n, f)]
    for m in range(l):
        Cs.append(Cs[m] * x - Ss[m] * y)
        Ss.append(Ss[m] * x + Cs[m] * y)
    Y = np.zeros((n, 2 * l + 1), f)
    D = np.zeros((n, 2 * l + 1, 3), f)
    for m in range(l + 1):
        qa = f(na[m]) * qs[m]
        Y[:, l + m] = qa * Cs[m]
        if m:
            Y[:, l - m] = qa * Ss[m]
            mq = f(m) * qa
            D[:, l + m, 0], D[:, l + m, 1] = mq * Cs[m - 1], -mq * Ss[m - 1]
            D[:, l - m, 0], D[:, l - m, 1] = mq * Ss[m - 1], mq * Cs[m - 1]
        if m < l:
            qz = f(nz[m]) * qs[m + 1]
            D[:, l + m, 2] = qz * Cs[m]
            if m:
                D[:, l - m, 2] = qz * Ss[m]
    s = np.stack([x, y, c], 1)
    D = D - s[:, None, :] * (D * s[:, None, :]).sum(-1, keepdims=True)
    return Y, D


def directions(n, seed):
    """float32 bond vectors of lengths 0.7 .. 1.6: random directions, then the poles, the axes, the equator and near-pole ones."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    special = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1],
               [1e-4, 0, 1], [0, 1e-4, -1], [1e-7, 1e-7, 1], [1, 1e-4, 1e-4], [3e-3, 4e-3, 1], [1, 2, 3]]
    v = np.concatenate([v, np.asarray(special, dtype=np.float64)])
    return (v * rng.uniform(0.7, 1.6, (len(v), 1))).astype(np.float32)


def measure_kappa(l, n=20000, seed=0):
    """(value figure, gradient figure) in units of 2^-24: the float32 transcription against the float64 one, largest over
    directions(n, seed)."""
    u = directions(n, seed)
    Y32, D32 = harmonics(u, l, np.float32)
    Y64, D64 = harmonics(u, l, np.float64)
    ynorm = math.sqrt((2 * l + 1) / (4 * math.pi))
    kv = np.linalg.norm(Y32.astype(np.float64) - Y64, axis=1).max() / ynorm / EPS
    kg = np.sqrt(((D32.astype(np.float64) - D64) ** 2).sum((1, 2))).max() / (ynorm * math.sqrt(l * (l + 1))) / EPS
    return float(kv), float(kg)


def moments32(x, L, cutoff, r_in, ls, mask=None):
    """(A [N, K], n [N]) of one frame in float32 numpy, bond by bond in row order as a kernel thread sums them."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    Lf = np.asarray(L, dtype=f).reshape(3)
    N = x.shape[0]
    idx, valid, _ = rows(torch.as_tensor(x.astype(np.float64)), torch.as_tensor(Lf.astype(np.float64)), float(f(cutoff)), mask)
    idx, valid = idx.numpy(), valid.numpy()
    inv_dr = f(1.0) / (f(cutoff) - f(r_in))
    A = np.zeros((N, sum(2 * l + 1 for l in ls)), f)
    n = np.zeros(N, f)
    for p in range(idx.shape[1]):
        d = x[idx[:, p]] - x
        u = d - np.clip(np.rint(d * (f(1.0) / Lf)), -1, 1).astype(f) * Lf
        u[~valid[:, p]] = (1.0, 0.0, 0.0)
        r = np.sqrt(u[:, 2] * u[:, 2] + (u[:, 1] * u[:, 1] + u[:, 0] * u[:, 0]))
        t = (r - f(r_in)) * inv_dr
        w = np.where(r <= f(r_in), f(1), np.where(r < f(cutoff), f(0.5) + f(0.5) * np.cos(np.pi * t.astype(np.float64)).astype(f), f(0)))
        w = (w * valid[:, p]).astype(f)
        n += w
        k = 0
        for l in ls:
            Y, _ = harmonics(u, l, f)          # (the kernel multiplies by its constant table once, after the sum)
            A[:, k:k + 2 * l + 1] += w[:, None] * Y
            k += 2 * l + 1
    return A, n


# ---------------------------------------------------------------------------------------------- configurations
def lattice(kind, reps, a=1.0):
    """(positions [N, 3], box [3]) of sc, fcc, bcc, diamond (cubic cells) or hcp (orthorhombic cell a, sqrt3 a, sqrt(8/3) a)."""
    basis = {"sc": [[0, 0, 0]], "bcc": [[0, 0, 0], [.5, .5, .5]], "fcc": [[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]],
             "diamond": [[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5], [.25, .25, .25], [.75, .75, .25], [.75, .25, .75],
                         [.25, .75, .75]],
             "hcp": [[0, 0, 0], [.5, .5, 0], [.5, 5.0 / 6.0, .5], [0, 1.0 / 3.0, .5]]}[kind]
    cell = np.array([1.0, math.sqrt(3.0), math.sqrt(8.0 / 3.0)]) * a if kind == "hcp" else np.array([a, a, a])
    reps = (reps,) * 3 if isinstance(reps, int) else reps
    pos = [(np.array([i, j, k]) + np.array(b)) * cell for i in range(reps[0]) for j in range(reps[1]) for k in range(reps[2])
           for b in basis]
    return np.array(pos), cell * np.array(reps)


# (kind, reps, cutoff / a, r_in / a, {l: q_l}) -- Steinhardt's values of the perfect shells
LATTICES = {
    "sc": ("sc", 3, 1.2, 1.1, {4: 0.76376, 6: 0.35355, 8: 0.71807}),
    "fcc": ("fcc", 2, 0.85, 0.8, {4: 0.19094, 6: 0.57452, 8: 0.40391, 12: 0.60008}),
    "bcc8": ("bcc", 3, 0.93, 0.9, {4: 0.50918, 6: 0.62854}),
    "bcc14": ("bcc", 3, 1.1, 1.05, {4: 0.03637, 6: 0.51069}),
    "hcp": ("hcp", (3, 2, 2), 1.2, 1.1, {3: 0.07607, 4: 0.09722, 6: 0.48476}),
    "tetrahedral": ("diamond", 2, 0.55, 0.5, {3: 0.74536, 4: 0.50918, 6: 0.62854}),
}
SHELL = {"sc": 6, "fcc": 12, "bcc8": 8, "bcc14": 14, "hcp": 12, "tetrahedral": 4}

DISORDERED = dict(N=70, box=5.0, cutoff=1.6, r_in=1.3, ls=(3, 4, 6, 12), seed=3)


def disordered(n_conf=1, N=None, seed=None):
    """float32 [n_conf, N, 3] uniform positions in the box of DISORDERED, no pair closer than 0.5 (rejection)."""
    N = DISORDERED["N"] if N is None else N
    rng = np.random.default_rng(DISORDERED["seed"] if seed is None else seed)
    box = DISORDERED["box"]
    out = []
    for _ in range(n_conf):
        pts = []
        while len(pts) < N:
            p = rng.uniform(0, box, 3)
            if all(np.linalg.norm((p - o + box / 2) % box - box / 2) >= 0.5 for o in pts):
                pts.append(p)
        out.append(pts)
    return np.asarray(out, dtype=np.float32)


SPARSE = dict(box=10.0, cutoff=1.5, r_in=1.2, ls=(4, 6))


def sparse9():
    """float32 [9, 3] in a box of 10: a chain of five atoms 1.1 apart, a pair, and two atoms with nobody within 1.5."""
    return np.array([[1, 1, 1], [2.1, 1, 1], [2.1, 2.1, 1], [2.1, 2.1, 2.2], [3.2, 2.1, 2.2], [6, 6, 6], [6.5, 6.9, 6.2], [1, 8, 4],
                     [8, 2, 7.5]], dtype=np.float32)


SWITCHING = dict(box=10.0, cutoff=1.5, r_in=1.25, ls=(3, 6))


def switching():
    """float32 [6, 3]: atom 0 has a bond in the switching zone (r = 1.375), one at r = cutoff exactly (2.5 - 1.0 = 1.5 in float32:
    weight 0) and two plain ones; box 10."""
    return np.array([[1, 1, 1], [2.375, 1, 1], [1, 2.5, 1], [1, 1, 2.0], [0.25, 0.5, 0.5], [1.75, 1.625, 1.75]], dtype=np.float32)


DENSE = dict(box=5.0, cutoff=1.9, r_in=1.5, ls=(4, 6), N=70)


def dense():
    """float32 [70, 3]: 70 atoms in a cube of side 1 inside a box of 5 -- every atom has all 69 others within the cutoff of 1.9."""
    return (2.0 + np.random.default_rng(11).uniform(0, 1.0, (DENSE["N"], 3))).astype(np.float32)
