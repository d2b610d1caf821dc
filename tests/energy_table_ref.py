"""Reference of the tabulated pair energy of csrc/energy_table.hip (thermo.TabulatedEnergy): numpy, CPU only, all pairs.

    U      = sum_{i<j selected, 0 < d^2 < rc^2} phi~(d^2)
    dq_i   = dU/dx_i   = -sum_j 2 (dphi~/du) D,      D = x_j - x_i (minimum image)
    dT_k   = dU/dnode_k = sum_{i<j} basis_k(d^2)      k over the 2 p packed entries (phi_g, du dphi/du_g)

phi~ = the cubic-Hermite interpolant of the float32 table on the float32 grid u_g = u0 + g du, evaluated with the kernel's grid
arithmetic: t = clamp((d^2 - u0) (1 / du), 0, p - 1) with the float32 value of 1 / du, cell g = min(int(t), p - 2), fr = t - g.  A
pair with d^2 < u0 (decided on the float32 d^2, like the membership) takes the constant first node value: no position gradient,
its node gradient into entry 0, and it is counted in n_below.

The pair set is pair_forms_ref's (membership: the float32 d^2 against the float32 rc^2, and the mask); `fragile` lists its
fragile pairs.  Every quantity comes with its SCALE, the sum of the absolute summands (per atom and component for dq, per entry
for dT); errors are measured over it (pair_forms_ref.error).  `dtype=np.float32` restates the same formulas in float32: the
rounding floor of the formula itself, CPU only."""
import collections

import numpy as np

import pair_forms_ref as PF

F32 = np.float32
Result = collections.namedtuple("Result", "U dq dT n_below sU sdq sdT n_pairs")


def carrier(cutoff, mask=None):
    """the pair_forms_ref term that carries a cutoff and a mask into membership() and fragile_pairs()"""
    return PF.Term("lj", cutoff, mask)


def fragile(x, cell, cutoff, mask=None):
    return PF.fragile_pairs(x, cell, [carrier(cutoff, mask)])


def grid(cutoff, nodes, r_min):
    """(u0, du) as float32 values: the grid thermo.TabulatedEnergy hands to the kernel"""
    u0 = F32((r_min * cutoff) ** 2)
    du = F32((cutoff * cutoff - float(u0)) / (nodes - 1))
    return float(u0), float(du)


def basis(d2, u0, du, p, dt):
    """(cell g, [b0 .. b3], [d b0/du .. d b3/du]) at squared distances d2, every operation in dtype dt"""
    c = dt.type
    inv_du = c(F32(1.0) / F32(du))
    tt = np.clip((d2 - c(F32(u0))) * inv_du, c(0), c(p - 1))
    g = np.minimum(tt.astype(np.int64), p - 2)
    fr = tt - g.astype(dt)
    om = c(1) - fr
    b = [(c(1) + c(2) * fr) * om * om, fr * om * om, fr * fr * (c(3) - c(2) * fr), fr * fr * (fr - c(1))]
    s = c(6) * fr * (fr - c(1))
    d = [s * inv_du, ((c(3) * fr - c(4)) * fr + c(1)) * inv_du, -s * inv_du, (c(3) * fr - c(2)) * fr * inv_du]
    return g, b, d


def interpolate(table, u0, du, u, dtype=np.float64):
    """phi~ and dphi~/du at the squared distances u (no below-range rule: the plain clamped interpolant)"""
    dt = np.dtype(dtype)
    T = np.asarray(table, F32).astype(dt)
    p = len(T) // 2
    g, b, d = basis(np.asarray(u).astype(dt), u0, du, p, dt)
    nd = [T[2 * g], T[2 * g + 1], T[2 * g + 2], T[2 * g + 3]]
    return sum(bk * nk for bk, nk in zip(b, nd)), sum(dk * nk for dk, nk in zip(d, nd))


def evaluate(x, cell, table, u0, du, cutoff, mask=None, dtype=np.float64, member=None):
    """Result for one frame x [N, 3] (float32 values) and the float32 table [2 p]"""
    dt = np.dtype(dtype)
    T = np.asarray(table, F32).astype(dt)
    p = len(T) // 2
    member = PF.membership(x, cell, [carrier(cutoff, mask)])[0] if member is None else member
    D, _, d2 = PF._images(x, cell, dt)
    d2_32 = PF._images(x, cell, np.dtype(F32))[2]
    n = len(d2)
    i, j = np.nonzero(member)                                        # directed pairs
    Dp, d2p = D[i, j], d2[i, j]
    below = d2_32[i, j] < F32(u0)
    g, b, d = basis(d2p, u0, du, p, dt)
    nd = [T[2 * g], T[2 * g + 1], T[2 * g + 2], T[2 * g + 3]]
    phi = ((b[0] * nd[0] + b[1] * nd[1]) + b[2] * nd[2]) + b[3] * nd[3]
    pu = ((d[0] * nd[0] + d[1] * nd[1]) + d[2] * nd[2]) + d[3] * nd[3]
    cc = np.where(below, dt.type(0), dt.type(-2) * pu)
    f = cc[:, None] * Dp
    dq, sdq = np.zeros((n, 3), dt), np.zeros((n, 3), dt)
    np.add.at(dq, i, f)
    np.add.at(sdq, i, np.abs(f))
    up = i < j                                                       # each pair once
    dT, sdT = np.zeros(2 * p, dt), np.zeros(2 * p, dt)
    for k in range(4):
        np.add.at(dT, 2 * g[up] + k, b[k][up])
        np.add.at(sdT, 2 * g[up] + k, np.abs(b[k][up]))
    return Result(phi[up].sum(dtype=dt), dq, dT, int((below & up).sum()), np.abs(phi[up]).sum(dtype=dt), sdq, sdT, int(up.sum()))


def floors(ref, r32):
    """{quantity: floor}: the float32 restatement against float64, at least 2^-24"""
    return {q: max(PF.EPS, PF.error(getattr(r32, q), ref, q)) for q in ("U", "dq", "dT")}


def lj_energy_table(u0, du, p, seed=None, noise=0.0):
    """phi of LJ 12-6 (sigma = epsilon = 1) and du dphi/du on the nodes u0 + g du as float32 [2 p]; with `seed`, every entry
    carries independent noise of `noise` times the node's magnitude, so neighbouring cells differ: a wrong cell, swapped basis
    functions or a lost 1 / du moves the result by the noise"""
    u = float(F32(u0)) + float(F32(du)) * np.arange(p, dtype=np.float64)
    v = 4.0 * (u ** -6 - u ** -3)
    s = float(F32(du)) * 4.0 * (-6.0 * u ** -7 + 3.0 * u ** -4)
    if seed is not None:
        rng = np.random.default_rng(seed)
        mag = np.maximum(np.abs(v), np.abs(s))
        v = v + noise * mag * rng.standard_normal(p)
        s = s + noise * mag * rng.standard_normal(p)
    return np.stack((v, s), 1).reshape(-1).astype(F32)
