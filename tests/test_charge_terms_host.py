"""Where the conversion factor of the three point-charge terms goes, without a GPU: ops.CoulombTerm, ops.EwaldTerm and
ops.EwaldExclTerm (the shared ops._ChargeTerm) and force_vjp of their module classes, run on host stand-ins of the two
launches they are written on -- the term's `_eval` and `coulomb_charge_grad` -- against autograd of the class's own
`_torch_energy` in float64.

The stand-in of `_eval` is written from the definitions in the class docstrings: the bare sum S(x, q) of every term in
float64 torch, its derivatives by autograd, and on every output exactly the factors of the table in docs/KERNELS.md ("What the
charge kernels' outputs carry") -- FACTORS below is that table.  A factor applied twice, or not at all, by `pot_scale` or a
term's `_own` shows as a factor 1.7 (the conversion) or as a missing self / background term.

24 atoms x 2 replicas, two charge types (0.5 and -0.25: a net charge of 3 per replica, so the background term is not zero;
dyadic, so the float32 device mirror of the charges is exact), conversion 1.7, shift="force" for the Coulomb term (self_s != 0),
five excluded pairs with scales 0, 0.5 and 1.

Tolerance: 1e-12 of the largest entry -- float64 round-off on numbers of order one, the bound and the reason of
test_term_autograd_host.py."""
import math

import numpy as np
import pytest
import torch

from mdgrad_amd import ops
from mdgrad_amd.interface import CoulombPotentials, EwaldExclusions, EwaldReciprocal
from mdgrad_amd.system import System

F64 = torch.float64
N, R = 24, 2
L = np.array([7.0, 8.0, 9.0])
CONV = 1.7
TYPES = np.arange(N) % 2
EX_PAIRS = np.array([[0, 1], [2, 3], [4, 7], [5, 6], [1, 2]])
EX_SCALE = np.array([0.0, 0.5, 1.0, 0.0, 0.5])
# what the kernel's outputs carry of the conversion: (energy, grad and hw, pot and potw); 0 = not carried
FACTORS = {"coulomb": (1, 1, 0), "recip": (1, 1, 1), "excl": (1, 1, 0)}


def close(got, want, what):
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(want.shape))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), what


def _modules():
    rng = np.random.default_rng(5)
    system = System(positions=rng.uniform(0, 1, (N, 3)) * L, cell=L, masses=np.full(N, 1.008), device="cpu").replicate(R)
    kw = dict(types=TYPES, conversion=CONV, trainable=True)
    mods = {"coulomb": CoulombPotentials(system, [0.5, -0.25], 3.0, alpha=0.3, shift="force", **kw)}
    real = CoulombPotentials(system, [0.5, -0.25], 3.0, alpha=0.6, shift="none", **kw)
    mods["recip"] = EwaldReciprocal(system, real, k_cutoff=2.5)
    masked = CoulombPotentials(system, [0.5, -0.25], 3.0, alpha=0.6, shift="none", ex_pairs=EX_PAIRS, **kw)
    mods["excl"] = EwaldExclusions(system, masked, scale=EX_SCALE)
    for m in (mods["coulomb"], real, masked):
        m.double()                               # the charges in float64 (in place: the Ewald members hold the same Parameter)
    x = torch.tensor(rng.uniform(0, 1, (R * N, 3)) * L, dtype=F64)
    w = torch.tensor(rng.normal(0, 1, (R * N, 3)), dtype=F64)
    return mods, x, w


# ------------------------------------------------------------------------------------------------ the bare sums S(x, q)
def _min_image(d):
    cell = torch.as_tensor(L)
    return d - cell * torch.floor(d / cell + 0.5)


def _coulomb_sum(mod, x, q):
    """1/2 sum_i sum_{j in row(i)} q_i q_j psi(r_ij) inside every replica (no conversion, no self term)."""
    k = mod._consts
    iu = torch.triu_indices(N, N, offset=1)
    total = 0.0
    for r in range(R):
        xr, qr = x[r * N:(r + 1) * N], q[r * N:(r + 1) * N]
        d2 = _min_image(xr[iu[0]] - xr[iu[1]]).pow(2).sum(-1)
        inside = d2 < k.rc ** 2
        rr = torch.where(inside, d2, torch.ones_like(d2)).sqrt()
        psi = torch.erfc(k.alpha * rr) / rr - k.c0 + k.c1 * (rr - k.rc)
        total = total + torch.where(inside, qr[iu[0]] * qr[iu[1]] * psi, torch.zeros_like(psi)).sum()
    return total


def _recip_sum(mod, x, q):
    """sum_replicas sum_{k in half space} c(k) |rho(k)|^2 (no conversion, no background)."""
    t = mod.table()
    kv = 2.0 * math.pi * t.n_host.to(F64) / torch.as_tensor(L)
    ph = x.matmul(kv.t())
    A = (q[:, None] * torch.cos(ph)).reshape(R, N, -1).sum(1)
    B = (q[:, None] * torch.sin(ph)).reshape(R, N, -1).sum(1)
    return (ops.ewald_coef(t.k2_host, float(np.prod(L)), mod.alpha) * (A * A + B * B)).sum()


def _excl_sum(mod, x, q):
    """sum_{p, every replica} q_i q_j (s_p - erf(alpha r)) / r (no conversion)."""
    rep = (torch.arange(R) * N)[:, None]
    i = (torch.as_tensor(EX_PAIRS[:, 0])[None, :] + rep).reshape(-1)
    j = (torch.as_tensor(EX_PAIRS[:, 1])[None, :] + rep).reshape(-1)
    s = torch.as_tensor(EX_SCALE).repeat(R)
    r = _min_image(x[i] - x[j]).pow(2).sum(-1).sqrt()
    return (q[i] * q[j] * (s - torch.erf(mod.alpha * r)) / r).sum()


SUMS = {"coulomb": _coulomb_sum, "recip": _recip_sum, "excl": _excl_sum}


# ------------------------------------------------------------------------------------------------ the stand-ins
def _eval_standin(name, mod):
    """`_eval` of the term's kernel on the host: dict(energy, grad, hw, pot, potw) with the factors of FACTORS[name]."""
    fe, fx, fq = (CONV if c else 1.0 for c in FACTORS[name])

    def _eval(term, xyz, w=None, energy=True, grad=True, into=None, scale=1.0, want_pot=False):
        assert into is None
        x = xyz.detach().to(F64).requires_grad_(True)
        q = term.q_atom.detach().to(F64).requires_grad_(True)
        S = SUMS[name](mod, x, q)
        gx, gq = torch.autograd.grad(S, (x, q), create_graph=True)
        o = dict(energy=None, grad=None, hw=None, pot=None, potw=None)
        if energy:
            e = fe * S.detach()
            if name == "coulomb":                                  # the kernel's energy holds the self term
                e = e - fe * mod._consts.self_s * q.detach().pow(2).sum()
            o["energy"] = e.reshape(1)
        if grad:
            o["grad"] = scale * fx * gx.detach()
        if w is None:
            o["pot"] = fq * gq.detach() if want_pot else None
        else:
            hx, hq = torch.autograd.grad((gx * w.to(F64)).sum(), (x, q))
            o["hw"] = scale * fx * hx
            o["potw"] = fq * hq if want_pot else None
        return o
    return _eval


def _charge_grad_standin(pot, slot, n_slots):
    group = int(slot.numel()) if slot is not None else int(n_slots)
    idx = (slot.long() if slot is not None else torch.arange(group)).repeat(pot.numel() // group)
    return torch.zeros(int(n_slots), dtype=pot.dtype).index_add_(0, idx, pot)


@pytest.fixture(scope="module")
def case():
    return _modules()


@pytest.mark.parametrize("name", ["coulomb", "recip", "excl"])
def test_first_and_second_order_and_force_vjp_carry_the_conversion_once(name, case, monkeypatch):
    mods, x, w = case
    mod = mods[name]
    cls = {"coulomb": ops.CoulombTerm, "recip": ops.EwaldTerm, "excl": ops.EwaldExclTerm}[name]
    monkeypatch.setattr(cls, "_eval", _eval_standin(name, mod))
    monkeypatch.setattr(ops, "coulomb_charge_grad", _charge_grad_standin)
    # autograd of the class's own restatement
    xr = x.clone().requires_grad_(True)
    U = mod._torch_energy(xr)
    gx, gq = torch.autograd.grad(U, (xr, mod.charges), create_graph=True)
    hx, hq = torch.autograd.grad((gx * w).sum(), (xr, mod.charges))
    gq = gq.detach()
    assert float(gq.abs().max()) > 0 and float(hq.abs().max()) > 0
    # the shared ops term, with the charges of every atom in float64
    term = mod._term()
    assert type(term) is cls and isinstance(term, ops._ChargeTerm)
    term.q_atom = mod._real[0]._expand(mod.charges.detach()) if name != "coulomb" else mod._expand(mod.charges.detach())
    e, g, packed = term.first_order(x, energy=True)
    close(e.reshape(()), U.detach(), "%s: the energy of first_order" % name)
    close(g, gx.detach(), "%s: dU/dx" % name)
    close(packed, gq.detach(), "%s: dU/dcharges" % name)
    e0, _, packed0 = term.first_order(x, energy=False)
    assert e0 is None and torch.equal(packed0, packed)
    hw, packed_w = term.second_order(x, w)
    close(hw, hx, "%s: H w" % name)
    close(packed_w, hq, "%s: d(w.dU/dx)/dcharges" % name)
    # force_vjp of the module class, no accum: minus the same
    F, dwF, tail = mod.force_vjp(x, w)
    close(F, -gx.detach(), "%s: F" % name)
    close(dwF, -hx, "%s: d(w.F)/dx" % name)
    assert len(tail) == 1
    close(tail[0], -hq, "%s: d(w.F)/dcharges" % name)
    assert mod.force_vjp(x, w, want_theta=False)[2] is None


def test_pot_scale_is_the_conversion_where_the_kernel_leaves_it_out(case):
    mods, _, _ = case
    assert CONV != 1.0
    assert [mods[k]._term().pot_scale for k in ("coulomb", "recip", "excl")] == [CONV, 1.0, CONV]
    assert ops._ChargeTerm.pot_scale == 1.0
