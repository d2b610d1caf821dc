"""A/B of two checkouts on the three point-charge terms (CoulombPotentials, EwaldReciprocal, EwaldExclusions): one SHA-256 per
output of every term on seeded inputs -- the energy, autograd's gradients in xyz and charges, the double backward, force, and
force_vjp plain, with `into=` and with an ops.ThetaAccum -- for 72 and 243 atoms, per-atom and per-type charges, 1 and 3
replicas, conversion 1.0 and units.ke.  Only the public classes are used, so the same file runs in a checkout from before a
change of the layers under them; the package imported is the one of the checkout the file lies in.

    python <checkout A>/tools/charge_ab.py > a.txt ; python <checkout B>/tools/charge_ab.py > b.txt ; diff a.txt b.txt

Every sum of these kernels runs in a fixed order, so equal bits are the expectation, not luck: a line that differs is a
changed operation, a changed order or a factor applied elsewhere."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd import ops, units  # noqa: E402
from mdgrad_amd.interface import CoulombPotentials, EwaldExclusions, EwaldReciprocal  # noqa: E402
from mdgrad_amd.system import System  # noqa: E402

DEV = "cuda:0"
SPACING = 2.0


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:24]


def case(n, per_type, n_rep, conversion):
    """The three terms on a jittered cubic lattice of n atoms (spacing 2.0, cutoff 4.5), and positions / a direction for
    n_rep replicas with their own jitter."""
    rng = np.random.default_rng(100 * n + 10 * n_rep + int(per_type))
    m = int(np.ceil(n ** (1.0 / 3.0)))
    L = np.full(3, m * SPACING)
    grid = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(m ** 3)[:n]] * SPACING
    system = System(positions=np.mod(grid + 0.5, L), cell=L, masses=np.full(n, 1.008), device=DEV)
    if n_rep > 1:
        system = system.replicate(n_rep)
    x = np.concatenate([np.mod(grid + 0.5 + rng.normal(0, 0.15, (n, 3)), L) for _ in range(n_rep)]).astype(np.float32)
    w = rng.normal(0, 1, (n_rep * n, 3)).astype(np.float32)
    if per_type:
        kw = dict(types=rng.integers(0, 3, n), conversion=conversion, trainable=True)
        q = np.array([0.41, -0.82, 0.27], dtype=np.float32)
    else:
        kw = dict(conversion=conversion, trainable=True)
        q = (rng.normal(0, 0.5, n) + 0.05).astype(np.float32)
    pairs = np.stack([np.arange(0, 2 * (n // 3), 2), np.arange(1, 2 * (n // 3), 2)], 1)
    scale = np.resize(np.array([0.0, 0.5, 1.0]), len(pairs))
    real = CoulombPotentials(system, q, 4.5, alpha=0.7, shift="none", **kw)
    masked = CoulombPotentials(system, q, 4.5, alpha=0.7, shift="none", ex_pairs=pairs, **kw)
    terms = [("coulomb", CoulombPotentials(system, q, 4.5, alpha=0.3, shift="force", **kw)),
             ("recip", EwaldReciprocal(system, real, k_cutoff=2.2)),
             ("excl", EwaldExclusions(system, masked, scale=scale))]
    return terms, torch.as_tensor(x, device=DEV), torch.as_tensor(w, device=DEV), rng


def outputs(mod, x, w, rng):
    """(name, tensor) of everything the term hands out at x with the direction w."""
    mod._reset_topology(x)
    xr = x.clone().requires_grad_(True)
    U = mod(xr)
    gx, gq = torch.autograd.grad(U, (xr, mod.charges), create_graph=True)
    hx, hq = torch.autograd.grad((gx * w).sum(), (xr, mod.charges))
    out = [("energy", U), ("dU/dx", gx), ("dU/dcharges", gq), ("H w", hx), ("d(w.dU/dx)/dcharges", hq)]
    out.append(("force", mod.force(x)))
    F, dq, gth = mod.force_vjp(x, w)
    out += [("force_vjp F", F), ("force_vjp dq", dq), ("force_vjp charges", gth[0])]
    bufs = tuple(torch.as_tensor(rng.normal(0, 1, x.shape).astype(np.float32), device=DEV) for _ in range(2))
    F, dq, gth = mod.force_vjp(x, w, into=bufs)
    out += [("force_vjp into F", F), ("force_vjp into dq", dq), ("force_vjp into charges", gth[0])]
    acc = ops.ThetaAccum([mod.charges])
    acc.flat.fill_(0.25)
    F, dq, none = mod.force_vjp(x, w, accum=acc)
    assert none is None
    out += [("force_vjp accum F", F), ("force_vjp accum dq", dq), ("force_vjp accum charges", acc.flat)]
    return out


def main():
    for n in (72, 243):
        for per_type in (False, True):
            for n_rep in (1, 3):
                for conversion in (1.0, units.ke):
                    terms, x, w, rng = case(n, per_type, n_rep, conversion)
                    tag = "%3d atoms x %d  %s charges  conversion %-8.6g" % (n, n_rep, "per-type" if per_type else "per-atom", conversion)
                    for name, mod in terms:
                        for what, t in outputs(mod, x, w, rng):
                            torch.cuda.synchronize()
                            print("%s  %-7s  %-26s %s" % (tag, name, what, sha(t)))


if __name__ == "__main__":
    main()
