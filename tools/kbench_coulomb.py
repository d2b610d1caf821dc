"""Times the Coulomb kernel (csrc/coulomb.hip through interface.CoulombPotentials): force and force_vjp, against the torch
composite on the half list (CoulombPotentials._torch_energy plus autograd, single and double backward) and against
ops.pair_eval of Yukawa -- the built-in pair form closest in arithmetic (one expf per pair) -- on the same list.

    python tools/kbench_coulomb.py [--reps 20] [--inner 20]

Sizes: one system of 4 096 ions (16^3 rock-salt sites with jitter, rc = 10, alpha = 0.25) and 1 024 replicas of 64 ions
(rc = 5, alpha = 0.4).  Every timed window runs `inner` evaluations and ends in a device synchronise; the figure is the median
over `reps` windows divided by `inner`, after two warm-up windows.  Neighbour lists are built once, outside the windows."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd import ops  # noqa: E402
from mdgrad_amd.interface import CoulombPotentials, PairPotentials  # noqa: E402
from mdgrad_amd.potentials import Yukawa  # noqa: E402
from mdgrad_amd.system import System  # noqa: E402

DEV = "cuda:0"


def nacl(cells, a=5.64):
    m = 2 * cells
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)
    return g * (0.5 * a), np.where(g.sum(1) % 2 == 0, 1.0, -1.0), cells * a


def timed(fn, reps, inner):
    for _ in range(2):
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / inner)
    return float(np.median(ts))


def case(label, cells, n_rep, rc, alpha, a):
    pos, q, L = nacl(cells)
    n = pos.shape[0]
    rng = np.random.default_rng(n)
    system = System(positions=pos, cell=np.array([L, L, L]), masses=np.full(n, 22.99), device=DEV)
    if n_rep > 1:
        system = system.replicate(n_rep)
    x = torch.tensor(np.mod(np.tile(pos, (n_rep, 1)) + rng.normal(0, 0.2, (n * n_rep, 3)), L), dtype=torch.float32, device=DEV)
    w = torch.randn(n * n_rep, 3, device=DEV)
    coul = CoulombPotentials(system, q, rc, alpha=alpha, trainable=True)
    yuk = PairPotentials(system, Yukawa(1.0, alpha), cutoff=rc)
    coul._reset_topology(x)
    yuk._reset_topology(x)
    pairs = int(coul._ell.cnt.sum().item()) // 2
    theta, _ = yuk._theta(x)
    term = yuk.mdg_term(0)

    def torch_force():
        xx = x.detach().requires_grad_(True)
        torch.autograd.grad(coul._torch_energy(xx), xx)

    def torch_vjp():
        xx = x.detach().requires_grad_(True)
        (g,) = torch.autograd.grad(coul._torch_energy(xx), xx, create_graph=True)
        torch.autograd.grad((g * w).sum(), (xx, coul.charges))

    coul._ell.half_list()                                   # (the composite's list: built once, outside the windows)
    rows = [("coulomb kernel  force", lambda: coul.force(x)),
            ("coulomb kernel  force_vjp", lambda: coul.force_vjp(x, w)),
            ("yukawa pair_eval force", lambda: ops.pair_eval(yuk._ell, x, term, theta, energy=False, grad=True, scale=-1.0, theta_grads=False)),
            ("yukawa pair_eval force_vjp", lambda: ops.pair_eval(yuk._ell, x, term, theta, w=w, energy=False, grad=True, scale=-1.0)),
            ("torch composite force", torch_force),
            ("torch composite force_vjp", torch_vjp)]
    print("%s: %d atoms (%d x %d), rc %.1f, alpha %.2f, %d pairs" % (label, n * n_rep, n_rep, n, rc, alpha, pairs), flush=True)
    res = {}
    for name, fn in rows:
        res[name] = timed(fn, a.reps, a.inner if "torch" not in name else max(1, a.inner // 4))
        print("  %-28s %9.1f us   %8.2f G pairs/s" % (name, 1e6 * res[name], pairs / res[name] * 1e-9), flush=True)
    print("  kernel vs composite: force x%.1f, force_vjp x%.1f;  kernel vs yukawa pair_eval: force x%.2f, force_vjp x%.2f"
          % (res["torch composite force"] / res["coulomb kernel  force"], res["torch composite force_vjp"] / res["coulomb kernel  force_vjp"],
             res["yukawa pair_eval force"] / res["coulomb kernel  force"], res["yukawa pair_eval force_vjp"] / res["coulomb kernel  force_vjp"]),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    case("one system", 8, 1, 10.0, 0.25, a)
    case("replicas", 2, 1024, 5.0, 0.4, a)


if __name__ == "__main__":
    main()
