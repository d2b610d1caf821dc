"""Times the tabulated embedded-atom kernels (csrc/eam_table.hip through interface.EAM) against the Sutton-Chen kernels
(csrc/eam.hip through interface.SuttonChen) on the same list: force (one evaluation, no node gradient) and force_vjp (forces,
H w and the parameter part) of both terms.

    python tools/kbench_eam_table.py [--reps 20] [--inner 20] [--replicas 64] [--nodes 64,1024]

Size: `replicas` copies of 108 jittered copper atoms (3 x 3 x 3 fcc cells, rc = 5.2: rows of ~54).  The tables are those of
EAM.from_sutton_chen on its default rho grid (half the lowest to 1.5 times the highest density of the lattice), so both terms
compute the same potential and every lookup falls inside its grid.  Every timed window runs `inner` evaluations and ends in a
device synchronise; the figure is the median over `reps` windows divided by `inner`, after two warm-up windows; the two terms
alternate window by window.  The neighbour list is built once, outside the windows.  For kernel times run the same command
under `rocprofv3 --kernel-trace --stats` (the kernels are et_density_kernel, et_force_kernel, et_zero_kernel, et_finish_kernel
against eam_density_kernel, eam_force_kernel)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd.interface import EAM, SuttonChen  # noqa: E402
from mdgrad_amd.system import System  # noqa: E402

DEV = "cuda:0"


def fcc(cells, a0):
    g = np.stack(np.meshgrid(np.arange(cells), np.arange(cells), np.arange(cells), indexing="ij"), -1).reshape(-1, 3)
    basis = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
    return ((g[:, None, :] + basis[None]).reshape(-1, 3)) * a0, cells * a0


def window(fn, inner):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--nodes", default="64,1024")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    pos, L = fcc(3, 3.61)
    n, R = pos.shape[0], a.replicas
    rng = np.random.default_rng(108)
    system = System(positions=pos, cell=np.array([L, L, L]), masses=np.full(n, 63.546), device=DEV).replicate(R)
    x = torch.tensor(np.mod(np.tile(pos, (R, 1)) + rng.normal(0, 0.15, (n * R, 3)), L), dtype=torch.float32, device=DEV)
    w = torch.randn(n * R, 3, device=DEV)
    sc = SuttonChen.copper(system, cutoff=5.2)
    sc._reset_topology(x)
    rows = [("sutton-chen force", lambda: sc.force(x)), ("sutton-chen force_vjp", lambda: sc.force_vjp(x, w))]
    for nodes in (int(v) for v in a.nodes.split(",")):
        tab = EAM.from_sutton_chen(system, "copper", cutoff=5.2, r_min=1.8, n_r=nodes, n_rho=nodes)
        tab._reset_topology(x)
        rows += [("table(%d) force" % nodes, lambda t=tab: t.force(x)), ("table(%d) force_vjp" % nodes, lambda t=tab: t.force_vjp(x, w)),
                 ("table(%d) force_vjp, frozen" % nodes, lambda t=tab: t.force_vjp(x, w, want_theta=False))]
    edges = int(sc._ell.cnt.sum().item())
    print("%d atoms (%d x %d), %d list entries" % (n * R, R, n, edges), flush=True)
    for _, fn in rows:
        for _ in range(2):
            window(fn, a.inner)
    ts = {name: [] for name, _ in rows}
    for _ in range(a.reps):
        for name, fn in rows:
            ts[name].append(window(fn, a.inner))
    for name, _ in rows:
        t = float(np.median(ts[name]))
        print("  %-32s %9.1f us   %8.2f G entries/s   (min %.1f, max %.1f us)" % (name, 1e6 * t, edges / t * 1e-9, 1e6 * min(ts[name]),
                                                                                1e6 * max(ts[name])), flush=True)


if __name__ == "__main__":
    main()
