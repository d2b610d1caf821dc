"""Times one ops.sw_multi_eval call (csrc/sw_multi.hip) at each level against ops.sw_eval (csrc/sw.hip) on the same positions
and the same neighbour list.

    python tools/kbench_sw_multi.py [--cells 7,28] [--repeats 7]

Jittered diamond silicon (a0 = 5.431, 0.1 A), cells^3 conventional cells of 8 atoms: 2 744 atoms at 7, 175 616 at 28.  Every
atom is silicon; the table kernel runs once with S = 1 and once with S = 2 identical sets and random types, so all three
compute the same potential.  The method is that of the "Time" table in docs/HISTORY.md: HIP events around the call from
Python, 5 warm-up calls, the median of 50 calls (30 at the large size), repeated `repeats` times with the kernels alternating;
printed are the minimum, the median and the maximum of those medians in microseconds.  LEVEL 0 = energy only, 1 = energy,
dU/dx and the per-atom parameter terms, 2 = dU/dx, H w and the parameter terms' directional derivatives."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd import ops  # noqa: E402
from mdgrad_amd.interface import StillingerWeber, StillingerWeberMulti  # noqa: E402
from mdgrad_amd.system import System  # noqa: E402

DEV = "cuda:0"
BASIS = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75], [.75, .75, .25]])


def diamond(cells, a0=5.431):
    g = np.stack(np.meshgrid(np.arange(cells), np.arange(cells), np.arange(cells), indexing="ij"), -1).reshape(-1, 3)
    return ((g[:, None, :] + BASIS[None]).reshape(-1, 3)) * a0, cells * a0


def timed(fn, calls):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="7,28")
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    for cells in (int(c) for c in a.cells.split(",")):
        pos, L = diamond(cells)
        n = pos.shape[0]
        rng = np.random.default_rng(cells)
        pos = np.mod(pos + rng.normal(0, 0.1, pos.shape), L)
        system = System(positions=pos, cell=np.array([L, L, L]), masses=np.full(n, 28.0855), device=DEV)
        x = torch.tensor(pos, dtype=torch.float32, device=DEV)
        w = torch.randn(n, 3, device=DEV)
        one = StillingerWeber.silicon(system)
        si = StillingerWeberMulti.PUBLISHED["silicon"]
        m1 = StillingerWeberMulti(system, np.zeros(n, dtype=np.int32), [si])
        m2 = StillingerWeberMulti(system, rng.integers(0, 2, n).astype(np.int32), [si, si])
        one._reset_topology(x)
        ell = one._ell
        levels = {0: dict(energy=True, grad=False), 1: dict(energy=True, grad=True, want_theta=True),
                  2: dict(w=w, energy=False, grad=True, want_theta=True)}
        rows = []
        for lv, kw in levels.items():
            rows.append(("one species, %d" % lv, lambda kw=kw: ops.sw_eval(ell, x, one._consts, one._theta(), **kw)))
            for name, m in (("table S = 1, %d" % lv, m1), ("table S = 2, %d" % lv, m2)):
                rows.append((name, lambda kw=kw, m=m: ops.sw_multi_eval(ell, x, m.types, m.n_species, m._tables(), **kw)))
        e = [float(fn()["energy"]) for _, fn in rows[:3]]
        print("%d atoms, %d list entries, U = %.4f / %.4f / %.4f eV" % (n, int(ell.cnt.sum()), e[0], e[1], e[2]), flush=True)
        calls = 50 if n < 100000 else 30
        med = {name: [] for name, _ in rows}
        for _ in range(a.repeats):
            for name, fn in rows:
                med[name].append(timed(fn, calls))
        for name, _ in rows:
            v = med[name]
            print("  %-20s min / median / max of %d medians: %7.1f / %7.1f / %7.1f us" % (name, len(v), min(v), float(np.median(v)), max(v)),
                  flush=True)


if __name__ == "__main__":
    main()
