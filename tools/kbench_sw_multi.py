"""Times one ops.sw_multi_eval call (csrc/sw_multi.hip) at each level against ops.sw_eval (csrc/sw.hip) on the same positions
and the same neighbour list, and one thermo.StillingerWeberEnergy call (csrc/sw_frames.hip) forward and forward + backward.

    python tools/kbench_sw_multi.py [--cells 7,28] [--repeats 7] [--frames 4096] [--against <another checkout> [--this-first]]

Jittered diamond silicon (a0 = 5.431, 0.1 A), cells^3 conventional cells of 8 atoms: 2 744 atoms at 7, 175 616 at 28.  Every
atom is silicon; the table kernel runs once with S = 1 and once with S = 2 identical sets and random types, so all three
compute the same potential.  The method is that of the "Time" table in docs/HISTORY.md: HIP events around the call from
Python, 5 warm-up calls, the median of 50 calls (30 at the large size), repeated `repeats` times with the kernels alternating;
printed are the minimum, the median and the maximum of those medians in microseconds.  LEVEL 0 = energy only, 1 = energy,
dU/dx and the per-atom parameter terms, 2 = dU/dx, H w and the parameter terms' directional derivatives.  The frame energy:
`frames` frames of 64 and of 216 atoms (jitter 0.3 A), the parameters requiring grad; backward = the gradient of sum_f g_f U_f
in (epsilon, sigma, lam).

--against: an A/B of two checkouts.  This file is run `repeats` times on each tree in turn, a fresh process each with
--repeats 1 (`--tree` names the checkout whose package is imported; only public entry points are used, so the file of the
newer checkout serves both); printed are min / median / max of each tree's `repeats` medians, side by side, and whether this
tree's median lies inside or below the other's min - max.  --this-first swaps the order inside a repeat (an order check)."""
import argparse
import os
import re
import subprocess
import sys

import numpy as np

DEV = "cuda:0"
BASIS = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75], [.75, .75, .25]])
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^  (.+?)\s+min / median / max of \d+ medians:\s+[\d.]+ /\s+([\d.]+) /\s+[\d.]+ us")


def diamond(cells, a0=5.431):
    g = np.stack(np.meshgrid(np.arange(cells), np.arange(cells), np.arange(cells), indexing="ij"), -1).reshape(-1, 3)
    return ((g[:, None, :] + BASIS[None]).reshape(-1, 3)) * a0, cells * a0


def timed(fn, calls):
    import torch
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


def report(rows, calls, repeats):
    med = {name: [] for name, _ in rows}
    for _ in range(repeats):
        for name, fn in rows:
            med[name].append(timed(fn, calls))
    for name, _ in rows:
        v = med[name]
        print("  %-34s min / median / max of %d medians: %8.1f / %8.1f / %8.1f us" % (name, len(v), min(v), float(np.median(v)), max(v)),
              flush=True)


def measure(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from mdgrad_amd import ops
    from mdgrad_amd.interface import StillingerWeber, StillingerWeberMulti
    from mdgrad_amd.system import System
    from mdgrad_amd.thermo import StillingerWeberEnergy
    print("device:", torch.cuda.get_device_name(0), " package:", os.path.dirname(os.path.abspath(ops.__file__)), flush=True)
    for cells in (int(c) for c in a.cells.split(",") if c):
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
            rows.append(("%d atoms: one species, %d" % (n, lv), lambda kw=kw: ops.sw_eval(ell, x, one._consts, one._theta(), **kw)))
            for name, m in (("%d atoms: table S = 1, %d" % (n, lv), m1), ("%d atoms: table S = 2, %d" % (n, lv), m2)):
                rows.append((name, lambda kw=kw, m=m: ops.sw_multi_eval(ell, x, m.types, m.n_species, m._tables(), **kw)))
        e = [float(fn()["energy"]) for _, fn in rows[:3]]
        print("%d atoms, %d list entries, U = %.4f / %.4f / %.4f eV" % (n, int(ell.cnt.sum()), e[0], e[1], e[2]), flush=True)
        report(rows, 50 if n < 100000 else 30, a.repeats)
    for cells in (2, 3) if a.frames > 0 else ():
        pos, L = diamond(cells)
        n = pos.shape[0]
        rng = np.random.default_rng(100 + cells)
        q = torch.tensor(np.mod(pos[None] + rng.normal(0, 0.3, (a.frames,) + pos.shape), L), dtype=torch.float32, device=DEV)
        system = System(positions=pos, cell=np.array([L, L, L]), masses=np.full(n, 28.0855), device=DEV)
        model = StillingerWeber.silicon(system)
        energy = StillingerWeberEnergy(system, model)
        g = torch.randn(a.frames, device=DEV)
        params = (model.epsilon, model.sigma, model.lam)
        print("%d frames of %d atoms, mean U = %.4f eV" % (a.frames, n, float(energy(q).mean())), flush=True)
        report([("%d x %d atoms: frame energy" % (a.frames, n), lambda: energy(q)),
                ("%d x %d atoms: frame energy + backward" % (a.frames, n), lambda: torch.autograd.grad((energy(q) * g).sum(), params))],
               50, a.repeats)


def against(a):
    trees = (("other", os.path.abspath(a.against)), ("this", HERE))[::-1 if a.this_first else 1]
    med = {t: {} for t, _ in trees}
    for r in range(a.repeats):
        for t, path in trees:
            cmd = [sys.executable, os.path.abspath(__file__), "--tree", path, "--repeats", "1", "--cells", a.cells, "--frames", str(a.frames)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                raise SystemExit("run %d on %s failed (%d):\n%s\n%s" % (r, path, out.returncode, out.stdout[-2000:], out.stderr[-4000:]))
            for line in out.stdout.splitlines():
                m = LINE.match(line)
                if m:
                    med[t].setdefault(m.group(1), []).append(float(m.group(2)))
            print("repeat %d on %s done" % (r + 1, path), flush=True)
    print("min / median / max of %d medians in us, one fresh process per median, the trees alternating: other = %s, this = %s"
          % (a.repeats, os.path.abspath(a.against), HERE))
    for name in med["this"]:
        o, t = med["other"].get(name, [float("nan")]), med["this"][name]
        print("  %-40s other %8.1f / %8.1f / %8.1f   this %8.1f / %8.1f / %8.1f   %s" % (
            name, min(o), float(np.median(o)), max(o), min(t), float(np.median(t)), max(t),
            "inside or below" if float(np.median(t)) <= max(o) else "ABOVE"), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="7,28")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--tree", default=HERE, help="the checkout whose mdgrad_amd is imported")
    ap.add_argument("--against", default=None, help="another checkout: alternate fresh processes on both trees")
    ap.add_argument("--this-first", action="store_true", help="with --against: start each repeat with this tree (an order check)")
    a = ap.parse_args()
    against(a) if a.against else measure(a)


if __name__ == "__main__":
    main()
