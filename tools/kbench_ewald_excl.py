"""Times one force_vjp of the Ewald correction for excluded pairs (csrc/ewald_excl.hip through interface.EwaldExclusions)
beside the real-space term's (csrc/coulomb.hip) and the reciprocal term's (csrc/ewald.hip) on the same system: what the third
member of the sum adds per adjoint step of a molecular model.

    python tools/kbench_ewald_excl.py [--reps 11] [--inner 200] [--molecules 16]

System: a water box of molecules^3 three-site molecules (default 16^3 = 4 096 molecules, 12 288 atoms, 12 288 excluded pairs)
on a grid of spacing 3.1 with seeded random orientations, through ewald(cutoff = 9.0, accuracy = 1e-4, ex_pairs = the
intramolecular pairs).  Rows: force and force_vjp (with the charge part; per-type charges trainable) called from Python, and
force_vjp without the charge part replayed from a captured HIP graph of `graph_len` calls (the device-side time of a step inside
a replayed trajectory).  Every timed window runs `inner` evaluations and ends in a device synchronise; the figure is the median
over `reps` windows divided by `inner`, after two warm-up windows."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd.interface import ewald  # noqa: E402
from mdgrad_amd.system import System  # noqa: E402

DEV = "cuda:0"
GRAPH_LEN = 20


def water_box(m, spacing=3.1, seed=0):
    """(positions [3 m^3, 3], types, intramolecular pairs [3 m^3, 2], box length): O at the grid points, H at distance 1 under
    109.47 degrees, every molecule rotated by the Q factor of a seeded normal matrix."""
    rng = np.random.default_rng(seed)
    th = np.radians(109.47)
    tmpl = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [np.cos(th), np.sin(th), 0.0]])
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)
    Q = np.linalg.qr(rng.normal(0, 1, (len(g), 3, 3)))[0]
    pos = ((g + 0.5) * spacing)[:, None, :] + np.einsum("ak,mjk->maj", tmpl, Q)
    o = 3 * np.arange(len(g))
    pairs = np.stack([np.stack([o, o + 1], 1), np.stack([o, o + 2], 1), np.stack([o + 1, o + 2], 1)], 1).reshape(-1, 2)
    return pos.reshape(-1, 3), np.tile(np.array([0, 1, 1]), len(g)), pairs, m * spacing


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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def graphed(fn):
    """fn captured GRAPH_LEN times in one graph; returns the replay callable."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_LEN):
            fn()
    return g.replay


def case(a):
    pos, types, pairs, L = water_box(a.molecules)
    n = pos.shape[0]
    rng = np.random.default_rng(1)
    system = System(positions=pos, cell=np.array([L, L, L]), masses=np.full(n, 15.999), device=DEV)
    x = torch.tensor(np.mod(pos + rng.normal(0, 0.05, pos.shape), L), dtype=torch.float32, device=DEV)
    w = torch.randn(n, 3, device=DEV)
    terms = ewald(system, [-0.82, 0.41], 9.0, accuracy=1e-4, types=types, trainable=True, ex_pairs=pairs)
    real, rec, excl = terms["coulomb_real"], terms["coulomb_recip"], terms["coulomb_excl"]
    real._reset_topology(x)
    real.prepare_pass()
    print("water box: %d atoms, %d excluded pairs, alpha %.3f, rc 9.0, %d real-space pairs; k_cutoff %.2f, %d vectors"
          % (n, excl.table().n_pairs, real.alpha, int(real._ell.cnt.sum().item()) // 2, rec.k_cutoff, rec.n_vectors), flush=True)
    members = (("real-space", real), ("reciprocal", rec), ("exclusions", excl))
    rows = [("%s  force" % nm, (lambda m: lambda: m.force(x))(m), 1) for nm, m in members]
    rows += [("%s  force_vjp" % nm, (lambda m: lambda: m.force_vjp(x, w))(m), 1) for nm, m in members]
    try:
        rows += [("%s  force_vjp, graph replay" % nm, graphed((lambda m: lambda: m.force_vjp(x, w, want_theta=False))(m)), GRAPH_LEN)
                 for nm, m in members]
    except Exception as e:                                   # (a capture that the runtime refuses: report, keep the eager rows)
        print("  graph capture failed: %r" % (e,), flush=True)
    for name, fn, per in rows:
        med, lo, hi = timed(fn, a.reps, max(1, a.inner // per))
        print("  %-38s %8.1f us   (windows %.1f .. %.1f)" % (name, 1e6 * med / per, 1e6 * lo / per, 1e6 * hi / per), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--molecules", type=int, default=16, help="molecules per box edge")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    case(a)


if __name__ == "__main__":
    main()
