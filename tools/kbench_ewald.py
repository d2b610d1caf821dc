"""Times one force_vjp of the Ewald reciprocal term (csrc/ewald.hip through interface.EwaldReciprocal) beside the real-space
term's (csrc/coulomb.hip) on the same system: what an ionic model adds per adjoint step.

    python tools/kbench_ewald.py [--reps 11] [--inner 500]

Systems: 64 NaCl ions (2^3 conventional cells, jittered) through ewald(cutoff = 5.5, accuracy = 1e-5) -- alpha 0.617, 895 wave
vectors -- once alone and once as 64 stacked replicas.  Rows: force and force_vjp (with the charge part; charges trainable)
called from Python, and force_vjp without the charge part replayed from a captured HIP graph of `graph_len` calls (the
device-side time of a step inside a replayed trajectory).  Every timed window runs `inner` evaluations and ends in a device
synchronise; the figure is the median over `reps` windows divided by `inner`, after two warm-up windows."""
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


def case(label, n_rep, a):
    pos, q, L = nacl(2)
    n = pos.shape[0]
    rng = np.random.default_rng(n_rep)
    system = System(positions=pos, cell=np.array([L, L, L]), masses=np.full(n, 22.99), device=DEV)
    if n_rep > 1:
        system = system.replicate(n_rep)
    x = torch.tensor(np.mod(np.tile(pos, (n_rep, 1)) + rng.normal(0, 0.2, (n * n_rep, 3)), L), dtype=torch.float32, device=DEV)
    w = torch.randn(n * n_rep, 3, device=DEV)
    terms = ewald(system, q, 5.5, accuracy=1e-5, trainable=True)
    real, rec = terms["coulomb_real"], terms["coulomb_recip"]
    real._reset_topology(x)
    real.prepare_pass()
    print("%s: %d atoms (%d x %d), alpha %.3f, rc 5.5, %d pairs; k_cutoff %.2f, %d vectors"
          % (label, n * n_rep, n_rep, n, real.alpha, int(real._ell.cnt.sum().item()) // 2, rec.k_cutoff, rec.n_vectors), flush=True)
    rows = [("real-space  force", lambda: real.force(x), 1),
            ("reciprocal  force", lambda: rec.force(x), 1),
            ("real-space  force_vjp", lambda: real.force_vjp(x, w), 1),
            ("reciprocal  force_vjp", lambda: rec.force_vjp(x, w), 1)]
    try:
        rows += [("real-space  force_vjp, graph replay", graphed(lambda: real.force_vjp(x, w, want_theta=False)), GRAPH_LEN),
                 ("reciprocal  force_vjp, graph replay", graphed(lambda: rec.force_vjp(x, w, want_theta=False)), GRAPH_LEN)]
    except Exception as e:                                   # (a capture that the runtime refuses: report, keep the eager rows)
        print("  graph capture failed: %r" % (e,), flush=True)
    for name, fn, per in rows:
        med, lo, hi = timed(fn, a.reps, max(1, a.inner // per))
        print("  %-38s %8.1f us   (windows %.1f .. %.1f)" % (name, 1e6 * med / per, 1e6 * lo / per, 1e6 * hi / per), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--inner", type=int, default=500)
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    case("one system", 1, a)
    case("64 replicas", 64, a)


if __name__ == "__main__":
    main()
