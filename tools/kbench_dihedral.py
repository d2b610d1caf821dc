"""Times the dihedral observable kernels (csrc/dihedral.hip through observable.dihedral_distribution): forward, and forward +
backward, and prints dihedral angles per second.

    python tools/kbench_dihedral.py [--reps 5] [--replicas 4096] [--frames 50] [--beads 24] [--nbins 72]

Shape: `replicas` x `frames` frames of a `beads`-bead helical chain (21 dihedrals at 24 beads) with Gaussian jitter, wrapped
into a box of 12; every frame goes through Dihedrals' per-term kernel and the periodic histogram, the backward pass through
the histogram's elementwise gradient and the atom-centric gradient kernel."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd.observable import dihedral_distribution  # noqa: E402
from mdgrad_amd.system import System  # noqa: E402
from mdgrad_amd.topology import chain_dihedrals  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replicas", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--beads", type=int, default=24)
    ap.add_argument("--nbins", type=int, default=72)
    a = ap.parse_args()
    i = np.arange(a.beads)
    base = np.stack([np.cos(1.0 * i), np.sin(1.0 * i), 0.5 * i], 1) + 3.0
    L = 12.0
    system = System(positions=np.mod(base, L), cell=np.array([L, L, L]), masses=np.full(a.beads, 1.008), device=DEV)
    obs = dihedral_distribution(system, chain_dihedrals(a.beads), a.nbins, keep_angles=False)
    F = a.replicas * a.frames
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.remainder(torch.tensor(base, dtype=torch.float32, device=DEV) + 0.1 * torch.randn(F, a.beads, 3, device=DEV, generator=g), L)
    target = torch.full((a.nbins,), 1.0 / a.nbins, device=DEV)
    n_angles = F * obs.n_terms

    def fwd():
        return obs(x)[1]

    def fwd_bwd():
        xx = x.detach().requires_grad_(True)
        torch.autograd.grad((obs(xx)[1] - target).pow(2).sum(), xx)

    print("device:", torch.cuda.get_device_name(0), flush=True)
    res = {}
    for label, fn in (("fwd", fwd), ("fwd+bwd", fwd_bwd)):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res[label] = float(np.median(ts))
    print("%d replicas x %d frames x %d beads, %d bins: %.3e angles  fwd %.3f ms (%.2e /s)  fwd+bwd %.3f ms (%.2e /s)  [medians of %d]"
          % (a.replicas, a.frames, a.beads, a.nbins, n_angles, 1e3 * res["fwd"], n_angles / res["fwd"], 1e3 * res["fwd+bwd"],
             n_angles / res["fwd+bwd"], a.reps), flush=True)


if __name__ == "__main__":
    main()
