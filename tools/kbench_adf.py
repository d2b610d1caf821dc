"""Times the bond-angle distribution kernels (csrc/adf.hip through ops.AdfRawFn): forward, and forward + backward, with the
neighbour-list builds of the frame chunks included, and prints ordered triplets per second.

    python tools/kbench_adf.py [--reps 3] [--quick | --headline]

Shapes: the 108-atom LJ liquid (FCC a = 1.6, jittered) at 1 024 and 16 384 replicas x 50 frames, cutoff 1.5, 180 bins over
(0, pi); a 512-bead CG-water box x 50 frames (jittered simple-cubic beads at 3.1 A, cutoff 3.6 A); one 4 096-bead frame set
(the same density, 10 frames)."""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"


def lattice_fcc(size, a):
    base = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
    return np.array([(np.array([i, j, k]) + b) * a for i in range(size) for j in range(size) for k in range(size) for b in base]), a * size


def lattice_sc(n, a):
    g = np.arange(n) * a
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), a * n


def frames_of(lat, L, n_frames, sigma, seed=0):
    """[n_frames, N, 3] on the device: jittered copies, generated on the GPU in slices."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    base = torch.tensor(lat, dtype=torch.float32, device=DEV)
    out = torch.empty(n_frames, base.shape[0], 3, device=DEV)
    for f0 in range(0, n_frames, 65536):
        f1 = min(n_frames, f0 + 65536)
        out[f0:f1] = torch.remainder(base + sigma * torch.randn(f1 - f0, *base.shape, device=DEV, generator=g), L)
    return out


def n_triplets(x, cs, cutoff):
    """Ordered triplets sum cnt (cnt - 1), from the list of the first 4 096 frames (scaled)."""
    F, N = x.shape[0], x.shape[1]
    fs = min(F, max(1, 4096 * 108 // N))
    ell = ops.build_ell(x[:fs].reshape(-1, 3), cs, cutoff, None, group=N)
    c = ell.cnt.double()
    return float((c * (c - 1)).sum()) * F / fs


def bench(name, x, L, cutoff, nbins, rng, reps):
    cs = _lib.make_cell(torch.tensor([L] * 3))
    mu = torch.linspace(rng[0], rng[1], nbins, device=DEV)
    spacing = float(mu[1] - mu[0])
    coeff = float(-0.5 / torch.tensor(spacing, dtype=torch.float32) ** 2)
    trip = n_triplets(x, cs, cutoff)
    g_raw = torch.randn(nbins, device=DEV)

    def fwd():
        return ops.AdfRawFn.apply(x, mu, coeff, cutoff, cs, None, spacing)

    def fwd_bwd():
        xx = x.detach().requires_grad_(True)
        raw = ops.AdfRawFn.apply(xx, mu, coeff, cutoff, cs, None, spacing)
        torch.autograd.grad((raw * g_raw).sum(), xx)

    res = {}
    for label, fn in (("fwd", fwd), ("fwd+bwd", fwd_bwd)):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res[label] = min(ts)
    print("%-34s frames %8d  N %5d  ordered triplets %.3e  fwd %9.2f ms (%.2e /s)  fwd+bwd %9.2f ms (%.2e /s)" % (
        name, x.shape[0], x.shape[1], trip, 1e3 * res["fwd"], trip / res["fwd"], 1e3 * res["fwd+bwd"],
        trip / res["fwd+bwd"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="skip the 16 384-replica shape")
    ap.add_argument("--headline", action="store_true", help="only the 16 384-replica shape (for profiler runs)")
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), " chunk bytes:", ops.ADF_CHUNK_BYTES, flush=True)
    lat, L = lattice_fcc(3, 1.6)
    for R in ((16384,) if a.headline else (1024,) if a.quick else (1024, 16384)):
        x = frames_of(lat, L, R * 50, 0.08)
        bench("LJ108 %d replicas x 50 frames" % R, x, L, 1.5, 180, (0.0, math.pi), a.reps)
        del x
        torch.cuda.empty_cache()
    if a.headline:
        return
    lat, L = lattice_sc(8, 3.1)
    bench("CG water 512 beads x 50 frames", frames_of(lat, L, 50, 0.35), L, 3.6, 180, (0.0, math.pi), a.reps)
    lat, L = lattice_sc(16, 3.1)
    bench("CG water 4096 beads x 10 frames", frames_of(lat, L, 10, 0.35), L, 3.6, 180, (0.0, math.pi), a.reps)


if __name__ == "__main__":
    main()
