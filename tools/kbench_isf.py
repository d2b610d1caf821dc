"""Times observable.intermediate_scattering (csrc/isf.hip through ops.IsfFn), coherent and self: forward, and forward + backward
with respect to the positions, with HIP events after warm-up, medians over the repeats.  Beside each, the torch composite on
the same device: cos / sin of q_t @ k.T, rho by a sum over the atoms (coherent) or the product of the phasors (self), a slice
per lag, autograd for the gradient, over as many replicas as fit in memory; both are reported per replica.

    python tools/kbench_isf.py [--reps 7] [--warmup 3]

Shapes (replicas x atoms x frames x lags): 1 024 x 108 x 64 x 32 and 1 x 4 096 x 128 x 64, the vectors of 24 bins over
k_range = (1, 12) with max_per_bin = 8; random walks with steps of 0.1.  Last, the self forward at 8 and at 64 lags on the
first shape: the ring in LDS makes its time grow more slowly than the number of lags."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd.observable import intermediate_scattering  # noqa: E402
from mdgrad_amd.system import System  # noqa: E402

DEV = "cuda:0"
NBINS, K_RANGE, MAX_PER_BIN = 24, (1.0, 12.0), 8
COMPOSED_BYTES = 32 << 30         # the composite's phase tensors (cos, sin and a few temporaries of their size) stay under this


def timed(fn, reps, warmup):
    """Median milliseconds of fn() over `reps` runs between HIP events, after `warmup` untimed runs."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def setup(R, N, T, L, kind):
    side = 5.0 * (N / 108.0) ** (1.0 / 3.0)
    g = torch.Generator(device=DEV).manual_seed(N + T)
    q = side * torch.rand(R, 1, N, 3, device=DEV, generator=g) + 0.1 * torch.randn(R, T, N, 3, device=DEV, generator=g).cumsum(1)
    system = System(positions=np.random.default_rng(0).uniform(0, side, (N, 3)), cell=np.array([side] * 3), masses=np.full(N, 1.008),
                    device=DEV)
    return q, intermediate_scattering(system, NBINS, K_RANGE, L, kind=kind, max_per_bin=MAX_PER_BIN)


def fwd(fn, x):
    with torch.no_grad():
        return fn(x)


def fwd_bwd(fn, x):
    xx = x.detach().requires_grad_(True)
    return torch.autograd.grad(fn(xx).pow(2).sum(), xx)


def bench(R, N, T, L, kind, reps, warmup):
    q, obs = setup(R, N, T, L, kind)
    M = len(obs.kvecs)
    k = (2 * np.pi * obs.kvecs.to(torch.float32) / obs.cell.cpu()).to(DEV)
    seg = obs._seg_host
    rc = max(1, min(R, COMPOSED_BYTES // (6 * 4 * T * N * M)))

    def composite(x):
        ph = x @ k.t()                                                  # [r, T, N, M]
        c, s = ph.cos(), ph.sin()
        if kind == "coherent":
            c, s = c.sum(2), s.sum(2)
        rows = []
        for tau in range(L):
            f = c[:, tau:] * c[:, :T - tau] + s[:, tau:] * s[:, :T - tau]
            rows.append((f.sum(2) if kind == "self" else f).mean(1) / N)            # [r, M]
        Fk = torch.stack(rows, 2)                                       # [r, M, L]
        return torch.stack([Fk[:, seg[b]:seg[b + 1]].mean(1) if seg[b + 1] > seg[b] else Fk.new_zeros(Fk.shape[0], L)
                            for b in range(obs.nbins)], 1)

    a, b = fwd(obs.per_replica, q[:rc]).reshape(rc, obs.nbins, L), fwd(composite, q[:rc])
    print("%s %d x %d x %d frames x %d lags x %d vectors: kernels vs composite float32 on %d replicas: max |dF| = %.3e" % (
        kind, R, N, T, L, M, rc, float((a - b).abs().max())), flush=True)
    for what, run in (("forward", fwd), ("forward+backward", fwd_bwd)):
        t_k = timed(lambda: run(obs.per_replica, q), reps, warmup)
        t_c = timed(lambda: run(composite, q[:rc]), reps, warmup)
        print("%-8s %d x %d x %d x %d  %-17s kernels %9.3f ms   composite %9.3f ms on %d replicas   ratio per replica %6.1f" % (
            kind, R, N, T, L, what, t_k, t_c, rc, (t_c / rc) / (t_k / R)), flush=True)


def lag_scaling(R, N, T, reps, warmup):
    times = {}
    for L in (8, 64):
        q, obs = setup(R, N, T, L, "self")
        times[L] = timed(lambda: fwd(obs.per_replica, q), reps, warmup)
    print("self forward %d x %d x %d frames: %9.3f ms at 8 lags, %9.3f ms at 64 lags: %.2f x the time for 8 x the lags" % (
        R, N, T, times[8], times[64], times[64] / times[8]), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_isf: no HIP device -- timings are taken on the GPU only")
    print("device:", torch.cuda.get_device_name(0), flush=True)
    for kind in ("coherent", "self"):
        bench(1024, 108, 64, 32, kind, args.reps, args.warmup)
        bench(1, 4096, 128, 64, kind, args.reps, args.warmup)
    lag_scaling(1024, 108, 64, args.reps, args.warmup)
