"""Times observable.msd (csrc/msd.hip through ops.MsdFn): forward, and forward + backward with respect to the positions, with
HIP events after warm-up, medians over the repeats.  Beside each, the torch composite on the same device: per lag, slice,
subtract, square, mean (autograd for the gradient), over as many replicas as fit in memory; both are reported per replica.

    python tools/kbench_msd.py [--reps 7] [--warmup 3]

Shapes (replicas x atoms x frames x lags): 16 384 x 108 x 50 x 25, 64 x 4 096 x 50 x 25, 1 x 4 096 x 200 x 100; random walks
with unit steps.  The compulsory HBM traffic is one read of the positions for the forward (12 T N R bytes) and one more read
plus the write of the gradient for the backward (24 T N R bytes more); the tool prints the rate at which the kernels move it
and that rate as a fraction of the 8 TB/s the HBM3E of an MI355X is specified at."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd.observable import msd  # noqa: E402
from mdgrad_amd.system import System  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12
COMPOSED_BYTES = 32 << 30         # what the composite's backward graph keeps (one difference tensor per lag) stays under this


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


def bench(R, N, T, L, reps, warmup):
    g = torch.Generator(device=DEV).manual_seed(N + T)
    q = torch.randn(R, T, N, 3, device=DEV, generator=g).cumsum(1)
    system = System(positions=np.random.default_rng(0).uniform(0, 5.0, (N, 3)), cell=np.array([5.0] * 3), masses=np.full(N, 1.008),
                    device=DEV)
    obs = msd(system, L)
    rc = max(1, min(R, COMPOSED_BYTES // (12 * L * T * N)))

    def composite(x):
        return torch.stack([x.new_zeros(x.shape[0])] + [(x[:, tau:] - x[:, :-tau]).pow(2).sum(-1).mean((1, 2)) for tau in range(1, L)], 1)

    def fwd(fn, x):
        with torch.no_grad():
            return fn(x)

    def fwd_bwd(fn, x):
        xx = x.detach().requires_grad_(True)
        return torch.autograd.grad(fn(xx).pow(2).sum(), xx)

    a, b = fwd(obs.per_replica, q[:rc]).reshape(rc, L), fwd(composite, q[:rc])
    print("%d x %d x %d frames x %d lags: kernels vs composite float32 on %d replicas: max |dM| / M = %.3e" % (
        R, N, T, L, rc, float(((a - b).abs()[:, 1:] / b[:, 1:]).max())), flush=True)
    need = {"forward": 12.0 * T * N * R, "forward+backward": 36.0 * T * N * R}
    for what, run in (("forward", fwd), ("forward+backward", fwd_bwd)):
        t_k = timed(lambda: run(obs.per_replica, q), reps, warmup)
        t_c = timed(lambda: run(composite, q[:rc]), reps, warmup)
        rate = need[what] / (1e-3 * t_k)
        print("%d x %d x %d x %d  %-17s kernels %9.3f ms   composite %9.3f ms on %d replicas   ratio per replica %6.1f   "
              "compulsory %.3f GB at %.2f TB/s = %.1f %% of the HBM peak" % (
                  R, N, T, L, what, t_k, t_c, rc, (t_c / rc) / (t_k / R), need[what] / 1e9, rate / 1e12, 100 * rate / HBM_PEAK),
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_msd: no HIP device -- timings are taken on the GPU only")
    print("device:", torch.cuda.get_device_name(0), flush=True)
    bench(16384, 108, 50, 25, args.reps, args.warmup)
    bench(64, 4096, 50, 25, args.reps, args.warmup)
    bench(1, 4096, 200, 100, args.reps, args.warmup)
