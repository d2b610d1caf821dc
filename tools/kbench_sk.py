"""Times observable.structure_factor (csrc/sk.hip through ops.SkFn): forward, and forward + backward with respect to the
positions, with HIP events after warm-up.  Beside each, the same definition composed in torch on the same device in float32
(x @ k^T -> cos / sin -> sums over the atoms -> bin means, autograd for the gradient) over as many frames as fit in memory;
both are reported per frame.

    python tools/kbench_sk.py [--reps 5] [--warmup 2]

Shapes (jittered lattices at the density of the 108-atom goldens): 8 192 frames x 108 atoms with every vector up to k = 16
(3 844 for the 4.8 box, 30 bins), and 64 frames x 4 096 atoms with max_per_bin = 64."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd.observable import structure_factor  # noqa: E402
from mdgrad_amd.system import System  # noqa: E402

DEV = "cuda:0"
COMPOSED_BYTES = 2 << 30          # the composition's [F, N, M] float32 phase tensor is kept under this


def lattice_fcc(size, a):
    base = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
    return np.array([(np.array([i, j, k]) + b) * a for i in range(size) for j in range(size) for k in range(size) for b in base]), a * size


def lattice_sc(n, a):
    g = np.arange(n) * a
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), a * n


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


def bench(lat, L, n_frames, max_per_bin, reps, warmup):
    N = len(lat)
    g = torch.Generator(device=DEV).manual_seed(N)
    base = torch.tensor(lat, dtype=torch.float32, device=DEV)
    q = torch.remainder(base + 0.05 * torch.randn(n_frames, N, 3, device=DEV, generator=g), L)
    system = System(positions=lat, cell=np.array([L] * 3), masses=np.full(N, 1.008), device=DEV)
    obs = structure_factor(system, 30, (1.0, 16.0), max_per_bin=max_per_bin)
    M = len(obs.kvecs)
    kv = (2 * np.pi / L) * obs.kvecs.to(DEV, torch.float32)
    cnt = obs.n_vectors.to(DEV)
    A = torch.zeros(M, obs.nbins, device=DEV)
    A[torch.arange(M, device=DEV), torch.repeat_interleave(torch.arange(obs.nbins, device=DEV), cnt)] = \
        1.0 / torch.repeat_interleave(cnt, cnt).float()
    fc = max(1, min(n_frames, COMPOSED_BYTES // (4 * N * M)))

    def composed(x):
        ph = x @ kv.t()
        return (ph.cos().sum(1).pow(2) + ph.sin().sum(1).pow(2)) / N @ A

    def fwd(fn, x):
        with torch.no_grad():
            return fn(x)

    def fwd_bwd(fn, x):
        xx = x.detach().requires_grad_(True)
        return torch.autograd.grad(fn(xx).pow(2).sum(), xx)

    a, b = fwd(obs.per_frame, q[:fc]), fwd(composed, q[:fc])
    print("%d x %d, %d vectors: kernels vs composed float32 on %d frames: max |dS| = %.3e (S up to %.3e)" % (
        n_frames, N, M, fc, float((a - b).abs().max()), float(b.max())), flush=True)
    for what, run in (("forward", fwd), ("forward+backward", fwd_bwd)):
        t_k = timed(lambda: run(obs.per_frame, q), reps, warmup)
        t_c = timed(lambda: run(composed, q[:fc]), reps, warmup)
        print("%d x %d  %-17s kernels %9.3f ms (%8.3f us/frame)   composed %9.3f ms on %d frames (%8.3f us/frame)   "
              "ratio per frame %.1f" % (n_frames, N, what, t_k, 1e3 * t_k / n_frames, t_c, fc, 1e3 * t_c / fc,
                                        (t_c / fc) / (t_k / n_frames)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_sk: no HIP device -- timings are taken on the GPU only")
    print("device:", torch.cuda.get_device_name(0), flush=True)
    bench(*lattice_fcc(3, 1.6), 8192, None, args.reps, args.warmup)                       # 108 atoms, 3 844 vectors
    bench(*lattice_sc(16, 1.6 / 4 ** (1 / 3)), 64, 64, args.reps, args.warmup)            # 4 096 atoms at the same density
