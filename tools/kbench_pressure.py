"""Times thermo.Pressure (csrc/virial.hip through ops.VirialFn): forward, and forward + backward with respect to q, v, sigma and
epsilon, with HIP events after warm-up.  Beside each, the same quantity composed from the pieces the package already had, on
the same device: ops.build_ell -> half_list -> topology.compute_dis -> torch autograd in float32.  That composition is the
yardstick: the kernels have to beat it.

    python tools/kbench_pressure.py [--reps 5] [--warmup 2]

Shapes (LJ 12-6, cutoff 2.5, jittered lattices at the density of the 108-atom goldens): 8 192 frames x 108 atoms and
64 frames x 4 096 atoms.  Prints one line per shape and direction: ms, us per frame, and the ratio composed / kernels."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd import ops, potentials  # noqa: E402
from mdgrad_amd.interface import PairPotentials  # noqa: E402
from mdgrad_amd.system import System  # noqa: E402
from mdgrad_amd.thermo import Pressure  # noqa: E402
from mdgrad_amd.topology import compute_dis  # noqa: E402

DEV = "cuda:0"
CUTOFF, MASS = 2.5, 1.008


def lattice_fcc(size, a):
    base = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
    return np.array([(np.array([i, j, k]) + b) * a for i in range(size) for j in range(size) for k in range(size) for b in base]), a * size


def lattice_sc(n, a):
    g = np.arange(n) * a
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), a * n


def frames_of(lat, L, n_frames, sigma, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    base = torch.tensor(lat, dtype=torch.float32, device=DEV)
    return torch.remainder(base + sigma * torch.randn(n_frames, *base.shape, device=DEV, generator=g), L)


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


def bench(lat, L, n_frames, reps, warmup):
    N = len(lat)
    q = frames_of(lat, L, n_frames, 0.05, seed=N)
    v = torch.randn(n_frames, N, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    system = System(positions=lat, cell=np.array([L] * 3), masses=np.full(N, MASS), device=DEV)
    mdl = potentials.LennardJones(1.0, 1.0).to(DEV)
    pair = PairPotentials(system, mdl, cutoff=CUTOFF)
    obs = Pressure(system, pair)
    mass = obs.mass
    dV = obs.dim * obs.volume
    cellm = torch.diag(torch.tensor([L] * 3, dtype=torch.float32, device=DEV))

    def composed(qq, vv):
        flat = qq.reshape(-1, 3)
        ell = ops.build_ell(flat.detach(), pair._cell_struct, CUTOFF, None, group=N)
        nbr, off = ell.half_list()
        r = compute_dis(flat, nbr, off, cellm).reshape(-1)
        rr = r if r.requires_grad else r.detach().requires_grad_(True)
        (du,) = torch.autograd.grad(mdl(rr).sum(), rr, create_graph=qq.requires_grad)
        W = torch.zeros(n_frames, device=DEV).index_add(0, nbr[:, 0] // N, -(rr * du))
        K = (mass[None, :, None] * vv * vv).sum((1, 2))
        return (K + W) / dV

    def fwd(fn):
        with torch.no_grad() if fn is obs else torch.enable_grad():
            return fn(q, v)

    def fwd_bwd(fn):
        qq, vv = q.detach().requires_grad_(True), v.detach().requires_grad_(True)
        return torch.autograd.grad(fn(qq, vv).sum(), [qq, vv, mdl.sigma, mdl.epsilon])

    a, b = fwd(obs), fwd(composed).detach()
    print("%d x %d  P kernels vs composed: max |dP| = %.3e (P ~ %.3e)" % (n_frames, N, float((a - b).abs().max()),
                                                                          float(b.abs().mean())), flush=True)
    for what, run in (("forward", fwd), ("forward+backward", fwd_bwd)):
        t_k = timed(lambda: run(obs), reps, warmup)
        t_c = timed(lambda: run(composed), reps, warmup)
        print("%d x %d  %-17s kernels %9.3f ms (%8.3f us/frame)   composed %9.3f ms (%8.3f us/frame)   ratio %.1f" % (
            n_frames, N, what, t_k, 1e3 * t_k / n_frames, t_c, 1e3 * t_c / n_frames, t_c / t_k), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_pressure: no HIP device -- timings are taken on the GPU only")
    print("device:", torch.cuda.get_device_name(0), flush=True)
    bench(*lattice_fcc(3, 1.6), 8192, args.reps, args.warmup)                       # 108 atoms
    bench(*lattice_sc(16, 1.6 / 4 ** (1 / 3)), 64, args.reps, args.warmup)          # 4 096 atoms at the same density
