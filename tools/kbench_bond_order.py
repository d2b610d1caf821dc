"""Times the bond-orientational order kernels (csrc/bond_order.hip): the forward and the backward launch on a prebuilt
neighbour list (device events around `--reps` launches after a warm-up, median and spread over `--rounds` rounds), and
ops.BondOrderFn end to end (forward, forward + backward) with the list builds of the frame chunks included (host clock
around a device synchronise).  Prints bonds per second.

    python tools/kbench_bond_order.py [--frames 64] [--atoms-side 16] [--ls 4 6] [--reps 500] [--rounds 5]

Shape: 64 frames x 4 096 atoms (a jittered simple-cubic liquid-like box at unit density), cutoff 1.5 (about 14 bonds per
atom), r_in 0.85 cutoff, ls = (4, 6).  There is no threshold here: the figures go into docs/KERNELS.md."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"


def frames_of(side, n_frames, sigma, seed=0):
    g = np.arange(side, dtype=np.float64)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    base = torch.tensor(lat, dtype=torch.float32, device=DEV)
    x = base + sigma * torch.randn(n_frames, *base.shape, device=DEV, generator=gen)
    return torch.remainder(x, float(side)).contiguous(), float(side)


def events(fn, reps, rounds):
    """Median and (min, max) over `rounds` of the mean time of `reps` back-to-back launches, in seconds."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / reps)
    return statistics.median(out), min(out), max(out)


def wall(fn, rounds, inner=50):
    """The same with a host clock around `inner` calls that end in a device synchronise."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / inner)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--atoms-side", type=int, default=16)
    ap.add_argument("--ls", type=int, nargs="+", default=[4, 6])
    ap.add_argument("--cutoff", type=float, default=1.5)
    ap.add_argument("--reps", type=int, default=500, help="launches per timed window (500 x ~0.1 .. 0.3 ms: 50 .. 150 ms a window)")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_bond_order: no HIP device; a timing needs one")
    x, L = frames_of(a.atoms_side, a.frames, 0.12)
    F, N = x.shape[0], x.shape[1]
    ls, cutoff, r_in = tuple(a.ls), a.cutoff, 0.85 * a.cutoff
    K = sum(2 * l + 1 for l in ls)
    cs = _lib.make_cell(torch.tensor([L] * 3))
    lib = _lib.load()
    flat = x.reshape(-1, 3)
    ell = ops.build_ell(flat, cs, cutoff, None, group=N)
    bonds = float(ell.cnt.double().sum())
    print("device: %s   frames %d  atoms %d  ls %s  cutoff %.2f  max_nbr %d  bonds %.3e (%.1f per atom)" % (
        torch.cuda.get_device_name(0), F, N, ls, cutoff, ell.max_nbr, bonds, bonds / (F * N)), flush=True)
    A, n = torch.empty(K, F * N, device=DEV), torch.empty(F * N, device=DEV)
    gA, gn, gx = torch.randn(F * N, K, device=DEV), torch.randn(F * N, device=DEV), torch.empty(F * N, 3, device=DEV)
    ls_c = (C.c_int32 * len(ls))(*ls)
    st = _lib.stream_ptr(x.device)
    args = (_lib.ptr(flat), F, N, C.byref(cs), cutoff, r_in, _lib.ptr(ell.col), _lib.ptr(ell.cnt), ell.max_nbr, ls_c, len(ls))

    def k_fwd():
        _lib.check(lib.mdg_bond_order_fwd(*args, _lib.ptr(A), _lib.ptr(n), st), "mdg_bond_order_fwd")

    def k_bwd():
        _lib.check(lib.mdg_bond_order_bwd(*args, _lib.ptr(gA), _lib.ptr(gn), _lib.ptr(gx), st), "mdg_bond_order_bwd")

    def op_fwd():
        return ops.BondOrderFn.apply(x, ls, cutoff, r_in, cs, None)

    def op_fwd_bwd():
        xx = x.detach().requires_grad_(True)
        Ao, no = ops.BondOrderFn.apply(xx, ls, cutoff, r_in, cs, None)
        torch.autograd.grad((Ao * gA.view(F, N, K)).sum() + (no * gn.view(F, N)).sum(), xx)

    for label, (med, lo, hi) in (("kernel fwd (device events)", events(k_fwd, a.reps, a.rounds)),
                                 ("kernel bwd (device events)", events(k_bwd, a.reps, a.rounds)),
                                 ("op fwd with list build (host clock)", wall(op_fwd, a.rounds)),
                                 ("op fwd+bwd with list build (host clock)", wall(op_fwd_bwd, a.rounds))):
        print("%-42s median %9.3f ms  (min %9.3f, max %9.3f)   %.3e bonds/s" % (label, 1e3 * med, 1e3 * lo, 1e3 * hi, bonds / med), flush=True)


if __name__ == "__main__":
    main()
