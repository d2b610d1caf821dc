"""A/B of two builds of libmdgrad_hip.so on the stand-alone RDF kernels (csrc/rdf.hip): a SHA-256 of the histogram `raw` and
of the gradient `g_xyz` for every shape of the RDF tests, seeded inputs, through the C ABI (mdg_rdf_fwd_uniform /
mdg_rdf_bwd_uniform) of the library that MDG_LIB names (default: this tree's build).  A different kernel variant, grid or
table changes the order of the partial sums and with it the hashes, so equal output of two builds means equal launches.

    MDG_LIB=<other build>/libmdgrad_hip.so python tools/rdf_ab.py [--time] [--rows 0:14] > a.txt
    python tools/rdf_ab.py [--time] [--rows 0:14] > b.txt ; diff a.txt b.txt

--time adds HIP-event times (median of 7 after 3 warm-up runs) of forward + backward at 1100 x 108, widths x 1.0 and x 0.4.
Only symbols that every build has are bound, so a build from before the plan queries can be compared."""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
TRI = [[4.8, 0, 0], [0.7, 4.8, 0], [-0.5, 0.4, 4.8]]
L = 4.8
# (frames, atoms, bins, width / spacing, triclinic, masked)
ROWS = [(1100, 108, 100, 1.0, 0, 0), (1100, 108, 100, 1.6, 0, 0), (1100, 108, 100, 0.4, 0, 0), (550, 108, 100, 1.0, 0, 0),
        (1100, 107, 100, 1.0, 0, 1), (1030, 108, 100, 1.0, 1, 0), (1030, 150, 100, 1.0, 0, 0), (1030, 108, 100, 1.0, 0, 1),
        (1040, 108, 37, 1.0, 0, 0), (1040, 108, 200, 1.0, 0, 0), (1040, 20, 100, 1.0, 0, 0), (1040, 7, 64, 1.0, 0, 0),
        (1040, 300, 100, 1.0, 0, 0), (1040, 400, 100, 1.0, 0, 0),
        (1024, 48, 100, 1.0, 0, 1), (1024, 48, 100, 1.0, 1, 0), (1024, 48, 100, 1.6, 0, 0), (1024, 48, 100, 1.6, 1, 0),
        (1024, 48, 100, 0.4, 0, 0), (1024, 48, 500, 1.6, 0, 0)]
NAMES = ("mdg_rdf_partial_size", "mdg_rdf_fwd_uniform", "mdg_rdf_bwd_uniform", "mdg_last_error")


def load():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    return lib


def case(row):
    F, N, nbins, ws, tri, masked = row
    rng = np.random.default_rng(1000 * N + nbins + F)
    base = rng.uniform(0, L, (N, 3))
    x = torch.as_tensor(np.mod(base + rng.normal(0, 0.05, (F, N, 3)), L).astype(np.float32), device=DEV)
    mu = torch.linspace(0.75, 2.5, nbins, device=DEV)
    spacing = float(mu[1] - mu[0])
    coeff = float(-0.5 / (ws * spacing) ** 2)
    cs = _lib.make_cell(np.array(TRI, np.float32) if tri else [L] * 3)
    mask = ops.build_mask(N, index_tuple=(list(range(0, 2 * N // 5)), list(range(2 * N // 5, N))), device=DEV) if masked else None
    g_raw = torch.linspace(-1, 1, nbins, device=DEV)
    return x, mu, spacing, coeff, cs, mask, g_raw, (2.3 if tri else 3.0)


def run(lib, row, x, mu, spacing, coeff, cs, mask, g_raw, cutoff):
    F, N, nbins = row[:3]
    raw, gx = torch.empty(nbins, device=DEV), torch.empty_like(x)
    partial = torch.empty(int(lib.mdg_rdf_partial_size(F, N, nbins)), device=DEV)
    st = _lib.stream_ptr(x.device)
    for rc in (lib.mdg_rdf_fwd_uniform(_lib.ptr(x), F, N, C.byref(cs), cutoff, _lib.ptr(mask), _lib.ptr(mu), spacing, coeff, nbins,
                                       _lib.ptr(raw), _lib.ptr(partial), st),
               lib.mdg_rdf_bwd_uniform(_lib.ptr(x), F, N, C.byref(cs), cutoff, _lib.ptr(mask), _lib.ptr(mu), spacing, coeff, nbins,
                                       _lib.ptr(g_raw), _lib.ptr(gx), st)):
        if rc != 0:
            raise RuntimeError("rdf launch failed (%d): %s" % (rc, lib.mdg_last_error()))
    return raw, gx


def sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()[:24]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--rows", default=":", help="slice of the table of shapes, e.g. 0:14 or 16:17")
    args = ap.parse_args()
    lib = load()
    lo, hi = (int(v) if v else None for v in args.rows.split(":"))
    for row in ROWS[lo:hi]:
        c = case(row)
        raw, gx = run(lib, row, *c)
        torch.cuda.synchronize()
        print("%5d x %3d atoms %3d bins width x%.1f tri %d mask %d  raw %s  g_xyz %s" % (row + (sha(raw), sha(gx))))
    if args.time:
        for row in (ROWS[0], ROWS[2]):
            c = case(row)
            for _ in range(3):
                run(lib, row, *c)
            ms = []
            for _ in range(7):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run(lib, row, *c)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            print("time %5d x %3d width x%.1f  fwd + bwd  median %.4f ms  min %.4f  max %.4f" % (row[0], row[1], row[3], np.median(ms),
                                                                                               min(ms), max(ms)))


if __name__ == "__main__":
    main()
