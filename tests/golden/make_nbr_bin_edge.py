"""Writes tests/golden/nbr_bin_edge.npz: pairs of atoms that the dense neighbour search lists and a cell list with bins of
exactly the cutoff never tests (csrc/nbr.hip before make_bins asked for a margin).  Found by tests/nbr_ref.py:
search_bin_edge -- boxes of a whole number of cutoffs per side, atoms within 5 ulps of two bin edges one bin apart, binned
with the float32 arithmetic of bin_coord and make_cell's inverse.  CPU only:

    python tests/golden/make_nbr_bin_edge.py

Arrays (raw float32): pos [K, 2, 3], lengths [K, 3], cutoff [K]; axis [K] the axis the pair lies along, bins [K] the bins
along it (= lengths / cutoff), edge [K] the bin the pair straddles."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import nbr_ref as R  # noqa: E402


def main():
    f32 = np.float32
    # the construction the search was first reported with (4 bins: bins 3 and 1)
    picks = [(f32(1.6618019), f32(6.6472077), 4, 2, f32(4.9854054), f32(3.3236036))]
    seen = set()
    for row in R.search_bin_edge(4000, 7):
        key = (row[2], row[3] + 1 == row[2])              # one per bin count, inside the box and across the face
        if key not in seen:
            seen.add(key)
            picks.append(row)
    picks = picks[:1] + sorted(picks[1:], key=lambda r: (r[2], r[3]))[:9]
    pos, lengths, cutoff, axis, bins, edge = [], [], [], [], [], []
    for m, (rc, L, n, k, xa, xb) in enumerate(picks):
        ax = m % 3
        Ls = np.full(3, L, f32) if m % 2 == 0 else np.array([f32(3.37) * rc, f32(4.61) * rc, f32(3.83) * rc], f32)
        Ls[ax] = L
        p = np.empty((2, 3), f32)
        p[:] = (f32(0.3) * Ls)[None, :]
        p[0, ax], p[1, ax] = xa, xb
        inv = R.cell_inv(Ls)
        nb = R.make_bins(Ls, rc, guarded=False)
        full = R.full_list32_diag(p, Ls, rc, inv)
        assert full.keep[0, 1] and full.keep[1, 0], "the float32 pair test must accept the pair"
        for coord in (R.bin_coord, R.bin_coord_plain):
            assert len(R.stencil_misses(full, p, Ls, inv, nb, coord)[0]) == 2, "the unguarded stencil must miss it"
        pos.append(p), lengths.append(Ls), cutoff.append(rc), axis.append(ax), bins.append(n), edge.append(k)
    out = os.path.join(HERE, "nbr_bin_edge.npz")
    np.savez(out, pos=np.array(pos, f32), lengths=np.array(lengths, f32), cutoff=np.array(cutoff, f32),
             axis=np.array(axis, np.int32), bins=np.array(bins, np.int32), edge=np.array(edge, np.int32))
    print("%d constructions -> %s" % (len(pos), out))
    for r in picks:
        print("  rc %.9g L %.9g bins %d edge %d xA %.9g xB %.9g" % tuple(float(v) for v in r))


if __name__ == "__main__":
    main()
