"""CPU-only: the launch plans of the stand-alone RDF kernels (csrc/rdf.hip) through mdg_rdf_fwd_variant /
mdg_rdf_bwd_variant and ops.rdf_route -- which variant the shapes of the GPU tests take, and that no plan over a sweep
of shapes asks for more than the hardware has."""
import ctypes

import numpy as np
import pytest

FWD = ("direct", "block8", "lane", "half", "fine")
BWD = ("atom", "table", "frame")
R, WAVES, GRID, LDS, STRIDE, LAST = range(6)          # words of the info array (MDG_RDF_PLAN_INFO)


def plan(direction, F, N, nbins, width_scale=1.0, diag=True, masked=False, r_range=(0.75, 2.5), spacing=None):
    """(variant name or None, info) for `nbins` linspace centres on r_range and width = width_scale * spacing, as the
    GPU tests build them (float32 spacing of torch.linspace)."""
    from mdgrad_amd import _lib
    lib = _lib.load()
    sp = float(np.float32((r_range[1] - r_range[0]) / (nbins - 1))) if spacing is None else spacing
    coeff = -0.5 / (width_scale * sp) ** 2 if sp > 0 else -0.5 / (width_scale * 0.0177) ** 2
    info = (ctypes.c_int32 * 6)()
    fn = lib.mdg_rdf_fwd_variant if direction == "fwd" else lib.mdg_rdf_bwd_variant
    v = fn(F, N, nbins, sp, coeff, int(diag), int(masked), info)
    names = FWD if direction == "fwd" else BWD
    return (names[v] if v >= 0 else None), list(info)


# (frames, atoms, bins, width / spacing, diagonal cell, masked) -> forward (variant, R, waves, 128-column rows), backward
# (variant, R): the shapes of tests/test_gpu_parity.py and tests/test_gpu_pins.py
TABLE = [
    # test_many_frame_rdf_kernels_vs_oracle, test_rdf_kernel_variants_agree
    ((1100, 108, 100, 1.0, True, False), ("fine", 0, 16, 0), ("table", 6)),
    ((1100, 108, 100, 1.6, True, False), ("fine", 0, 16, 0), ("table", 11)),
    ((1100, 108, 100, 0.4, True, False), ("lane", 5, 4, 1), ("frame", 6)),
    ((550, 108, 100, 1.0, True, False), ("block8", 0, 8, 0), ("atom", 0)),
    ((550, 108, 100, 0.4, True, False), ("direct", 0, 8, 0), ("atom", 0)),
    ((1100, 107, 100, 1.0, True, True), ("fine", 0, 16, 0), ("table", 6)),
    # test_rdf_lane_kernels_general_variants: translated, triclinic, 150 atoms, masked
    ((1030, 108, 100, 1.0, True, False), ("fine", 0, 16, 0), ("table", 6)),
    ((1030, 108, 100, 1.0, False, False), ("fine", 0, 16, 0), ("table", 6)),
    ((1030, 150, 100, 1.0, True, False), ("fine", 0, 16, 0), ("table", 6)),
    ((1030, 108, 100, 1.0, True, True), ("fine", 0, 16, 0), ("table", 6)),
    # test_rdf_lane_kernels_other_bin_and_atom_counts
    ((1040, 108, 37, 1.0, True, False), ("fine", 0, 16, 0), ("table", 6)),
    ((1040, 300, 100, 1.0, True, False), ("fine", 0, 16, 0), ("table", 6)),
    ((1040, 108, 200, 1.0, True, False), ("lane", 5, 2, 1), ("table", 6)),
    ((1040, 20, 100, 1.0, True, False), ("half", 5, 8, 1), ("table", 6)),
    ((1040, 7, 64, 1.0, True, False), ("half", 5, 8, 1), ("table", 6)),
    ((1040, 400, 100, 1.0, True, False), ("lane", 5, 4, 0), ("table", 6)),
    # test_rdf_variants_below_the_fine_histogram: 48 atoms
    ((1024, 48, 100, 1.0, True, True), ("half", 5, 8, 0), ("table", 6)),
    ((1024, 48, 100, 1.0, False, False), ("half", 5, 8, 0), ("table", 6)),
    ((1024, 48, 100, 1.6, True, False), ("lane", 11, 4, 1), ("table", 11)),
    ((1024, 48, 100, 1.6, False, False), ("lane", 11, 4, 0), ("table", 11)),
    ((1024, 48, 100, 0.4, True, False), ("lane", 5, 4, 1), ("frame", 6)),
    ((1024, 48, 500, 1.6, True, False), ("lane", 11, 1, 1), ("frame", 11)),
]


@pytest.mark.parametrize("shape,fwd,bwd", TABLE)
def test_variants_of_the_tested_shapes(shape, fwd, bwd):
    F, N, nbins, ws, diag, masked = shape
    v, info = plan("fwd", F, N, nbins, ws, diag, masked)
    assert (v, info[R], info[WAVES], info[LAST]) == fwd
    v, info = plan("bwd", F, N, nbins, ws, diag, masked)
    assert (v, info[R]) == bwd


def test_arbitrary_centres_take_the_direct_kernels():
    assert plan("fwd", 1100, 108, 100, spacing=0.0)[0] == "direct"
    v, info = plan("bwd", 1100, 108, 100, spacing=0.0)
    assert (v, info[R]) == ("frame", 0)
    assert plan("bwd", 500, 108, 100, spacing=0.0)[0] == "atom"


def test_bad_arguments_are_refused():
    for direction in ("fwd", "bwd"):
        assert plan(direction, 1100, 108, 100)[0] is not None
        assert plan(direction, 1100, 1, 100)[0] is None                    # N <= 1
        assert plan(direction, 1100, 0, 100)[0] is None
        assert plan(direction, 0, 108, 100)[0] is None
        from mdgrad_amd import _lib
        fn = getattr(_lib.load(), "mdg_rdf_%s_variant" % direction)
        for nbins in (0, -3):
            assert fn(1100, 108, nbins, 0.0177, -1600.0, 1, 0, None) == -1
        for coeff in (0.0, 2.5):
            assert fn(1100, 108, 100, 0.0177, coeff, 1, 0, None) == -1
    assert plan("fwd", 1100, 108, 513)[0] is None                          # more bins than the forward kernels hold
    assert plan("fwd", 1100, 108, 512)[0] is not None


def _edges(lo, hi, thresholds, step):
    s = set(range(lo, min(hi, lo + 24) + 1)) | set(range(lo, hi + 1, step)) | {hi}
    for t in thresholds:
        s |= {t - 1, t, t + 1}
    return sorted(v for v in s if lo <= v <= hi)


def test_no_plan_exceeds_the_hardware_over_a_sweep_of_shapes():
    """N = 2 .. 4096 (and past the 4096 of the frame kernels), nbins = 2 .. 512, width / spacing from 0.3 to 2.5, both cells,
    with and without a mask, on either side of the 1 024-frame switch: every plan fits 160 KB of LDS, has a grid and
    waves, and the backward `frame` variant is only named where the launch holds the frame: its LDS is the 2 nbins + 6 R
    table floats plus 6 N floats per wave that rdf_bwd_kernel lays out, within 160 KB (the gather takes over above 4 096
    atoms, so up to 512 bins no shape of the sweep is refused)."""
    atoms = _edges(2, 4200, (48, 63, 64, 108, 126, 128, 1024, 2048, 3300, 4096), 173)
    bins = _edges(2, 512, (16, 100, 120, 200, 256, 488, 489, 500), 37)
    seen_f, seen_b = set(), set()
    for F in (1023, 1024, 100000):
        for N in atoms:
            for nb in bins:
                for ws in (0.3, 0.4, 0.6, 1.0, 1.6, 2.5):
                    vb, ib = plan("bwd", F, N, nb, ws)
                    assert vb is not None, (F, N, nb, ws)
                    assert 0 <= ib[LDS] <= 160 * 1024 and ib[GRID] >= 1 and ib[WAVES] >= 1, (F, N, nb, ws, vb, ib)
                    if vb == "frame":
                        need = 4 * (2 * nb + 6 * ib[R] + ib[WAVES] * 6 * N)
                        assert F >= 1024 and N <= 4096 and need == ib[LDS], (F, N, nb, ws, ib)
                    seen_b.add((vb, ib[R]))
                    for diag in (True, False):
                        for masked in (False, True):
                            vf, jf = plan("fwd", F, N, nb, ws, diag, masked)
                            assert vf is not None
                            assert 0 <= jf[LDS] <= 160 * 1024 and jf[GRID] >= 1 and jf[WAVES] >= 1, (F, N, nb, ws, vf, jf)
                            rows = jf[GRID] * jf[WAVES] if vf in ("lane", "half") else jf[GRID]
                            assert rows <= 2048 or vf == "fine"                      # mdg_rdf_partial_size: 2048 rows
                            seen_f.add((vf, jf[R], bool(jf[LAST]), diag, masked) if vf in ("lane", "half") else (vf,))
    # every instantiation of the dispatchers is reached by some legal shape
    lane = {("lane", r, False, d, m) for r in (5, 11) for d in (True, False) for m in (True, False)}
    lane |= {("lane", 5, True, True, False), ("lane", 11, True, True, False)}
    half = {("half", 5, False, d, m) for d in (True, False) for m in (True, False)} | {("half", 5, True, True, False)}
    assert seen_f == lane | half | {("fine",), ("block8",), ("direct",)}
    assert seen_b == {("atom", 0), ("table", 6), ("table", 11), ("frame", 0), ("frame", 6), ("frame", 11)}


def test_rdf_route_picks_the_cell_sweep_for_large_systems():
    from mdgrad_amd import _lib, ops
    sp = 1.75 / 99
    coeff = -0.5 / sp ** 2
    big = ops.rdf_route(11, 4096, 100, sp, coeff, 2.62, _lib.make_cell([17.1] * 3), None)
    assert big == ("cell", None, None)
    small = ops.rdf_route(1100, 108, 100, sp, coeff, 3.0, _lib.make_cell([4.8] * 3), None)
    assert small == ("frames", "fine", "table")
    assert ops.rdf_route(10, 108, 100, sp, coeff, 3.0, _lib.make_cell([4.8] * 3), None) == ("frames", "block8", "atom")
    assert ops.rdf_route(10, 108, 100, 0.0, coeff, 3.0, _lib.make_cell([4.8] * 3), None) == ("frames", "direct", "atom")
