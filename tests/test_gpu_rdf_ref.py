"""Every RDF kernel variant of csrc/rdf.hip and csrc/rdf_cell.hip (through ops.RdfRawFn, forward and backward) against the
float64 definitions of tests/rdf_ref.py (pinned to the reference's goldens, to finite differences and to the oracle by
tests/test_rdf_ref_host.py, which also builds and checks every input used here).  Every case first asserts the route and the
variants it means to run (ops.rdf_route, ops.rdf_plan: R, waves per workgroup, 128-column rows), then runs them.

Error measure.  Forward: |raw_k - ref64_k| / max_k ref64.  Backward: |g - ref64| per frame, atom and component over that
atom's scale A = sum over its pairs of |dL/dd| -- not taken below one float32 roundoff of a single unit contribution
(rdf_ref.scale_floor: it matters for the one-hot upstream gradients only); an atom with A = 0 must hold exact zeros.

Tolerance.  Nothing is fixed in advance and nothing comes from the kernel.  Per case, on the CPU: floor = the variant's model
(rdf_ref: the exact sum, the 2R+1 bins of the lane / recurrence kernels, the cubic Hermite derivative table, the fine
integer histogram, the u-space pair table of the list routes) evaluated in float32 against the same model in float64, at least
2^-24; model_gap = the float64 model against the exact float64 sum; allowed = MARGIN x floor + model_gap, MARGIN = 10 as for
the bonded and pressure kernels (fused multiply-adds, v_exp_f32 / v_rsq_f32 at 1 ulp where the CPU uses libm, the recurrence
multipliers, another summation order).  Inputs carry no fragile pair (rdf_ref.fragile_pairs: a fractional coordinate within
1e-6 of +-0.5 or a distance within 1e-5 of the cutoff, within reach of the centres); the sibling tests of test_gpu_parity.py
keep their seeds, which contain such pairs, and cover image consistency between kernels.

Upstream gradients: linspace(-1, 1) everywhere; one-hot on the first and on the last bin (the padded table ends; a wrong
neighbour bin) on the R = 6, R = 11, table and edge cases.

Floors, allowances and what the kernels showed on an MI355X (floor and model_gap are CPU figures; "kernel" is against the exact
float64 sum, in brackets against the variant's own float64 model where that differs):

    forward, of the largest bin               variant          floor    model_gap allowed  kernel
    3 frames, arbitrary centres               direct           5.6e-7   0         5.6e-6   5.7e-7
    8 frames / not a linspace / coincident    block8, direct   3.0 .. 3.4e-7   0  3.0 .. 3.4e-6   4.0 .. 7.3e-7
    half/table R=6: ortho / tricl. / masked   half  R=5        1.6 / 1.8 / 1.3e-7   3.3e-8   1.65 / 1.87 / 1.38e-6   1.2 / 1.3 / 1.4e-7
    tail / edge / translated / unwrapped      half  R=5        2.3 / 1.3 / 1.5 / 1.2e-7   3.3e-8   2.4 / 1.3 / 1.5 / 1.2e-6   1.0 / 1.3 / 0.8 / 0.7e-7
    tiny, 2 / 7 atoms                         half  R=5        3.5 / 1.2e-7   2.5 / 2.9e-8   3.5 / 1.3e-6   3.9 / 1.1e-7
    lane/table R=11: ortho / triclinic        lane  R=11       2.3 / 2.0e-7   6e-13     2.28 / 1.98e-6   0.9 / 1.2e-7
    lane/frame R=6 width 0.4                  lane  R=5        2.1e-7   2e-16     2.14e-6  1.3e-7
    lane/frame R=11 500 centres               lane  R=11       3.2e-7   6e-13     3.19e-6  2.9e-7
    direct/frame R=0                          direct           1.5e-7   0         1.5e-6   1.4e-7
    fine/table 64 / 65 / 65 masked            fine             0.9 / 0.9 / 1.3e-6   4.7 / 8.8 / 11.5e-6   1.4 / 1.8 / 2.5e-5
                                                               kernel 4.6 / 8.4 / 10.9e-6 (1.3 / 1.2 / 1.2e-6)
    cell sweep / list                         fine grid        2.6e-6   2.1e-5    4.8e-5   2.2e-5 (2.8e-6)

    What these tests found in the forward, and what csrc/rdf.hip does about it now.  The lane and half kernels measured
    1.7e-6 .. 8.2e-6 of the largest bin, 10 .. 25 x floor (seven cases outside their allowance), for two reasons of the same
    kind, a shift that is common to all pairs of a bin and so does not average out as the rounding of the distances does, and
    that weighs 1 / sigma in the histogram: (1) the recurrences step from a centre to its neighbours by s dmu, i.e. take the
    float32 linspace centres as exactly equidistant, which they are to an ulp (restated in float64 on the CPU: 2.3e-6 half,
    1.3e-6 lane at width 1.6, 3.3e-6 at width 0.4, 7.2e-6 at 500 centres); every deposited value now carries the first-order
    factor of its centre's offset (rdf_centre_offset), which left a third: half 8e-7, lane 0.5 .. 2.9e-6; (2) v_sqrt_f32 (1
    ulp) errs with a mean that is not zero; both kernels now take the correctly rounded root: lane 0.9 .. 2.9e-7, half
    0.7 .. 3.9e-7.

    backward, of the atom's scale; linspace(-1, 1) upstream      variant       floor    model_gap allowed  kernel
    3 frames / 8 frames / not a linspace / coincident            atom          3.2 / 5.8 / 5.4 / 4.4e-6   0   3.2 .. 5.8e-5   4.6 / 4.6 / 3.8 / 5.4e-6
    half/table R=6: orthorhombic / triclinic / masked            table R=6     1.4e-5 / 8.2e-6 / 2.2e-5   6.3 / 5.6 / 11e-7   1.4e-4 / 8.2e-5 / 2.2e-4
                                                                               kernel 1.1e-5 / 8.0e-6 / 2.0e-5
    lane/table R=11: orthorhombic / triclinic                    table R=11    4.9 / 3.1e-6   7.0 / 5.5e-8   4.9 / 3.1e-5   5.4 / 3.0e-6
    lane/frame R=6 width 0.4 (the xfail shape of test_gpu_parity) frame R=6    3.13e-5  0         3.13e-4  4.59e-5
    lane/frame R=11 500 centres                                  frame R=11    4.1e-5   2.8e-10   4.1e-4   9.6e-5
    direct/frame R=0                                             frame R=0     7.2e-6   0         7.2e-5   9.0e-6
    fine/table 64 / 65 / 65 masked                               table R=6     1.1e-5 / 9.6e-6 / 2.1e-5   5.4 / 5.3 / 11e-7   1.2e-4 / 9.7e-5 / 2.1e-4
                                                                               kernel 9.0e-6 / 9.5e-6 / 2.4e-5
    tail / edge / 2 atoms / 7 atoms / translated / unwrapped     table R=6     1.4e-5 / 8.2e-6 / 1.8e-6 / 1.7e-5 / 1.2e-5 / 1.9e-5
                                                                               kernel 1.1e-5 / 7.2e-6 / 1.6e-6 / 2.2e-5 / 1.3e-5 / 1.6e-5
    cell sweep / list                                            pair table    4.3e-6   2.7e-10   4.3e-5   3.2e-6 / 3.6e-6

    Every backward figure is within its allowance: the kernels sit at 0.7 .. 2.3 x the float32 floor of the formula.  For
    rdf_bwd_kernel<., 6> at width 0.4 that settles the expected failure of test_rdf_variants_below_the_fine_histogram: its 3e-5
    of max |g| is the float32 floor of the shape, the kernel is sound.  The derivative table has ten nodes per centre spacing
    (it had eight: its stated 2e-6 of a unit contribution measured 3.6e-6, tests/test_rdf_ref_host.py); its model_gap fell
    from 1.3 .. 2.8e-6 to 5 .. 11e-7.

    one-hot upstream gradients (first bin / last bin) on the R = 6, R = 11, table and edge cases: all within their
    allowance; where pairs reach the bin the floors are 3e-4 .. 2.3e-2, the largest kernel figure 4.7e-2 where 2.3e-1 is
    allowed (lane/frame, last bin).  These floors are large because an atom whose only contributing pair sits next to the zero
    of dL/dd at d = mu has a scale A as small as the float32 error of that pair (one pair at d - mu = 2.2e-6 sets the
    2.3e-2); a wrong neighbour bin shows as O(1).

(Every test prints floor, model_gap, allowed, the kernel's figure and its distance to its own float64 model per case and
quantity; MDG_TEST_REPORT=<file> collects them.)"""
import os

import numpy as np
import pytest
import torch

import rdf_ref as R
from test_gpu_parity import T, mk_system, DEV  # noqa: F401  (mk_system: the shared fixtures of the GPU tests)

pytestmark = pytest.mark.gpu
MARGIN = 10.0


def _report(line):
    print(line)
    if os.environ.get("MDG_TEST_REPORT"):
        with open(os.environ["MDG_TEST_REPORT"], "a") as fh:
            fh.write(line + "\n")


def _run(case):
    """raw and one gradient per upstream form from ops.RdfRawFn on the case's inputs, under the case's route."""
    from mdgrad_amd import _lib, ops
    cs = _lib.make_cell(case.cell())
    it = case.index_tuple()
    mask = ops.build_mask(case.n_atoms, index_tuple=it, device=DEV) if it is not None else None
    mu = T(case.centres(), DEV)
    x = T(case.frames()[0], DEV).requires_grad_(True)
    saved = ops.RDF_LIST_ATOMS, ops.RDF_CELL_DIRECT
    try:
        if case.liquid:
            ops.RDF_LIST_ATOMS, ops.RDF_CELL_DIRECT = 256, case.expect[0] == "cell"
            cutoff = case.r_range[1] + 0.5
            assert ops._rdf_list_cutoff(cutoff, case.coeff(), case.mu_last()) == case.cutoff()
        else:
            cutoff = case.cutoff()
        raw = ops.RdfRawFn.apply(x, mu, case.coeff(), cutoff, cs, mask, case.spacing(), case.mu_last())
        grads = [torch.autograd.grad((raw * T(g, DEV)).sum(), x, retain_graph=True)[0].cpu().numpy() for g in case.upstream()]
    finally:
        ops.RDF_LIST_ATOMS, ops.RDF_CELL_DIRECT = saved
    return raw.detach().cpu().numpy(), grads


def _check(case):
    route, fwd, bwd, model = R.plan_of(case)
    want = case.expect
    assert route == want[:3], "the case runs %s, not %s" % (route, want[:3])
    if want[0] == "frames":
        assert want[3] is None or (fwd["R"], fwd["waves"], int(fwd["rows128"])) == want[3], fwd
        assert bwd["R"] == want[4], bwd
    al = case.allowances(model)                                   # (CPU only, before the kernel runs)
    ref, m64 = case.reference(), case.reference(model=model)
    raw, grads = _run(case)
    figures = [("raw", R.forward_error(raw, ref), float(np.abs(raw - m64.raw).max() / ref.raw.max()))]
    for k, form in enumerate(case.forms):
        figures.append((form, R.backward_error(grads[k], ref, k, case.a_min(k)),
                        R.backward_error(grads[k], ref, k, case.a_min(k), m64.g_xyz[k])))
    bad = []
    for (q, v, to_model) in figures:
        floor, gap = al[q]
        allowed = MARGIN * floor + gap
        _report("%-34s %-8s floor %.3e  model_gap %.3e  allowed %.3e  kernel %.3e  (to its model %.3e)%s" % (
            case.name, q, floor, gap, allowed, v, to_model, "" if v <= allowed else "   <-- FAILS"))
        if not v <= allowed:
            bad.append((q, v, allowed))
    assert np.isfinite(raw).all() and all(np.isfinite(g).all() for g in grads)
    assert not bad, "%s: %s" % (case.name, bad)
    return raw, grads


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_rdf_variant_against_float64(name):
    """One case of rdf_ref.CASES: few frames (direct / block8 forward, atom backward; arbitrary and non-linspace centres),
    1 024 frames of 48 atoms for half and lane with the table (R = 6, 11: orthorhombic, triclinic with the cutoff inside the
    centres, masked) and the recurrence backward (R = 6 at width 0.4, R = 11 with 500 centres and one wave per workgroup),
    the direct sum of rdf_bwd_kernel, the fine histogram at 64 and 65 atoms (odd, second lane group, masked), a tail
    workgroup (1 025 frames), centres whose first and last bins have accepted pairs beyond them, 2 and 7 atoms, translated and
    unwrapped frames (clamped minimum image), two coincident atoms, and the cell sweep and the list route at 512 atoms."""
    case = R.BY_NAME[name]
    raw, grads = _check(case)
    if "coincident" in name:                   # (the pair at d = 0 is rejected: _check found the reference's finite gradient)
        x = case.frames()[0]
        assert (x[:, 17] == x[:, 3]).all() and np.isfinite(grads[0]).all() and np.abs(grads[0][:, 17]).max() > 0


# ------------------------------------------------------------------ the cell sweep in a box of a whole number of cutoffs
def _bin_edge_inputs(k):
    """Construction k of tests/golden/nbr_bin_edge.npz (tests/nbr_ref.py case F: a pair at the cutoff across one bin, four
    filler atoms) as one frame for the C entry points of csrc/rdf_cell.hip: 20 centres over the last length unit below the
    cutoff, sigma = two spacings, and an upstream gradient on the centre one sigma below the cutoff, where a pair at the
    cutoff pulls hardest (|dL/dd| = exp(-1/2) / sigma, about 5.8)."""
    import nbr_ref
    c = nbr_ref.cases()["F construction %d" % k]
    rc = float(np.float32(c.cutoff))
    mu = torch.linspace(rc - 1.0, rc, 20).numpy().copy()
    dmu = float(mu[1] - mu[0])
    g = np.zeros(20, np.float32)
    g[17] = 1.0
    return c, mu, dmu, -0.5 / (2.0 * dmu) ** 2, g


@pytest.mark.parametrize("k", range(6))
def test_cell_sweep_gradient_in_a_box_of_a_whole_number_of_cutoffs(k):
    """mdg_rdf_fwd_cell + mdg_rdf_bwd_cell, called directly (ops.RdfRawFn takes this route from 512 atoms only, and puts the
    list cutoff 5.3 widths beyond the last centre, where a pair at the cutoff weighs 2^-28): the gradient on the two atoms of
    a pair that sits at the cutoff, two x- or y-bins apart when bins are exactly one cutoff wide, against the float64
    reference -- measure and allowance as above (u-space pair table).  make_grid's x and y bins had no margin over the cutoff;
    the sweep then never met these pairs (z is binned finer, with a margin of its own).  The forward histogram is not judged:
    its fine grid ends at the cutoff by design, so a pair within float32 rounding of it is outside.
    On an MI355X: floor 6.0e-8 (1.1e-7 for construction 5), allowed 6.0e-7 (1.1e-6), kernel 2.6e-8 .. 1.2e-7; with
    floor(L / cutoff) bins along x and y the four constructions along x or y measured 1.0 (no gradient at all), the two
    along z 2.6e-8 and 1.1e-7."""
    from mdgrad_amd import _lib, ops
    from mdgrad_amd._lib import check, ptr, stream_ptr
    import ctypes as C
    lib = _lib.load()
    c, mu, dmu, coeff, g = _bin_edge_inputs(k)
    n, cutoff = len(c.pos), float(np.float32(c.cutoff))
    cs = _lib.make_cell(c.cell)
    assert lib.mdg_rdf_cell_supported(n, C.byref(cs), cutoff) == 1 and lib.mdg_rdf_ell_supported(dmu, coeff, 20) == 1
    frames = c.pos[None]
    kw = dict(g_raw=g[None], dtype=np.float64)
    ref = R.rdf_reference(frames, c.cell, mu, coeff, cutoff, **kw)
    m64 = R.rdf_reference(frames, c.cell, mu, coeff, cutoff, model=("utable", 4096), **kw)
    m32 = R.rdf_reference(frames, c.cell, mu, coeff, cutoff, g_raw=g[None], dtype=np.float32, model=("utable", 4096))
    assert ref.A[0][0, 0] > 5.0 and ref.A[0][0, 1] > 5.0, "the pair must pull visibly"
    a_min = R.scale_floor(g, coeff)
    scale = (ref.A[0] + a_min)[..., None]
    floor = max(float((np.abs(m32.g_xyz[0].astype(np.float64) - m64.g_xyz[0]) / scale).max()), R.ULP)
    gap = float((np.abs(m64.g_xyz[0] - ref.g_xyz[0]) / scale).max())
    allowed = MARGIN * floor + gap
    x, muc = T(c.pos, DEV), T(mu, DEV)
    raw = torch.empty(20, device=DEV)
    scratch = torch.empty(int(lib.mdg_rdf_cell_scratch(1, n, C.byref(cs), cutoff)) + 4, dtype=torch.int32, device=DEV)
    check(lib.mdg_rdf_fwd_cell(ptr(x), 1, n, C.byref(cs), cutoff, ptr(muc), dmu, coeff, 20, ptr(raw), ptr(scratch),
                               stream_ptr(x.device)), "mdg_rdf_fwd_cell")
    table, u0, du = ops._rdf_pair_table(T(g, DEV), muc, coeff, cutoff, 4096)
    term = ops.make_term(dict(kind=ops.MDG_PAIR_TABLE, p=4096, a=u0, phi=du, c=1.0), cutoff, 0, 2 * 4096, None)
    gx = torch.full_like(x, float("nan"))
    check(lib.mdg_rdf_bwd_cell(1, n, C.byref(cs), cutoff, C.byref(term), ptr(table), ptr(scratch), ptr(gx), stream_ptr(x.device)),
          "mdg_rdf_bwd_cell")
    torch.cuda.synchronize()
    got = gx.cpu().numpy()[None]
    v = R.backward_error(got, ref, 0, a_min)
    _report("cell sweep, bin-edge construction %d  floor %.3e  model_gap %.3e  allowed %.3e  kernel %.3e%s" % (
        k, floor, gap, allowed, v, "" if v <= allowed else "   <-- FAILS"))
    assert np.isfinite(raw.cpu().numpy()).all()
    assert v <= allowed, (k, v, allowed, got[0, :2], ref.g_xyz[0][0, :2])
