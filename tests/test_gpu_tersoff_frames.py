"""K38: the Tersoff energy of every frame (thermo.TersoffEnergy, ops.TersoffFramesFn / ops.TersoffMultiFramesFn,
mdg_tersoff_frames_fwd / mdg_tersoff_multi_frames_fwd, csrc/tersoff_frames.hip) against the float64 definitions of
tests/tersoff_ref.py and tests/tersoff_multi_ref.py, frame by frame, and against the list kernels K25 / K26.

Tolerance: that of tests/test_gpu_tersoff.py for the same formulas, K * 2^-24 * A per component with K = 64 and A = the float64 sum
of the absolute contributions of the bond halves and the triplet terms to that component of that frame (evaluate: A_U, A_dth,
A_grad) at the module's float32 parameters; for L = sum_f gU_f U_f the scale is sum_f |gU_f| A_f.  U[f] against the list
kernel's model(q[f]): 2 K (two float32 kernels).  `within` (tests/test_gpu_sw.py) prints the largest observed err / (2^-24 A)
of every comparison.  No case is left out: the model is C1 at both taper edges and at zeta -> 0.  The fixtures
(tests/tersoff_frames_cases.py) keep their cutoffs below half the box and their rows inside the cap; that is asserted on the
CPU by tests/test_tersoff_frames_host.py.

Largest observed err / (2^-24 A) on an MI355X: U[f] 3.99 (long_rows; si 2.83, sic 0.67, gas37 3.82, c64 0.15, s3 1.24),
dU[f]/dtheta 5.60 for one species (si, lam3), 4.59 for SiC and 23.22 for the three species of s3_frames, d(sum g U)/dtheta 4.94
(lam3; gas37 4.82, long_rows 4.64, s3 3.74, sic_asym 2.81), d(sum g U)/dx through K25 / K26 20.02 / 13.45 with the parameter
gradient on that route 2.33 / 3.08, U[f] against K25 / K26 0.01 / 0.08 (of the doubled scale), after the parameter edit 2.61 /
0.59 (U) and 4.06 / 3.18 (gradient), the shifted and wrapped twins 2.42 at most.  K stays 64.

The float64 references of all frames are computed once per module and shared."""
import ctypes

import numpy as np
import pytest
import torch

import tersoff_frames_cases as TC
from test_gpu_sw import within
from test_gpu_parity import DEV, mk_system

pytestmark = pytest.mark.gpu
F32 = np.float32


def modules(case):
    return case.modules(mk_system(case.frames[0], case.cell))


def params(model):
    return (model.A, model.B, model.h)


def flat_grad(loss, model, **kw):
    return torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, params(model), **kw)])


def q_of(case, n=None, requires_grad=False):
    return torch.tensor(case.frames[:n], device=DEV).requires_grad_(requires_grad)


def fn_of(case):
    from mdgrad_amd import ops
    return ops.TersoffMultiFramesFn if case.multi else ops.TersoffFramesFn


def check_values(case, n=None, rows=3):
    """U, the first dU/dtheta rows and d(sum g U)/dtheta of one launch against float64; returns (model, energy, reference, U)"""
    tag = case.name if n is None else "%s F=%d" % (case.name, n)
    model, energy = modules(case)
    ref = case.reference(model, n)
    q = q_of(case, n)
    U = energy(q)
    assert U.shape == (q.shape[0],) and U.dtype == torch.float32
    within(U, ref["U"], ref["A_U"], tag + " U[f]")
    eye = torch.eye(q.shape[0], device=DEV)
    k = min(q.shape[0], rows)
    dU = torch.stack([flat_grad(U, model, grad_outputs=eye[f], retain_graph=True) for f in range(k)])
    within(dU, ref["dth"][:k], ref["A_dth"][:k], tag + " dU[f]/dtheta (first frames)")
    assert fn_of(case).last_route == "theta"
    g = torch.tensor(np.random.default_rng(5).normal(0, 1, q.shape[0]), dtype=torch.float32, device=DEV)
    gth = flat_grad((U * g).sum(), model)
    g64 = g.double().cpu()
    within(gth, (g64[:, None] * ref["dth"]).sum(0), (g64.abs()[:, None] * ref["A_dth"]).sum(0), tag + " d(sum g U)/dtheta")
    return model, energy, ref, U


@pytest.fixture(scope="module")
def si():
    return TC.si_frames(6)


@pytest.fixture(scope="module")
def sic():
    return TC.sic_frames(6)


@pytest.fixture(scope="module", params=["si", "sic"])
def both(request, si, sic):
    return si if request.param == "si" else sic


# ------------------------------------------------------------------------------------------------ 1, 2: values against float64
@pytest.mark.parametrize("n", [1, 3, 6])
def test_values_and_per_frame_parameter_rows(both, n):
    """64 atoms: a wave per frame, four frames per workgroup; six frames end in a workgroup that is half empty."""
    check_values(both, n, rows=n)


@pytest.mark.parametrize("make", [TC.si216, TC.long_rows, TC.lam3, TC.c64, TC.sic_asym, TC.s3_frames],
                         ids=["si216", "long_rows", "lam3", "c64", "sic_asym", "s3_frames"])
def test_weighted_parameter_gradient(make):
    case = make()
    model, energy, ref, U = check_values(case)
    if case.name == "sic_asym":
        dA = ref["dth"][:, :4].reshape(-1, 2, 2)
        assert bool((dA[:, 0, 1] != dA[:, 1, 0]).all()), "the two directed Si-C pairs differ in their supports"


def test_gas37_empty_row_dimer_hub_and_coincident_atoms():
    case = TC.gas37()
    assert case.N == 37
    model, energy, ref, U = check_values(case)
    rows = ref["rows"][0].tolist()
    assert rows[0] == 18 and rows[31] == 0 and rows[32] == rows[33] == 1
    assert bool(torch.isfinite(U).all()) and float(U[0].detach()) != float(U[1].detach())


# ------------------------------------------------------------------------------------------------ 3: position gradient
def test_position_gradient_against_float64(both):
    case, n = both, 5
    model, energy = modules(case)
    ref = case.reference(model, n)
    q = q_of(case, n, requires_grad=True)
    g = torch.tensor([1.0, -0.5, 0.0, 2.0, 0.25], device=DEV)
    U = energy(q)
    out = torch.autograd.grad((U * g).sum(), (q,) + params(model))
    assert fn_of(case).last_route == "full"
    gq, gth = out[0], torch.cat([t.reshape(-1) for t in out[1:]])
    g64 = g.double().cpu()
    within(gq, g64[:, None, None] * ref["grad"], g64.abs()[:, None, None] * ref["A_grad"], case.name + " d(sum g U)/dx")
    assert float(gq[2].abs().max()) == 0.0
    within(gth, (g64[:, None] * ref["dth"]).sum(0), (g64.abs()[:, None] * ref["A_dth"]).sum(0),
           case.name + " d(sum g U)/dtheta on the full route")
    # shapes: a single frame, [R, T, N, 3], replica-stacked
    qd = q.detach()
    assert energy(qd[1]).shape == () and float(energy(qd[1]).detach()) == float(U[1].detach())
    assert torch.equal(energy(qd[:4].reshape(2, 2, 64, 3)).reshape(4).detach(), U[:4].detach())
    st = energy(torch.cat([qd[:2], qd[2:4]], dim=1)).detach()
    assert st.shape == (2, 2) and torch.equal(st[:, 0], U[:2].detach()) and torch.equal(st[:, 1], U[2:4].detach())


# ------------------------------------------------------------------------------------------------ 4: detached frames
def test_detached_frames_take_the_no_walk_backward(both):
    case, n = both, 6
    model, energy = modules(case)
    q = q_of(case, n)
    g = torch.tensor(np.random.default_rng(9).normal(0, 1, n), dtype=torch.float32, device=DEV)
    fn_of(case).last_route = None
    U = energy(q)
    th = flat_grad((U * g).sum(), model)
    assert fn_of(case).last_route == "theta" and not q.requires_grad
    qg = q_of(case, n, requires_grad=True)
    U2 = energy(qg)
    out = torch.autograd.grad((U2 * g).sum(), (qg,) + params(model))
    assert fn_of(case).last_route == "full"
    assert torch.equal(th, torch.cat([t.reshape(-1) for t in out[1:]])), "the same launch and the same sum serve both routes"
    # the value part does not depend on whether dU/dtheta is emitted
    with torch.no_grad():
        U0 = energy(q)
    for p in params(model):
        p.requires_grad_(False)
    U1 = energy(q)
    assert not U1.requires_grad and torch.equal(U0, U.detach()) and torch.equal(U1, U.detach()) and torch.equal(U2.detach(), U0)


# ------------------------------------------------------------------------------------------------ 5: the list kernels
def test_against_the_list_kernel(both):
    case, n = both, 6
    model, energy = modules(case)
    ref = case.reference(model, n)
    q = q_of(case, n)
    with torch.no_grad():
        U = energy(q)
        Um = []
        for f in range(n):
            model._reset_topology(q[f])                     # (the list of K25 / K26 follows the positions only when asked to)
            Um.append(model(q[f]).reshape(()))
        Um = torch.stack(Um)
    within(U, Um.double().cpu(), 2 * ref["A_U"], case.name + " U[f] against model(q[f]) (K25 / K26)")


# ------------------------------------------------------------------------------------------------ 6: bits
def _launch(case, model, energy, x):
    """U and the rows dU_dtheta of a launch of its own, through the C entry point"""
    from mdgrad_amd import _lib
    lib = _lib.load()
    F, S = x.shape[0], getattr(model, "n_species", 1)
    P = 2 * S * S + S if case.multi else 3
    U, dU = torch.empty(F, device=DEV), torch.empty(F, P, device=DEV)
    cs = ctypes.byref(energy._cell_struct)
    if case.multi:
        _lib.check(lib.mdg_tersoff_multi_frames_fwd(_lib.ptr(x), F, case.N, cs, _lib.ptr(energy._types), S,
                                                    _lib.ptr(model._tables()), _lib.ptr(U), _lib.ptr(dU),
                                                    _lib.stream_ptr(x.device)), "mdg_tersoff_multi_frames_fwd")
    else:
        _lib.check(lib.mdg_tersoff_frames_fwd(_lib.ptr(x), F, case.N, cs, ctypes.byref(model._consts), _lib.ptr(model._theta()),
                                              _lib.ptr(U), _lib.ptr(dU), _lib.stream_ptr(x.device)), "mdg_tersoff_frames_fwd")
    return U, dU


@pytest.mark.parametrize("which", ["si", "sic"])
def test_bitwise_reproducible_and_frame_order(which):
    """130 frames, flipped: needs no float64 reference"""
    case = TC.si_frames(130) if which == "si" else TC.sic_frames(130)
    model, energy = modules(case)
    q = q_of(case)
    g = torch.tensor(np.random.default_rng(11).normal(0, 1, 130), dtype=torch.float32, device=DEV)

    def run(x, gx):
        U = energy(x)
        th = flat_grad((U * gx).sum(), model)
        U2, dU = _launch(case, model, energy, x)
        assert torch.equal(U2, U.detach())
        return U.detach(), dU, th

    U1, d1, t1 = run(q, g)
    U2, d2, t2 = run(q, g)
    assert torch.equal(U1, U2) and torch.equal(d1, d2) and torch.equal(t1, t2)
    assert bool(torch.isfinite(U1).all()) and bool(torch.isfinite(d1).all()) and len(set(U1.tolist())) == 130
    Ur, dr, tr = run(q.flip(0).contiguous(), g.flip(0).contiguous())
    assert torch.equal(Ur.flip(0), U1) and torch.equal(dr.flip(0), d1)


# ------------------------------------------------------------------------------------------------ 7: images
def test_shifted_and_wrapped_frames_equal_their_unwrapped_twin():
    for base in (TC.si_frames(8), TC.sic_frames(8)):
        x, cell = base.frames[7], base.cell
        shifted = x + np.array([cell[0], 0.0, -cell[2]], dtype=F32)
        # atoms within 0.6 A of a face carried across it: x holds them wrapped into [0, L), this twin unwrapped
        wrapped = x.copy()
        lo, hi = x[:, 1] < 0.6, x[:, 0] > cell[0] - 0.6
        wrapped[lo, 1] += cell[1]
        wrapped[hi, 0] -= cell[0]
        assert lo.sum() >= 2 and hi.sum() >= 2
        case = TC.Case(base.name, np.stack([x, shifted, wrapped]), cell, params=base.params, tab=base.tab, types=base.types)
        model, energy = modules(case)
        ref = case.reference(model, 1)
        U = energy(q_of(case))
        for f, what in ((1, "shifted by a cell vector"), (2, "wrapped across the boundary")):
            within(U[f:f + 1], ref["U"], ref["A_U"], "%s %s: U against the unwrapped twin's float64" % (case.name, what))
            within(U[f:f + 1], U[:1].double().cpu(), 2 * ref["A_U"],
                   "%s %s: U against the unwrapped twin's kernel value" % (case.name, what))


# ------------------------------------------------------------------------------------------------ 8: the row cap
@pytest.mark.parametrize("multi", [False, True], ids=["si", "sige"])
def test_a_row_beyond_the_cap_gives_nan_for_its_frame_alone(multi):
    from mdgrad_amd import ops
    case = TC.overflow(multi)
    cap = ops.tersoff_frames_row_cap()
    assert case.longest_row(1) > cap and case.longest_row(0) < cap
    model, energy = modules(case)
    q = q_of(case)
    U = energy(q)
    assert bool(torch.isnan(U[1])) and bool(torch.isfinite(U[0])) and torch.equal(U[0].detach(), U[2].detach())
    U2, dU = _launch(case, model, energy, q)
    assert torch.equal(U2[[0, 2]], U.detach()[[0, 2]]) and bool(torch.isnan(U2[1]))
    assert bool(torch.isnan(dU[1]).all()) and bool(torch.isfinite(dU[0]).all()) and torch.equal(dU[0], dU[2])


# ------------------------------------------------------------------------------------------------ 9: live parameters
def test_an_edit_of_the_parameters_is_followed_without_any_other_action(both):
    case, n = both, 3
    model, energy = modules(case)
    q = q_of(case, n)
    with torch.no_grad():
        U0 = energy(q)
    if case.multi:
        model.B.data[0, 1] *= 1.05
    else:
        model.A.data *= 1.05
    ref = case.reference(model, n)                      # (keyed by the parameters: float64 at the edited set)
    U = energy(q)
    within(U, ref["U"], ref["A_U"], case.name + " U[f] after the edit")
    assert not torch.equal(U.detach(), U0)
    gth = flat_grad(U.sum(), model)
    within(gth, ref["dth"].sum(0), ref["A_dth"].sum(0), case.name + " d(sum U)/dtheta after the edit")
