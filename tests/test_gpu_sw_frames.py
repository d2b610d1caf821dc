"""K34: the Stillinger-Weber energy of every frame (thermo.StillingerWeberEnergy, ops.SWFramesFn, mdg_sw_frames_fwd,
csrc/sw_frames.hip) against the float64 definition of tests/sw_ref.py, frame by frame, and against the list kernel K23.

Tolerance: that of tests/test_gpu_sw.py for the same formulas, K * 2^-24 * A per component with K = 64 and A = the float64 sum of
the absolute pair and triplet contributions to that component of that frame (sw_ref.evaluate: A_U, A_dth, A_grad); for
L = sum_f gU_f U_f the scale is sum_f |gU_f| A_f.  U[f] against K23's model(q[f]): 2 K (two float32 kernels).  `within` prints
the largest observed err / (2^-24 A) of every comparison.  No case is left out: the Stillinger-Weber terms vanish smoothly at
the cutoff, and a sigma stays below half the box in every fixture (asserted).

Largest observed err / (2^-24 A) on an MI355X: U 3.93 (130 frames) and 4.22 (the shifted frame, whose float32 positions are not
its twin's), dU[f]/dtheta 21.80, d(sum g U)/dtheta 21.60, d(sum g U)/dx 17.48, U against K23 0.45 (of the doubled scale), the long rows 0.75 / 1.72.
dU/dtheta beyond 16 is K23's own figure on the same frame (21.80 on Si-64, tests/test_gpu_sw.py: the two product-rule terms of
phi2' cancel and each carries the rounding of r); K stays 64.

The float64 references of all frames are computed once per module and shared."""
import ctypes

import numpy as np
import pytest
import torch

import sw_ref as R
from test_gpu_sw import K, SI, within
from test_gpu_parity import DEV, mk_system

pytestmark = pytest.mark.gpu
F32 = np.float32
A0 = 5.431


class Case:
    """frames [F, N, 3] of one box at theta, with the float64 U, dU/dtheta, dU/dx and their scales per frame"""

    def __init__(self, frames, cell, theta=SI):
        self.frames, self.cell, self.theta = np.ascontiguousarray(frames, dtype=F32), np.asarray(cell, dtype=F32), theta
        self.F, self.N = self.frames.shape[0], self.frames.shape[1]
        self._ref = {}

    def modules(self, system=None):
        from mdgrad_amd.interface import StillingerWeber
        from mdgrad_amd.thermo import StillingerWeberEnergy
        system = mk_system(self.frames[0], self.cell) if system is None else system
        model = StillingerWeber(system, self.theta[0], self.theta[1], lam=self.theta[2])
        assert K["a"] * float(model.sigma.detach()) < 0.5 * float(self.cell.min()), "a sigma below half the box"
        return model, StillingerWeberEnergy(system, model)

    def reference(self, model, n=None):
        """dict of stacked float64 arrays for the first n frames at the module's float32 parameters"""
        th = tuple(float(p.detach()) for p in (model.epsilon, model.sigma, model.lam))
        n = self.F if n is None else n
        for f in range(n):
            if (th, f) not in self._ref:
                lst = R.pairs_and_triplets(self.frames[f], self.cell, K["a"] * th[1])
                self._ref[(th, f)] = (R.evaluate(self.frames[f], th, lst, self.cell, K), lst)
        refs = [self._ref[(th, f)][0] for f in range(n)]
        out = {k: torch.stack([r[k] for r in refs]) for k in ("U", "A_U", "dth", "A_dth", "grad", "A_grad")}
        out["rows"] = [self._ref[(th, f)][1]["rows"] for f in range(n)]
        return out

    def q(self, n=None, requires_grad=False):
        return torch.tensor(self.frames[:n], device=DEV).requires_grad_(requires_grad)


def check_values(case, n=None, tag=""):
    """U and dU/dtheta of one launch against float64; returns (model, energy, reference, U, dU)"""
    from mdgrad_amd import ops
    model, energy = case.modules()
    ref = case.reference(model, n)
    q = case.q(n)
    U = energy(q)
    assert U.shape == (q.shape[0],) and U.dtype == torch.float32
    within(U, ref["U"], ref["A_U"], tag + " U[f]")
    # dU/dtheta per frame: the rows the launch emits = the gradient of each U[f] on its own
    eye = torch.eye(q.shape[0], device=DEV)
    dU = torch.stack([torch.cat(torch.autograd.grad(U, (model.epsilon, model.sigma, model.lam), eye[f], retain_graph=True))
                      for f in range(min(q.shape[0], 3))])
    within(dU, ref["dth"][:dU.shape[0]], ref["A_dth"][:dU.shape[0]], tag + " dU[f]/dtheta (first frames)")
    assert ops.SWFramesFn.last_route == "theta"
    # L = sum_f g_f U_f over all frames: scale sum_f |g_f| A_f
    g = torch.tensor(np.random.default_rng(5).normal(0, 1, q.shape[0]), dtype=torch.float32, device=DEV)
    gth = torch.cat(torch.autograd.grad((U * g).sum(), (model.epsilon, model.sigma, model.lam)))
    g64 = g.double().cpu()
    within(gth, (g64[:, None] * ref["dth"]).sum(0), (g64.abs()[:, None] * ref["A_dth"]).sum(0), tag + " d(sum g U)/dtheta")
    return model, energy, ref, U, g


@pytest.fixture(scope="module")
def si64():
    xs = [R.jittered_diamond(2, A0, 0.3, 64 + s) for s in range(130)]
    return Case(np.stack([x for x, _ in xs]), xs[0][1])


# ------------------------------------------------------------------------------------------------ values against float64
@pytest.mark.parametrize("n", [1, 3, 130])
def test_si64_values_and_parameter_gradients(si64, n):
    """64 atoms: a wave per frame, four frames per workgroup; 130 frames end in a workgroup that is half empty."""
    model, energy, ref, U, g = check_values(si64, n, "si64 F=%d" % n)
    rows = torch.cat(ref["rows"])
    assert int(rows.min()) >= 4 and int(rows.max()) >= 12


def test_si216_spans_several_waves():
    x, cell = R.jittered_diamond(3, A0, 0.3, 216)
    x2, _ = R.jittered_diamond(3, A0, 0.25, 217)
    check_values(Case(np.stack([x, x2]), cell), None, "si216")


def _subset37():
    """37 atoms of the 64-atom frame: atom 0 of the subset without a neighbour, atoms 1 and 2 an isolated dimer; frame 1 is the
    same with atom 4 moved onto atom 3 (r = 0: skipped)."""
    x, cell = R.jittered_diamond(2, A0, 0.3, 64)
    lst = R.pairs_and_triplets(x, cell, K["a"] * float(F32(SI[1])))
    nb = [set() for _ in range(64)]
    for i, j in zip(lst["i"].tolist(), lst["j"].tolist()):
        nb[i].add(j), nb[j].add(i)
    best = None
    for a in range(64):
        for b in range(64):
            for c in nb[b]:
                if a in (b, c) or a in nb[b] or a in nb[c] or c < b:
                    continue
                gone = nb[a] | (nb[b] - {c}) | (nb[c] - {b})
                if best is None or len(gone) < len(best[3]):
                    best = (a, b, c, gone)
    a, b, c, gone = best
    assert len(gone) <= 27
    rest = [i for i in range(64) if i not in gone and i not in (a, b, c)]
    keep = [a, b, c] + rest[:34]
    assert len(keep) == 37
    f0 = x[keep]
    f1 = f0.copy()
    f1[4] = f1[3]
    return Case(np.stack([f0, f1]), cell)


def test_subset37_empty_row_dimer_and_coincident_atoms():
    case = _subset37()
    assert case.N == 37 and 37 % 64 != 0
    model, energy, ref, U, g = check_values(case, None, "sub37")
    rows = ref["rows"][0].tolist()
    assert rows[0] == 0 and rows[1] == rows[2] == 1 and max(rows) >= 4
    assert bool((torch.tensor(case.frames[1][3]) == torch.tensor(case.frames[1][4])).all())
    assert bool(torch.isfinite(U).all()) and float(U[0].detach()) != float(U[1].detach())


def test_long_rows_are_finite_and_within_tolerance():
    """sigma = 2.9 on the 64-atom box jittered by 0.15: a sigma = 5.22 < 5.431, rows of 28 - 31 neighbours."""
    xs = [R.jittered_diamond(2, A0, 0.15, 64 + s)[0] for s in range(2)]
    case = Case(np.stack(xs), R.jittered_diamond(2, A0, 0.15, 64)[1], theta=(SI[0], 2.9, SI[2]))
    model, energy, ref, U, g = check_values(case, None, "long rows")
    rows = ref["rows"][0]
    assert int(rows.min()) >= 28 and int(rows.max()) <= 31, (int(rows.min()), int(rows.max()))
    from mdgrad_amd import ops
    assert int(torch.cat(ref["rows"]).max()) <= ops.sw_frames_row_cap()


def test_shifted_and_wrapped_frames_equal_their_unwrapped_twin():
    x, cell = R.jittered_diamond(2, A0, 0.3, 71)
    shifted = x + np.array([cell[0], 0.0, -cell[2]], dtype=F32)
    # atoms within 0.6 A of a face carried across it: x holds them wrapped into [0, L), this twin unwrapped (every difference
    # stays inside one and a half cells, where the minimum image of the definition holds)
    wrapped = x.copy()
    lo, hi = x[:, 1] < 0.6, x[:, 0] > cell[0] - 0.6
    wrapped[lo, 1] += cell[1]
    wrapped[hi, 0] -= cell[0]
    assert lo.sum() >= 2 and hi.sum() >= 2
    case = Case(np.stack([x, shifted, wrapped]), cell)
    model, energy = case.modules()
    ref = case.reference(model, 1)
    U = energy(case.q())
    for f, what in ((1, "shifted by a cell vector"), (2, "wrapped across the boundary")):
        within(U[f:f + 1], ref["U"], ref["A_U"], "si64 " + what + ": U against the unwrapped twin's float64")
        within(U[f:f + 1], U[:1].double().cpu(), 2 * ref["A_U"], "si64 " + what + ": U against the unwrapped twin's kernel value")


# ------------------------------------------------------------------------------------------------ position gradient
def test_position_gradient_against_float64(si64):
    from mdgrad_amd import ops
    n = 5
    model, energy = si64.modules()
    ref = si64.reference(model, n)
    q = si64.q(n, requires_grad=True)
    g = torch.tensor([1.0, -0.5, 0.0, 2.0, 0.25], device=DEV)
    U = energy(q)
    gq, ge, gs, gl = torch.autograd.grad((U * g).sum(), (q, model.epsilon, model.sigma, model.lam))
    assert ops.SWFramesFn.last_route == "full"
    g64 = g.double().cpu()
    within(gq, g64[:, None, None] * ref["grad"], g64.abs()[:, None, None] * ref["A_grad"], "si64 d(sum g U)/dx")
    assert float(gq[2].abs().max()) == 0.0
    within(torch.cat([ge, gs, gl]), (g64[:, None] * ref["dth"]).sum(0), (g64.abs()[:, None] * ref["A_dth"]).sum(0),
           "si64 d(sum g U)/dtheta on the full route")
    # shapes: a single frame, [R, T, N, 3], replica-stacked
    qd = q.detach()
    assert energy(qd[1]).shape == () and float(energy(qd[1]).detach()) == float(U[1].detach())
    assert torch.equal(energy(qd[:4].reshape(2, 2, 64, 3)).reshape(4), U[:4].detach())
    st = energy(torch.cat([qd[:2], qd[2:4]], dim=1))
    assert st.shape == (2, 2) and torch.equal(st[:, 0], U[:2].detach()) and torch.equal(st[:, 1], U[2:4].detach())


# ------------------------------------------------------------------------------------------------ detached frames: reweighting
def test_detached_frames_take_the_no_walk_backward(si64):
    from mdgrad_amd import ops
    n = 9
    model, energy = si64.modules()
    q = si64.q(n)
    g = torch.tensor(np.random.default_rng(9).normal(0, 1, n), dtype=torch.float32, device=DEV)
    ops.SWFramesFn.last_route = None
    U = energy(q)
    th = torch.cat(torch.autograd.grad((U * g).sum(), (model.epsilon, model.sigma, model.lam)))
    assert ops.SWFramesFn.last_route == "theta" and not q.requires_grad
    # ... equal to the parameter gradient of the full route within the tolerance of the two
    qg = si64.q(n, requires_grad=True)
    U2 = energy(qg)
    out = torch.autograd.grad((U2 * g).sum(), (qg, model.epsilon, model.sigma, model.lam))
    assert ops.SWFramesFn.last_route == "full"
    ref = si64.reference(model, n)
    A = (g.double().cpu().abs()[:, None] * ref["A_dth"]).sum(0)
    within(th, torch.cat(out[1:]).double().cpu(), 2 * A, "si64 parameter gradient: no-walk route against the full route")
    assert torch.equal(th, torch.cat(out[1:])), "the same launch and the same sum serve both routes"
    # the value part does not depend on whether dU/dtheta is emitted
    with torch.no_grad():
        U0 = energy(q)
    for p in (model.epsilon, model.sigma, model.lam):
        p.requires_grad_(False)
    U1 = energy(q)
    assert not U1.requires_grad and torch.equal(U0, U.detach()) and torch.equal(U1, U.detach())


def test_against_the_list_kernel(si64):
    n = 6
    model, energy = si64.modules()
    ref = si64.reference(model, n)
    q = si64.q(n)
    with torch.no_grad():
        U = energy(q)
        Um = []
        for f in range(n):
            model._reset_topology(q[f])                     # (the list of K23 follows the positions only when asked to)
            Um.append(model(q[f]).reshape(()))
        Um = torch.stack(Um)
    within(U, Um.double().cpu(), 2 * ref["A_U"], "si64 U[f] against StillingerWeber(q[f]) (K23)")


def test_bitwise_reproducible_and_frame_order(si64):
    model, energy = si64.modules()
    q = si64.q(130)
    g = torch.tensor(np.random.default_rng(11).normal(0, 1, 130), dtype=torch.float32, device=DEV)

    def run(x, gx):
        from mdgrad_amd import _lib, ops
        U = energy(x)
        th = torch.cat(torch.autograd.grad((U * gx).sum(), (model.epsilon, model.sigma, model.lam)))
        # the rows dU_dtheta [F, 3] of a launch of its own
        lib = _lib.load()
        theta = torch.cat([p.detach().reshape(-1) for p in (model.epsilon, model.sigma, model.lam)])
        U2, dU = torch.empty(x.shape[0], device=DEV), torch.empty(x.shape[0], 3, device=DEV)
        _lib.check(lib.mdg_sw_frames_fwd(_lib.ptr(x.contiguous()), x.shape[0], 64, ctypes.byref(energy._cell_struct),
                                         ctypes.byref(model._consts), _lib.ptr(theta), _lib.ptr(U2), _lib.ptr(dU),
                                         _lib.stream_ptr(x.device)), "mdg_sw_frames_fwd")
        assert torch.equal(U2, U.detach())
        return U.detach(), dU, th

    U1, d1, t1 = run(q, g)
    U2, d2, t2 = run(q, g)
    assert torch.equal(U1, U2) and torch.equal(d1, d2) and torch.equal(t1, t2)
    Ur, dr, tr = run(q.flip(0).contiguous(), g.flip(0).contiguous())
    assert torch.equal(Ur.flip(0), U1) and torch.equal(dr.flip(0), d1)


def test_a_step_of_sigma_moves_the_support_without_a_list(si64):
    n = 3
    model, energy = si64.modules()
    q = si64.q(n)
    with torch.no_grad():
        U0 = energy(q)
    ell0, ver0 = model._ell, model._cut_ver
    model.sigma.data.mul_(1.03)
    assert K["a"] * float(model.sigma.detach()) < 0.5 * float(si64.cell.min())
    ref = si64.reference(model, n)                     # (keyed by the parameters: float64 at the new sigma)
    U = energy(q)
    within(U, ref["U"], ref["A_U"], "si64 U[f] after sigma *= 1.03")
    dth = torch.cat(torch.autograd.grad(U.sum(), (model.epsilon, model.sigma, model.lam)))
    within(dth, ref["dth"].sum(0), ref["A_dth"].sum(0), "si64 d(sum U)/dtheta after sigma *= 1.03")
    assert not torch.equal(U.detach(), U0)
    assert model._ell is ell0 and model._cut_ver == ver0, "the energy path searched no list"
    old = si64.reference(si64.modules()[0], n)
    assert sum(int(r.sum()) for r in ref["rows"]) > sum(int(r.sum()) for r in old["rows"]), "the larger support holds more pairs"


def test_a_row_beyond_the_cap_gives_nan_for_its_frame_alone():
    """128 atoms (two shifted copies of the 64-atom frame): in the middle frame 70 of them sit in a ball of radius ~1 A, so their
    rows hold 69 neighbours, beyond the cap of 64.  That frame comes out NaN; its neighbours in the batch do not."""
    from mdgrad_amd import ops
    rng = np.random.default_rng(3)
    x, cell = R.jittered_diamond(2, A0, 0.3, 64)
    ok = np.concatenate([x, np.mod(x + 1.1, cell)]).astype(F32)
    bad = ok.copy()
    bad[:70] = (np.array([5.0, 5.0, 5.0]) + rng.normal(0, 0.5, (70, 3))).astype(F32)
    case = Case(np.stack([ok, bad, ok]), cell)
    model, energy = case.modules()
    rc = K["a"] * float(model.sigma.detach())

    def longest(fr):
        d = fr[None, :, :].astype(np.float64) - fr[:, None, :]
        d -= np.rint(d / cell) * cell
        r = np.sqrt((d ** 2).sum(-1))
        return int(((r < rc) & (r > 0)).sum(1).max())
    assert longest(bad) > ops.sw_frames_row_cap() and longest(ok) < ops.sw_frames_row_cap()
    for p in (model.epsilon, model.sigma, model.lam):
        p.requires_grad_(True)
    U = energy(case.q())
    assert bool(torch.isnan(U[1])) and bool(torch.isfinite(U[0])) and torch.equal(U[0].detach(), U[2].detach())


@pytest.mark.parametrize("F", [1, 257])
def test_sw_theta_bwd_is_the_shared_reducer_with_three_columns(F):
    """mdg_sw_frames_theta_bwd(gU, dU, F) and mdg_frames_theta_bwd(gU, dU, F, 3) give the same bits (one kernel,
    csrc/frames_reduce.hip): one frame, and 257 = one more than a workgroup's stride, so both the strided loop and the tree
    run."""
    from mdgrad_amd import _lib
    lib = _lib.load()
    gen = torch.Generator(device="cpu").manual_seed(41 + F)
    gU = torch.randn(F, generator=gen).to(DEV)
    dU = torch.randn(F, 3, generator=gen).to(DEV)
    a, b = torch.full((3,), float("nan"), device=DEV), torch.full((3,), float("nan"), device=DEV)
    _lib.check(lib.mdg_sw_frames_theta_bwd(_lib.ptr(gU), _lib.ptr(dU), F, _lib.ptr(a), _lib.stream_ptr(gU.device)),
               "mdg_sw_frames_theta_bwd")
    _lib.check(lib.mdg_frames_theta_bwd(_lib.ptr(gU), _lib.ptr(dU), F, 3, _lib.ptr(b), _lib.stream_ptr(gU.device)),
               "mdg_frames_theta_bwd")
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
