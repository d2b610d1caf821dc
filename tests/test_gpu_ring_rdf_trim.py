"""The trimmed fused RDF gradient of the ring adjoint (ring_pair RDF = 2, csrc/traj_ring.hpp: a rejected pair is sent to an
all-zero cell behind the table instead of being selected away twice, the cell fraction is v_fract_f32, the grid coordinate one
packed fma, the accumulation two packed fmas) and the LJ 12-6 polynomial with sigma folded into the launch constants.

One small launch per case: block = 64, R = 6, the 4.8 cell.  `python tests/test_gpu_ring_rdf_trim.py --measure` prints every
figure without asserting (the same script runs in the parent commit's tree: the bounds below are twice what it printed there,
the project's convention for a change at rounding level; profiles/ring_rdf_trim_ab.txt carries both builds' figures).

Frame gradient: a two-frame NVE launch, t = [0, 1e-4], the observable on both frames, the loss fed by g(r) alone with a
non-uniform weight; figure = max |adj_q0(fused) - adj_q0(separate observable launches)| / max |adj_q0(separate)| per replica,
the largest over the replicas.  The interpolation error of the derivative table (up to 2e-5 per bin) dominates it in both builds.
The observable is rdf(nbins = 10, r_range = (1.2, 2.0)): its pair cutoff 2.5 lies INSIDE the derivative grid (which reaches
2.62), so tmax = 166.4 falls inside cell 166 and the range compare cannot be a clamp; the grid starts at d = 0.578.
Replica 0 holds a pair at d = 0.55 (below the grid: t < 0), a pair at d = 2.4985 (inside the last, partial cell:
2.49706 <= d < 2.5) and pairs beyond the cutoff; N = 108 runs the FULL sweep (in-lane, ring and antipodal steps), N = 107 the
general flagged sweep, whose absent atom must land in the zero cell and add +-0, N = 4 in-lane and antipodal operations only.

Zero cell is inert: the observable rdf(nbins = 10, r_range = (0.3, 0.45)) accepts d < 0.567 only; replica 0 is the
undisturbed lattice (every pair rejected), the other replicas hold one pair at d ~ 0.5 that feeds g(r).  With the loss scaled
so that the derivative table is about 1e6, replica 0's adj_q0 is the bits of the launch whose g(r) term is multiplied by 0.

Polynomial: force, H.w, d(w.F)/dsigma and d(w.F)/deps of one evaluation against float64 (the measurement of
tests/test_gpu_ring_trim.py) at sigma = 0.9, eps = 1.3, where sigma^6 and sigma^12 are not 1."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (run as a script: this puts the repository root on sys.path)
from test_gpu_parity import T, mk_system, DEV
from test_gpu_ring_trim import _lattice, lj_reference

pytestmark = pytest.mark.gpu

F32 = np.float32
R, CELL = 6, 4.8
SHAPES = (108, 107, 4)
# the figures of the parent commit (python tests/test_gpu_ring_rdf_trim.py --measure there; profiles/ring_rdf_trim_ab.txt)
PARENT_FRAME_GRAD = {108: 1.068e-05, 107: 4.300e-05, 4: 1.308e-03}
PARENT_POLY = {"force": 3.060e-06, "hw": 2.406e-06, "dsigma": 4.773e-07, "deps": 4.958e-07}


def _mindist(p, rest):
    d = rest.astype(np.float64) - p.astype(np.float64)
    d -= CELL * np.rint(d / CELL)
    return float(np.sqrt((d * d).sum(-1)).min()) if len(rest) else 9.0


def _put_at(pos, a, b, dist, rng, keep=0.75):
    """move atom b to distance `dist` from atom a, in the direction (of 400 random ones) that keeps it farthest from the rest"""
    rest = np.delete(pos, [a, b], axis=0)
    best, best_d = None, -1.0
    for _ in range(400):
        u = rng.normal(size=3)
        c = np.mod(pos[a].astype(np.float64) + dist * u / np.linalg.norm(u), CELL).astype(F32)
        dm = _mindist(c, rest)
        if dm > best_d:
            best, best_d = c, dm
    assert best_d > keep or len(rest) == 0, "no room for atom %d at %.4f from atom %d (%.3f)" % (b, dist, a, best_d)
    pos[b] = best
    return pos


def _pair_dist(pos, a, b):
    d = pos[b].astype(np.float64) - pos[a].astype(np.float64)
    d -= CELL * np.rint(d / CELL)
    return float(np.sqrt((d * d).sum()))


def _positions(n_atoms, kind):
    """[R, N, 3].  kind "edges": replica 0 with the pairs at the edges of the derivative grid; "inert": replica 0 the plain
    lattice, every other replica with one close pair."""
    base = _lattice(n_atoms, CELL)
    rng = np.random.default_rng(100 + n_atoms)
    if n_atoms == 4 and kind == "edges":
        # four atoms per replica with every distance inside the observable's range (0.9 .. 2.4)
        pos = np.zeros((R, 4, 3), F32)
        for r in range(R):
            while True:
                c = rng.uniform(1.2, 3.6, (4, 3)).astype(F32)
                dd = [_pair_dist(c, i, j) for i in range(4) for j in range(i)]
                if min(dd) > 0.9 and max(dd) < 2.4:
                    pos[r] = c
                    break
        # replica 0: (0, 1) in-lane at 0.55, (0, 2) antipodal at 2.4985, atom 3 beyond the cutoff from all three
        p = np.zeros((4, 3), F32)
        p[0] = (1.0, 1.0, 1.0)
        p[1] = p[0] + np.array([0.55, 0.0, 0.0], F32)
        p[2] = p[0] + np.array([2.4985 / np.sqrt(2.0), 2.4985 / np.sqrt(2.0), 0.0], F32)    # (every component below half a cell)
        p[3] = (1.2, 3.3, 3.3)
        pos[0] = p
        assert min(_pair_dist(p, 3, j) for j in range(3)) > 2.6
    else:
        jitter = 0.05 if kind == "edges" else 0.02
        pos = np.mod(base[None] + rng.normal(0, jitter, (R,) + base.shape), CELL).astype(F32)
    if kind == "edges" and n_atoms != 4:
        _put_at(pos[0], 0, 1, 0.55, rng)                 # in-lane pair below the grid
        _put_at(pos[0], 40, 60, 2.4985, rng)             # ring-step pair (ten lanes apart) in the last, partial cell
    if kind == "edges":
        a, b = (0, 2) if n_atoms == 4 else (40, 60)
        assert abs(_pair_dist(pos[0], 0, 1) - 0.55) < 1e-3 and 2.4975 < _pair_dist(pos[0], a, b) < 2.4995
    if kind == "inert":
        pos[0] = base
        for r in range(1, R):
            _put_at(pos[r], 0, 1, 0.44 + 0.02 * r, rng, keep=0.75 if n_atoms != 4 else 0.0)
        dd = [_pair_dist(base, i, j) for i in range(n_atoms) for j in range(i)]
        assert min(dd) > 1.0, "replica 0: every pair is beyond the narrow observable's cutoff 0.95"
    return base, pos


def _launches(n_atoms, kind, scales):
    """len(scales) + 1 launches of a two-frame NVE trajectory: the first registers the observable (separate observable launches),
    the others are fused; loss = scale * sum (g w)^2 [+ terms on q_t, v_t for "inert"].  scale "big": whatever makes the
    derivative table about 1e6 (from the first launch's dL/dq_t).  Returns the adj_q0 of every launch."""
    from mdgrad_amd import ops, potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NVE
    from mdgrad_amd.observable import rdf
    base, pos = _positions(n_atoms, kind)
    system = mk_system(base, np.full(3, CELL), np.zeros_like(base), np.full(n_atoms, 1.008))
    mdl = P.LennardJones(1.0, 1.0)
    integ = NVE(Stack({"pair": PairPotentials(system, mdl, cutoff=2.5)}), system).to(DEV)
    integ.fuse_observables = True
    spec = integ.fused_spec("verlet")
    assert spec is not None and not spec.large
    spec.block = 64
    obs = rdf(system, nbins=10, r_range=(1.2, 2.0) if kind == "edges" else (0.3, 0.45))
    t = torch.Tensor([0.0, 1e-4]).to(DEV)
    vel = np.zeros_like(pos)
    out, big = [], 1.0
    for launch, scale in enumerate((1.0,) + tuple(scales)):
        v0, q0 = T(vel, DEV).requires_grad_(True), T(pos, DEV).requires_grad_(True)
        res = ops.fused_traj(v0, q0, None, t, spec.flat_params(), spec)
        v_t, q_t = res[0], res[1]
        assert (q_t._mdg_traj[3] is not None) == (launch > 0), "launch %d: fused observable" % launch
        gr = obs(q_t)[2]
        wgt = torch.linspace(0.5, 1.5, gr.shape[0], device=DEV)
        term = (gr * wgt).pow(2).sum()
        assert float(term) > 0, "no pair fed g(r)"
        if launch == 0 and "big" in scales:
            (gq,) = torch.autograd.grad(term, q_t, retain_graph=True)        # ~ table x distance: the table's magnitude
            big = 1e6 / float(gq.abs().max())
        loss = (big if scale == "big" else scale) * term
        if kind == "inert":
            loss = loss + q_t.pow(2).sum() / 100.0 + v_t[:, -1].pow(2).sum() / 50.0
        mdl.zero_grad()
        loss.backward()
        out.append(q0.grad.detach().cpu().numpy().copy())
    torch.cuda.synchronize()
    return out


def measure_frame_gradient(n_atoms):
    ref, fus = _launches(n_atoms, "edges", (1.0,))
    assert np.isfinite(ref).all() and np.isfinite(fus).all()
    assert all(float(np.abs(ref[r]).max()) > 0 for r in range(R))
    return max(float(np.abs(fus[r].astype(np.float64) - ref[r]).max() / np.abs(ref[r]).max()) for r in range(R))


@pytest.mark.parametrize("n_atoms", SHAPES)
def test_frame_gradient_equals_separate_launches_within_twice_the_parent(n_atoms):
    e = measure_frame_gradient(n_atoms)
    print("frame gradient N = %d: max |fused - separate| / max |separate| = %.3e (parent %.3e)" % (n_atoms, e, PARENT_FRAME_GRAD[n_atoms]))
    assert e <= 2.0 * PARENT_FRAME_GRAD[n_atoms]


@pytest.mark.parametrize("n_atoms", SHAPES)
def test_zero_cell_is_inert(n_atoms):
    _, big, zero = _launches(n_atoms, "inert", ("big", 0.0))
    assert np.isfinite(zero).all() and float(np.abs(zero[0]).max()) > 0
    # the other replicas do feel the table (how much depends on where their pair sits on dL/dd) ...
    assert float(np.abs(big[1:].astype(np.float64) - zero[1:]).max()) > 1e5, "the scaled table did not act"
    # ... replica 0, whose every pair is rejected, not at all: the same bits
    assert np.array_equal(big[0].view(np.uint32), zero[0].view(np.uint32)), "max |diff| %.3e" % float(
        np.abs(big[0].astype(np.float64) - zero[0]).max())


# ------------------------------------------------------------------------------------------------ polynomial, sigma != 1
def measure_polynomial(sigma=0.9, eps=1.3):
    """{force, hw, dsigma, deps}: max |gpu - float64| / max |float64| of one evaluation, N = 108, R = 6 (the measurement of
    tests/test_gpu_ring_trim.py::measure_one_evaluation with sigma, eps not 1, the two parameter entries apart)"""
    from mdgrad_amd import _lib, potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NVE
    lib = _lib.load()
    n_atoms = 108
    base = _lattice(n_atoms, CELL)
    system = mk_system(base, np.full(3, CELL), np.zeros_like(base), np.full(n_atoms, 1.008))
    mdl = P.LennardJones(sigma, eps)
    integ = NVE(Stack({"pair": PairPotentials(system, mdl, cutoff=2.5)}), system).to(DEV)
    spec = integ.fused_spec("verlet")
    assert spec is not None and not spec.large
    spec.block = 64
    prm = spec.params(R, 2)
    cs, terms = spec.cell_struct, spec.terms
    assert lib.mdg_traj_ring_taken(C.byref(prm), C.byref(cs), C.byref(terms)), "the wave-per-replica kernels must run"
    rng = np.random.default_rng(7)
    pos = np.mod(base[None] + rng.normal(0, 0.05, (R,) + base.shape), CELL).astype(F32)
    v0, q0 = torch.zeros(R, n_atoms, 3, device=DEV), T(pos, DEV).contiguous()
    theta = spec.flat_params().detach().contiguous()
    Pr, ptr, st = C.byref, _lib.ptr, _lib.stream_ptr(DEV)
    shape = (R, 2, n_atoms, 3)
    v_t, q_t, f_t = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV), torch.zeros(shape, device=DEV)
    bad = torch.zeros(R, dtype=torch.int32, device=DEV)
    t_fwd = torch.Tensor([0.0, 0.004]).to(DEV)
    _lib.check(lib.mdg_traj_fwd_small_ft(Pr(prm), Pr(cs), Pr(terms), ptr(theta), ptr(spec.mass), ptr(t_fwd), ptr(v0), ptr(q0), None,
                                         ptr(v_t), ptr(q_t), None, ptr(f_t), ptr(bad), st), "fwd_ft")
    torch.cuda.synchronize()
    assert int(bad.abs().sum()) == 0
    w = torch.randn(R, n_atoms, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    g_v = torch.zeros(shape, device=DEV)
    g_v[:, 1] = w
    g_q = torch.zeros(shape, device=DEV)
    t_adj = torch.Tensor([0.0, 1.0]).to(DEV)
    adj_v0, adj_q0 = torch.empty(R, n_atoms, 3, device=DEV), torch.empty(R, n_atoms, 3, device=DEV)
    adj_th = torch.zeros(R, spec.n_theta_total, device=DEV)
    _lib.check(lib.mdg_traj_adj_small_ft(Pr(prm), Pr(cs), Pr(terms), ptr(theta), ptr(spec.mass), ptr(t_adj), ptr(v_t), ptr(q_t), None,
                                         ptr(f_t), ptr(g_v), ptr(g_q), None, ptr(adj_v0), ptr(adj_q0), None, ptr(adj_th), st),
               "adj_ft")
    torch.cuda.synchronize()
    x1 = q_t[:, 1].cpu().numpy()
    s = x1 / CELL
    assert s.min() > -0.2 and s.max() < 1.2                                   # (the window form of the image ran)
    wn = w.cpu().numpy()
    gpu_f = f_t[:, 1].cpu().numpy().astype(np.float64)
    gpu_dq = 2.0 * (adj_v0.cpu().numpy().astype(np.float64) - wn.astype(np.float64))
    gpu_th = adj_th.cpu().numpy().astype(np.float64)
    sg, ep = float(F32(sigma)), float(F32(eps))
    refs = [lj_reference(x1[r], wn[r], float(F32(CELL)), sigma=sg, eps=ep) for r in range(R)]
    err = {"force": max(float(np.abs(gpu_f[r] - refs[r][0]).max() / np.abs(refs[r][0]).max()) for r in range(R)),
           "hw": max(float(np.abs(gpu_dq[r] - refs[r][1]).max() / np.abs(refs[r][1]).max()) for r in range(R))}
    th = np.stack([ref[2] for ref in refs])
    for k, nm in ((0, "dsigma"), (1, "deps")):
        err[nm] = float(np.abs(gpu_th[:, k] - th[:, k]).max() / np.abs(th[:, k]).max())
    return err


def test_polynomial_with_sigma_folded_matches_float64_within_twice_the_parent():
    err = measure_polynomial()
    print("one evaluation, sigma 0.9, eps 1.3, max |gpu - float64| / max |float64|: " +
          "  ".join("%s %.3e" % kv for kv in sorted(err.items())))
    for nm, e in err.items():
        assert e <= 2.0 * PARENT_POLY[nm], "%s: %.3e against twice the parent's %.3e" % (nm, e, PARENT_POLY[nm])


if __name__ == "__main__":
    assert sys.argv[1:] == ["--measure"], "usage: python tests/test_gpu_ring_rdf_trim.py --measure"
    for n in SHAPES:
        print("frame gradient N = %d: max |fused - separate| / max |separate| = %.3e" % (n, measure_frame_gradient(n)), flush=True)
    print("one evaluation, sigma 0.9, eps 1.3, max |gpu - float64| / max |float64|: " +
          "  ".join("%s %.3e" % kv for kv in sorted(measure_polynomial().items())), flush=True)
    for n in SHAPES:
        _, big, zero = _launches(n, "inert", ("big", 0.0))
        print("zero cell N = %d: replica 0 bitwise %s, max |big - zero| over the other replicas %.3e" % (
            n, np.array_equal(big[0].view(np.uint32), zero[0].view(np.uint32)),
            float(np.abs(big[1:].astype(np.float64) - zero[1:]).max())), flush=True)
