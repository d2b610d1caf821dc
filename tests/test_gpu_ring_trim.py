"""The three-instruction minimum image of the full-ring sweep (min_image_diag2_near_fused, csrc/traj_ring.hpp: the multiply folded
into the rounding add, with the multiplier of mdg_min_image_fused_inv) against the four-instruction form of the same build
(MDG_RING_LEAN=0 keeps it everywhere), and the shared-power form of the LJ 12-6 polynomial (ring_pair, csrc/traj_ring.hpp)
against a float64 evaluation of the same formulas.

Bitwise part, in the pattern of test_gpu_ring_lean.py: one child process per setting (this file, run as a script, is the
worker), forward + adjoint through ops.fused_traj with block = 64, R = 6, 6 frames, NHC and NVE, with and without the fused RDF;
v_t, q_t, pv_t, the per-frame forces, g(r), the costates and the parameter gradient are the same bits.  The shapes:

  n4-* / n108-*   the 4.8 cell, whose multiplier is the float BELOW inv.  In replica 0 (1, 2) the x (y, z) separation of a few
                  pairs is exactly s = pred(tau), tau or succ(tau), tau = the smallest float whose rounded product with inv
                  exceeds 0.5 -- the only floats at which the two forms could pick different images -- and the other two
                  components are 0.3 and 0.2 at most, so the pair is inside the cutoff whichever image is taken and the other
                  image flips a force component.  Both signs occur: N = 4 and the in-lane and antipodal pairs of N = 108 are
                  evaluated from both ends, and the two ring-step pairs of N = 108 are laid out with opposite orientations.
  h64             N = 108 in a 6.4 cell: no multiplier, the launch must fall back to the flagged window sweep (equal trivially)
  h52             N = 108 in a 5.2 cell: inv itself is the multiplier

The time step is small (2e-4): the displaced atoms sit closer to their neighbours than a lattice site does, and the replicas
must stay inside the window of the fast image for all six frames.

Accuracy part: force (the forward's LEVEL 1 sweep), H.w and the two parameter-gradient entries (the adjoint's LEVEL 3 sweep
with sums) of ONE evaluation, N = 108, R = 6, read through a two-frame NVE launch: f_t[:, 1] is F(q_1); with the costate
g_v[:, 1] = w, nothing else incoming and an interval h = 1 the adjoint returns adj_v0 = w + dq / 2 (sovlers.py:71-72) and
adj_theta = d(w.F)/dtheta of that single evaluation.  Figures: max |gpu - float64| / max |float64| over the six replicas.
The same measurement on the parent commit (separately rounded s12 and 1/d2^2) gave PARENT_ERR; both are rounding noise of a
different association, so the bound is twice the parent's figure."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (the worker runs as a script: this puts the repository root on sys.path)
from test_gpu_parity import T, mk_system, DEV

pytestmark = pytest.mark.gpu

F32 = np.float32
R, NT, DT = 6, 6, 0.0002
SHAPES = [("n4-pred", 4, 4.8), ("n4-tau", 4, 4.8), ("n4-succ", 4, 4.8), ("n108-pred", 108, 4.8), ("n108-tau", 108, 4.8),
          ("n108-succ", 108, 4.8), ("h64", 108, 6.4), ("h52", 108, 5.2)]
CASES = [(s, ens, rdf) for s, _, _ in SHAPES for ens in ("nhc", "nve") for rdf in (False, True)]
NAMES = ("v_t", "q_t", "pv_t", "f_t", "g", "adj_v0", "adj_q0", "adj_pv0", "adj_theta")
# max |gpu - float64| / max |float64| of one evaluation on the parent commit (profiles/ring_trim_ab.txt)
PARENT_ERR = {"force": 2.860e-06, "hw": 2.299e-06, "theta": 3.946e-06}


def _key(shape, ens, rdf):
    return "%s-%s-%s" % (shape, ens, "rdf" if rdf else "plain")


def _lattice(n_atoms, cell):
    """the first n_atoms sites of a 3 x 3 x 3 fcc box (the headline's lattice at cell = 4.8); N = 4: one unit cell's basis"""
    a = cell / 3.0
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    if n_atoms == 4:
        return ((basis + 0.25) * (cell / 2.0)).astype(F32)
    c = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    return (((c + basis[None]).reshape(-1, 3) + 0.25) * a)[:n_atoms].astype(F32)


def _tau(h, inv):
    """smallest float d > 0 with fl(d inv) > 0.5 (as tests/test_fused_image_multiplier.py)"""
    t = F32(0.5) * F32(h)
    while F32(np.nextafter(t, F32(0)) * inv) > F32(0.5):
        t = np.nextafter(t, F32(0))
    while not F32(t * inv) > F32(0.5):
        t = np.nextafter(t, F32(np.inf))
    return F32(t)


def _adversarial_pairs(n_atoms, base, axis):
    """Atom pairs (a, b), a = anchor, b = moved: x_b - x_a is set to +s along `axis`.  The anchors have a lattice coordinate
    below 1.5 there, so that anchor + s stays below 4 and is exact in float32.  N = 4: every pair is in-lane or antipodal and
    evaluated from both ends: both signs.  N = 108 (nl = 54 lanes, lane l meets lane l - k at ring step k <= 27): an in-lane
    pair (b = a + 1) and an antipodal one (b = a + 54, 27 lanes apart) -- both ends, both signs; b = a + 60 (30 lanes apart:
    lane(a) evaluates it with lane(b) visiting, D = x_b - x_a = +s) and b = a + 20 (10 lanes apart: lane(b) evaluates it with
    lane(a) visiting, D = x_a - x_b = -s)."""
    low = [a for a in range(n_atoms) if base[a, axis] < 1.5]
    if n_atoms == 4:
        assert len(low) == 2
        return list(zip(low, [a for a in range(4) if a not in low]))
    pairs, used = [], set()
    for step in (1, 54, 60, 20):
        a = next(a for a in low if a % 2 == 0 and a + step < n_atoms and not {a, a + step} & used)
        pairs.append((a, a + step))
        used |= {a, a + step}
    return pairs


def _place(pos, rep, axis, s, pairs, cell):
    """replica `rep`: for every pair move the second atom to (first atom) + s along `axis`, + (0.3, 0.2) at most along the others"""
    others = [k for k in range(3) if k != axis]
    for a, b in pairs:
        p = pos[rep, a].copy()
        p[axis] = F32(np.clip(np.round(float(p[axis]) * 2 ** 18) / 2 ** 18, 0.25, 1.55))    # (x + s is then exact in float32)
        pos[rep, a] = p
        best, best_d = None, -1.0
        for sa in (0.3, -0.3):
            for sb in (0.2, -0.2):
                c = p.copy()
                c[axis] = F32(p[axis] + s)
                c[others[0]] = F32(np.mod(p[others[0]] + sa, cell))
                c[others[1]] = F32(np.mod(p[others[1]] + sb, cell))
                rest = np.delete(pos[rep], [a, b], axis=0).astype(np.float64)
                d = rest - c.astype(np.float64)
                d -= cell * np.rint(d / cell)
                dmin = float(np.sqrt((d * d).sum(-1)).min()) if len(rest) else 9.0
                if dmin > best_d:
                    best, best_d = c, dmin
        pos[rep, b] = best
        assert F32(pos[rep, b, axis] - pos[rep, a, axis]) == s and float(pos[rep, b, axis]) - float(pos[rep, a, axis]) == float(s)
    return pos


def _system(shape, n_atoms, cell_len, h, inv):
    base = _lattice(n_atoms, cell_len)
    rng = np.random.default_rng(n_atoms + len(shape))
    pos = np.mod(base[None] + rng.normal(0, 0.02, (R,) + base.shape), cell_len).astype(F32)
    vel = rng.normal(0, 0.5, pos.shape).astype(F32)
    pairs = []
    if "-" in shape:
        tau = _tau(h, inv)
        s = {"pred": np.nextafter(tau, F32(0)), "tau": tau, "succ": np.nextafter(tau, F32(np.inf))}[shape.split("-")[1]]
        pairs = [_adversarial_pairs(n_atoms, base, axis) for axis in range(3)]
        for axis in range(3):
            _place(pos, axis, axis, F32(s), pairs[axis], cell_len)
        # the adversarial pairs are inside the cutoff at frame 0, whichever image is taken
        for axis in range(3):
            for a, b in pairs[axis]:
                d = pos[axis, b].astype(np.float64) - pos[axis, a].astype(np.float64)
                assert abs(d[axis]) == float(s)
                d -= float(h) * np.rint(d / float(h))
                assert 2.3 < abs(d[axis]) < 2.41 and float((d * d).sum()) < 2.5 ** 2 - 0.3, (shape, axis, a, b, d)
    return base, pos, vel


def _integrator(base, cell_len, vel0, nhc):
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NVE, NoseHooverChain
    system = mk_system(base, np.full(3, cell_len), vel0, np.full(len(base), 1.008))
    mdl = P.LennardJones(1.0, 1.0)
    stack = Stack({"pair": PairPotentials(system, mdl, cutoff=2.5)})
    integ = (NoseHooverChain(stack, system, T=1.0, num_chains=5, Q=50.0) if nhc else NVE(stack, system)).to(DEV)
    return system, mdl, integ


def _run_case(shape, n_atoms, cell_len, ens, rdf):
    from mdgrad_amd import _lib, ops
    from mdgrad_amd.observable import rdf as rdf_obs
    nhc = ens == "nhc"
    base = _lattice(n_atoms, cell_len)
    system, mdl, integ = _integrator(base, cell_len, np.zeros_like(base), nhc)
    integ.fuse_observables = rdf
    spec = integ.fused_spec("NH_verlet" if nhc else "verlet")
    assert spec is not None and not spec.large
    spec.block = 64
    cs = spec.cell_struct
    h, inv = F32(cs.h[0]), F32(cs.inv[0])
    assert h == F32(cell_len) and cs.h[4] == cs.h[0] == cs.h[8] and cs.inv[4] == cs.inv[0] == cs.inv[8]
    # the multiplier the launch will find: the float below inv at 4.8, inv itself at 5.2, none at 6.4
    out = C.c_float(0.0)
    ok = _lib.load().mdg_min_image_fused_inv(C.c_float(float(h)), C.c_float(float(inv)), C.byref(out))
    want = {4.8: np.nextafter(inv, F32(0)), 5.2: inv, 6.4: None}[cell_len]
    assert (F32(out.value) if ok else None) == want, (cell_len, ok, out.value)
    # ... and the sweep the launches of this process take (the code they decide with): the full ring with the fused image in
    # the lean child wherever a multiplier exists, the flagged window sweep at 6.4 and everywhere in the MDG_RING_LEAN=0 child
    prm = spec.params(R, NT)
    fused = bool(_lib.load().mdg_traj_ring_fused_image(C.byref(prm), C.byref(cs), C.byref(spec.terms)))
    assert fused == (os.environ.get("MDG_RING_LEAN") != "0" and want is not None), (shape, fused)
    base, pos, vel = _system(shape, n_atoms, cell_len, h, inv)
    t = torch.Tensor([DT * i for i in range(NT)]).to(DEV)
    obs = rdf_obs(system, nbins=100, r_range=(0.75, 2.5))
    params = list(mdl.parameters())
    res_np = {}
    for launch in range(2 if rdf else 1):                # (the first launch registers the observable, the second one fuses it)
        v0, q0 = T(vel, DEV).requires_grad_(True), T(pos, DEV).requires_grad_(True)
        pv0 = torch.zeros(R, 5, device=DEV, requires_grad=True) if nhc else None
        res = ops.fused_traj(v0, q0, pv0, t, spec.flat_params(), spec)
        v_t, q_t = res[0], res[1]
        assert (q_t._mdg_traj[3] is not None) == (rdf and launch == 1), "fused observable: launch %d" % launch
        f_t = getattr(v_t.grad_fn, "f_t", None)
        assert f_t is not None, "the wave-per-replica kernels keep the per-frame forces"
        gr = obs(q_t)[2]
        wgt = torch.linspace(0.5, 1.5, gr.shape[0], device=DEV)
        loss = (gr * wgt).pow(2).sum() + q_t[:, ::2].pow(2).sum() / 100.0 + v_t[:, -1].pow(2).sum() / 50.0
        if nhc:
            loss = loss + res[2][:, -1].sum()
        for p in params:
            p.grad = None
        f_keep = f_t[:, 1:].detach().clone()
        loss.backward()
        res_np = {"v_t": v_t, "q_t": q_t, "pv_t": res[2] if nhc else None, "f_t": f_keep, "g": gr, "adj_v0": v0.grad,
                  "adj_q0": q0.grad, "adj_pv0": pv0.grad if nhc else None,
                  "adj_theta": torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params])}
    torch.cuda.synchronize()
    res_np = {k: v.detach().cpu().numpy() for k, v in res_np.items() if v is not None}
    # every replica stayed inside the window of the fast image ([-0.24, 1.24] cell lengths): the sweeps under test ran
    s = res_np["q_t"] / float(h)
    assert s.min() > -0.2 and s.max() < 1.2, "%s: a replica left the window (%.3f .. %.3f)" % (shape, s.min(), s.max())
    return res_np


def _worker(path):
    res = {}
    for (shape, ens, rdf) in CASES:
        n_atoms, cell_len = next((n, c) for s, n, c in SHAPES if s == shape)
        for k, v in _run_case(shape, n_atoms, cell_len, ens, rdf).items():
            res[_key(shape, ens, rdf) + "/" + k] = v
    np.savez(path, **res)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """{setting: arrays}: one child process per setting of MDG_RING_LEAN, started together"""
    d = tmp_path_factory.mktemp("ring_trim")
    procs = {}
    for name, val in (("lean", None), ("general", "0")):
        env = dict(os.environ)
        env.pop("MDG_RING_LEAN", None)
        if val is not None:
            env["MDG_RING_LEAN"] = val
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), str(d / (name + ".npz"))], env=env,
                                       cwd=os.path.dirname(os.path.abspath(__file__)), stdout=subprocess.PIPE,
                                       stderr=subprocess.STDOUT, text=True)
    out = {}
    for name, p in procs.items():
        log, _ = p.communicate()
        assert p.returncode == 0, "worker (%s) failed:\n%s" % (name, log[-4000:])
        out[name] = dict(np.load(str(d / (name + ".npz")), allow_pickle=False))
    return out


@pytest.mark.parametrize("shape,ens,rdf", CASES, ids=[_key(*c) for c in CASES])
def test_fused_image_is_bitwise_the_four_instruction_one(both, shape, ens, rdf):
    key = _key(shape, ens, rdf)
    seen = 0
    for nm in NAMES:
        a, b = both["lean"].get(key + "/" + nm), both["general"].get(key + "/" + nm)
        assert (a is None) == (b is None), nm
        if a is None:
            assert nm in ("pv_t", "adj_pv0") and ens == "nve", nm
            continue
        seen += 1
        assert np.isfinite(b).all(), "%s %s: the four-instruction form's output is not finite" % (key, nm)
        assert torch.equal(torch.from_numpy(a), torch.from_numpy(b)), "%s %s: max |diff| %.3e" % (
            key, nm, float(np.abs(a.astype(np.float64) - b).max()))
    assert seen == (9 if ens == "nhc" else 7)
    assert float(np.abs(both["lean"][key + "/adj_q0"]).max()) > 0 and float(np.abs(both["lean"][key + "/adj_theta"]).max()) > 0


# ------------------------------------------------------------------------------------------------ accuracy of the polynomial
def lj_reference(x, w, cell_len, sigma=1.0, eps=1.0, rc=2.5):
    """float64, all pairs, the formulas of ring_pair / ring_theta: force F_i = sum_j c1 D (D = x_j - x_i, minimum image),
    dq = d(w.F)/dq = -sum_j [kk (w_ij.D) D + c1 w_ij] (w_ij = w_i - w_j), and d(w.F)/d(sigma, eps) from the sums over directed
    pairs T6 = sum s6 (w_ij.D)/d2, T12 = sum s12 (w_ij.D)/d2."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    D = x[None, :, :] - x[:, None, :]
    D -= cell_len * np.rint(D / cell_len)
    d2 = (D * D).sum(-1)
    ok = (d2 < rc * rc) & (d2 > 0)
    i2 = np.where(ok, 1.0 / np.where(ok, d2, 1.0), 0.0)
    s6 = (sigma * sigma * i2) ** 3
    s12 = s6 * s6
    e4 = 4.0 * eps
    c1 = e4 * (6.0 * s6 - 12.0 * s12) * i2                       # phi'/r
    kk = e4 * (168.0 * s12 - 48.0 * s6) * i2 * i2                # (phi'' - phi'/r)/r^2
    wij = w[:, None, :] - w[None, :, :]
    b = (wij * D).sum(-1)
    force = (c1[..., None] * D).sum(1)
    dq = -((kk * b)[..., None] * D + c1[..., None] * wij).sum(1)
    t6, t12 = (s6 * i2 * b).sum(), (s12 * i2 * b).sum()
    theta = np.array([(18.0 * e4 / sigma) * t6 - (72.0 * e4 / sigma) * t12, 12.0 * t6 - 24.0 * t12])
    return force, dq, theta


def measure_one_evaluation():
    """{force, hw, theta}: max |gpu - float64| / max |float64| of one evaluation, N = 108, R = 6, the 4.8 cell"""
    from mdgrad_amd import _lib
    lib = _lib.load()
    n_atoms, cell_len = 108, 4.8
    base = _lattice(n_atoms, cell_len)
    system, mdl, integ = _integrator(base, cell_len, np.zeros_like(base), False)
    spec = integ.fused_spec("verlet")
    assert spec is not None and not spec.large
    spec.block = 64
    prm = spec.params(R, 2)
    cs, terms = spec.cell_struct, spec.terms
    assert lib.mdg_traj_ring_taken(C.byref(prm), C.byref(cs), C.byref(terms)), "the wave-per-replica kernels must run"
    rng = np.random.default_rng(7)
    pos = np.mod(base[None] + rng.normal(0, 0.05, (R,) + base.shape), cell_len).astype(F32)
    v0, q0 = torch.zeros(R, n_atoms, 3, device=DEV), T(pos, DEV).contiguous()
    theta = spec.flat_params().detach().contiguous()
    P, ptr, st = C.byref, _lib.ptr, _lib.stream_ptr(DEV)
    shape = (R, 2, n_atoms, 3)
    v_t, q_t, f_t = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV), torch.zeros(shape, device=DEV)
    bad = torch.zeros(R, dtype=torch.int32, device=DEV)
    t_fwd = torch.Tensor([0.0, 0.004]).to(DEV)
    _lib.check(lib.mdg_traj_fwd_small_ft(P(prm), P(cs), P(terms), ptr(theta), ptr(spec.mass), ptr(t_fwd), ptr(v0), ptr(q0), None,
                                         ptr(v_t), ptr(q_t), None, ptr(f_t), ptr(bad), st), "fwd_ft")
    torch.cuda.synchronize()
    assert int(bad.abs().sum()) == 0
    # the adjoint of ONE interval of length 1 from frame 1: costate w on the velocities, nothing else incoming
    w = torch.randn(R, n_atoms, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    g_v = torch.zeros(shape, device=DEV)
    g_v[:, 1] = w
    g_q = torch.zeros(shape, device=DEV)
    t_adj = torch.Tensor([0.0, 1.0]).to(DEV)
    adj_v0, adj_q0 = torch.empty(R, n_atoms, 3, device=DEV), torch.empty(R, n_atoms, 3, device=DEV)
    adj_th = torch.zeros(R, spec.n_theta_total, device=DEV)
    _lib.check(lib.mdg_traj_adj_small_ft(P(prm), P(cs), P(terms), ptr(theta), ptr(spec.mass), ptr(t_adj), ptr(v_t), ptr(q_t), None,
                                         ptr(f_t), ptr(g_v), ptr(g_q), None, ptr(adj_v0), ptr(adj_q0), None, ptr(adj_th), st),
               "adj_ft")
    torch.cuda.synchronize()
    x1 = q_t[:, 1].cpu().numpy()
    s = x1 / cell_len
    assert s.min() > -0.2 and s.max() < 1.2                                   # (the window form of the image ran)
    wn = w.cpu().numpy()
    gpu_f = f_t[:, 1].cpu().numpy().astype(np.float64)
    gpu_dq = 2.0 * (adj_v0.cpu().numpy().astype(np.float64) - wn.astype(np.float64))
    gpu_th = adj_th.cpu().numpy().astype(np.float64)
    err = {"force": 0.0, "hw": 0.0, "theta": 0.0}
    for r in range(R):
        f, dq, th = lj_reference(x1[r], wn[r], float(F32(cell_len)))
        for nm, a, b in (("force", gpu_f[r], f), ("hw", gpu_dq[r], dq), ("theta", gpu_th[r], th)):
            err[nm] = max(err[nm], float(np.abs(a - b).max() / np.abs(b).max()))
    return err


def test_polynomial_matches_float64_within_twice_the_parent():
    err = measure_one_evaluation()
    print("one evaluation, max |gpu - float64| / max |float64|: " + "  ".join("%s %.3e" % kv for kv in sorted(err.items())))
    for nm, e in err.items():
        assert e <= 2.0 * PARENT_ERR[nm], "%s: %.3e against twice the parent's %.3e" % (nm, e, PARENT_ERR[nm])


if __name__ == "__main__":
    if sys.argv[1] == "--measure":
        print("one evaluation, max |gpu - float64| / max |float64|: " +
              "  ".join("%s %.3e" % kv for kv in sorted(measure_one_evaluation().items())))
    else:
        _worker(sys.argv[1])
