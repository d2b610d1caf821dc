"""Structure factor observable on the GPU (csrc/sk.hip, ops.SkFn, observable.structure_factor) against the float64 definition
(tests/sk_ref.py: torch float64 on the CPU from the same float32 positions and cell lengths, k in float64) and the fixtures
sk_s1 .. sk_s3 (tests/golden/make_sk_goldens.py).

Error measure per (frame, bin):   e = |S - S64| / (sqrt(N_eff S64) + 1),   N_eff = (sum w)^2 / sum w^2
(a per-atom phase error eps moves |rho|^2 by at most 2 |rho| N eps, so e is an eps-scale at peaks and in troughs alike).

Tolerances, with what the MI355X showed (every comparison prints its figure before it asserts):
  forward    e <= TOL = 10 x OBSERVED_FWD; OBSERVED_FWD = the largest e over the fixture cases sk_s1 / sk_s2
             = 8.1e-8 (sk_s1 8.1e-8, sk_s2 5.2e-8); TOL must stay <= 1e-5.  The other cases: shape boundaries 5e-9 .. 1.0e-7
             (the largest at 200 atoms and a single vector), atoms at +7 L / -3 L 3.9e-8, perfect lattice 2e-11, S3 1.1e-7
  dS/dq      against float64 autograd: rtol 1e-4, atol = A x max|g64| with A = 10 x OBSERVED_GRAD, OBSERVED_GRAD = the largest
             |g - g64| / max|g64| over the fixtures = 4.8e-7 (sk_s1 4.7e-7, sk_s2 2.0e-7); A must stay <= 1e-5.  Shape boundaries
             1.3e-7 .. 7.7e-7 (the largest on the tiled route, 1025 atoms), atoms at +7 L / -3 L 4.2e-7; the per-frame sum of
             dS/dx over the atoms 1.7e-6 of the largest entry (bound 1e-5)
  S3         dL/dsigma, dL/depsilon: rtol 2e-3, atol 1e-4 |dL/dsigma| (test_fused_traj_and_adjoint_golden, as P3);
             S_t: TOL plus the trajectory's own float32 divergence, taken as the largest per-bin |S64(q_kernel) - S64(q_golden)|
             of the last frame (1.1e-7); observed dL/dsigma off by 7.6e-6 of 0.12 allowed, dL/depsilon 7.2e-7 of 0.013
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from sk_ref import err_measure, n_eff, sk64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBSERVED_FWD = 8.1e-8     # largest e over sk_s1 / sk_s2 (MI355X)
OBSERVED_GRAD = 4.8e-7    # largest |g - g64| / max|g64| over sk_s1 / sk_s2 (MI355X)
TOL = 10 * OBSERVED_FWD
A_TOL = 10 * OBSERVED_GRAD
assert TOL <= 1e-5 and A_TOL <= 1e-5


def figure(what, observed, allowed):
    print("FIGURE %-64s observed %.3e  allowed %.3e" % (what, observed, allowed))


def fwd_close(S, S64, neff, what, extra=0.0):
    S = S.detach().cpu().double().numpy() if torch.is_tensor(S) else np.asarray(S, dtype=np.float64)
    assert S.shape == np.shape(S64), "%s: shape %s vs %s" % (what, S.shape, np.shape(S64))
    e = err_measure(S, S64, neff)
    figure(what + " e", e.max(), TOL)
    assert np.isfinite(S).all(), what + ": non-finite"
    assert (np.abs(S - S64) <= TOL * (np.sqrt(neff * np.abs(S64)) + 1.0) + extra).all(), "%s: e = %.3e, TOL %.1e" % (what, e.max(), TOL)


def grad_close(g, g64, what):
    g = g.detach().cpu().double().numpy()
    top = float(np.abs(g64).max())
    err, tol = np.abs(g - g64), A_TOL * top + 1e-4 * np.abs(g64)
    figure(what + " |g - g64| / max|g64|", err.max() / max(top, 1e-300), A_TOL)
    assert np.isfinite(g).all(), what + ": non-finite"
    assert (err <= tol).all(), "%s: gradient off by %.3e of its largest entry" % (what, err.max() / top)


def close(a, b, rtol, atol, what):
    a, b = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err, tol = np.abs(a - b), atol + rtol * np.abs(b)
    k = np.argmax(err - tol)
    figure(what, err.flat[k], tol.flat[k])
    assert (err <= tol).all(), "%s: err %.3e, allowed %.3e" % (what, err.flat[k], tol.flat[k])


def mk_system(pos, cell, vel=None, mass=None, n_rep=0):
    from mdgrad_amd.system import System
    s = System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
               masses=(np.asarray(mass, dtype=np.float64) if mass is not None else np.full(len(pos), 1.008)), device=DEV)
    if vel is not None:
        s.set_velocities(np.asarray(vel, dtype=np.float64))
    return s.replicate(n_rep) if n_rep else s


def run_obs(obs, xyz, gS):
    """(S_f, d sum(gS * S_f) / dq) through the kernels."""
    q = torch.as_tensor(np.asarray(xyz, dtype=np.float32)).to(DEV).requires_grad_(True)
    S = obs.per_frame(q)
    (g,) = torch.autograd.grad((S * torch.as_tensor(np.asarray(gS, dtype=np.float32)).to(DEV)).sum(), q)
    return S.detach(), g


def run_raw(xyz, cell, n, seg, gS, weights=None):
    """The same through ops.SkFn with a vector table of the test's own."""
    from mdgrad_amd import _lib, ops
    q = torch.as_tensor(np.asarray(xyz, dtype=np.float32)).to(DEV).requires_grad_(True)
    w = None if weights is None else torch.as_tensor(np.asarray(weights, dtype=np.float32)).to(DEV)
    norm = float(q.shape[1]) if weights is None else float((np.asarray(weights, dtype=np.float64) ** 2).sum())
    S = ops.SkFn.apply(q, _lib.make_cell(torch.as_tensor(np.asarray(cell, dtype=np.float32))), w, norm,
                       torch.as_tensor(np.asarray(n), dtype=torch.int32).to(DEV), torch.as_tensor(np.asarray(seg), dtype=torch.int32).to(DEV))
    (g,) = torch.autograd.grad((S * torch.as_tensor(np.asarray(gS, dtype=np.float32)).to(DEV)).sum(), q)
    return S.detach(), g


def fixture_obs(name):
    from mdgrad_amd.observable import structure_factor
    g = load_golden(name)
    w = g["weights"] if "weights" in g else None
    obs = structure_factor(mk_system(g["xyz"][0], g["cell"]), int(g["nbins"]), tuple(g["k_range"]), weights=w,
                           max_per_bin=int(g["max_per_bin"]) or None)
    return g, w, obs


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["sk_s1", "sk_s2"])
def test_fixtures(name):
    g, w, obs = fixture_obs(name)
    assert np.array_equal(obs.n_vectors.numpy(), g["n_vectors"])
    S, gq = run_obs(obs, g["xyz"], g["gS"])
    assert S.shape == (3, 30)
    fwd_close(S, g["S64"], n_eff(w, 108), name)
    grad_close(gq, g["dS_dq"], name)
    k, Sm = obs(torch.as_tensor(g["xyz"]).to(DEV))
    assert k.shape == (30,) and Sm.shape == (30,) and torch.equal(Sm, S.mean(0))
    fwd_close(Sm, g["S64"].mean(0), n_eff(w, 108), name + " forward() vs the frame mean")


# ---------------------------------------------------------------------------------------------- 2
def test_perfect_lattice():
    """One vector per bin: the 32 Bragg vectors below k = 16 of the 3 x 3 x 3 FCC lattice (S = 108) and every fourth of the
    others (S = 0)."""
    from mdgrad_amd.observable import sk_vectors
    from test_sk_host import fcc
    pos, cell = fcc()
    n, _, _, _ = sk_vectors(cell, 30, (1.0, 16.0))
    hkl = n // 3
    bragg = (n % 3 == 0).all(1) & ((hkl % 2 == 0).all(1) | (hkl % 2 == 1).all(1))
    pick = np.sort(np.concatenate([np.nonzero(bragg)[0], np.nonzero(~bragg)[0][::4]]))
    n, bragg = n[pick], bragg[pick]
    assert bragg.sum() == 32 and len(n) <= 1024
    S, _ = run_raw(pos[None], cell, n, np.arange(len(n) + 1), np.ones((1, len(n))))
    fwd_close(S, np.where(bragg, 108.0, 0.0)[None], 108.0, "perfect lattice")


# ---------------------------------------------------------------------------------------------- 3
# wave per frame up to 128 atoms (chunks of 64 vectors, 4 frames per workgroup), workgroup per frame up to 1024 (chunks of
# 256), beyond that atom blocks of 1024 x chunks of 256: both sides of every limit, ragged last blocks and chunks
SHAPES = ([(n, 65, 5) for n in (1, 2, 3, 63, 64, 65, 108, 127, 128)] + [(108, 1, 1), (108, 63, 4), (108, 64, 4)] +
          [(129, 257, 2), (200, 1, 1), (200, 63, 1), (200, 64, 1), (200, 65, 5), (1023, 255, 1), (1024, 256, 1)] +
          [(1025, 257, 2), (1026, 1, 1), (1500, 65, 1), (1500, 255, 1), (2049, 256, 1)])


@pytest.mark.parametrize("n_atoms,n_vecs,frames", SHAPES)
def test_shape_boundaries(n_atoms, n_vecs, frames):
    from mdgrad_amd.observable import sk_vectors
    rng = np.random.default_rng(1000 * n_atoms + n_vecs)
    L = (n_atoms / 0.845) ** (1 / 3)
    cell = np.array([L, L, L], dtype=np.float32)
    xyz = rng.uniform(0, L, (frames, n_atoms, 3)).astype(np.float32)
    n, _, _, _ = sk_vectors(cell.astype(np.float64), 8, (0.5 * 2 * np.pi / L, 12 * 2 * np.pi / L))
    n = n[:n_vecs]
    assert len(n) == n_vecs
    seg = np.array([0, n_vecs // 3, n_vecs // 3, (2 * n_vecs) // 3, n_vecs])          # (bin 1 is always empty)
    gS = rng.uniform(-1, 1, (frames, 4)).astype(np.float32)
    S, g = run_raw(xyz, cell, n, seg, gS)
    S64, Sk64, g64 = sk64(xyz, cell, n, seg, None, gS)
    what = "N=%d M=%d F=%d" % (n_atoms, n_vecs, frames)
    fwd_close(S, S64, float(n_atoms), what)
    assert (S[:, np.diff(seg) == 0] == 0).all()
    if n_atoms == 1:
        assert np.allclose(Sk64, 1.0, rtol=0, atol=1e-12)
        # S = 1 whatever x: the gradient is rounding alone, measured against the size of its two cancelling halves
        size = 2 * np.abs(gS).sum(1).max() * (2 * np.pi * np.sqrt((n * n).sum(1)).max() / L)
        figure(what + " |g| / size of the cancelling halves", float(g.abs().max()) / size, 1e-5)
        assert float(g.abs().max()) <= 1e-5 * size
    else:
        grad_close(g, g64, what)
    if n_atoms == 2:
        k = 2 * np.pi * n / cell.astype(np.float64)
        d = xyz[:, 1].astype(np.float64) - xyz[:, 0].astype(np.float64)
        assert np.allclose(Sk64, 1.0 + np.cos(d @ k.T), rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------- 4
def test_periodicity_and_translation():
    g, w, obs = fixture_obs("sk_s1")
    xyz = g["xyz"][:1].copy()
    xyz[:, :36] += np.float32(7) * g["cell"]
    xyz[:, 36:72] -= np.float32(3) * g["cell"]
    from mdgrad_amd.observable import sk_vectors
    n, seg, _, _ = sk_vectors(g["cell"].astype(np.float64), 30, (1.0, 16.0))
    S64, _, g64 = sk64(xyz, g["cell"], n, seg, None, g["gS"][:1])
    S, gq = run_obs(obs, xyz, g["gS"][:1])
    fwd_close(S, S64, 108.0, "a third of the atoms at +7 L, a third at -3 L")
    grad_close(gq, g64, "a third of the atoms at +7 L, a third at -3 L")
    for what, grad in (("shifted", gq), ("fixture", run_obs(obs, g["xyz"], g["gS"])[1])):
        drift = float(grad.sum(1).abs().max() / grad.abs().max())
        figure("translation: |sum_i dS/dx_i| / max|dS/dx| (%s)" % what, drift, 1e-5)
        assert drift <= 1e-5


# ---------------------------------------------------------------------------------------------- 5
def test_leading_shapes_and_bitwise_repeatability():
    from mdgrad_amd.observable import structure_factor
    g, w, obs = fixture_obs("sk_s1")
    q = torch.as_tensor(g["xyz"]).to(DEV)
    S_T = obs.per_frame(q)
    assert S_T.shape == (3, 30)
    for t in range(3):
        one = obs.per_frame(q[t])
        assert one.shape == (30,) and torch.equal(one, S_T[t])
    S_RT = obs.per_frame(torch.stack([q, q.flip(0)]))
    assert S_RT.shape == (2, 3, 30) and torch.equal(S_RT[0], S_T) and torch.equal(S_RT[1], S_T.flip(0))
    k = 3
    obs_k = structure_factor(mk_system(g["xyz"][0], g["cell"], n_rep=k), 30, (1.0, 16.0))
    qs = torch.stack([torch.cat([q[(t + r) % 3] for r in range(k)]) for t in range(3)])
    S_k = obs_k.per_frame(qs)
    assert S_k.shape == (3, k, 30) and obs_k.per_frame(qs[0]).shape == (k, 30)
    for t in range(3):
        for r in range(k):
            assert torch.equal(S_k[t, r], S_T[(t + r) % 3])
    assert torch.equal(obs_k(qs)[1], S_k.reshape(-1, 30).mean(0))
    for name, xyz in (("sk_s1", g["xyz"]), ("big", None)):
        if xyz is None:                                   # the tiled route: 1500 atoms
            rng = np.random.default_rng(3)
            xyz = rng.uniform(0, 12.0, (2, 1500, 3)).astype(np.float32)
            o = structure_factor(mk_system(xyz[0], [12.0] * 3), 10, (1.0, 6.0), max_per_bin=40)
        else:
            o = obs
        gS = np.random.default_rng(4).uniform(-1, 1, (len(xyz), o.nbins))
        a, b = run_obs(o, xyz, gS), run_obs(o, xyz, gS)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name


# ---------------------------------------------------------------------------------------------- 6
def test_weights_and_partials():
    from mdgrad_amd.observable import structure_factor
    g = load_golden("sk_s1")
    sel = np.zeros(108, dtype=bool)
    sel[np.random.default_rng(9).permutation(108)[:54]] = True
    wA, wB = sel.astype(np.float32), (~sel).astype(np.float32)
    args = (30, (1.0, 16.0))
    full = mk_system(g["xyz"][0], g["cell"])
    q = torch.as_tensor(g["xyz"]).to(DEV)
    S_AA = structure_factor(full, *args, weights=wA).per_frame(q)
    S_BB = structure_factor(full, *args, weights=wB).per_frame(q)
    S_AB = structure_factor(full, *args).per_frame(q)
    sub = structure_factor(mk_system(g["xyz"][0][sel], g["cell"]), *args).per_frame(q[:, torch.as_tensor(sel).to(DEV)])
    n, seg = structure_factor(full, *args).kvecs.numpy(), np.concatenate([[0], np.cumsum(structure_factor(full, *args).n_vectors.numpy())])
    A64, _, _ = sk64(g["xyz"], g["cell"], n, seg, wA)
    B64, _, _ = sk64(g["xyz"], g["cell"], n, seg, wB)
    fwd_close(S_AA, A64, 54.0, "0/1 weights vs float64")
    fwd_close(sub, A64, 54.0, "sub-system vs float64")
    fwd_close(S_AA, sub.cpu().double().numpy(), 54.0, "0/1 weights vs the sub-system of the selected atoms")
    # |rho_A + rho_B|^2 = |rho_A|^2 + |rho_B|^2 + 2 Re rho_A rho_B*, bin means are linear: the cross term from three calls
    cross = (108.0 * S_AB - 54.0 * S_AA - 54.0 * S_BB).cpu().double().numpy() / 2
    cross64 = (108.0 * g["S64"] - 54.0 * A64 - 54.0 * B64) / 2
    allowed = 0.5 * TOL * (108.0 * (np.sqrt(108.0 * g["S64"]) + 1) + 54.0 * (np.sqrt(54.0 * A64) + 1) + 54.0 * (np.sqrt(54.0 * B64) + 1))
    figure("cross partial Re rho_A rho_B* from three calls (worst bin, of its allowance)", (np.abs(cross - cross64) / allowed).max(), 1.0)
    assert (np.abs(cross - cross64) <= allowed).all()


# ---------------------------------------------------------------------------------------------- 7
def s3_run(n_rep):
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NoseHooverChain, Simulations
    from mdgrad_amd.observable import structure_factor
    g, g3 = load_golden("pressure_p3"), load_golden("sk_s3")
    system = mk_system(g["pos"], g["cell"], g["vel"], g["mass"], n_rep)
    mdl = P.LennardJones(1.0, 1.0)
    model = Stack({"pair": PairPotentials(system, mdl, cutoff=float(g["cutoff"]))})
    integ = NoseHooverChain(model, system, T=float(g["T"]), num_chains=int(g["chains"]), Q=float(g["Q"])).to(DEV)
    assert integ.fused_spec("NH_verlet") is not None
    n = int(g["n_steps"])
    v_t, q_t, pv_t = Simulations(system, integ).simulate(steps=n, frequency=n, dt=float(g["dt"]))
    fn = q_t.grad_fn                                  # (a replica batch comes back as a view of the fused launch's output)
    while fn is not None and not type(fn).__name__.startswith("FusedTrajFn"):
        fn = fn.next_functions[0][0] if fn.next_functions else None
    assert fn is not None, "the trajectory did not come from the fused kernels"
    obs = structure_factor(system, int(g3["nbins"]), tuple(g3["k_range"]))
    k, S = obs(q_t)
    loss = (S - 1.0).pow(2).sum()
    loss.backward()
    return g3, obs, q_t.detach(), obs.per_frame(q_t.detach()), loss.detach(), mdl


@pytest.mark.parametrize("n_rep", [0, 2])
def test_s3_through_the_fused_trajectory(n_rep):
    g3, obs, q_t, S_t, loss, mdl = s3_run(n_rep)
    n, seg = obs.kvecs.numpy(), np.concatenate([[0], np.cumsum(obs.n_vectors.numpy())])
    for r in range(max(n_rep, 1)):
        q_r = q_t.reshape(21, max(n_rep, 1), 108, 3)[:, r].cpu().numpy()
        S_r = S_t.reshape(21, max(n_rep, 1), 18)[:, r]
        last64, _, _ = sk64(q_r[-1:], g3["cell"], n, seg)
        div = float(np.abs(last64[0] - g3["S_t"][-1]).max())
        figure("S3 replica %d: float32 divergence of the last frame in S" % r, div, float("nan"))
        fwd_close(S_r, g3["S_t"], 108.0, "S3 replica %d S_t" % r, extra=div)
    atol = 1e-4 * abs(float(g3["grad_sigma"][0]))
    figure("S3 loss (golden %.6e)" % float(g3["loss"][0]), float(loss), float("nan"))
    close(mdl.sigma.grad, g3["grad_sigma"], 2e-3, atol, "S3 dL/dsigma")
    close(mdl.epsilon.grad, g3["grad_epsilon"], 2e-3, atol, "S3 dL/depsilon")


# ---------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("name", ["sk_s1", "sk_s2"])
def test_torch_ops_equal_the_ctypes_path(name):
    from mdgrad_amd import _torch_ops
    ns = _torch_ops.get()
    assert ns is not None
    g, w, obs = fixture_obs(name)
    S, gq = run_obs(obs, g["xyz"], g["gS"])
    q, gS = torch.as_tensor(g["xyz"]).to(DEV), torch.as_tensor(g["gS"]).to(DEV)
    cell = _torch_ops.cell_args(obs._cell_struct)
    S_t = ns.sk_fwd(q, cell, obs.weights, obs._norm, obs._kvec, obs._seg, obs._seg_host)
    g_t = ns.sk_bwd(q, cell, obs.weights, obs._norm, obs._kvec, obs._seg, obs._seg_host, gS)
    assert torch.equal(S_t, S) and torch.equal(g_t, gq)
    with pytest.raises(RuntimeError, match="kvec"):
        ns.sk_fwd(q, cell, obs.weights, obs._norm, obs._kvec[:-1].contiguous(), obs._seg, obs._seg_host)
