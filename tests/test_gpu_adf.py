"""Bond-angle distribution on the GPU (csrc/adf.hip, ops.AdfRawFn, observable.angle_distribution / Angles) against the
reference's goldens (A1-A5, tests/golden/make_adf_goldens.py) and an independent float64 torch implementation."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -20          # the degenerate-triplet rule of csrc/adf.hip: |u x v| <= EPS |u| |v| -> zero gradient
# f32 acos is ill-conditioned near cos = +-1: a cosine that differs by 4 ulp (2^-21) moves the angle by 2^-21 / sin(theta).
# Angles are compared within max(2e-6, min(1e-3, 2^-21 / sin theta)): 2e-6 rad wherever sin theta >= 0.24, i.e. away from
# 0 and pi; 1e-3 rad (the 4-ulp error at sin theta = 0, sqrt(2 * 2^-21)) caps it at the ends.
ANGLE_TOL = 2e-6


def system_of(pos, cell, n_rep=None):
    from mdgrad_amd.system import System
    s = System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
               masses=np.full(len(pos), 1.008), device=DEV)
    return s.replicate(n_rep) if n_rep else s


def close(a, b, rtol, atol, what):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, a.shape, b.shape)
    err = np.abs(a - b) - (atol + rtol * np.abs(b))
    assert err.max() <= 0, "%s: worst excess %.3e at %s (%.6e vs %.6e)" % (
        what, err.max(), np.unravel_index(err.argmax(), err.shape), a.flat[err.argmax()], b.flat[err.argmax()])


def check_angles(got, want, what):
    got, want = got.detach().cpu().double().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    tol = np.maximum(ANGLE_TOL, np.minimum(1e-3, 2.0 ** -21 / np.maximum(np.sin(want), 1e-30)))
    err = np.abs(got - want) - tol
    assert err.max() <= 0, "%s: worst excess %.3e at angle %.6f" % (what, err.max(), want[err.argmax()])


def run_golden(g, p, index_tuple=None, width=None):
    from mdgrad_amd.observable import angle_distribution
    frames = g[p + "xyz"]
    obs = angle_distribution(system_of(frames[0], g["cell"]), int(g[p + "nbins"]), tuple(float(x) for x in g[p + "range"]),
                             cutoff=float(g[p + "cutoff"]), index_tuple=index_tuple, width=width)
    xyz = torch.tensor(frames, device=DEV, requires_grad=True)
    bins, count, angles = obs(xyz)
    close(bins, g[p + "bins"], 0, 0, "bins")
    close(count, g[p + "count"], 1e-4, 1e-6 * np.abs(g[p + "count"]).max(), "count")
    loss = (count - torch.tensor(g[p + "target"], device=DEV)).pow(2).sum()
    loss.backward()
    want = g[p + "grad"]
    close(xyz.grad, want, 0, 1e-3 * np.abs(want).max(), "xyz.grad")
    assert angles.shape[0] == int(g[p + "n_angles"])
    if p + "sub_idx" in g:
        angles = angles[torch.as_tensor(g[p + "sub_idx"], device=DEV)]
    check_angles(angles, g[p + "angles"], "angles")


@pytest.mark.parametrize("case", ["c15_", "c20_", "c25_"])
def test_a1_golden(case):
    run_golden(load_golden("adf_a1"), case)


def test_a2_golden_width_range_and_index_tuple():
    g = load_golden("adf_a2")
    run_golden(g, "", index_tuple=(g["idx_a"].tolist(), g["idx_b"].tolist()), width=0.05)


def test_a3_angles_cos():
    from mdgrad_amd.observable import Angles
    g = load_golden("adf_a3")
    cos = Angles(system_of(g["xyz"][0], g["cell"]), int(g["nbins"]), (0.0, math.pi), cutoff=float(g["cutoff"]))(
        torch.tensor(g["xyz"], device=DEV))
    close(cos, g["cos"], 0, 1e-6, "cos")


# ------------------------------------------------------------------------------------------------ float64 cross-check
def ref64(frames, L, cutoff, mu, coeff, mask=None, g_raw=None, chunk=16):
    """Independent float64 implementation of the semantics: raw[b] = sum over ordered triplets exp(coeff (theta - mu_b)^2)
    and, given g_raw, d(g_raw . raw)/dx with zero gradient for |u x v| <= EPS |u| |v|."""
    x_all = torch.as_tensor(frames, dtype=torch.float64, device=DEV)
    L = torch.as_tensor(L, dtype=torch.float64, device=DEV)
    mu = torch.as_tensor(mu, dtype=torch.float64, device=DEV)
    F, N = x_all.shape[0], x_all.shape[1]
    raw = torch.zeros(mu.shape[0], dtype=torch.float64, device=DEV)
    grad = torch.zeros_like(x_all)
    for f0 in range(0, F, chunk):
        x = x_all[f0:f0 + chunk].clone().requires_grad_(g_raw is not None)
        with torch.no_grad():
            d = x[:, None, :, :] - x[:, :, None, :]
            s = d / L
            d = d + (-(s > 0.5).double() + (s < -0.5).double()) * L
            d2 = d.pow(2).sum(-1)
            adj = (d2 < cutoff ** 2) & (d2 != 0)
            if mask is not None:
                adj &= torch.as_tensor(mask, device=DEV).bool()
            K = int(adj.sum(-1).max())
            nb = torch.argsort((~adj).to(torch.int8), dim=-1, stable=True)[..., :K]
            ok = torch.gather(adj, 2, nb)
            p, q = torch.triu_indices(K, K, 1, device=DEV)
            live = ok[..., p] & ok[..., q]
        fi = torch.arange(x.shape[0], device=DEV)[:, None, None]
        centre = x[:, :, None, :]

        def bond(idx):
            b = x[fi, idx] - centre
            return b + (-(b >= 0.5 * L).double() + (b < -0.5 * L).double()) * L
        u, v = bond(nb[..., p]), bond(nb[..., q])
        w = torch.cross(u, v, dim=-1)
        w2, uu, vv, dot = w.pow(2).sum(-1), u.pow(2).sum(-1), v.pow(2).sum(-1), (u * v).sum(-1)
        deg = w2 <= EPS ** 2 * uu * vv
        th_live = torch.atan2(torch.where(deg, torch.ones_like(w2), w2).sqrt(), dot)
        th = torch.where(deg, torch.atan2(torch.zeros_like(dot), dot).detach(), th_live)[live]
        part = 2.0 * torch.exp(coeff * (th[:, None] - mu[None, :]) ** 2).sum(0)
        raw += part.detach()
        if g_raw is not None:
            (gx,) = torch.autograd.grad((part * g_raw).sum(), x)
            grad[f0:f0 + chunk] = gx
    return raw, grad


def lj_frames(n_frames, seed, sigma=0.08, size=3, a=1.6):
    base = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
    lat = np.array([(np.array([i, j, k]) + b) * a for i in range(size) for j in range(size) for k in range(size) for b in base])
    cell = np.array([a * size] * 3)
    rng = np.random.default_rng(seed)
    fr = np.stack([np.mod(lat + rng.normal(0, sigma, lat.shape), cell) for _ in range(n_frames)])
    return fr.astype(np.float32), cell


def kernel_raw_and_grad(obs, frames, g_raw):
    from mdgrad_amd import ops
    x = torch.tensor(np.asarray(frames).reshape(-1, obs.natoms, 3), device=DEV, requires_grad=True)
    raw = ops.AdfRawFn.apply(x, obs.smear.offsets, obs.coeff, obs.cutoff, obs._cell_struct, obs._mask, obs.spacing)
    (gx,) = torch.autograd.grad((raw * g_raw).sum(), x)
    return raw, gx


def cross_check(obs, frames, L, mask=None, seed=3, g_scale=None):
    g_raw = torch.tensor(np.random.default_rng(seed).normal(0, 1, obs.nbins), dtype=torch.float32, device=DEV)
    raw, gx = kernel_raw_and_grad(obs, frames, g_raw)
    r64, g64 = ref64(frames.reshape(-1, obs.natoms, 3), L, obs.cutoff, obs.smear.offsets.double(), obs.coeff, mask,
                     g_raw.double())
    close(raw, r64, 0, 2e-6 * float(r64.abs().max()), "raw vs f64")
    scale = float(g64.abs().max()) if g_scale is None else g_scale
    close(gx.reshape(g64.shape), g64, 0, 1e-4 * scale, "grad vs f64")
    return raw, gx


def test_f64_256_frames():
    from mdgrad_amd.observable import angle_distribution
    frames, cell = lj_frames(256, 21)
    obs = angle_distribution(system_of(frames[0], cell), 180, (0.0, math.pi), cutoff=1.5)
    cross_check(obs, frames, cell)


def test_f64_replicated_trajectory_equals_per_replica_frames():
    from mdgrad_amd.observable import angle_distribution
    T_, R = 3, 4
    frames, cell = lj_frames(T_ * R, 22)
    traj = frames.reshape(T_, R * 108, 3)
    sys_r = system_of(frames[0], cell, n_rep=R)
    obs = angle_distribution(sys_r, 90, (0.0, math.pi), cutoff=2.0)
    assert obs.natoms == 108
    xt = torch.tensor(traj, device=DEV, requires_grad=True)
    _, count, angles = obs(xt)
    count.pow(2).sum().backward()
    xf = torch.tensor(frames, device=DEV, requires_grad=True)
    obs1 = angle_distribution(system_of(frames[0], cell), 90, (0.0, math.pi), cutoff=2.0)
    _, count1, angles1 = obs1(xf)
    count1.pow(2).sum().backward()
    assert torch.equal(count, count1) and torch.equal(angles, angles1)
    assert torch.equal(xt.grad.reshape(-1), xf.grad.reshape(-1))
    cross_check(obs, traj, cell)


def test_f64_cell_list_box():
    from mdgrad_amd import ops
    from mdgrad_amd.observable import angle_distribution
    L = (1024 / 0.95) ** (1.0 / 3.0)
    cell = np.array([L] * 3)
    frames = np.random.default_rng(23).uniform(0, L, (1, 1024, 3)).astype(np.float32)
    obs = angle_distribution(system_of(frames[0], cell), 60, (0.0, math.pi), cutoff=1.5)
    assert ops._use_cell_list(1024, obs._cell_struct, 1.5)        # the cell-list builder
    cross_check(obs, frames, cell)


def test_f64_masked_mixture():
    from mdgrad_amd import ops
    from mdgrad_amd.observable import angle_distribution
    frames, cell = lj_frames(8, 24)
    idx = (list(range(0, 108, 3)), list(range(108)))
    obs = angle_distribution(system_of(frames[0], cell), 72, (0.3, 3.0), cutoff=1.8, index_tuple=idx, width=0.08)
    cross_check(obs, frames, cell, mask=ops.build_mask(108, idx, None, DEV))


def test_a4_lattice_collinear_forward_and_zero_rule():
    from mdgrad_amd.observable import angle_distribution
    g = load_golden("adf_a4")
    obs = angle_distribution(system_of(g["xyz"][0], g["cell"]), int(g["nbins"]), (0.0, math.pi), cutoff=float(g["cutoff"]))
    xyz = torch.tensor(g["xyz"], device=DEV, requires_grad=True)
    _, count, angles = obs(xyz)
    close(count, g["count"], 1e-4, 1e-6 * np.abs(g["count"]).max(), "count")
    check_angles(angles, g["angles"], "angles")
    # on the exact lattice the f64 gradient vanishes by symmetry, and what f32 leaves of the cancelling terms is compared with
    # the gradient scale of the same lattice jittered by 0.02
    jit = (g["xyz"] + np.random.default_rng(4).normal(0, 0.02, g["xyz"].shape)).astype(np.float32)
    g_raw = torch.tensor(np.random.default_rng(3).normal(0, 1, obs.nbins), dtype=torch.float64, device=DEV)
    _, gj = ref64(jit, g["cell"], obs.cutoff, obs.smear.offsets.double(), obs.coeff, None, g_raw)
    cross_check(obs, g["xyz"], g["cell"], g_scale=float(gj.abs().max()))
    count.pow(2).sum().backward()
    assert torch.isfinite(xyz.grad).all()


# ------------------------------------------------------------------------------------------------ determinism, chunks, ops
def test_bitwise_reproducible_and_chunked(monkeypatch):
    from mdgrad_amd import ops
    from mdgrad_amd.observable import angle_distribution
    frames, cell = lj_frames(24, 25)
    obs = angle_distribution(system_of(frames[0], cell), 120, (0.0, math.pi), cutoff=1.6)
    g_raw = torch.tensor(np.random.default_rng(5).normal(0, 1, 120), dtype=torch.float32, device=DEV)
    r1, g1 = kernel_raw_and_grad(obs, frames, g_raw)
    r2, g2 = kernel_raw_and_grad(obs, frames, g_raw)
    assert torch.equal(r1, r2) and torch.equal(g1, g2)
    monkeypatch.setattr(ops, "ADF_CHUNK_FRAMES", 5)         # 5 chunks, the last one short
    r3, g3 = kernel_raw_and_grad(obs, frames, g_raw)
    close(r3, r1, 0, 1e-6 * float(r1.detach().abs().max()), "chunked raw")   # (each chunk has its own fixed-point scale)
    assert torch.equal(g3, g1)                              # (the gradient of a frame does not depend on the chunking)


def test_torch_ops_equal_ctypes_path():
    from mdgrad_amd import _torch_ops, ops
    from mdgrad_amd.observable import angle_distribution
    ns = _torch_ops.get()
    assert ns is not None
    frames, cell = lj_frames(4, 26)
    obs = angle_distribution(system_of(frames[0], cell), 60, (0.0, math.pi), cutoff=1.5)
    g_raw = torch.tensor(np.random.default_rng(6).normal(0, 1, 60), dtype=torch.float32, device=DEV)
    raw, gx = kernel_raw_and_grad(obs, frames, g_raw)
    x = torch.tensor(frames, device=DEV).reshape(-1, 3)
    ell = ops.build_ell(x, obs._cell_struct, obs.cutoff, None, group=108)
    cl = _torch_ops.cell_args(obs._cell_struct)
    mu = obs.smear.offsets.float().contiguous()
    raw_t = ns.adf_fwd(x, 4, 108, cl, obs.cutoff, ell.col, ell.cnt, mu, obs.spacing, obs.coeff)
    g_t = ns.adf_bwd(x, 4, 108, cl, obs.cutoff, ell.col, ell.cnt, mu, obs.spacing, obs.coeff, g_raw)
    assert torch.equal(raw_t, raw) and torch.equal(g_t.reshape(-1), gx.reshape(-1))


def test_keep_angles_false_and_invalid_arguments():
    from mdgrad_amd.observable import angle_distribution
    frames, cell = lj_frames(2, 27)
    s = system_of(frames[0], cell)
    x = torch.tensor(frames, device=DEV)
    b1, c1, a1 = angle_distribution(s, 60, (0.0, math.pi), cutoff=1.5)(x)
    b2, c2, a2 = angle_distribution(s, 60, (0.0, math.pi), cutoff=1.5, keep_angles=False)(x)
    assert a1 is not None and a2 is None
    assert torch.equal(b1, b2) and torch.equal(c1, c2)
    for nbins, rng in [(0, (0.0, 3.0)), (1, (0.0, 3.0)), (-2, (0.0, 3.0)), (10, (1.0,))]:
        with pytest.raises((IndexError, RuntimeError)):
            angle_distribution(s, nbins, rng, cutoff=1.5)


# ------------------------------------------------------------------------------------------------ A5: trajectory + adjoint
@pytest.mark.parametrize("path", ["fused", "generic"])
def test_a5_trajectory_adjoint_golden(path):
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.observable import angle_distribution
    from mdgrad_amd.sovlers import odeint_adjoint
    g = load_golden("adf_a5")
    system = system_of(g["pos"], g["cell"])
    system.set_velocities(np.asarray(g["vel"], dtype=np.float64))
    mdl = P.LennardJones(1.0, 1.0)
    integ = NoseHooverChain(Stack({"pair": PairPotentials(system, mdl, cutoff=float(g["cutoff"]))}), system, T=float(g["T"]),
                            num_chains=int(g["chains"]), Q=float(g["Q"]), adjoint=True).to(DEV)
    if path == "generic":
        integ.fused_spec = lambda method: None
    else:
        assert integ.fused_spec("NH_verlet") is not None
    y0 = [s_.clone().requires_grad_(True) for s_ in integ.get_inital_states(wrap=True)]
    t = torch.Tensor([float(g["dt"]) * i for i in range(int(g["n_steps"]))]).to(DEV)
    v_t, q_t, pv_t = odeint_adjoint(integ, tuple(y0), t, method="NH_verlet")
    assert (type(q_t.grad_fn).__name__.startswith("FusedTrajFn")) == (path == "fused")
    obs = angle_distribution(system, int(g["nbins"]), (0.0, math.pi), cutoff=float(g["adf_cutoff"]), keep_angles=False)
    _, count, _ = obs(q_t[::int(g["stride"])])
    close(count, g["count"], 1e-3, 1e-6, "count")
    loss = (count - 1.0 / int(g["nbins"])).pow(2).sum() * 1e3
    close(loss.reshape(1), g["loss"], 1e-3, 1e-5, "loss")
    loss.backward()
    close(mdl.sigma.grad, g["grad_sigma"], 2e-3, 1e-4 * abs(float(g["grad_sigma"][0])), "dL/dsigma")
    close(mdl.epsilon.grad, g["grad_epsilon"], 2e-3, 1e-4 * abs(float(g["grad_sigma"][0])), "dL/depsilon")
    for y, k in zip(y0, ["grad_v0", "grad_q0", "grad_pv0"]):
        close(y.grad, g[k], 5e-3, 2e-3 * np.abs(g[k]).max(), k)


def test_f64_wide_width_spans_the_range():
    """width 0.5 over 180 centres in (0, pi): the reach covers every centre, so the recurrence runs ~180 steps from the
    nearest centre (re-anchored every 8)."""
    from mdgrad_amd.observable import angle_distribution
    frames, cell = lj_frames(16, 28)
    obs = angle_distribution(system_of(frames[0], cell), 180, (0.0, math.pi), cutoff=1.5, width=0.5)
    cross_check(obs, frames, cell)


def test_chunked_lists_are_not_kept_alive(monkeypatch):
    """With several chunks, at most about one chunk's neighbour list is allocated at a time, forward and backward."""
    from mdgrad_amd import ops
    from mdgrad_amd.observable import angle_distribution
    frames, cell = lj_frames(96, 29)
    obs = angle_distribution(system_of(frames[0], cell), 60, (0.0, math.pi), cutoff=1.5)
    x = torch.tensor(frames, device=DEV, requires_grad=True)
    one = ops.build_ell(x.detach()[:6].reshape(-1, 3), obs._cell_struct, obs.cutoff, None, group=108)
    chunk_bytes = 4 * (one.col.numel() + one.shift.numel() + one.cnt.numel())
    del one
    monkeypatch.setattr(ops, "ADF_CHUNK_FRAMES", 6)                       # 16 chunks
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    raw = ops.AdfRawFn.apply(x, obs.smear.offsets, obs.coeff, obs.cutoff, obs._cell_struct, obs._mask, obs.spacing)
    raw.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 3 * chunk_bytes + 4 * x.numel() * 4, "peak %d B for chunk lists of %d B" % (peak, chunk_bytes)


def test_angle_list_limit_names_keep_angles(monkeypatch):
    from mdgrad_amd import topology
    from mdgrad_amd.observable import angle_distribution, Angles
    frames, cell = lj_frames(4, 30)
    s = system_of(frames[0], cell)
    x = torch.tensor(frames, device=DEV)
    monkeypatch.setattr(topology, "ANGLE_LIST_MAX", 4000)
    with pytest.raises(ValueError, match="keep_angles=False"):
        angle_distribution(s, 60, (0.0, math.pi), cutoff=1.5)(x)
    with pytest.raises(ValueError, match="keep_angles=False"):
        Angles(s, 60, (0.0, math.pi), cutoff=1.5)(x)
    _, count, angles = angle_distribution(s, 60, (0.0, math.pi), cutoff=1.5, keep_angles=False)(x)
    assert angles is None and torch.isfinite(count).all()


def test_angles_chunked_equal_single_list(monkeypatch):
    from mdgrad_amd import ops
    from mdgrad_amd.observable import Angles
    frames, cell = lj_frames(7, 31)
    a = Angles(system_of(frames[0], cell), 60, (0.0, math.pi), cutoff=1.6)
    x = torch.tensor(frames, device=DEV)
    one = a(x)
    monkeypatch.setattr(ops, "ADF_CHUNK_FRAMES", 3)
    assert torch.equal(a(x), one)


def test_torch_ops_reject_bad_arguments():
    from mdgrad_amd import _torch_ops, ops
    from mdgrad_amd.observable import angle_distribution
    ns = _torch_ops.get()
    frames, cell = lj_frames(2, 32)
    obs = angle_distribution(system_of(frames[0], cell), 60, (0.0, math.pi), cutoff=1.5)
    x = torch.tensor(frames, device=DEV).reshape(-1, 3)
    ell = ops.build_ell(x, obs._cell_struct, obs.cutoff, None, group=108)
    cl = _torch_ops.cell_args(obs._cell_struct)
    mu = obs.smear.offsets.float().contiguous()
    with pytest.raises(RuntimeError, match="g_raw"):
        ns.adf_bwd(x, 2, 108, cl, obs.cutoff, ell.col, ell.cnt, mu, obs.spacing, obs.coeff, torch.zeros(60))
    with pytest.raises(RuntimeError, match="2\\^31"):
        ns.adf_fwd(x, 2 ** 32 + 2, 108, cl, obs.cutoff, ell.col, ell.cnt, mu, obs.spacing, obs.coeff)
