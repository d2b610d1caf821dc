"""Pressure observable on the GPU (csrc/virial.hip, ops.VirialFn, thermo.Pressure) against the reference-built goldens
(P1-P3, tests/golden/make_pressure_goldens.py), an independent float64 torch implementation and the scaling identity
W = -dU/ds at s = 1 (q -> s q, L -> s L, pair set frozen).

Tolerances, with what the MI355X showed (every comparison prints its figure before it asserts):
  forward     |W - W64| <= TOL * S per frame, S = sum |r phi'| from the fixture (tests 2, 3: from the float64 route itself).
              TOL = 10 x OBSERVED_FWD, the largest |W - W64| / S over the P1 / P2 cases = 4.1e-7 (the two-term stack; single
              forms 0.6e-7 .. 1.4e-7); must stay <= 1e-5.  The size cases show 1.3e-7 .. 3.0e-7, and 8.1e-7 / 1.2e-6 for
              the frames of three atoms / one pair (one v_rsq_f32 ulp carried to the twelfth power, nothing to average over).
              Against the float32 golden: the same bound plus the golden's own |W32 - W64|.
  dW/dq       rtol 1e-4, atol 2e-6 max|.|   (test_pair_forms_golden's bound on H w, the same phi''); observed at most 0.28 of
              the allowance (4 096 atoms), 0.01 .. 0.08 of it on the fixtures
  dW/dtheta   rtol 2e-4, atol 1e-5 max|.|   (test_pair_forms_golden's bound on d(w.F)/dtheta); observed <= 1e-3 of it
  K           rtol 1e-6 (a float32 sum of 324 positive terms); observed 1e-7
  P3          dL/dsigma, dL/depsilon: rtol 2e-3, atol 1e-4 |dL/dsigma| (test_fused_traj_and_adjoint_golden); observed
              6.3e-3 of 11.1 allowed and 3.0e-4 of 0.73.
              P_t: atol 1e-3 -- the fixture's closest pair sits 3.3e-6 from the cutoff, and one LJ pair changing sides moves
              a frame's P by 2.9e-4 (make_pressure_goldens.py): room for three -- plus rtol 1e-4; observed 1.4e-6 (no flip)
"""
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBSERVED_FWD = 4.1e-7     # largest |W - W64| / S over the P1 / P2 cases and all three float64 routes (MI355X): the stack
TOL = 10 * OBSERVED_FWD
assert TOL <= 1e-5
P1_FORMS = ["lj", "ljfam_8_4", "lj69", "exvol12", "exvol10", "morse_pos", "morse_neg", "buck"]
FIGURES = []              # (what, observed, allowed): printed by every comparison, before it asserts


def figure(what, observed, allowed):
    FIGURES.append((what, observed, allowed))
    print("FIGURE %-60s observed %.3e  allowed %.3e" % (what, observed, allowed))


def close(a, b, rtol, atol, what):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, a.shape, b.shape)
    err, tol = np.abs(a - b), atol + rtol * np.abs(b)
    k = np.argmax(err - tol)
    figure(what, err.flat[k], tol.flat[k])
    assert np.isfinite(a).all(), what + ": non-finite"
    assert (err <= tol).all(), "%s: err %.3e, allowed %.3e" % (what, err.flat[k], tol.flat[k])


def fwd_close(W, W64, S, extra, what):
    W, W64, S = (np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float64) for x in (W, W64, S))
    rel = np.divide(np.abs(W - W64), S, out=np.zeros_like(S), where=S > 0)
    figure(what + " |W - W64| / S", rel.max(), TOL)
    assert (np.abs(W - W64) <= TOL * S + extra).all(), "%s: |W - W64| / S = %.3e, TOL %.1e" % (what, rel.max(), TOL)


def mk_system(pos, cell, vel=None, mass=None, n_rep=0):
    from mdgrad_amd.system import System
    s = System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
               masses=(np.asarray(mass, dtype=np.float64) if mass is not None else np.full(len(pos), 1.008)), device=DEV)
    if vel is not None:
        s.set_velocities(np.asarray(vel, dtype=np.float64))
    return s.replicate(n_rep) if n_rep else s


def form(name):
    from mdgrad_amd import potentials as P
    return {"lj": lambda: P.LennardJones(sigma=1.05, epsilon=0.9),
            "ljfam_8_4": lambda: P.LJFamily(sigma=0.95, epsilon=1.1, attr_pow=4, rep_pow=8),
            "lj69": lambda: P.LennardJones69(sigma=1.0, epsilon=1.2),
            "exvol12": lambda: P.ExcludedVolume(sigma=1.0, epsilon=1.0, power=12),
            "exvol10": lambda: P.ExcludedVolume(sigma=1.1, epsilon=0.7, power=10),
            "morse_pos": lambda: P.ModifiedMorse(a=3.0, phi=1.5),
            "morse_neg": lambda: P.ModifiedMorse(a=2.5, phi=-1.2),
            "buck": lambda: P.Buck(A=1000.0, B=3.5, C=5.0),
            "yukawa": lambda: P.Yukawa(epsilon=1.3, kappa=0.8)}[name]()


def case(name):
    """(golden, prefix, system, Pressure, [(module, cutoff, index_tuple, ex_pairs)]) of a P1 form or of P2 ("stack")."""
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.thermo import Pressure
    if name == "stack":
        g = load_golden("pressure_p2")
        system = mk_system(g["xyz"][0], g["cell"])
        lj, ev = P.LennardJones(sigma=1.05, epsilon=0.9), P.ExcludedVolume(sigma=0.9, epsilon=0.6, power=12)
        it, ex = (g["idx_a"].tolist(), g["idx_b"].tolist()), torch.as_tensor(g["ex_pairs"])
        model = Stack({"lj": PairPotentials(system, lj, cutoff=float(g["cutoff_lj"]), index_tuple=it),
                       "ev": PairPotentials(system, ev, cutoff=float(g["cutoff_ev"]), ex_pairs=ex)})
        terms = [(lj, float(g["cutoff_lj"]), it, None), (ev, float(g["cutoff_ev"]), None, g["ex_pairs"])]
        return g, "", system, Pressure(system, model), terms
    g = load_golden("pressure_p1")
    system = mk_system(g["xyz"][0], g["cell"])
    mdl = form(name)
    obs = Pressure(system, PairPotentials(system, mdl, cutoff=float(g["cutoff"])))
    return g, (name + "_" if name != "yukawa" else None), system, obs, [(mdl, float(g["cutoff"]), None, None)]


def params_of(terms):
    return [p for m, *_ in terms for p in m.mdg_params()]


def run_gpu(obs, terms, xyz, gw):
    """(W, dL/dq, dL/dtheta) of L = sum_f gw_f W_f through the kernels."""
    q = torch.as_tensor(xyz).to(DEV).requires_grad_(True)
    W = obs.virial(q)
    ps = params_of(terms)
    grads = torch.autograd.grad((W * torch.as_tensor(gw).to(DEV)).sum(), [q] + ps)
    return W.detach(), grads[0], (torch.stack([x.reshape(()) for x in grads[1:]]) if ps else None)


# ---------------------------------------------------------------------------------------------- float64 routes (CPU)
def half_list(x32, cell32, cutoff, index_tuple, ex_pairs):
    """Pairs i < j of one frame with the strict +-1/2 minimum image and 0 < d^2 < cutoff^2, selected in float32 like the
    kernels and the reference; returns (i, j, image offsets as float64 [P, 3])."""
    x = torch.as_tensor(x32, dtype=torch.float32)
    L = torch.as_tensor(cell32, dtype=torch.float32)
    N = x.shape[0]
    D = x[None, :, :] - x[:, None, :]                         # D[i, j] = x_j - x_i
    s = D * (1.0 / L)
    off = -(s > 0.5).float() + (s < -0.5).float()
    Dm = D + off * L
    d2 = Dm.pow(2).sum(-1)
    keep = torch.triu(torch.ones(N, N, dtype=torch.bool), 1) & (d2 < cutoff ** 2) & (d2 != 0)
    if index_tuple is not None:
        sel = torch.zeros(N, N, dtype=torch.bool)
        sel[torch.as_tensor(index_tuple[0])[:, None], torch.as_tensor(index_tuple[1])[None, :]] = True
        keep &= sel | sel.t()
    if ex_pairs is not None:
        ex = torch.as_tensor(np.asarray(ex_pairs)).long()
        keep[ex[:, 0], ex[:, 1]] = False
        keep[ex[:, 1], ex[:, 0]] = False
    i, j = torch.nonzero(keep, as_tuple=True)
    return i, j, off[i, j].double()


def route64(xyz, cell32, terms, gw, scaling):
    """W, S per frame and the gradients of sum_f gw_f W_f in float64 on the CPU.  scaling=False: the pair sum
    -sum r phi'(r); scaling=True: -dU/ds at s = 1 of U(s) = sum phi(|s (x_i - x_j - o L)|) with the pairs frozen."""
    mods = [copy.deepcopy(m).cpu().double() for m, *_ in terms]
    ps = [p for m in mods for p in m.mdg_params()]
    L = torch.as_tensor(cell32, dtype=torch.float32).double()
    q = torch.as_tensor(xyz, dtype=torch.float32).double().requires_grad_(True)
    Ws, Ss = [], []
    for f in range(q.shape[0]):
        W, S = 0.0, 0.0
        for m, (_, cutoff, it, ex) in zip(mods, terms):
            i, j, off = half_list(xyz[f], cell32, cutoff, it, ex)
            vec = q[f, j] - q[f, i] + off * L
            if scaling:
                s = torch.ones((), dtype=torch.float64, requires_grad=True)
                U = m((s * vec).pow(2).sum(-1).sqrt()).sum()
                (dU,) = torch.autograd.grad(U, s, create_graph=True)
                W = W - dU
            r = vec.pow(2).sum(-1).sqrt()
            rr = r.detach().requires_grad_(True)
            (du,) = torch.autograd.grad(m(rr).sum(), rr)
            S = S + float((rr * du).abs().sum().detach())
            if not scaling:
                (du,) = torch.autograd.grad(m(r).sum(), r, create_graph=True)
                W = W - (r * du).sum()
        Ws.append(W)
        Ss.append(S)
    W = torch.stack(Ws)
    grads = torch.autograd.grad((W * torch.as_tensor(gw).double()).sum(), [q] + ps)
    return W.detach(), np.array(Ss), grads[0], (torch.stack([x.reshape(()) for x in grads[1:]]) if ps else None)


def grads_close(gq, gth, rq, rth, what):
    close(gq, rq, 1e-4, 2e-6 * float(np.abs(np.asarray(rq)).max()), what + " dW/dq")
    if rth is not None:
        close(gth, rth, 2e-4, 1e-5 * float(np.abs(np.asarray(rth)).max()), what + " dW/dtheta")


# ---------------------------------------------------------------------------------------------- 1-3
@pytest.mark.parametrize("name", P1_FORMS + ["stack"])
def test_virial_against_goldens(name):
    g, pre, system, obs, terms = case(name)
    W, gq, gth = run_gpu(obs, terms, g["xyz"], g[pre + "gw"])
    fwd_close(W, g[pre + "W64"], g[pre + "S"], 0.0, name + " vs float64 golden")
    dev32 = np.abs(g[pre + "W32"].astype(np.float64) - g[pre + "W64"])          # the golden's own float32 - float64 deviation
    fwd_close(W, g[pre + "W32"], g[pre + "S"], dev32, name + " vs float32 golden")
    gw = torch.as_tensor(g[pre + "gw"]).to(DEV)
    grads_close(gq / gw[:, None, None], gth, g[pre + "dW_dq"], g[pre + "dW_dtheta"] if pre + "dW_dtheta" in g else None,
                name + " golden")
    # P = (K + W) / (d V): K is a float32 sum of 324 positive terms (1e-6 relative ~ 16 ulp), W as above
    q, v = torch.as_tensor(g["xyz"]).to(DEV), torch.as_tensor(g["vel"]).to(DEV)
    close(obs.kinetic(v), g[pre + "K"], 1e-6, 0.0, name + " K")
    dV = int(g["dim"]) * float(np.prod(g["cell"].astype(np.float64)))
    allowed = (TOL * g[pre + "S"] + dev32 + 1e-6 * g[pre + "K"]) / dV + 1e-6 * np.abs(g[pre + "P"])
    err = np.abs(obs(q, v).detach().cpu().double().numpy() - g[pre + "P"])
    figure(name + " P", (err / allowed).max(), 1.0)
    assert (err <= allowed).all()


@pytest.mark.parametrize("scaling", [False, True], ids=["pair_sum", "scaling_identity"])
@pytest.mark.parametrize("name", P1_FORMS + ["yukawa", "stack"])
def test_virial_against_float64_routes(name, scaling):
    g, pre, system, obs, terms = case(name)
    gw = np.array([0.7, 1.2, 0.9], dtype=np.float32)
    W, gq, gth = run_gpu(obs, terms, g["xyz"], gw)
    W64, S, rq, rth = route64(g["xyz"], g["cell"], terms, gw, scaling)
    what = "%s vs %s" % (name, "-dU/ds" if scaling else "pair sum")
    fwd_close(W, W64, S, 0.0, what)
    grads_close(gq, gth, rq, rth, what)


# ---------------------------------------------------------------------------------------------- 4
def p3_run(n_rep):
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NoseHooverChain, Simulations
    from mdgrad_amd.thermo import Pressure
    g = load_golden("pressure_p3")
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
    P_t = Pressure(system, model)(q_t, v_t)
    loss = (P_t - float(g["target"])).pow(2).sum()
    loss.backward()
    return g, P_t.detach(), loss.detach(), mdl


def test_p3_trajectory_end_to_end():
    g, P_t, loss, mdl = p3_run(0)
    assert P_t.shape == (int(g["n_steps"]),)
    close(P_t, g["P_t"], 1e-4, 1e-3, "P3 P_t")
    atol = 1e-4 * abs(float(g["grad_sigma"][0]))
    close(mdl.sigma.grad, g["grad_sigma"], 2e-3, atol, "P3 dL/dsigma")
    close(mdl.epsilon.grad, g["grad_epsilon"], 2e-3, atol, "P3 dL/depsilon")


def test_p3_replica_batch_through_the_fused_kernels():
    g, P_t, loss, mdl = p3_run(4)
    assert P_t.shape == (int(g["n_steps"]), 4)
    for r in range(4):
        close(P_t[:, r], g["P_t"], 1e-4, 1e-3, "P3 replica %d P_t" % r)
    atol = 1e-4 * abs(float(g["grad_sigma"][0]))
    close(mdl.sigma.grad / 4, g["grad_sigma"], 2e-3, atol, "P3 x4 dL/dsigma / 4")
    close(mdl.epsilon.grad / 4, g["grad_epsilon"], 2e-3, atol, "P3 x4 dL/depsilon / 4")


# ---------------------------------------------------------------------------------------------- 5
def test_shapes_and_stacked_replicas():
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials
    from mdgrad_amd.thermo import Pressure
    g, _, system, obs, _ = case("lj")
    q, v = torch.as_tensor(g["xyz"]).to(DEV), torch.as_tensor(g["vel"]).to(DEV)
    P_T = obs(q, v)
    assert P_T.shape == (3,)
    one = obs(q[1], v[1])
    assert one.shape == () and torch.equal(one, P_T[1])
    P_RT = obs(torch.stack([q, q.flip(0)]), torch.stack([v, v.flip(0)]))
    assert P_RT.shape == (2, 3) and torch.equal(P_RT[0], P_T) and torch.equal(P_RT[1], P_T.flip(0))
    k = 3
    rep = mk_system(g["xyz"][0], g["cell"], n_rep=k)
    obs_k = Pressure(rep, PairPotentials(rep, P.LennardJones(sigma=1.05, epsilon=0.9), cutoff=float(g["cutoff"])))
    # frame t of the stacked state holds the frames t, t + 1, t + 2 (mod 3) as its three replicas
    qs = torch.stack([torch.cat([q[(t + r) % 3] for r in range(k)]) for t in range(3)])
    vs = torch.stack([torch.cat([v[(t + r) % 3] for r in range(k)]) for t in range(3)])
    P_k = obs_k(qs, vs)
    assert P_k.shape == (3, k)
    for t in range(3):
        for r in range(k):
            assert torch.equal(P_k[t, r], P_T[(t + r) % 3])
    assert obs_k.virial(qs).shape == (3, k) and obs_k.kinetic(vs[0]).shape == (k,)


# ---------------------------------------------------------------------------------------------- 6
def liquid(n, rho=0.8, seed=0, frames=1):
    rng = np.random.default_rng(seed)
    L = (n / rho) ** (1 / 3)
    side = int(np.ceil(n ** (1 / 3)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n] * (L / side)
    xyz = np.stack([np.mod(grid + rng.uniform(-0.12, 0.12, grid.shape) * (L / side), L) for _ in range(frames)])
    return xyz.astype(np.float32), np.array([L, L, L], dtype=np.float32)


@pytest.mark.parametrize("n,frames", [(2, 3), (3, 3), (107, 3), (1000, 2), (4096, 3), (108, 4096)])
def test_sizes(n, frames):
    """Every kernel shape (wave per frame: 2, 3, 107, 108; workgroup per frame: 1000; tiles: 4096) against the float64 pair
    sum; for the 4096 frames the float64 route takes 5 of them."""
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials
    from mdgrad_amd.thermo import Pressure
    xyz, cell = liquid(n, seed=n, frames=frames)
    if n <= 3:
        cell = np.array([4.0, 4.0, 4.0], dtype=np.float32)
        xyz = (np.random.default_rng(n).uniform(1.2, 2.6, xyz.shape)).astype(np.float32)
    system = mk_system(xyz[0], cell)
    mdl = P.LennardJones(sigma=1.0, epsilon=1.0)
    cutoff = min(2.5, 0.49 * float(cell[0]))
    obs = Pressure(system, PairPotentials(system, mdl, cutoff=cutoff))
    terms = [(mdl, cutoff, None, None)]
    gw = np.random.default_rng(1).uniform(0.5, 1.5, frames).astype(np.float32)
    W, gq, gth = run_gpu(obs, terms, xyz, gw)
    pick = np.arange(frames) if frames <= 3 else np.array([0, 1, 2047, 4094, 4095])
    gw_sub = np.zeros(frames, dtype=np.float32)
    gw_sub[pick] = gw[pick]
    W64, S, rq, rth = route64(xyz[pick], cell, terms, gw[pick], False)
    fwd_close(W[pick], W64, S, 0.0, "N=%d F=%d" % (n, frames))
    if frames > 3:                                    # the parameter gradient is a sum over frames: restrict it to the five
        _, gq, gth = run_gpu(obs, terms, xyz, gw_sub)
        assert float(gq[3].abs().max()) == 0.0        # (a frame of zero weight gets a zero gradient)
    grads_close(gq[pick], gth, rq, rth, "N=%d F=%d" % (n, frames))


def test_no_pair_inside_the_cutoff_gives_exact_zeros():
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials
    from mdgrad_amd.thermo import Pressure
    xyz = np.array([[[0.5, 0.5, 0.5], [3.5, 0.6, 0.4], [0.4, 3.5, 3.6], [3.4, 3.6, 0.5]]] * 2, dtype=np.float32)
    cell = np.array([6.0, 6.0, 6.0], dtype=np.float32)
    system = mk_system(xyz[0], cell)
    mdl = P.Buck(A=1000.0, B=3.5, C=5.0)
    obs = Pressure(system, PairPotentials(system, mdl, cutoff=1.5))
    W, gq, gth = run_gpu(obs, [(mdl, 1.5, None, None)], xyz, np.ones(2, dtype=np.float32))
    assert torch.equal(W, torch.zeros_like(W)) and torch.equal(gq, torch.zeros_like(gq)) and torch.equal(gth, torch.zeros_like(gth))


# ---------------------------------------------------------------------------------------------- 7, 8
@pytest.mark.parametrize("name,n,frames", [("lj", 108, 64), ("stack", 108, 3), ("buck", 300, 4), ("lj", 1500, 2)])
def test_bitwise_repeatable(name, n, frames):
    from mdgrad_amd.interface import PairPotentials
    from mdgrad_amd.thermo import Pressure
    if name == "stack":
        g, _, system, obs, terms = case(name)
        xyz = g["xyz"]
    else:
        xyz, cell = liquid(n, seed=7, frames=frames)
        system, mdl = mk_system(xyz[0], cell), form(name)
        obs, terms = Pressure(system, PairPotentials(system, mdl, cutoff=2.5)), [(mdl, 2.5, None, None)]
    gw = np.linspace(0.5, 1.5, len(xyz)).astype(np.float32)
    a, b = run_gpu(obs, terms, xyz, gw), run_gpu(obs, terms, xyz, gw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_virial_plus_kinetic_reproduces_P_in_any_call_order():
    g, _, system, obs, _ = case("lj69")
    q, v = torch.as_tensor(g["xyz"]).to(DEV), torch.as_tensor(g["vel"]).to(DEV)
    K = obs.kinetic(v)
    W = obs.virial(q)
    P = obs(q, v)
    dV = obs.dim * obs.volume
    assert torch.equal(P, (K + W) / dV) and torch.equal(P, (obs.kinetic(v) + obs.virial(q)) / dV)
    v2 = v.clone().requires_grad_(True)
    (gv,) = torch.autograd.grad(obs(q, v2).sum(), v2)
    close(gv, 2.0 * 1.008 * v / dV, 1e-6, 0.0, "dP/dv = 2 m v / (d V)")


# ---------------------------------------------------------------------------------------------- 9
def test_errors():
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, GNNPotentials, Stack
    from mdgrad_amd.nn import get_model
    from mdgrad_amd.thermo import Pressure
    g, _, system, obs, _ = case("lj")
    pair = PairPotentials(system, P.LennardJones(1.0, 1.0), cutoff=2.5)
    gnn = GNNPotentials(system, get_model({"n_atom_basis": 16, "n_filters": 16, "n_gaussians": 8, "n_convolutions": 1,
                                           "cutoff": 2.5}), cutoff=2.5)
    with pytest.raises(NotImplementedError, match="LennardJones"):
        Pressure(system, Stack({"pair": pair, "gnn": gnn}))
    mlp = P.pairMLP(n_gauss=8, r_start=0.5, r_end=2.5, n_layers=1, n_width=8, nonlinear="ELU")
    with pytest.raises(NotImplementedError, match="Yukawa"):
        Pressure(system, PairPotentials(system, mlp, cutoff=2.5))
    tric = mk_system(g["xyz"][0], np.array([[4.8, 0, 0], [0.6, 4.8, 0], [0, 0, 4.8]]))
    with pytest.raises(ValueError, match="diagonal"):
        Pressure(tric, PairPotentials(tric, P.LennardJones(1.0, 1.0), cutoff=2.0))
    q, v = torch.as_tensor(g["xyz"]).to(DEV), torch.as_tensor(g["vel"]).to(DEV)
    with pytest.raises(ValueError, match="agree"):
        obs(q, v[:2])
    q = q.requires_grad_(True)
    (gq,) = torch.autograd.grad(obs(q, v).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):
        gq.pow(2).sum().backward()


# ---------------------------------------------------------------------------------------------- 10
@pytest.mark.parametrize("name", ["lj", "stack"])
def test_torch_ops_equal_the_ctypes_path(name):
    from mdgrad_amd import _torch_ops
    ns = _torch_ops.get()
    assert ns is not None
    g, pre, system, obs, terms = case(name)
    gw = np.array([0.7, 1.2, 0.9], dtype=np.float32)
    W, gq, gth = run_gpu(obs, terms, g["xyz"], gw)
    q = torch.as_tensor(g["xyz"]).to(DEV)
    theta = torch.cat([p.detach().reshape(-1) for p in params_of(terms)])
    ti, tf = _torch_ops.terms_args(obs._terms)
    cell = _torch_ops.cell_args(obs._cell_struct)
    W_t = ns.virial_fwd(q, cell, ti, tf, obs._masks, theta)
    gq_t, gth_t = ns.virial_bwd(q, cell, ti, tf, obs._masks, theta, torch.as_tensor(gw).to(DEV))
    assert torch.equal(W_t, W) and torch.equal(gq_t, gq) and torch.equal(gth_t, gth)
    with pytest.raises(RuntimeError, match="theta"):
        ns.virial_fwd(q, cell, ti, tf, obs._masks, theta[:1])
