"""Langevin dynamics (md.Langevin, method 'baoab', csrc/langevin.hip) on the device against the float64 reference of
tests/langevin_ref.py.

Tolerances: allowed = 10 x floor.  The floor of a quantity is |float32 restatement - float64| of langevin_ref for the same
fixture (largest entry), at least 2^-24 of the quantity's scale; nothing comes from the code under test.  The scale is the
largest |float64 entry| of the quantity; for dL/dgamma, one number added up from M x 3 x (T - 1) terms of both signs, it is the
sum of their absolute values (langevin_ref.adjoint's A_gamma): a float32 sum is accurate to roundings of what was added, not
of what is left -- the convention of tests/pair_forms_ref.py.  Every comparison prints a FIGURE line (observed, allowed)
before it asserts.

Whole-path references: the Lennard-Jones box is driven by the float64 callables of tests/pair_forms_ref.py (F, H w and
d(w.F)/dtheta of `evaluate`), the silicon cell by tests/sw_ref.py (SWTerm.force_vjp, float64 autograd of the definition);
neither uses the package.

Largest observed / allowed on an MI355X (the FIGURE lines of one run): noise 0.100 (the torch stream in float32, 1.06e-06 /
1.06e-05; the kernel's own largest is 0.100 at n = 5, 2.7e-07 / 2.7e-06); algebra kernels: v_t 0.057, q_t 0.100, dL/dv0
0.071, dL/dq0 0.120, dL/dgamma 0.095 (N = 5; 0.002 at N = 257 on its absolute-sum scale); LJ-108: v_t 0.103 (1.3e-05 /
1.3e-04), q_t 0.100, dL/dv0 0.177, dL/dq0 0.288, dL/dtheta 0.426 (2.7e-04 / 6.4e-04), dL/dgamma 0.003; Si-64: v_t 0.105,
q_t 0.100, dL/dv0 0.075, dL/dq0 0.214, dL/dtheta 0.309, dL/dgamma 0.009.  A ratio of exactly 0.100 means the observed error
equals the float32 floor itself (at the worst entry the device and the restatement differ from float64 alike).  Equipartition: m<v^2>/T 1.006 and
1.017 after 64 steps, 0.0940 and 0.0974 after one step (wanted 0.0952), bound 0.090 relative."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import langevin_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
ULP = 2.0 ** -24
T_GRID = np.array([0.0, 0.1, 0.25, 0.3, 0.4, 0.55])                    # 6 frames, uneven; float32 rounds them once


def t32(t=T_GRID):
    return np.asarray(t, F32)


def figure(what, got, ref64, ref32, scale=None):
    """observed = max |got - ref64| against allowed = 10 max(|ref32 - ref64|, 2^-24 scale); scale = max |ref64| unless the
    quantity is a sum whose terms cancel: then the sum of their absolute values (langevin_ref.adjoint's A_gamma)."""
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref64, ref32 = np.asarray(ref64, np.float64), np.asarray(ref32, np.float64)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert np.isfinite(got).all(), what + ": non-finite"
    scale = (float(np.abs(ref64).max()) if ref64.size else 0.0) if scale is None else float(scale)
    floor = max(float(np.abs(ref32 - ref64).max()) if ref64.size else 0.0, ULP * scale)
    obs = float(np.abs(got - ref64).max()) if ref64.size else 0.0
    print("FIGURE %-58s observed %.3e  allowed %.3e  (observed/allowed %.3f, scale %.3e)" % (what, obs, 10 * floor, obs / (10 * floor) if floor else 0.0, scale))
    assert obs <= 10 * floor, "%s: observed %.3e > allowed %.3e" % (what, obs, 10 * floor)


def mk_system(pos, cell, vel=None, mass=None):
    from mdgrad_amd.system import System
    s = System(positions=np.asarray(pos, np.float64), cell=np.asarray(cell, np.float64),
               masses=np.asarray(mass, np.float64) if mass is not None else np.ones(len(pos)), device=DEV)
    if vel is not None:
        s.set_velocities(np.asarray(vel, np.float64))
    return s


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, F32))).to(DEV)


# ------------------------------------------------------------------------------------------------ the stream
BIG_SEED = 2 ** 32 + 12345


@pytest.mark.parametrize("n", [1, 5, 257, 4096])
def test_noise_kernel_matches_the_reference_stream(n):
    from mdgrad_amd import ops
    for seed, step in ((BIG_SEED, 0), (BIG_SEED, 1), (BIG_SEED, 2 ** 32 + 3), (7, 2 ** 32 + 3)):
        xi = ops.lgv_noise(seed, step, n, DEV)
        figure("xi n=%d seed=%d step=%d" % (n, seed, step), xi, R.normals(seed, step, n), R.normals(seed, step, n, F32))
    # the torch stream of the fallback path, on the device: the same integers
    figure("torch xi on the device n=%d" % n, ops.lgv_noise_torch(BIG_SEED, 2 ** 32 + 3, n, torch.float32, DEV),
           R.normals(BIG_SEED, 2 ** 32 + 3, n), R.normals(BIG_SEED, 2 ** 32 + 3, n, F32))


# ------------------------------------------------------------------------------------------------ algebra kernels alone
TEMP, GAMMA, SEED, STEP0 = 0.8, 1.7, 11, 2 ** 32 - 2                  # (the step counter crosses 2^32 inside the run)


def _algebra_case(n, n_rep=1):
    """A harmonic model with a stiffness per atom, F = -k q, H w = -k w: the test itself supplies the force and dwF buffers."""
    rng = np.random.default_rng(100 + n)
    N = n * n_rep
    mass = np.tile(np.where(np.arange(n) % 2 == 0, 1.0, 4.0), n_rep)
    kk = rng.uniform(0.5, 2.0, (N, 1)).astype(F32).astype(np.float64)
    v0, q0 = rng.normal(size=(N, 3)).astype(F32), rng.normal(size=(N, 3)).astype(F32)
    g_v, g_q = rng.normal(size=(len(T_GRID), N, 3)).astype(F32), rng.normal(size=(len(T_GRID), N, 3)).astype(F32)
    return N, mass, kk, v0, q0, g_v, g_q


def _algebra_integ(n, n_rep, mass, q0):
    from mdgrad_amd.md import Langevin
    system = mk_system(q0[:n], [50.0] * 3, mass=mass[:n])
    if n_rep > 1:
        system = system.replicate(n_rep)
    integ = Langevin(torch.nn.Module(), system, TEMP, float(F32(GAMMA)), seed=SEED, trainable_gamma=True).to(DEV)
    integ.reseed(SEED, STEP0)
    return integ


@pytest.mark.parametrize("n,n_rep", [(5, 1), (257, 1), (5, 3)], ids=["n5", "n257", "3x5"])
def test_algebra_kernels_forward_and_adjoint(n, n_rep):
    from mdgrad_amd import ops
    N, mass, kk, v0, q0, g_v, g_q = _algebra_case(n, n_rep)
    integ = _algebra_integ(n, n_rep, mass, q0)
    gam = float(F32(GAMMA))
    F = lambda q: (-kk.astype(q.dtype) * q)
    Hw = lambda q, w: (-kk.astype(w.dtype) * w)
    Pw = lambda q, w: np.zeros(0, w.dtype)
    ref = [R.forward(F, v0, q0, t32(), mass, TEMP, gam, SEED, STEP0, dt) for dt in (np.float64, F32)]
    # ---- forward: kick / finish with the force buffers handed in
    Tn = len(T_GRID)
    kd = dev(kk)
    v, q = dev(v0), dev(q0)
    t = dev(t32())
    out = [torch.zeros(Tn, N, 3, device=DEV), torch.zeros(Tn, N, 3, device=DEV)]
    out[0][0], out[1][0] = v, q
    w = ops.LgvWork(integ, v)
    w.set_rng(SEED, STEP0)
    k = torch.zeros(1, dtype=torch.int64, device=DEV)
    f = (-kd * q).contiguous()
    for s in range(Tn - 1):
        qn = w.kick(v, q, f, t, k)
        w.finish(v, q, f, (-kd * qn).contiguous(), t, k, out, advance=True)
        assert int(k) == s + 1
    figure("algebra forward v_t N=%d" % N, out[0], ref[0][0], ref[1][0])
    figure("algebra forward q_t N=%d" % N, out[1], ref[0][1], ref[1][1])
    # ---- adjoint over the REFERENCE's frames (float32 copies), the dwF buffers handed in
    v_t, q_t = ref[0][0].astype(F32), ref[0][1].astype(F32)
    adj = [R.adjoint(F, Hw, Pw, v_t, q_t, g_v, g_q, t32(), mass, TEMP, gam, SEED, STEP0, dt) for dt in (np.float64, F32)]
    ans, gout = [dev(v_t), dev(q_t)], [dev(g_v), dev(g_q)]
    lam = [gout[0][-1].clone(), gout[1][-1].clone()]
    i = torch.full((1,), Tn - 1, dtype=torch.int64, device=DEV)
    w.gpart.zero_()
    qi, wv = w.adj_pre(ans, lam[0], t, i)
    for s in range(Tn - 1, 0, -1):
        assert torch.equal(qi, ans[1][s])
        qi, wv = w.adj_step(ans, lam, (-kd * qi).contiguous(), (-kd * wv).contiguous(), t, i, gout, want_gamma=True, advance=True)
        assert int(i) == s - 1
    lam[1] += -kd * wv
    figure("algebra adjoint dL/dv0 N=%d" % N, lam[0], adj[0][0], adj[1][0])
    figure("algebra adjoint dL/dq0 N=%d" % N, lam[1], adj[0][1], adj[1][1])
    gb = w.gamma_bar()
    figure("algebra adjoint dL/dgamma N=%d" % N, gb.reshape(()), adj[0][3], adj[1][3], scale=adj[0][4])
    assert torch.equal(gb, w.gamma_bar()), "the friction gradient is a fixed-order sum"
    assert int(w.ticket) == 0


def _zero_force_run(gamma_h, steps, v0=None):
    """N = 4096 atoms of alternating mass 1 and 4 under a zero force buffer; m <v^2> / T per species after `steps` steps."""
    from mdgrad_amd import ops
    from mdgrad_amd.md import Langevin
    N, T = 4096, 0.7
    mass = np.where(np.arange(N) % 2 == 0, 1.0, 4.0)
    system = mk_system(np.zeros((N, 3)), [50.0] * 3, mass=mass)
    h = 0.25
    integ = Langevin(torch.nn.Module(), system, T, gamma_h / h, seed=2024).to(DEV)
    v, q, f = torch.zeros(N, 3, device=DEV), torch.zeros(N, 3, device=DEV), torch.zeros(N, 3, device=DEV)
    t = dev(np.arange(steps + 1) * h)
    out = [torch.zeros(steps + 1, N, 3, device=DEV) for _ in range(2)]
    w = ops.LgvWork(integ, v)
    w.set_rng(2024, 0)
    k = torch.zeros(1, dtype=torch.int64, device=DEV)
    for _ in range(steps):
        w.kick(v, q, f, t, k)
        w.finish(v, q, f, f, t, k, out, advance=True)
    m = torch.as_tensor(mass, dtype=torch.float32, device=DEV)[:, None]
    e = (m * v * v / T).cpu().double()
    return float(e[0::2].mean()), float(e[1::2].mean())


def test_equipartition_and_relaxation_on_the_device():
    bound = 5 * np.sqrt(2 / 6144)                                      # 6144 samples per species
    for name, gh, steps, want in (("equilibrium", 0.5, 64, 1.0), ("one step from rest", 0.05, 1, 1 - np.exp(-0.1))):
        for species, got in zip(("m=1", "m=4"), _zero_force_run(gh, steps)):
            print("FIGURE m<v^2>/T %s %s: %.4f, wanted %.4f within %.4f (relative)" % (name, species, got, want, bound))
            assert abs(got / want - 1) <= bound, (name, species, got)


# ------------------------------------------------------------------------------------------------ whole path, real models
class _LJ:
    """PairPotentials(LennardJones) on the 108-atom jittered fcc box (4.8 cell) of pair_forms_ref.liquid."""
    gamma, temp, seed, step0 = 2.0, 1.0, 5, 17

    def __init__(self):
        import pair_forms_ref as P
        self.P = P
        self.fx = P.liquid(108)
        self.terms = [P.Term("lj", 2.5)]
        rng = np.random.default_rng(42)
        self.mass = np.where(np.arange(108) % 2 == 0, 1.0, 4.0)
        self.v0 = (rng.normal(size=(108, 3)) * np.sqrt(self.temp / self.mass)[:, None]).astype(F32)
        self.q0 = self.fx.x
        self.t = t32(T_GRID * 0.05)
        self.n_theta = 2

    def callables(self, dt):
        P, cell, terms = self.P, self.fx.cell, self.terms
        ev = lambda q, w: P.evaluate(q, w, cell, terms, dtype=dt)        # noqa: E731
        return (lambda q: ev(q, np.zeros_like(q)).F), (lambda q, w: ev(q, w).dq), (lambda q, w: ev(q, w).dth[0])

    def integrator(self):
        from mdgrad_amd.interface import PairPotentials
        from mdgrad_amd.md import Langevin
        from mdgrad_amd.potentials import LennardJones
        th = self.terms[0].theta
        system = mk_system(self.q0, self.fx.cell, self.v0, self.mass)
        pair = PairPotentials(system, LennardJones(sigma=th[0], epsilon=th[1]), cutoff=2.5)
        integ = Langevin(pair, system, self.temp, self.gamma, seed=self.seed, trainable_gamma=True).to(DEV)
        return integ, [pair.model.sigma, pair.model.epsilon]


class _SW:
    """Stack(StillingerWeber.silicon) on the 64-atom jittered diamond cell of sw_ref."""
    gamma, temp, seed, step0 = 5.0, 0.05, 9, 3

    def __init__(self):
        import sw_ref as S
        self.S = S
        self.q0, self.cell = S.jittered_diamond(2, 5.431, 0.15, 71)
        self.mass = np.where(np.arange(64) % 2 == 0, 2.0, 4.0)
        rng = np.random.default_rng(710)
        self.v0 = (rng.normal(size=(64, 3)) * np.sqrt(self.temp / self.mass)[:, None]).astype(F32)
        self.t = t32(T_GRID * 0.1)
        self.n_theta = 3
        self.theta32 = [float(F32(S.SILICON[k])) for k in ("epsilon", "sigma", "lam")]

    def callables(self, dt):
        S = self.S
        term = S.SWTerm(*self.theta32, self.cell)
        term.theta = torch.tensor(self.theta32, dtype=torch.float64)
        tdt = torch.float64 if dt == np.float64 else torch.float32
        last = {}

        def both(q, w):
            key = (q.tobytes(), w.tobytes())
            if last.get("key") != key:
                qq = torch.as_tensor(np.ascontiguousarray(q)).to(tdt)
                term.reset(qq)
                last["key"], last["out"] = key, [x.numpy().astype(dt) for x in term.force_vjp(qq, torch.as_tensor(np.ascontiguousarray(w)).to(tdt))]
            return last["out"]
        return (lambda q: both(q, np.zeros_like(q))[0]), (lambda q, w: both(q, w)[1]), (lambda q, w: both(q, w)[2])

    def integrator(self):
        from mdgrad_amd.interface import Stack, StillingerWeber
        from mdgrad_amd.md import Langevin
        system = mk_system(self.q0, self.cell, self.v0, self.mass)
        sw = StillingerWeber.silicon(system)
        integ = Langevin(Stack({"sw": sw}), system, self.temp, self.gamma, seed=self.seed, trainable_gamma=True).to(DEV)
        return integ, [sw.epsilon, sw.sigma, sw.lam]


_REF = {}


def _whole_path_reference(case):
    """(forward64, forward32, adjoint64, adjoint32, g_v, g_q) of a case: computed once, shared, never written to."""
    name = type(case).__name__
    if name not in _REF:
        Tn, N = len(case.t), len(case.q0)
        rng = np.random.default_rng(8)
        g_v, g_q = rng.normal(size=(Tn, N, 3)).astype(F32), rng.normal(size=(Tn, N, 3)).astype(F32)
        gam = float(F32(case.gamma))
        fwd, adj = [], []
        for dt in (np.float64, F32):
            F, Hw, Pw = case.callables(dt)
            fwd.append(R.forward(F, case.v0, case.q0, case.t, case.mass, case.temp, gam, case.seed, case.step0, dt))
            adj.append(R.adjoint(F, Hw, Pw, fwd[0][0].astype(F32), fwd[0][1].astype(F32), g_v, g_q, case.t, case.mass, case.temp, gam,
                                 case.seed, case.step0, dt))
        _REF[name] = (fwd[0], fwd[1], adj[0], adj[1], g_v, g_q)
    return _REF[name]


def _run(integ, case, g_v, g_q, graphs_on=True):
    from mdgrad_amd.sovlers import odeint_adjoint
    integ.use_graphs = graphs_on
    integ.reseed(case.seed, case.step0)
    for p in integ.parameters():
        p.grad = None
    y0 = [dev(case.v0).requires_grad_(True), dev(case.q0).requires_grad_(True)]
    v_t, q_t = odeint_adjoint(integ, tuple(y0), dev(case.t), method="baoab")
    ((dev(g_v) * v_t).sum() + (dev(g_q) * q_t).sum()).backward()
    return v_t.detach(), q_t.detach(), y0[0].grad, y0[1].grad


@pytest.mark.parametrize("case_cls", [_LJ, _SW], ids=["lj108", "sw64"])
def test_whole_path_against_the_float64_reference(case_cls):
    """Trajectory, dL/dy0, dL/dtheta and dL/dgamma of 6 frames through odeint_adjoint(method='baoab') with graph replay.  The
    adjoint of the reference runs over the float32 copy of ITS OWN frames, the device's over the device's frames: the
    difference of the two trajectories is part of what is compared."""
    from mdgrad_amd import graphs
    case = case_cls()
    f64, f32, a64, a32, g_v, g_q = _whole_path_reference(case)
    integ, thetas = case.integrator()
    assert integ.fused_spec("baoab") is None and graphs.enabled(integ)
    calls = {"n": 0}
    orig = integ.model.force_vjp

    def counted(*a, **k):
        calls["n"] += 1
        return orig(*a, **k)
    integ.model.force_vjp = counted
    v_t, q_t, gv0, gq0 = _run(integ, case, g_v, g_q, graphs_on=False)
    assert calls["n"] == len(case.t), "T force-vjp evaluations for T - 1 intervals"
    tag = type(case).__name__
    figure(tag + " v_t", v_t, f64[0], f32[0])
    figure(tag + " q_t", q_t, f64[1], f32[1])
    figure(tag + " dL/dv0", gv0, a64[0], a32[0])
    figure(tag + " dL/dq0", gq0, a64[1], a32[1])
    figure(tag + " dL/dtheta", torch.cat([p.grad.reshape(-1) for p in thetas]), a64[2], a32[2])
    figure(tag + " dL/dgamma", integ.gamma.grad.reshape(()), a64[3], a32[3], scale=a64[4])


# ------------------------------------------------------------------------------------------------ reproducibility
def test_graph_replay_equals_eager_and_follows_seed_and_temperature():
    from mdgrad_amd import graphs
    case = _LJ()
    case.t = case.t[:5]                                                # 5 frames: the smallest that replays
    rng = np.random.default_rng(3)
    g_v, g_q = rng.normal(size=(5, 108, 3)).astype(F32), rng.normal(size=(5, 108, 3)).astype(F32)
    integ, thetas = case.integrator()
    captures = {"n": 0}
    orig = graphs._capture

    def counting(*a, **k):
        captures["n"] += 1
        return orig(*a, **k)
    graphs._capture = counting
    try:
        def both():
            outs = []
            for on in (True, False):
                r = _run(integ, case, g_v, g_q, graphs_on=on)
                outs.append(list(r) + [p.grad.clone() for p in integ.parameters()])
            for a, b, nm in zip(outs[0], outs[1], ("v_t", "q_t", "dL/dv0", "dL/dq0", "dL/dgamma", "dL/dsigma", "dL/depsilon")):
                assert torch.equal(a, b), "graph replay differs from the eager path: " + nm
            return outs[0]
        first = both()
        assert captures["n"] == 2, "one forward and one adjoint graph"
        again = both()
        for a, b in zip(first, again):
            assert torch.equal(a, b), "two runs with one seed differ"
        case.seed = 6
        other_seed = both()
        assert not torch.equal(other_seed[0], first[0])
        integ.T = 2.0 * case.temp
        hot = both()
        assert not torch.equal(hot[0], other_seed[0])
        assert captures["n"] == 2, "a new seed or temperature must not rebuild the graphs"
    finally:
        graphs._capture = orig


def test_two_epochs_equal_one_long_integration():
    from mdgrad_amd.md import Simulations
    from mdgrad_amd.sovlers import odeint_adjoint
    case = _LJ()
    dt, f = 2.0 ** -8, 4                                               # a power of two: every t[k] and every h is exact
    integ, _ = case.integrator()
    integ.reseed(case.seed, case.step0)
    sim = Simulations(integ.system, integ, wrap=False, method="baoab")
    v_t, q_t = sim.simulate(steps=2 * f, frequency=f, dt=dt)
    first = [sim.log[k][0] for k in ("velocities", "positions")]
    assert integ.step0 == case.step0 + 2 * (f - 1)
    integ2, _ = case.integrator()
    integ2.reseed(case.seed, case.step0)
    y0 = integ2.get_inital_states(wrap=False)
    t = torch.Tensor([dt * k for k in range(2 * f - 1)]).to(DEV)
    lv, lq = odeint_adjoint(integ2, tuple(y0), t, method="baoab")
    assert np.array_equal(first[0], lv[f - 1].detach().cpu().numpy()) and np.array_equal(first[1], lq[f - 1].detach().cpu().numpy())
    assert torch.equal(v_t.detach(), lv[f - 1:].detach()) and torch.equal(q_t.detach(), lq[f - 1:].detach())
