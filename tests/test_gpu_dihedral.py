"""K19: the torsion term (DihedralPotentials, mdg_dihedral_eval) and the dihedral observables (Dihedrals, dihedral_distribution)
as HIP kernels (csrc/dihedral.hip) against the reference's goldens D1 / D2 (tests/golden/make_dihedral_goldens.py), the float64
definitions of tests/dihedral_ref.py (pinned to the same goldens by tests/test_dihedral_host.py) and, in a polymer Stack, the
CPU oracle's trajectory and adjoint."""
import math

import numpy as np
import pytest
import torch

import dihedral_ref as R
import oracle as O
from conftest import load_golden
from test_gpu_parity import T, close, mk_system, DEV, oracle_run

pytestmark = pytest.mark.gpu
F32 = np.float32


def _wrapped_d2():
    g = load_golden("dihedral_d2")
    L = g["cell"].astype(np.float64)
    wrapped = np.mod(g["pos"].astype(np.float64), L).astype(F32)
    assert int((np.abs(np.diff(wrapped, axis=0)) >= 0.5 * L).any(1).sum()) >= 3, "imaging must be exercised"
    return g, wrapped, L


def _rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


# ------------------------------------------------------------------------------------------------ 1: term kernel vs D2
def test_term_kernel_energy_force_hvp_and_parameter_gradients_golden():
    """One launch of mdg_dihedral_eval on the wrapped chain: U, F = -dU/dx, d(w.F)/dx = -H w and d(w.F)/dA against the
    reference (D2: autograd and double autograd of the polynomial on compute_dihe, float64); the same through autograd
    (TermEnergyFn -> TermGradFn on ops.DihedralTerm) with dU/dA, added onto another member's buffers, and bitwise reproducible."""
    from mdgrad_amd import ops
    from mdgrad_amd.interface import DihedralPotentials
    g, wrapped, L = _wrapped_d2()
    system = mk_system(wrapped, L)
    mod = DihedralPotentials(system, torch.as_tensor(g["dihes"].astype(np.int64)), torch.tensor(g["coeffs"], dtype=torch.float32),
                             types=torch.as_tensor(g["types"].astype(np.int64)))
    assert mod.supports_force_vjp() and mod.supports_static_topology() and mod.coeffs.requires_grad
    q, w = T(wrapped, DEV), T(g["w"], DEV)
    fmax, hmax = float(np.abs(g["force"]).max()), float(np.abs(g["hw"]).max())
    umax, wmax = float(np.abs(g["dU_dA"]).max()), float(np.abs(g["dwF_dA"]).max())
    close(mod(q).reshape(1), g["energy"], 1e-5, 1e-5, "energy")
    close(mod.force(q), g["force"], 1e-4, 1e-5 * fmax, "force")
    F, dq, gth = mod.force_vjp(q, w)
    assert len(gth) == 1 and gth[0].shape == mod.coeffs.shape
    close(F, g["force"], 1e-4, 1e-5 * fmax, "force (vjp launch)")
    close(-dq, g["hw"], 1e-4, 2e-5 * hmax, "H.w")
    close(gth[0], g["dwF_dA"], 1e-4, 2e-5 * wmax, "d(w.F)/dA")
    assert mod.force_vjp(q, w, want_theta=False)[2] is None
    # autograd route: first and second order, in the positions and the coefficients
    x = q.clone().requires_grad_(True)
    gq, gA = torch.autograd.grad(mod(x), (x, mod.coeffs), create_graph=True)
    close(-gq, g["force"], 1e-4, 1e-5 * fmax, "force (autograd)")
    close(gA, g["dU_dA"], 1e-4, 2e-5 * umax, "dU/dA (autograd)")
    hw, hA = torch.autograd.grad((gq * w).sum(), (x, mod.coeffs))
    close(hw, g["hw"], 1e-4, 2e-5 * hmax, "H.w (double autograd)")
    close(-hA, g["dwF_dA"], 1e-4, 2e-5 * wmax, "d(w.F)/dA (double autograd)")
    # accumulation onto existing buffers (Stack.force / force_vjp hand the running sums down)
    F0, D0 = torch.randn_like(q), torch.randn_like(q)
    F1, D1, _ = mod.force_vjp(q, w, into=(F0.clone(), D0.clone()))
    close(F1 - F0, g["force"], 1e-4, 1e-5 * fmax + 1e-6, "force added onto a buffer")
    close(-(D1 - D0), g["hw"], 1e-4, 2e-5 * hmax + 1e-6, "H.w added onto a buffer")
    acc = ops.ThetaAccum(list(mod.parameters()))
    acc.flat.fill_(0.25)
    assert mod.force_vjp(q, w, accum=acc)[2] is None
    close(acc.flat.reshape(2, 5) - 0.25, g["dwF_dA"], 1e-4, 2e-5 * wmax + 1e-6, "d(w.F)/dA added into a ThetaAccum")
    # two launches are bitwise equal
    two = ops.dihedral_eval(mod.table(), q, mod.coeffs, w=w, terms=True)
    gw2 = ops.dihedral_coeff_grad(mod.table(), two["c_term"], two["cd_term"], want_u=False)[1]
    assert torch.equal(two["grad"], -F) and torch.equal(two["hw"], -dq) and torch.equal(-gw2, gth[0]), "two launches are bitwise equal"


# ------------------------------------------------------------------------------------------------ 2: incidence edge cases
def _eval_vs_ref(pos, top, types, coeffs, L, n_atoms, tag):
    from mdgrad_amd import ops
    rng = np.random.default_rng(len(tag))
    w = rng.normal(0, 1, pos.shape).astype(F32)
    tab = ops.DihedralTable(top, n_atoms, list(L), DEV, types=types, n_types=coeffs.shape[0])
    o = ops.dihedral_eval(tab, T(pos.astype(F32), DEV), T(coeffs.astype(F32), DEV), w=T(w, DEV), energy=True, terms=True)
    gu, gw = ops.dihedral_coeff_grad(tab, o["c_term"], o["cd_term"])
    x = torch.tensor(pos.astype(F32)).double().requires_grad_(True)
    A = torch.tensor(coeffs.astype(F32)).double().requires_grad_(True)
    U = R.energy(x, top, A, types, L)
    gq, gA = torch.autograd.grad(U, (x, A), create_graph=True)
    hq, hA = torch.autograd.grad((gq * torch.tensor(w).double()).sum(), (x, A))
    fmax, hmax = float(gq.detach().abs().max()), float(hq.abs().max())
    close(o["e_atom"].sum().reshape(1), U.detach().reshape(1), 1e-5, 1e-5, tag + " energy")
    close(o["grad"], gq.detach(), 1e-4, 1e-5 * fmax, tag + " dU/dx")
    close(o["hw"], hq, 1e-4, 2e-5 * hmax, tag + " H.w")
    close(gu, gA.detach(), 1e-4, 2e-5 * float(gA.detach().abs().max()), tag + " dU/dA")
    close(gw, hA, 1e-4, 2e-5 * float(hA.abs().max()), tag + " d(w.dU/dx)/dA")
    c64 = R.cos_phi(x.detach(), top, L)
    close(o["c_term"], c64, 0, 1e-6, tag + " cos phi per term")
    return o


def test_incidence_list_edge_cases_vs_float64():
    """A 7-atom chain (+ 1 free atom) with all four dihedrals and the reversed row (6, 5, 4, 3): atoms with 0, 1 and 5
    incidences and every role; and 75 disjoint 4-atom molecules (300 atoms: a second, partly filled workgroup)."""
    coeffs = np.array([[0.3, -1.1, 0.8, 0.5, -0.4], [0.1, 0.7, -0.2, 0.0, 0.3]])
    L = np.array([30.0, 30.0, 30.0])
    pos = np.concatenate([R.random_chain(7, 3), [[9.0, 9.0, 9.0]]])
    top = np.array([[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5], [3, 4, 5, 6], [6, 5, 4, 3]])
    o = _eval_vs_ref(pos, top, np.array([0, 1, 0, 1, 1]), coeffs, L, 8, "chain7")
    assert float(o["grad"][7].abs().max()) == 0.0 and float(o["hw"][7].abs().max()) == 0.0 and float(o["e_atom"][7]) == 0.0
    assert float(o["c_term"][3]) == float(o["c_term"][4]), "a reversed row has the same cosine"
    rng = np.random.default_rng(75)
    mols = np.concatenate([R.random_chain(4, 100 + m, start=rng.uniform(2, 28, 3)) for m in range(75)])
    top = np.arange(300).reshape(75, 4)
    assert 300 % 256 != 0
    _eval_vs_ref(np.mod(mols, L), top, np.arange(75) % 2, coeffs, L, 300, "molecules75")


# ------------------------------------------------------------------------------------------------ 3: degenerate terms
def test_degenerate_terms_are_skipped_everywhere():
    """x_0, x_1, x_2 collinear in exactly representable coordinates: every output is finite, the term's contributions are
    exactly zero, and the regular second term of the table is bitwise what it is alone."""
    from mdgrad_amd import ops
    from mdgrad_amd.observable import Dihedrals, dihedral_distribution
    pos = np.array([[0.5, 0.5, 0.5], [1.0, 0.5, 0.5], [1.5, 0.5, 0.5], [1.5, 1.0, 1.0], [2.0, 1.5, 0.5], [2.5, 1.0, 1.5]], dtype=F32)
    L = [8.0, 8.0, 8.0]
    q, w = T(pos, DEV), T(np.random.default_rng(1).normal(0, 1, pos.shape).astype(F32), DEV)
    A = T(np.array([0.3, -1.1, 0.8, 0.5, -0.4], dtype=F32), DEV)
    both = ops.DihedralTable([[0, 1, 2, 3], [2, 3, 4, 5]], 6, L, DEV)
    alone = ops.DihedralTable([[2, 3, 4, 5]], 6, L, DEV)
    a = ops.dihedral_eval(both, q, A, w=w, energy=True, terms=True)
    b = ops.dihedral_eval(alone, q, A, w=w, energy=True, terms=True)
    for k in ("e_atom", "grad", "hw"):
        assert bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k]), k
    assert float(a["grad"][:2].abs().max()) == 0.0 and float(a["hw"][:2].abs().max()) == 0.0 and float(a["e_atom"][0]) == 0.0
    assert float(a["c_term"][0]) == 2.0 and float(a["cd_term"][0]) == 0.0 and torch.equal(a["c_term"][1:], b["c_term"])
    ga, gb = ops.dihedral_coeff_grad(both, a["c_term"], a["cd_term"]), ops.dihedral_coeff_grad(alone, b["c_term"], b["cd_term"])
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1]) and float(ga[0][0, 0]) == 1.0
    system = mk_system(pos, np.array(L))
    x = q[None].clone().requires_grad_(True)
    obs, one = Dihedrals(system, [[0, 1, 2, 3], [2, 3, 4, 5]]), Dihedrals(system, [[2, 3, 4, 5]])
    phi, cos = obs(x), obs.cos(x)
    assert phi.shape == (1, 2) and float(phi[0, 0]) == 0.0 and float(cos[0, 0]) == 0.0
    assert torch.equal(phi[:, 1:], one(q[None])) and torch.equal(cos[:, 1:], one.cos(q[None]))
    (gx,) = torch.autograd.grad(phi.sum() * 0.7 + cos.sum() * 1.3, x)
    assert bool(torch.isfinite(gx).all()) and float(gx[0, :2].abs().max()) == 0.0 and float(gx[0, 2:].abs().max()) > 0.0
    d2, d1 = dihedral_distribution(system, [[0, 1, 2, 3], [2, 3, 4, 5]], 36), dihedral_distribution(system, [[2, 3, 4, 5]], 36)
    x2 = q[None].clone().requires_grad_(True)
    c2 = d2(x2)[1]
    assert torch.equal(c2, d1(q[None])[1]) and abs(float(c2.sum()) - 1.0) < 1e-5, "a skipped term carries no histogram weight"
    (g2,) = torch.autograd.grad(c2[:18].sum(), x2)
    assert bool(torch.isfinite(g2).all()) and float(g2[0, :2].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 4: phi, cos phi, gradient
def _phi_case(frames32, top, L, tag, d1=None):
    """phi / cos phi of the kernels against float64 on the same float32 frames, and the gradient of a random linear
    functional of both.  Allowed (from D1: the reference's own float32 compute_dihe is err32 off its float64 run, and
    float32 summation order differs): cos 10 err32, phi 10 err32 / (the smallest |sin phi| of the input)."""
    from mdgrad_amd.observable import Dihedrals
    g1 = load_golden("dihedral_d1")
    err32 = float(g1["err32"])
    obs = Dihedrals(mk_system(frames32[0], L), top)
    x = T(frames32, DEV).requires_grad_(True)
    phi, cos = obs(x), obs.cos(x)
    x64 = torch.tensor(frames32).double().requires_grad_(True)
    c64, p64, ok = R.geometry(x64, top, L)
    assert bool(ok.all()) and phi.shape == p64.shape
    min_sin = float(p64.detach().sin().abs().min())
    if d1 is not None:
        close(cos, d1, 0, 10 * err32, tag + " cos phi vs D1 (reference, float64)")
    close(cos, c64.detach(), 0, 10 * err32, tag + " cos phi vs float64")
    close(phi, p64.detach(), 0, 10 * err32 / min_sin, tag + " phi vs float64")
    rng = np.random.default_rng(phi.numel())
    a, b = rng.normal(0, 1, phi.shape), rng.normal(0, 1, phi.shape)
    (gx,) = torch.autograd.grad((phi * T(a.astype(F32), DEV)).sum() + (cos * T(b.astype(F32), DEV)).sum(), x)
    (g64,) = torch.autograd.grad((p64 * torch.tensor(a.astype(F32)).double()).sum() + (c64 * torch.tensor(b.astype(F32)).double()).sum(), x64)
    close(gx, g64, 1e-4, 1e-5 * float(g64.abs().max()), tag + " gradient of a linear functional of phi and cos phi")
    # each output alone (the other cotangent absent)
    (gp,) = torch.autograd.grad(obs(x).sum(), x)
    (gp64,) = torch.autograd.grad(R.phi(x64, top, L).sum(), x64)
    close(gp, gp64, 1e-4, 1e-5 * float(gp64.abs().max()), tag + " gradient of sum phi")


def test_phi_and_cos_147_terms_vs_d1_and_float64():
    """7 frames x 21 terms = 147 (not a multiple of 64): the five frames of D1 and two more jittered ones, wrapped into the
    cell (compared with float64 on the wrapped float32 frames), and the five frames of D1 as stored against D1 itself.
    Observed on an MI355X (MDG_TEST_REPORT), observed / allowed: wrapped frames cos phi 5.6e-07 / 1.0e-06, phi 5.6e-07 / 2.4e-04
    (D1 holds a term with |sin phi| = 4.2e-3), gradient 1.0e-05 / 5.0e-03 at its worst entry; D1's own frames cos phi 1.3e-07 /
    1.0e-06 against the reference's float64 run, phi 2.4e-07 / 2.4e-04."""
    g = load_golden("dihedral_d1")
    L = g["cell"].astype(np.float64)
    rng = np.random.default_rng(147)
    extra = np.stack([g["xyz"][0].astype(np.float64) + rng.normal(0, 0.05, (24, 3)) for _ in range(2)])
    frames = np.concatenate([g["xyz"].astype(np.float64), extra])
    wrapped = np.mod(frames, L).astype(F32)
    # (wrapping in float32 rounds the coordinates: the frames of D1 are compared through the float64 of the wrapped ones)
    assert frames.shape[0] * 21 == 147
    _phi_case(wrapped, g["dihes"].astype(np.int64), L, "7x21", d1=None)
    _phi_case(g["xyz"], g["dihes"].astype(np.int64), np.array([60.0, 60.0, 60.0]), "5x21 unwrapped", d1=g["cos64"])


def test_phi_and_cos_13_frames_of_61_terms_vs_float64():
    """A 64-bead chain (61 dihedrals), 13 jittered frames wrapped into a box of 7: 793 terms, 832 atoms -- several
    workgroups, the last partly filled.  Observed on an MI355X, observed / allowed: cos phi 2.5e-07 / 1.0e-06, phi 6.0e-07 /
    2.0e-04, gradient 2.4e-06 / 1.0e-03 at its worst entry."""
    x0 = R.random_chain(64, 61)
    L = np.array([7.0, 7.0, 7.0])
    rng = np.random.default_rng(13)
    frames = np.mod(np.stack([x0 + rng.normal(0, 0.05, x0.shape) for _ in range(13)]), L).astype(F32)
    top = np.array([[i, i + 1, i + 2, i + 3] for i in range(61)])
    _phi_case(frames, top, L, "13x61")


def test_phi_gradient_is_finite_and_correct_near_0_and_pi():
    """Hand-built terms at phi = +-(pi - 1e-3) and |phi| = 1e-3 (three 4-atom molecules, and their mirror images in a second
    frame): x_j = 0, x_k = e_z, x_i = e_x, x_l = x_k + (cos a, sin a, 0).  float32 coordinates of order 1 carry 6e-8, a
    dihedral of bonds at right angles moves by a few times that: 5e-6 allowed for phi and cos phi; the gradient like the forces
    (rtol 1e-4, 1e-5 of the largest entry)."""
    from mdgrad_amd.observable import Dihedrals
    def mol(a, shift):
        return np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [math.cos(a), math.sin(a), 1.0]]) + shift
    angles = [math.pi - 1e-3, 1e-3, 2.0]
    f0 = np.concatenate([mol(a, np.array([2.0 + 3 * m, 2.0, 2.0])) for m, a in enumerate(angles)])
    f1 = np.concatenate([mol(-a, np.array([2.0 + 3 * m, 2.0, 2.0])) for m, a in enumerate(angles)])
    frames = np.stack([f0, f1]).astype(F32)
    top, L = np.arange(12).reshape(3, 4), np.array([12.0, 12.0, 12.0])
    x64 = torch.tensor(frames).double().requires_grad_(True)
    c64, p64, ok = R.geometry(x64, top, L)
    assert bool(ok.all())
    want = np.array([angles, [-a for a in angles]])
    # (the float32 coordinates move the two small angles by up to ~2e-4: still 1e-3 from 0 and pi to within a fifth)
    assert np.abs(np.abs(p64.detach().numpy()) - np.abs(want)).max() < 5e-4 and (np.sign(p64.detach().numpy()[0]) == -np.sign(p64.detach().numpy()[1])).all()
    obs = Dihedrals(mk_system(frames[0], L), top)
    x = T(frames, DEV).requires_grad_(True)
    phi, cos = obs(x), obs.cos(x)
    close(phi, p64.detach(), 0, 5e-6, "phi near 0 and +-pi")
    close(cos, c64.detach(), 0, 5e-6, "cos phi near 0 and +-pi")
    a = np.array([[1.0, -0.7, 0.4], [0.6, 1.1, -0.9]])
    (gx,) = torch.autograd.grad((phi * T(a.astype(F32), DEV)).sum() + 0.5 * cos.sum(), x)
    (g64,) = torch.autograd.grad((p64 * torch.tensor(a)).sum() + 0.5 * c64.sum(), x64)
    assert bool(torch.isfinite(gx).all())
    close(gx, g64, 1e-4, 1e-5 * float(g64.abs().max()), "gradient near 0 and +-pi")


# ------------------------------------------------------------------------------------------------ 5: distribution
def _zigzag_frames(n_frames, seed, n=24, sigma=0.08):
    """A planar all-trans zigzag (phi = pi) with Gaussian jitter: the angles scatter around +-pi, across the periodic seam."""
    i = np.arange(n)
    x0 = np.stack([0.9 * i, 0.6 * (i % 2), np.zeros(n)], 1) + 1.0
    rng = np.random.default_rng(seed)
    return np.stack([x0 + rng.normal(0, sigma, x0.shape) for _ in range(n_frames)]).astype(F32)


@pytest.mark.parametrize("nbins,width", [(36, None), (50, None), (36, 0.1), (50, 0.1)])
def test_distribution_and_gradient_vs_float64(nbins, width):
    """count and the gradient of ((count - target)^2).sum() against float64 on the same frames.  Allowed: 10 x the error of a
    float32 torch restatement of the same definition (tests/dihedral_ref.py run in float32) against float64 on this input,
    computed here and quoted in the assertion message."""
    from mdgrad_amd.observable import dihedral_distribution
    frames = _zigzag_frames(16, nbins)
    L = np.array([40.0, 40.0, 40.0])
    top = np.array([[i, i + 1, i + 2, i + 3] for i in range(21)])
    target = torch.tensor(np.random.default_rng(nbins + 1).uniform(0.5, 1.5, nbins))
    target = target / target.sum()

    def ref(dtype):
        x = torch.tensor(frames).to(dtype).requires_grad_(True)
        count, ph = R.distribution(x, top, nbins, width, L)
        (gx,) = torch.autograd.grad((count - target.to(dtype)).pow(2).sum(), x)
        return count.detach().double().numpy(), gx.double().numpy(), ph.detach().double().numpy()
    c64, g64, p64 = ref(torch.float64)
    c32, g32, _ = ref(torch.float32)
    w = 2 * math.pi / nbins if width is None else width
    near = (math.pi - np.abs(p64) <= w).mean()
    assert near >= 0.05, "only %.3f of the angles lie within one width of +-pi" % near
    tol_c, tol_g = 10 * np.abs(c32 - c64).max(), 10 * np.abs(g32 - g64).max()
    obs = dihedral_distribution(mk_system(frames[0], L), top, nbins, width=width)
    x = T(frames, DEV).requires_grad_(True)
    bins, count, phi = obs(x)
    (gx,) = torch.autograd.grad((count - target.to(torch.float32).to(DEV)).pow(2).sum(), x)
    assert bins.shape == (nbins + 1,) and phi.shape == (16, 21) and abs(float(count.sum()) - 1.0) < 1e-5
    ec, eg = _rel(count.detach().cpu(), c64), _rel(gx.cpu(), g64)
    print("dihedral_distribution nbins=%d width=%s: count err %.3e (allowed %.3e), gradient err %.3e (allowed %.3e)"
          % (nbins, width, ec, tol_c, eg, tol_g))
    assert bool(torch.isfinite(count).all()) and bool(torch.isfinite(gx).all())
    assert ec <= tol_c, "count: err %.3e, allowed %.3e = 10 x the float32 restatement's %.3e" % (ec, tol_c, tol_c / 10)
    assert eg <= tol_g, "gradient: err %.3e, allowed %.3e = 10 x the float32 restatement's %.3e" % (eg, tol_g, tol_g / 10)
    # bitwise reproducible, forward and backward
    x2 = T(frames, DEV).requires_grad_(True)
    count2 = obs(x2)[1]
    (gx2,) = torch.autograd.grad((count2 - target.to(torch.float32).to(DEV)).pow(2).sum(), x2)
    assert torch.equal(count, count2) and torch.equal(gx, gx2)


def test_distribution_keep_angles_false_and_replicated_input():
    from mdgrad_amd.observable import dihedral_distribution
    frames = _zigzag_frames(12, 5)                                   # T = 3 times R = 4 replicas of 24 beads
    L = np.array([40.0, 40.0, 40.0])
    top = np.array([[i, i + 1, i + 2, i + 3] for i in range(21)])
    one = mk_system(frames[0], L)
    x = T(frames, DEV)
    b1, c1, p1 = dihedral_distribution(one, top, 36)(x)
    b2, c2, p2 = dihedral_distribution(one, top, 36, keep_angles=False)(x)
    assert p1 is not None and p2 is None and torch.equal(b1, b2) and torch.equal(c1, c2)
    stacked = one.replicate(4)
    q_t = T(frames.reshape(3, 4 * 24, 3), DEV)                       # what Simulations returns: [T, R N, 3]
    b3, c3, p3 = dihedral_distribution(stacked, top, 36)(q_t)
    assert torch.equal(c3, c1) and torch.equal(p3, p1), "frames = time x replica"
    # a table over the whole stacked system: the same terms, grouped per time frame
    top_all = np.concatenate([top + 24 * r for r in range(4)])
    b4, c4, p4 = dihedral_distribution(stacked, top_all, 36)(q_t)
    assert p4.shape == (3, 84) and torch.equal(p4.reshape(12, 21), p1) and torch.equal(c4, c1)


# ------------------------------------------------------------------------------------------------ 6: trajectory + adjoint
NBINS_TRAJ = 36
_oracle_cache = {}


def _traj_target():
    t = torch.tensor(np.random.default_rng(6).uniform(0.5, 1.5, NBINS_TRAJ).astype(F32))
    return t / t.sum()


def _oracle_traj(g, dihes, coeffs, t):
    if "run" not in _oracle_cache:
        cell = T(g["cell"])
        n = g["pos"].shape[0]
        angles = np.array([[i, i + 1, i + 2] for i in range(n - 2)])
        terms = [O.PairTerm("lj", torch.tensor([0.9, 0.5]), 2.5, cell, ex_pairs=g["bonds"], p=10, q=0, c=0),
                 O.BondTerm(g["bonds"], 3.0, 1.21, cell), O.AngleTerm(angles, 2.0, 1.9, cell),
                 R.DihedralTerm(dihes, coeffs, g["cell"])]
        target = _traj_target()

        def loss_fn(Ls):
            count, _ = R.distribution(Ls[1][::2], dihes, NBINS_TRAJ, None, g["cell"])
            return (count - target).pow(2).sum() * 1e2 + Ls[0][-1].pow(2).mean() + 0.0 * Ls[2][-1].sum()
        _oracle_cache["run"] = oracle_run(g["pos"], g["cell"], g["vel"], g["masses"], terms, 0.5, 50.0, 5, t, loss_fn)
    return _oracle_cache["run"]


@pytest.mark.parametrize("graphs_on", [True, False], ids=["graph_replay", "eager"])
def test_dihedral_term_in_a_stack_trajectory_and_adjoint_vs_oracle(graphs_on):
    """Stack(pair + bond + angle + dihedral) on the chain of fold_traj: 10 NHC steps, the loss on dihedral_distribution of
    q_t[::2], and the adjoint -- trajectories, adjoint of y0, dL/d(sigma, epsilon) and dL/dcoeffs against the oracle with
    dihedral_ref.DihedralTerm appended.  The stack stays on the analytic adjoint (force_vjp) and HIP-graph replay although
    the term's coefficients require grad."""
    from mdgrad_amd import graphs
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import AnglePotentials, BondPotentials, DihedralPotentials, PairPotentials, Stack
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.observable import dihedral_distribution
    from mdgrad_amd.sovlers import odeint_adjoint
    from mdgrad_amd.topology import chain_dihedrals
    g = load_golden("fold_traj")
    n = g["pos"].shape[0]
    coeffs = np.array(load_golden("dihedral_d2")["coeffs"][0], dtype=F32)
    angles = np.array([[i, i + 1, i + 2] for i in range(n - 2)])
    dihes = chain_dihedrals(n)
    system = mk_system(g["pos"], g["cell"], g["vel"], g["masses"], g["numbers"])
    bonds = torch.as_tensor(g["bonds"])
    mdl = P.ExcludedVolume(0.9, 0.5, 10)
    dihe = DihedralPotentials(system, dihes, torch.tensor(coeffs))
    stack = Stack({"pair": PairPotentials(system, mdl, cutoff=2.5, ex_pairs=bonds),
                   "bond": BondPotentials(system, bonds, 3.0, 1.21),
                   "angle": AnglePotentials(system, torch.as_tensor(angles), 2.0, 1.9),
                   "dihe": dihe})
    integ = NoseHooverChain(stack, system, T=0.5, num_chains=5, Q=50.0, adjoint=True).to(DEV)
    assert integ.model.supports_force_vjp() and integ.supports_rhs_vjp(), "the term must not push the stack onto the autograd branch"
    assert graphs.enabled(integ)
    integ.use_graphs = graphs_on
    calls = {"n": 0}
    orig = integ.model.force_vjp

    def counted(*a, **k):
        calls["n"] += 1
        return orig(*a, **k)
    integ.model.force_vjp = counted
    t = torch.Tensor([0.005 * i for i in range(11)])
    y0 = [s.clone().requires_grad_(True) for s in integ.get_inital_states(wrap=True)]
    v_t, q_t, pv_t = odeint_adjoint(integ, tuple(y0), t.to(DEV), method="NH_verlet")
    obs = dihedral_distribution(system, dihes, NBINS_TRAJ)
    count = obs(q_t[::2])[1]
    loss = (count - _traj_target().to(DEV)).pow(2).sum() * 1e2 + v_t[-1].pow(2).mean() + 0.0 * pv_t[-1].sum()
    loss.backward()
    assert calls["n"] > 0, "the adjoint did not go through force_vjp"
    traj, lam, gth = _oracle_traj(g, dihes.numpy(), coeffs, t)
    close(q_t, traj[1], 0, 2e-5, "q_t")
    close(v_t, traj[0], 1e-3, 1e-4 * float(traj[0].abs().max()), "v_t")
    close(pv_t, traj[2], 2e-3, 1e-5, "pv_t")
    for x, l, nm in zip(y0, lam, ("adj v0", "adj q0", "adj pv0")):
        close(x.grad, l, 5e-3, 2e-3 * float(l.abs().max()) + 1e-9, nm)
    got = torch.stack([mdl.sigma.grad.reshape(()), mdl.epsilon.grad.reshape(())])
    close(got, gth[:2], 5e-3, 5e-4 * float(gth[:2].abs().max()), "dL/d(sigma, epsilon)")
    assert gth.numel() == 7 and dihe.coeffs.grad is not None
    close(dihe.coeffs.grad, gth[2:], 5e-3, 5e-4 * float(gth[2:].abs().max()), "dL/dcoeffs")


# ------------------------------------------------------------------------------------------------ 7: torch ops
def test_torch_ops_equal_ctypes_path_and_reject_bad_input():
    from mdgrad_amd import _torch_ops, ops
    ns = _torch_ops.get()
    assert ns is not None
    g, wrapped, L = _wrapped_d2()
    Ll = [float(v) for v in L]
    tab = ops.DihedralTable(g["dihes"].astype(np.int64), 24, Ll, DEV, types=g["types"].astype(np.int64), n_types=2)
    q, w, A = T(wrapped, DEV), T(g["w"], DEV), T(g["coeffs"].astype(F32), DEV)
    a = ops.dihedral_eval(tab, q, A, w=w, energy=True, terms=True)
    e, gr, hw, ct, cd = ns.dihedral_eval(q, Ll, tab.top, A, tab.types, tab.inc_ptr, tab.inc, w, True, True)
    assert all(torch.equal(x, y) for x, y in zip((e, gr, hw, ct, cd), (a["e_atom"], a["grad"], a["hw"], a["c_term"], a["cd_term"])))
    e0, g0, h0, c0, d0 = ns.dihedral_eval(q, Ll, tab.top, A, tab.types, tab.inc_ptr, tab.inc, None, False, False)
    assert torch.equal(g0, gr) and e0.numel() == h0.numel() == c0.numel() == d0.numel() == 0
    frames = torch.stack([q, q + 0.01, q - 0.02]).contiguous()
    phi, cos = ops.DihedralPhiFn.apply(frames, tab)
    phi_t, cos_t = ns.dihedral_phi_fwd(frames, Ll, tab.top)
    assert torch.equal(phi, phi_t) and torch.equal(cos, cos_t)
    gp = torch.randn_like(phi)
    x = frames.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad((ops.DihedralPhiFn.apply(x, tab)[0] * gp).sum(), x)
    assert torch.equal(gx, ns.dihedral_phi_bwd(frames, Ll, tab.top, tab.inc_ptr, tab.inc, gp, None))
    raw = ops.DihedralHistFn.apply(phi, cos, 36, 0.2)
    assert torch.equal(raw, ns.dihedral_hist_fwd(phi, cos, 36, 0.2))
    g_raw = torch.randn(36, device=DEV)
    p = phi.clone().requires_grad_(True)
    (gphi,) = torch.autograd.grad((ops.DihedralHistFn.apply(p, cos, 36, 0.2) * g_raw).sum(), p)
    assert torch.equal(gphi, ns.dihedral_hist_bwd(phi, cos, 36, 0.2, g_raw))
    bad = [lambda: ns.dihedral_eval(q.double(), Ll, tab.top, A, tab.types, tab.inc_ptr, tab.inc, None, False, False),
           lambda: ns.dihedral_eval(q, Ll[:2], tab.top, A, tab.types, tab.inc_ptr, tab.inc, None, False, False),
           lambda: ns.dihedral_eval(q, Ll, tab.top.long(), A, tab.types, tab.inc_ptr, tab.inc, None, False, False),
           lambda: ns.dihedral_eval(q, Ll, tab.top, A[0, :4].contiguous(), tab.types, tab.inc_ptr, tab.inc, None, False, False),
           lambda: ns.dihedral_eval(q, Ll, tab.top, A, tab.types[:5].contiguous(), tab.inc_ptr, tab.inc, None, False, False),
           lambda: ns.dihedral_eval(q, Ll, tab.top, A, tab.types, tab.inc_ptr[:-1].contiguous(), tab.inc, None, False, False),
           lambda: ns.dihedral_eval(q, Ll, tab.top, A, tab.types, tab.inc_ptr, tab.inc, w[:5].contiguous(), False, False),
           lambda: ns.dihedral_phi_fwd(q, Ll, tab.top),
           lambda: ns.dihedral_phi_bwd(frames, Ll, tab.top, tab.inc_ptr, tab.inc, None, None),
           lambda: ns.dihedral_phi_bwd(frames, Ll, tab.top, tab.inc_ptr, tab.inc, gp[:2].contiguous(), None),
           lambda: ns.dihedral_hist_fwd(phi, cos, 0, 0.2),
           lambda: ns.dihedral_hist_fwd(phi, cos, 36, 0.7),
           lambda: ns.dihedral_hist_fwd(phi, cos[:2].contiguous(), 36, 0.2),
           lambda: ns.dihedral_hist_bwd(phi, cos, 36, 0.2, g_raw[:10].contiguous()),
           lambda: ns.dihedral_hist_fwd(phi.cpu(), None, 36, 0.2)]
    for k, fn in enumerate(bad):
        with pytest.raises((RuntimeError, NotImplementedError)):
            fn()
            pytest.fail("bad input %d was accepted" % k)
