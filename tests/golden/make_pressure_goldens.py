"""Golden-vector generator for the pressure observable (BUILD CONTAINER ONLY), in the style of make_adf_goldens.py.

The reference's own Pressure (torchmd/thermo.py:17-54) does not run, so the fixtures are assembled from the reference's
components with torch autograd over them: generate_nbr_list(..., get_dis=True), compute_dis, the torchmd.potentials
modules, build_lj_sim and odeint_adjoint.  Definition (mdgrad_amd/thermo.py):

    K = sum_i m_i |v_i|^2      W = -sum_terms sum_pairs r phi'(r)      P = (K + W) / (d V)

    python tests/golden/make_pressure_goldens.py

  P1 pressure_p1   jittered 108-atom FCC frames, one case per pair form of make_goldens.PAIR_FORMS: W in the reference's
                   float32, W recomputed in float64 from the same pair list, S = sum |r phi'| per frame, dW/dq, dW/dtheta,
                   K and P for seeded velocities
  P2 pressure_p2   a two-term Stack with different cutoffs: LJ (cutoff 2.5) under an index_tuple, ExcludedVolume
                   (cutoff 1.3) under ex_pairs
  P3 pressure_p3   the NHC LJ-108 trajectory of the existing goldens, 20 steps, L = sum_t (P(q_t, v_t) - target)^2,
                   odeint_adjoint backward: dL/dsigma, dL/depsilon and the initial-state gradients

Asserted here: no pair of a stored frame (P1, P2) lies within PAIR_MARGIN of a cutoff (phi is unshifted: a pair that changes
sides moves W by a finite step; frames that have one are redrawn from the seeded stream), every output is finite, and the
reference's float32 W is within FWD_TOL * S of its float64 value (the bound the kernels are held to).
P3 stores no frame, and the margin cannot hold along a trajectory: ~4 100 pairs per unit length sit around r = 2.5 in this
system, i.e. 0.8 per frame inside +-1e-4, and 21 consecutive frames are not free to choose.  Its closest approach is stored
as `cut_margin` (3.3e-6); one LJ pair changing sides moves that frame's P by r phi'(2.5) / (3 V) = 2.9e-4.
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import F32, PAIR_FORMS, make_system, save, build_lj_sim, lj_inputs  # noqa: E402
from make_adf_goldens import finite  # noqa: E402

import torch  # noqa: E402
from torchmd import potentials as P  # noqa: E402
from torchmd.topology import generate_nbr_list, compute_dis  # noqa: E402
from torchmd.sovlers import odeint_adjoint  # noqa: E402

PAIR_MARGIN = 1e-4
FWD_TOL = 1e-5           # tests/test_gpu_pressure.py: |W - W64| <= tol * S with tol <= 1e-5
MASS = 1.008
DIM = 3


def virial_terms(q, cell, terms, dtype=torch.float32):
    """(W, S, closest distance to a cutoff) of one frame q [N, 3] over `terms` = [(model, cutoff, index_tuple, ex_pairs)]:
    the pair list always comes from the reference's float32 search, the distances and phi' run in `dtype`."""
    cell_t = torch.tensor(cell, dtype=torch.float32)
    W, S, margin = 0.0, 0.0, np.inf
    for model, cutoff, index_tuple, ex_pairs in terms:
        nbr, dis, off = generate_nbr_list(q.detach().float(), cutoff, cell_t, index_tuple=index_tuple, ex_pairs=ex_pairs,
                                          get_dis=True)
        mdl = model if dtype == torch.float32 else copy.deepcopy(model).to(dtype)
        r = compute_dis(q.to(dtype), nbr, off.to(dtype), torch.diag(cell_t).to(dtype))
        rr = r if r.requires_grad else r.requires_grad_(True)
        (du,) = torch.autograd.grad(mdl(rr).sum(), rr, create_graph=True)
        W = W - (rr * du).sum()
        S = S + (rr * du).abs().sum().detach()
        margin = min(margin, float((r.detach() - cutoff).abs().min()))
    return W, S, margin


def virial_case(prefix, frames, cell, terms, params, vel):
    """Fixture entries of one set of frames: per frame W32, W64, S, dW/dq; dW/dtheta summed with the weights gw; K and P."""
    F = len(frames)
    rng = np.random.default_rng(F + len(prefix))
    gw = rng.uniform(0.5, 1.5, F).astype(F32)
    W32, W64, S, gq = [], [], [], []
    gth = [torch.zeros_like(p) for p in params]
    for f in range(F):
        q = torch.tensor(frames[f], requires_grad=True)
        w, _, margin = virial_terms(q, cell, terms)
        assert margin > PAIR_MARGIN, "%s frame %d: a pair within %g of a cutoff" % (prefix, f, margin)
        grads = torch.autograd.grad(w, [q] + params, allow_unused=True)
        w64, s64, _ = virial_terms(q.detach(), cell, terms, torch.float64)
        assert abs(float(w.detach()) - float(w64.detach())) <= FWD_TOL * float(s64), "%s frame %d: the reference misses the forward bound" % (prefix, f)
        W32.append(w.detach()); W64.append(w64.detach()); S.append(s64); gq.append(grads[0])
        for k, g in enumerate(grads[1:]):
            if g is not None:
                gth[k] += float(gw[f]) * g
    W32, W64, S = torch.stack(W32), torch.stack(W64), torch.stack(S)
    V = float(np.prod(cell))
    K = (MASS * torch.tensor(vel).pow(2)).sum((1, 2))
    Pr = (K + W32) / (DIM * V)
    finite(W32, W64, S, K, Pr, *gq, *gth)
    out = {prefix + "W32": W32, prefix + "W64": W64.numpy(), prefix + "S": S.numpy(), prefix + "dW_dq": torch.stack(gq),
           prefix + "gw": gw, prefix + "K": K, prefix + "P": Pr}
    if params:
        out[prefix + "dW_dtheta"] = torch.stack([g.reshape(()) for g in gth])
        out[prefix + "theta"] = torch.stack([p.detach().reshape(()) for p in params])
    return out


def clear_frames(seed, n_frames, cutoffs, sigma=0.08):
    """n_frames jittered frames (as make_adf_goldens.jittered_frames) drawn from one seeded stream, keeping those without a
    pair within 2 PAIR_MARGIN of any of `cutoffs`: at ~4 100 pairs per unit length around r = 2.5 every other draw has one."""
    pos, cell, _ = lj_inputs(seed=seed)
    rng = np.random.default_rng(seed + 100)
    cell_t, frames = torch.tensor(cell, dtype=torch.float32), []
    while len(frames) < n_frames:
        fr = np.mod(pos + rng.normal(0, sigma, pos.shape), cell).astype(F32)
        _, dis, _ = generate_nbr_list(torch.tensor(fr), max(cutoffs) + 0.1, cell_t, get_dis=True)
        if all(float((dis - c).abs().min()) > 2 * PAIR_MARGIN for c in cutoffs):
            frames.append(fr)
    return np.stack(frames), cell


def seeded_velocities(seed, shape):
    return np.random.default_rng(seed).normal(0, np.sqrt(1.0 / MASS), shape).astype(F32)


def p1():
    frames, cell = clear_frames(21, 3, [2.5])
    vel = seeded_velocities(22, frames.shape)
    out = dict(xyz=frames, vel=vel, cell=cell.astype(F32), cutoff=2.5, mass=MASS, dim=DIM)
    for name, mk in PAIR_FORMS.items():
        model = mk()
        out.update(virial_case(name + "_", frames, cell, [(model, 2.5, None, None)], list(model.parameters()), vel))
    save("pressure_p1", **out)


def p2():
    frames, cell = clear_frames(23, 3, [2.5, 1.3])
    vel = seeded_velocities(24, frames.shape)
    idx_a, idx_b = list(range(0, 108, 2)), list(range(0, 108, 3))
    ex = torch.LongTensor([[0, 1], [2, 3], [10, 50], [4, 7], [5, 41], [20, 21]])
    lj, ev = P.LennardJones(sigma=1.05, epsilon=0.9), P.ExcludedVolume(sigma=0.9, epsilon=0.6, power=12)
    terms = [(lj, 2.5, (idx_a, idx_b), None), (ev, 1.3, None, ex)]
    out = dict(xyz=frames, vel=vel, cell=cell.astype(F32), mass=MASS, dim=DIM, cutoff_lj=2.5, cutoff_ev=1.3,
               idx_a=np.array(idx_a), idx_b=np.array(idx_b), ex_pairs=ex)
    out.update(virial_case("", frames, cell, terms, list(lj.parameters()) + list(ev.parameters()), vel))
    save("pressure_p2", **out)


def p3():
    pos, cell, vel = lj_inputs(seed=0)
    mdl = P.LennardJones(1.0, 1.0)
    system, integ = build_lj_sim(pos, cell, vel, mdl)
    y0 = [s.clone().requires_grad_(True) for s in integ.get_inital_states(wrap=True)]
    t = torch.Tensor([0.005 * i for i in range(21)])
    v_t, q_t, pv_t = odeint_adjoint(integ, tuple(y0), t, method="NH_verlet")
    mass = torch.Tensor(system.get_masses())
    V, target = float(np.prod(cell)), 1.0
    Pt, margin = [], np.inf
    for k in range(len(t)):
        w, _, m = virial_terms(q_t[k], cell, [(mdl, 2.5, None, None)])
        margin = min(margin, m)
        Pt.append(((mass[:, None] * v_t[k].pow(2)).sum() + w) / (DIM * V))
    print("P3: closest pair to the cutoff over the %d frames: %.3e" % (len(t), margin))
    Pt = torch.stack(Pt)
    loss = (Pt - target).pow(2).sum()
    loss.backward()
    th = list(mdl.parameters())
    finite(Pt, th[0].grad, th[1].grad, y0[0].grad, y0[1].grad, y0[2].grad)
    save("pressure_p3", pos=pos.astype(F32), cell=cell.astype(F32), vel=vel.astype(F32), mass=system.get_masses().astype(F32),
         T=1.0, Q=50.0, chains=5, cutoff=2.5, dt=0.005, n_steps=21, target=target, dim=DIM, P_t=Pt.detach(), cut_margin=margin,
         loss=loss.detach().reshape(1), grad_sigma=th[0].grad, grad_epsilon=th[1].grad, grad_v0=y0[0].grad,
         grad_q0=y0[1].grad, grad_pv0=y0[2].grad)


if __name__ == "__main__":
    which = sys.argv[1:] or ["p1", "p2", "p3"]
    table = {"p1": p1, "p2": p2, "p3": p3}
    for w in which:
        table[w]()
