"""Golden-vector generator for the bond-angle distribution (BUILD CONTAINER ONLY), in the style of make_goldens.py.

Runs the reference's CPU path (with the ase stand-ins of _ase_stub.py) on seeded inputs and writes small .npz fixtures next
to this file: inputs and reference outputs only.

    python tests/golden/make_adf_goldens.py

  A1 adf_a1    angle_distribution on the jittered 108-atom FCC liquid, cutoffs 1.5 (3 frames), 2.0 and 2.5 (2 frames, above
               half the 4.8 box): bins, count, angles, generate_angle_list, xyz.grad of ((count - target)^2).sum()
               torchmd/observable.py:120-151, topology.py:83-122
  A2 adf_a2    the same configuration with width 0.05, angle_range (0.5, 2.8) and an index_tuple subset
  A3 adf_a3    Angles (cos) on the first A1 case                                  torchmd/observable.py:89-118
  A4 adf_a4    the unperturbed lattice (a = 1.5, first shell only) at cutoff 1.3, exactly collinear triplets: forward only,
               the reference's gradient there is NaN.  With a = 1.6 the f32 positions make some cosines -1 - 2^-23 and the
               reference's angles NaN; multiples of 0.75 are exact, so its cosines there are exactly -1
  A5 adf_a5    NHC LJ108 trajectory (20 steps) -> odeint_adjoint -> angle_distribution(q_t[::5]) -> loss -> backward
               torchmd/sovlers.py:196-293

The angle lists of the larger cutoffs hold 10^5-10^6 triplets; to keep the fixtures small, those cases store the list length
and every ANGLE_STRIDE-th row and angle (rows `sub_idx`).  Every stored reference output is asserted finite.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import F32, fcc, make_system, save, build_lj_sim, lj_inputs  # noqa: E402

import torch  # noqa: E402
from torchmd import potentials as P  # noqa: E402
from torchmd.observable import angle_distribution, Angles  # noqa: E402
from torchmd.topology import generate_nbr_list, generate_angle_list  # noqa: E402
from torchmd.sovlers import odeint_adjoint  # noqa: E402

ANGLE_STRIDE = 53
NBINS = 60
I16 = np.int16


def finite(*arrs):
    for a in arrs:
        a = a.detach().numpy() if torch.is_tensor(a) else np.asarray(a)
        assert np.all(np.isfinite(a)), "non-finite reference output"


def jittered_frames(seed, n_frames, sigma=0.08):
    pos, cell, _ = lj_inputs(seed=seed)
    rng = np.random.default_rng(seed + 100)
    frames = np.stack([np.mod(pos + rng.normal(0, sigma, pos.shape), cell) for _ in range(n_frames)])
    return frames.astype(F32), cell, pos


def adf_case(prefix, frames, cell, cutoff, nbins, angle_range, width=None, index_tuple=None, full_list=True):
    system = make_system(frames[0].astype(np.float64), cell)
    obs = angle_distribution(system, nbins, angle_range, cutoff=cutoff, index_tuple=index_tuple, width=width)
    xyz = torch.tensor(frames, requires_grad=True)
    bins, count, angles = obs(xyz)
    target = torch.tensor(np.random.default_rng(len(prefix) + nbins).uniform(0.5, 1.5, nbins).astype(F32))
    target = target / target.sum()
    loss = (count - target).pow(2).sum()
    (gx,) = torch.autograd.grad(loss, xyz)
    nbr, _ = generate_nbr_list(xyz.detach(), cutoff, torch.Tensor(cell), index_tuple=index_tuple)
    alist = generate_angle_list(nbr)
    finite(count, angles, gx)
    assert len(alist) == len(angles)
    out = {prefix + "xyz": xyz.detach(), prefix + "cutoff": cutoff, prefix + "nbins": nbins,
           prefix + "range": np.array(angle_range, dtype=F32), prefix + "bins": bins, prefix + "count": count.detach(),
           prefix + "target": target, prefix + "grad": gx, prefix + "n_angles": len(angles),
           prefix + "width": obs.width, prefix + "nbr": nbr.numpy().astype(I16)}
    if full_list:
        out[prefix + "angles"] = angles.detach()
        out[prefix + "angle_list"] = alist.numpy().astype(I16)
    else:
        idx = np.arange(0, len(angles), ANGLE_STRIDE)
        out[prefix + "sub_idx"] = idx
        out[prefix + "angles"] = angles.detach()[idx]
        out[prefix + "angle_list"] = alist.numpy()[idx].astype(I16)
    return out


def a1_a2_a3():
    out = {"cell": None}
    # (cutoff 2.0 takes seed 14: with seed 12 a near-collinear triplet puts the reference's f32 acos gradient 3e-3 of its
    #  largest component off the float64 gradient of the same triplets, more than the tests allow the kernel)
    cases = [("c15_", 11, 3, 1.5, True), ("c20_", 14, 2, 2.0, False), ("c25_", 13, 2, 2.5, False)]
    for prefix, seed, nf, cut, full in cases:
        frames, cell, _ = jittered_frames(seed, nf)
        out.update(adf_case(prefix, frames, cell, cut, NBINS, (0.0, np.pi), full_list=full))
        out["cell"] = cell.astype(F32)
    save("adf_a1", **out)

    frames, cell, _ = jittered_frames(11, 3)
    idx_a, idx_b = list(range(0, 108, 2)), list(range(0, 108, 3))
    out = adf_case("", frames, cell, 1.5, 40, (0.5, 2.8), width=0.05, index_tuple=(idx_a, idx_b))
    out.update(cell=cell.astype(F32), idx_a=np.array(idx_a), idx_b=np.array(idx_b))
    save("adf_a2", **out)

    system = make_system(frames[0].astype(np.float64), cell)
    cos = Angles(system, NBINS, (0.0, np.pi), cutoff=1.5)(torch.tensor(frames))
    finite(cos)
    save("adf_a3", xyz=frames, cell=cell.astype(F32), cutoff=1.5, nbins=NBINS, cos=cos)


def a4():
    lat, cell = fcc(3, 1.5)            # (multiples of 0.75: exact in f32, so collinear bond vectors are exactly opposite)
    frames = lat[None].astype(F32)
    system = make_system(lat, cell)
    obs = angle_distribution(system, NBINS, (0.0, np.pi), cutoff=1.3)
    bins, count, angles = obs(torch.tensor(frames))
    finite(count, angles)
    save("adf_a4", xyz=frames, cell=cell.astype(F32), cutoff=1.3, nbins=NBINS, bins=bins, count=count, angles=angles)


def a5():
    pos, cell, vel = lj_inputs(seed=0)
    mdl = P.LennardJones(1.0, 1.0)
    system, integ = build_lj_sim(pos, cell, vel, mdl)
    y0 = [s.clone().requires_grad_(True) for s in integ.get_inital_states(wrap=True)]
    t = torch.Tensor([0.005 * i for i in range(21)])
    obs = angle_distribution(system, NBINS, (0.0, np.pi), cutoff=1.5)
    v_t, q_t, pv_t = odeint_adjoint(integ, tuple(y0), t, method="NH_verlet")
    _, count, _ = obs(q_t[::5])
    target = torch.full((NBINS,), 1.0 / NBINS)
    loss = (count - target).pow(2).sum() * 1e3
    loss.backward()
    th = list(mdl.parameters())
    finite(count, th[0].grad, th[1].grad, y0[0].grad, y0[1].grad, y0[2].grad)
    save("adf_a5", pos=pos.astype(F32), cell=cell.astype(F32), vel=vel.astype(F32), mass=system.get_masses().astype(F32),
         T=1.0, Q=50.0, chains=5, cutoff=2.5, adf_cutoff=1.5, dt=0.005, n_steps=21, stride=5, nbins=NBINS,
         count=count.detach(), loss=loss.detach().reshape(1), grad_sigma=th[0].grad, grad_epsilon=th[1].grad,
         grad_v0=y0[0].grad, grad_q0=y0[1].grad, grad_pv0=y0[2].grad)


if __name__ == "__main__":
    which = sys.argv[1:] or ["a123", "a4", "a5"]
    table = {"a123": a1_a2_a3, "a4": a4, "a5": a5}
    for w in which:
        table[w]()
