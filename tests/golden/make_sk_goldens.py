"""Golden-vector generator for the structure factor observable, in the style of make_pressure_goldens.py.

    python tests/golden/make_sk_goldens.py [s1 s2 s3]

The reference has no S(k); the definition is mdgrad_amd/observable.py structure_factor, evaluated here in float64
(tests/sk_ref.py) from float32 positions and cell lengths.  s1 and s2 need no reference program; s3 (BUILD CONTAINER ONLY)
runs the reference's trajectory and adjoint.

  S1 sk_s1   the three pressure_p1 frames (108 atoms, L = 4.8), k_range (1, 16), 30 bins, unit weights: all 3 844 vectors
  S2 sk_s2   the same frames rescaled into a 4.8 x 6.0 x 7.2 cell, seeded weights in [0.5, 2], max_per_bin = 16
             both: S64 [3, 30], a seeded cotangent gS and dS_dq = d sum(gS * S) / dq by float64 autograd
  S3 sk_s3   the NHC LJ-108 trajectory of pressure_p3 (build_lj_sim, odeint_adjoint, 21 frames): S_t over k_range (1, 10),
             18 bins from the float32 frames in float64, L = sum_b (mean_t S_t[b] - 1)^2, the reference adjoint's dL/dsigma
             and dL/depsilon, and the frames themselves
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from sk_ref import sk64  # noqa: E402
from mdgrad_amd.observable import sk_vectors  # noqa: E402

F32 = np.float32


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    print("wrote", path, {k: np.asarray(v).shape for k, v in arrs.items()})


def case(name, xyz, cell, nbins, k_range, weights, max_per_bin, seed):
    n, seg, kabs, edges = sk_vectors(cell.astype(np.float64), nbins, k_range, 3, max_per_bin)
    gS = np.random.default_rng(seed).uniform(-1.0, 1.0, (len(xyz), nbins)).astype(F32)
    S64, _, g = sk64(xyz, cell, n, seg, weights, gS)
    assert np.isfinite(S64).all() and np.isfinite(g).all()
    out = dict(xyz=xyz.astype(F32), cell=cell.astype(F32), nbins=nbins, k_range=np.array(k_range, dtype=np.float64),
               max_per_bin=(0 if max_per_bin is None else max_per_bin), n_vectors=np.diff(seg), S64=S64, gS=gS, dS_dq=g)
    if weights is not None:
        out["weights"] = weights.astype(F32)
    save(name, **out)


def s1():
    g = np.load(os.path.join(HERE, "pressure_p1.npz"))
    case("sk_s1", g["xyz"].astype(F32), g["cell"].astype(F32), 30, (1.0, 16.0), None, None, seed=11)


def s2():
    g = np.load(os.path.join(HERE, "pressure_p1.npz"))
    cell = np.array([4.8, 6.0, 7.2], dtype=F32)
    xyz = (g["xyz"].astype(np.float64) / g["cell"].astype(np.float64) * cell.astype(np.float64)).astype(F32)
    w = np.random.default_rng(5).uniform(0.5, 2.0, xyz.shape[1]).astype(F32)
    case("sk_s2", xyz, cell, 30, (1.0, 16.0), w, 16, seed=12)


def s3():
    from make_goldens import build_lj_sim, lj_inputs
    from torchmd import potentials as P
    from torchmd.sovlers import odeint_adjoint
    pos, cell, vel = lj_inputs(seed=0)
    mdl = P.LennardJones(1.0, 1.0)
    system, integ = build_lj_sim(pos, cell, vel, mdl)
    y0 = [s.clone().requires_grad_(True) for s in integ.get_inital_states(wrap=True)]
    t = torch.Tensor([0.005 * i for i in range(21)])
    v_t, q_t, pv_t = odeint_adjoint(integ, tuple(y0), t, method="NH_verlet")
    nbins, k_range = 18, (1.0, 10.0)
    cell32 = np.asarray(cell, dtype=F32).reshape(-1)[:3] if np.asarray(cell).ndim == 1 else np.diag(np.asarray(cell)).astype(F32)
    n, seg, kabs, edges = sk_vectors(cell32.astype(np.float64), nbins, k_range, 3, None)
    k = 2 * np.pi * torch.as_tensor(n).double() / torch.as_tensor(cell32).double()
    cnt = np.diff(seg)
    A = torch.zeros(len(n), nbins, dtype=torch.float64)
    b = np.repeat(np.arange(nbins), cnt)
    A[torch.arange(len(n)), torch.as_tensor(b)] = torch.as_tensor(1.0 / cnt[b])
    ph = q_t.double() @ k.t()                                                   # [T, N, M] from the float32 frames
    S_t = (ph.cos().sum(1).pow(2) + ph.sin().sum(1).pow(2)) / q_t.shape[1] @ A
    loss = (S_t.mean(0) - 1.0).pow(2).sum()
    loss.backward()
    th = list(mdl.parameters())
    S_chk, _, _ = sk64(q_t.detach().numpy(), cell32, n, seg)
    assert np.abs(S_chk - S_t.detach().numpy()).max() < 1e-10
    assert all(np.isfinite(x.detach().numpy()).all() for x in (S_t, th[0].grad, th[1].grad))
    save("sk_s3", cell=cell32, nbins=nbins, k_range=np.array(k_range), n_steps=21, q_t=q_t.detach().numpy().astype(F32),
         S_t=S_t.detach().numpy(), loss=loss.detach().numpy().reshape(1), grad_sigma=th[0].grad.detach().numpy(),
         grad_epsilon=th[1].grad.detach().numpy())


if __name__ == "__main__":
    which = sys.argv[1:] or ["s1", "s2", "s3"]
    table = {"s1": s1, "s2": s2, "s3": s3}
    for w in which:
        table[w]()
