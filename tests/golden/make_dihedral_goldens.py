"""Golden-vector generator for the dihedral terms (BUILD CONTAINER ONLY), in the style of make_adf_goldens.py.

Runs the reference's CPU path (with the ase stand-ins of _ase_stub.py) on seeded inputs and writes small .npz fixtures next
to this file: inputs and reference outputs only.

    python tests/golden/make_dihedral_goldens.py

  D1 dihedral_d1   compute_dihe (torchmd/observable.py:181-197) on the 24-bead self-avoiding chain of fold_traj.npz, unwrapped
                   along its bonds: frame 0 plus four jittered copies (sigma = 0.05), all 21 chain quadruples; float32 as the
                   reference runs it and float64 of the same call, and their largest difference
  D2 dihedral_d2   on frame 0: energy, force -dU/dx and H.w (double autograd) of U = sum_m A[type, m] cos^m phi built on the
                   reference's compute_dihe output (the "multiharmonic" form of nff/nn/modules.py:253-257), two types
                   alternating along the chain, in float64; dU/dA and d(w.F)/dA as well

Neither the number of frames nor the number of quadruples may be 3: the reference's torch.cross without `dim` takes the
first axis of size 3.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import F32, save  # noqa: E402  (sets up the import path of the reference)

import torch  # noqa: E402
from torchmd.observable import compute_dihe  # noqa: E402

COEFFS = [[0.3, -1.1, 0.8, 0.5, -0.4], [0.1, 0.7, -0.2, 0.0, 0.3]]
N_FRAMES, SIGMA = 5, 0.05


def unwrapped_chain():
    g = np.load(os.path.join(HERE, "fold_traj.npz"))
    pos, L = g["pos"].astype(np.float64), g["cell"].astype(np.float64)
    b = np.diff(pos, axis=0)
    b -= L * np.round(b / L)
    return np.concatenate([pos[:1], pos[:1] + np.cumsum(b, 0)], 0), L


def main():
    x0, L = unwrapped_chain()
    n = x0.shape[0]
    dihes = np.array([[i, i + 1, i + 2, i + 3] for i in range(n - 3)])
    rng = np.random.default_rng(2024)
    frames = np.stack([x0] + [x0 + rng.normal(0, SIGMA, x0.shape) for _ in range(N_FRAMES - 1)]).astype(F32)
    assert frames.shape[0] != 3 and dihes.shape[0] != 3
    dt = torch.as_tensor(dihes)
    cos32 = compute_dihe(torch.tensor(frames), dt)
    cos64 = compute_dihe(torch.tensor(frames).double(), dt)
    assert cos32.shape == (N_FRAMES, n - 3) and bool(torch.isfinite(cos64).all())
    err32 = float((cos32.double() - cos64).abs().max())
    save("dihedral_d1", xyz=frames, cell=L.astype(F32), dihes=dihes.astype(np.int16), cos32=cos32, cos64=cos64,
         err32=np.float64(err32), min_abs_sin=np.float64(float((1 - cos64.pow(2)).sqrt().min())))

    # every bond angle well away from 0 and pi: the torsion of frame 0 is regular
    b = np.diff(frames[0].astype(np.float64), axis=0)
    ca = (b[:-1] * b[1:]).sum(1) / np.sqrt((b[:-1] ** 2).sum(1) * (b[1:] ** 2).sum(1))
    assert np.sqrt(1 - ca ** 2).min() > 0.2, "a bond angle of the chain is too close to 0 or pi"

    A = torch.tensor(COEFFS, dtype=torch.float64, requires_grad=True)
    types = np.arange(n - 3) % 2
    w = np.random.default_rng(2025).normal(0, 1, x0.shape).astype(F32)
    q = torch.tensor(frames[0]).double().requires_grad_(True)
    c = compute_dihe(q[None], dt)[0]
    a = A[torch.as_tensor(types)]
    U = sum(a[:, m] * c.pow(m) for m in range(5)).sum()
    gq, gA = torch.autograd.grad(U, (q, A), create_graph=True)
    wF = -(gq * torch.tensor(w).double()).sum()
    dq, dA = torch.autograd.grad(wF, (q, A))
    for t in (U, gq, gA, dq, dA):
        assert bool(torch.isfinite(t).all())
    save("dihedral_d2", pos=frames[0], cell=L.astype(F32), dihes=dihes.astype(np.int16), types=types.astype(np.int16),
         coeffs=np.array(COEFFS), w=w, energy=U.detach().reshape(1), force=-gq.detach(), hw=-dq, dU_dA=gA.detach(),
         dwF_dA=dA)


if __name__ == "__main__":
    main()
