"""Golden-vector generator for the Coulomb term (BUILD CONTAINER ONLY), in the style of make_dihedral_goldens.py.

Runs the reference's CPU path (with the ase stand-ins of _ase_stub.py) on seeded inputs and writes small .npz fixtures next
to this file: inputs and reference outputs only.

    python tests/golden/make_coulomb_goldens.py

The reference's Electrostatics (torchmd/interface.py:303-361) has two bugs: it overwrites q1, so it multiplies q_j * q_j,
and it carries a minus sign.  With uniform charges q_j^2 = q_i q_j, and its energy is exactly minus the bare truncated
Coulomb sum.  The goldens therefore record  -U_ref  (energy_*) and  +dU_ref/dx  (grad_*, autograd: the force -dU/dx of the
right sum), which CoulombPotentials must match with shift="none", alpha=0 -- they pin the pair set, the images, the masks and
the unit constant.

  E1 coulomb_e1   40 seeded atoms in an 8 A cube, cutoff 3.5: all charges 1.0; a second call with all charges 0.8 and
                  ex_pairs of 10 pairs
  E2 coulomb_e2   the triclinic cell and positions of nbr_tric64.npz (cutoff 2.2) with an index_tuple selection: all charges
                  1.0, then all charges 0.8
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import F32, save  # noqa: E402  (sets up the import path of the reference)

import torch  # noqa: E402
from torchmd.interface import Electrostatics  # noqa: E402


def run(xyz, cell, charge, cutoff, index_tuple=None, ex_pairs=None):
    """(-U_ref [1], +dU_ref/dx [N,3]) of the reference class with every charge equal to `charge` (float32, as it runs)."""
    n = xyz.shape[0]
    mod = Electrostatics(torch.full((n,), float(charge)), cell, device="cpu", cutoff=cutoff, index_tuple=index_tuple,
                         ex_pairs=None if ex_pairs is None else torch.as_tensor(ex_pairs))
    x = torch.tensor(xyz, requires_grad=True)
    U = mod(x)
    (g,) = torch.autograd.grad(U, x)
    assert bool(torch.isfinite(U)) and bool(torch.isfinite(g).all())
    return (-U.detach()).reshape(1), g, float(mod.conversion)


def main():
    rng = np.random.default_rng(303)
    L = 8.0
    pts = []
    while len(pts) < 40:                                       # seeded atoms, no two closer than 1.2
        p = rng.uniform(0, L, 3)
        if pts:
            d = np.array(pts) - p
            d -= L * np.round(d / L)
            if np.sqrt((d ** 2).sum(1)).min() < 1.2:
                continue
        pts.append(p)
    xyz = np.array(pts).astype(F32)
    cell = np.array([L, L, L], dtype=F32)
    ex = np.stack([np.arange(0, 20, 2), np.arange(1, 20, 2)], 1)        # 10 pairs (0,1), (2,3) ...
    e_a, g_a, conv = run(xyz, cell, 1.0, 3.5)
    e_b, g_b, _ = run(xyz, cell, 0.8, 3.5, ex_pairs=ex)
    save("coulomb_e1", xyz=xyz, cell=cell, cutoff=np.float64(3.5), ex_pairs=ex.astype(np.int16), q_a=np.float64(1.0),
         q_b=np.float64(0.8), energy_a=e_a, grad_a=g_a, energy_b=e_b, grad_b=g_b, conversion=np.float64(conv))

    t = np.load(os.path.join(HERE, "nbr_tric64.npz"))
    xyz, cell, cutoff = t["xyz"].astype(F32), t["cell"].astype(F32), float(t["cutoff"])
    idx_a, idx_b = list(range(0, 40)), list(range(24, 64))               # overlapping selections
    e_a, g_a, conv = run(xyz, cell, 1.0, cutoff, index_tuple=(idx_a, idx_b))
    e_b, g_b, _ = run(xyz, cell, 0.8, cutoff, index_tuple=(idx_a, idx_b))
    save("coulomb_e2", xyz=xyz, cell=cell, cutoff=np.float64(cutoff), idx_a=np.array(idx_a, dtype=np.int16),
         idx_b=np.array(idx_b, dtype=np.int16), q_a=np.float64(1.0), q_b=np.float64(0.8), energy_a=e_a, grad_a=g_a,
         energy_b=e_b, grad_b=g_b, conversion=np.float64(conv))


if __name__ == "__main__":
    main()
