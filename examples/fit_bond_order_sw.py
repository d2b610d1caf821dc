#!/usr/bin/env python
"""Fit the three-body strength lam of monatomic (mW) water to the local order of a target liquid by back-propagating through
the MD trajectory: simulate -> bond_order_distribution of q_3 and q_6 -> loss -> backward (analytic adjoint, HIP-graph replay)
-> Adam.  q_3 is large for a tetrahedral shell (0.745 for the perfect one), so its distribution moves with lam where g(r) barely
does.  The target is the pair of distributions of the published lam = 23.15; the fit starts from a less tetrahedral liquid.

    python examples/fit_bond_order_sw.py --epochs 20
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fit_adf_sw import build  # noqa: E402   (the 64-molecule mW box of the angle-distribution example)

CUTOFF = 3.5        # Angstrom: the first shell of mW water ends before 3.5; the box is 12.4


def order_of(integ, observables, frames, dt, dev):
    """The q_3 and q_6 distributions of the second half of one trajectory, concatenated."""
    from mdgrad_amd.sovlers import odeint_adjoint
    t = torch.Tensor([dt * i for i in range(frames)]).to(dev)
    y0 = tuple(integ.get_inital_states(wrap=True))
    v_t, q_t, pv_t = odeint_adjoint(integ, y0, t, method="NH_verlet")
    return torch.cat([obs(q_t[frames // 2:])[1] for obs in observables])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--dt", type=float, default=0.25, help="in Angstrom sqrt(amu / eV): 0.25 is about 2.5 fs")
    ap.add_argument("--lam0", type=float, default=18.0)
    ap.add_argument("--lr", type=float, default=0.3)
    args = ap.parse_args(argv)
    from mdgrad_amd.observable import bond_order_distribution
    dev = "cuda:0"
    system, _, integ_true = build(23.15, dev)
    observables = [bond_order_distribution(system, l, nbins=32, q_range=(0.0, 1.0), cutoff=CUTOFF, keep_values=False) for l in (3, 6)]
    with torch.no_grad():
        target = order_of(integ_true, observables, args.frames, args.dt, dev)
    system, sw, integ = build(args.lam0, dev)
    for p in (sw.epsilon, sw.sigma):
        p.requires_grad_(False)               # the local order is what lam controls
    opt = torch.optim.Adam([sw.lam], lr=args.lr)
    hist = []
    for epoch in range(args.epochs):
        opt.zero_grad()
        loss = (order_of(integ, observables, args.frames, args.dt, dev) - target).pow(2).sum()
        loss.backward()
        opt.step()
        hist.append((float(loss.detach()), float(sw.lam.detach())))
        print("epoch %3d  loss %.3e  lam %.3f" % ((epoch,) + hist[-1]), flush=True)
    return hist


if __name__ == "__main__":
    main()
