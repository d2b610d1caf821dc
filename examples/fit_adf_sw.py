#!/usr/bin/env python
"""Fit the three-body strength lam of monatomic (mW) water to a target angle distribution by back-propagating through the MD
trajectory: simulate -> angle_distribution -> loss -> backward (analytic adjoint, HIP-graph replay) -> Adam.  The target is
the distribution of the published lam = 23.15; the fit starts from a less tetrahedral liquid.

    python examples/fit_adf_sw.py --epochs 20
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KT = 300.0          # K
A0 = 6.2            # Angstrom: 64 molecules in (2 A0)^3 is 1.0 g/cm^3
BASIS = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75],
                  [.75, .75, .25]])


def build(lam, dev, seed=0):
    from mdgrad_amd import units
    from mdgrad_amd.interface import StillingerWeber, Stack
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.system import System
    rng = np.random.default_rng(seed)
    pos = np.array([(np.array([i, j, k]) + b) * A0 for i in range(2) for j in range(2) for k in range(2) for b in BASIS])
    pos = np.mod(pos + rng.normal(0, 0.15, pos.shape), 2 * A0)
    system = System(positions=pos, cell=np.array([2 * A0] * 3), masses=np.full(64, 18.015), device=dev)
    kT = units.kB * KT
    system.set_velocities(rng.normal(0, np.sqrt(kT / 18.015), pos.shape))
    sw = StillingerWeber.mW(system, lam=lam)
    integ = NoseHooverChain(Stack({"sw": sw}), system, T=kT, num_chains=3, Q=100.0, adjoint=True).to(dev)
    return system, sw, integ


def adf_of(system, integ, obs, frames, dt, dev):
    from mdgrad_amd.sovlers import odeint_adjoint
    t = torch.Tensor([dt * i for i in range(frames)]).to(dev)
    y0 = tuple(integ.get_inital_states(wrap=True))
    v_t, q_t, pv_t = odeint_adjoint(integ, y0, t, method="NH_verlet")
    return obs(q_t[frames // 2:])[1]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--dt", type=float, default=0.25, help="in Angstrom sqrt(amu / eV): 0.25 is about 2.5 fs")
    ap.add_argument("--lam0", type=float, default=18.0)
    ap.add_argument("--lr", type=float, default=0.3)
    args = ap.parse_args(argv)
    from mdgrad_amd.observable import angle_distribution
    dev = "cuda:0"
    system, _, integ_true = build(23.15, dev)
    obs = angle_distribution(system, nbins=32, angle_range=(0.0, math.pi), cutoff=3.5, keep_angles=False)
    with torch.no_grad():
        target = adf_of(system, integ_true, obs, args.frames, args.dt, dev)
    system, sw, integ = build(args.lam0, dev)
    for p in (sw.epsilon, sw.sigma):
        p.requires_grad_(False)               # the angle distribution is what lam controls
    opt = torch.optim.Adam([sw.lam], lr=args.lr)
    hist = []
    for epoch in range(args.epochs):
        opt.zero_grad()
        loss = (adf_of(system, integ, obs, args.frames, args.dt, dev) - target).pow(2).sum()
        loss.backward()
        opt.step()
        hist.append((float(loss.detach()), float(sw.lam.detach())))
        print("epoch %3d  loss %.3e  lam %.3f" % ((epoch,) + hist[-1]), flush=True)
    return hist


if __name__ == "__main__":
    main()
