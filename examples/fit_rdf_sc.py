#!/usr/bin/env python
"""Fit the Sutton-Chen parameters (epsilon, a) of copper to a radial distribution function by back-propagating through the
MD trajectory: simulate -> rdf -> loss -> backward (analytic adjoint, HIP-graph replay) -> Adam.  The target is the RDF of a
short trajectory of 108 hot copper atoms generated with the published values; the fit starts 5 % off in both.  At fixed volume
the RDF of a solid constrains the stiffness, which a dominates: a comes back towards 3.61, epsilon is barely determined.

    python examples/fit_rdf_sc.py --epochs 8
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KT = 1000.0         # K
A0 = 3.61           # Angstrom: 3 x 3 x 3 fcc cells
CUTOFF = 5.2        # Angstrom (the usual 2 a = 7.22 exceeds half of this small cell)
EPS, A, C, N, M = 1.2382e-2, 3.61, 39.432, 9, 6
BASIS = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])


def build(eps, a, dev, seed=0):
    from mdgrad_amd import units
    from mdgrad_amd.interface import SuttonChen, Stack
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.system import System
    rng = np.random.default_rng(seed)
    pos = np.array([(np.array([i, j, k]) + b) * A0 for i in range(3) for j in range(3) for k in range(3) for b in BASIS])
    pos = np.mod(pos + rng.normal(0, 0.1, pos.shape), 3 * A0)
    system = System(positions=pos, cell=np.array([3 * A0] * 3), masses=np.full(108, 63.546), device=dev)
    kT = units.kB * KT
    system.set_velocities(rng.normal(0, np.sqrt(kT / 63.546), pos.shape))
    sc = SuttonChen(system, eps, a, C, N, M, CUTOFF)
    integ = NoseHooverChain(Stack({"sc": sc}), system, T=kT, num_chains=3, Q=100.0, adjoint=True).to(dev)
    return system, sc, integ


def rdf_of(system, integ, obs, frames, dt, dev):
    from mdgrad_amd.sovlers import odeint_adjoint
    t = torch.Tensor([dt * i for i in range(frames)]).to(dev)
    y0 = tuple(integ.get_inital_states(wrap=True))
    v_t, q_t, pv_t = odeint_adjoint(integ, y0, t, method="NH_verlet")
    return obs(q_t[frames // 2:])[2]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--dt", type=float, default=0.5, help="in Angstrom sqrt(amu / eV): 0.5 is about 5 fs")
    ap.add_argument("--off", type=float, default=0.05, help="relative error of the starting epsilon (above) and a (below)")
    ap.add_argument("--lr", type=float, default=0.01, help="Adam step, relative to the published value of each parameter")
    args = ap.parse_args(argv)
    from mdgrad_amd.observable import rdf
    dev = "cuda:0"
    system, _, integ_true = build(EPS, A, dev)
    obs = rdf(system, nbins=64, r_range=(2.0, CUTOFF))
    with torch.no_grad():
        target = rdf_of(system, integ_true, obs, args.frames, args.dt, dev)
    system, sc, integ = build(EPS * (1 + args.off), A * (1 - args.off), dev)
    sc.c.requires_grad_(False)                # c and epsilon enter the cohesion together; the fit is over (epsilon, a)
    opt = torch.optim.Adam([{"params": [sc.epsilon], "lr": args.lr * EPS}, {"params": [sc.a], "lr": args.lr * A}])
    hist = []
    for epoch in range(args.epochs):
        opt.zero_grad()
        loss = (rdf_of(system, integ, obs, args.frames, args.dt, dev) - target).pow(2).mean()
        loss.backward()
        opt.step()
        hist.append((float(loss.detach()), float(sc.epsilon.detach()), float(sc.a.detach())))
        print("epoch %3d  loss %.3e  epsilon %.5e  a %.4f" % ((epoch,) + hist[-1]), flush=True)
    return hist


if __name__ == "__main__":
    main()
