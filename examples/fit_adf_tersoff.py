#!/usr/bin/env python
"""Fit the preferred angle h (and the strengths A, B) of Tersoff silicon to a target angle distribution plus RDF by
back-propagating through the MD trajectory: simulate -> angle_distribution, rdf -> loss -> backward (analytic adjoint,
HIP-graph replay) -> Adam.  The targets are the distributions of the published set (h = -0.59825); the fit starts from a
less tetrahedral preferred angle.

    python examples/fit_adf_tersoff.py --epochs 20
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KT = 1200.0         # K: hot enough for the angles to spread within 60 frames
A0 = 5.432          # Angstrom
MASS = 28.0855
BASIS = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75],
                  [.75, .75, .25]])


def build(h, dev, scale=1.0, seed=0):
    from mdgrad_amd import units
    from mdgrad_amd.interface import Stack, Tersoff
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.system import System
    rng = np.random.default_rng(seed)
    pos = np.array([(np.array([i, j, k]) + b) * A0 for i in range(2) for j in range(2) for k in range(2) for b in BASIS])
    pos = np.mod(pos + rng.normal(0, 0.1, pos.shape), 2 * A0)
    system = System(positions=pos, cell=np.array([2 * A0] * 3), masses=np.full(64, MASS), device=dev)
    kT = units.kB * KT
    system.set_velocities(rng.normal(0, np.sqrt(kT / MASS), pos.shape))
    p = Tersoff.PUBLISHED["silicon"]
    ts = Tersoff.silicon(system, h=h, A=scale * p["A"], B=scale * p["B"])
    integ = NoseHooverChain(Stack({"tersoff": ts}), system, T=kT, num_chains=3, Q=100.0, adjoint=True).to(dev)
    return system, ts, integ


def observe(system, integ, adf, gr, frames, dt, dev):
    from mdgrad_amd.sovlers import odeint_adjoint
    t = torch.Tensor([dt * i for i in range(frames)]).to(dev)
    y0 = tuple(integ.get_inital_states(wrap=True))
    v_t, q_t, pv_t = odeint_adjoint(integ, y0, t, method="NH_verlet")
    return adf(q_t[frames // 2:])[1], gr(q_t[frames // 2:])[2]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--dt", type=float, default=0.1, help="in Angstrom sqrt(amu / eV): 0.1 is about 1 fs")
    ap.add_argument("--h0", type=float, default=-0.45)
    ap.add_argument("--scale0", type=float, default=0.97, help="A and B start at this multiple of the published values")
    ap.add_argument("--lr", type=float, default=0.01)
    args = ap.parse_args(argv)
    from mdgrad_amd.observable import angle_distribution, rdf
    dev = "cuda:0"
    system, _, integ_true = build(-0.59825, dev)
    adf = angle_distribution(system, nbins=32, angle_range=(0.0, math.pi), cutoff=2.8, keep_angles=False)
    gr = rdf(system, nbins=48, r_range=(1.8, 4.8))
    with torch.no_grad():
        target_adf, target_gr = observe(system, integ_true, adf, gr, args.frames, args.dt, dev)
    system, ts, integ = build(args.h0, dev, scale=args.scale0)
    opt = torch.optim.Adam([{"params": [ts.h], "lr": args.lr},
                            {"params": [ts.A, ts.B], "lr": args.lr * 300.0}])       # A, B are of order 10^3 eV
    hist = []
    for epoch in range(args.epochs):
        opt.zero_grad()
        a, g = observe(system, integ, adf, gr, args.frames, args.dt, dev)
        loss = (a - target_adf).pow(2).sum() + (g - target_gr).pow(2).mean()
        loss.backward()
        opt.step()
        hist.append((float(loss.detach()), float(ts.h.detach()), float(ts.A.detach()), float(ts.B.detach())))
        print("epoch %3d  loss %.3e  h %.4f  A %.1f  B %.2f" % ((epoch,) + hist[-1]), flush=True)
    return hist


if __name__ == "__main__":
    main()
