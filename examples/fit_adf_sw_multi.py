#!/usr/bin/env python
"""Fit the cross three-body strengths of a binary Stillinger-Weber liquid to a target angle distribution and RDF by
back-propagating through the MD trajectory: simulate -> angle_distribution + rdf -> loss -> backward (analytic adjoint,
HIP-graph replay) -> Adam.  The system is mW water (species 0) with a second, slightly smaller and less tetrahedral
coarse-grained species (1), built with StillingerWeberMulti's mixing rule.  The target comes from a run whose cross strengths
lam[0, 1, 1] and lam[1, 0, 0] (a centre with two unlike ends) are `--scale` times the mixed value; the fit starts from the
mixed value and moves the two entries together (their gradients are summed and written to both).

    python examples/fit_adf_sw_multi.py --epochs 20
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KT = 300.0          # K
A0 = 6.2            # Angstrom
BASIS = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75],
                  [.75, .75, .25]])
CROSS = ((0, 1, 1), (1, 0, 0))


def build(dev, scale=1.0, seed=0):
    from mdgrad_amd import units
    from mdgrad_amd.interface import StillingerWeberMulti, Stack
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.system import System
    rng = np.random.default_rng(seed)
    pos = np.array([(np.array([i, j, k]) + b) * A0 for i in range(2) for j in range(2) for k in range(2) for b in BASIS])
    pos = np.mod(pos + rng.normal(0, 0.15, pos.shape), 2 * A0)
    types = (np.arange(64) % 8 >= 4).astype(np.int32)          # the two fcc sublattices: every atom starts among unlike neighbours
    system = System(positions=pos, cell=np.array([2 * A0] * 3), masses=np.full(64, 18.015), device=dev)
    kT = units.kB * KT
    system.set_velocities(rng.normal(0, np.sqrt(kT / 18.015), pos.shape))
    mW = StillingerWeberMulti.PUBLISHED["mW"]
    solute = dict(epsilon=0.9 * mW["epsilon"], sigma=0.97 * mW["sigma"], lam=18.0)
    sw = StillingerWeberMulti(system, types, [mW, solute])
    with torch.no_grad():
        for idx in CROSS:
            sw.lam[idx] *= scale
    integ = NoseHooverChain(Stack({"sw": sw}), system, T=kT, num_chains=3, Q=100.0, adjoint=True).to(dev)
    return system, sw, integ


def observe(integ, adf, gr, frames, dt, dev):
    from mdgrad_amd.sovlers import odeint_adjoint
    t = torch.Tensor([dt * i for i in range(frames)]).to(dev)
    y0 = tuple(integ.get_inital_states(wrap=True))
    v_t, q_t, pv_t = odeint_adjoint(integ, y0, t, method="NH_verlet")
    return adf(q_t[frames // 2:])[1], gr(q_t[frames // 2:])[2]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--dt", type=float, default=0.25, help="in Angstrom sqrt(amu / eV): 0.25 is about 2.5 fs")
    ap.add_argument("--scale", type=float, default=1.25, help="the target's cross strengths, as a multiple of the mixed value")
    ap.add_argument("--lr", type=float, default=0.3)
    args = ap.parse_args(argv)
    from mdgrad_amd.observable import angle_distribution, rdf
    dev = "cuda:0"
    system, sw_true, integ_true = build(dev, scale=args.scale)
    adf = angle_distribution(system, nbins=32, angle_range=(0.0, math.pi), cutoff=3.5, keep_angles=False)
    gr = rdf(system, nbins=48, r_range=(2.0, 5.5))
    with torch.no_grad():
        t_adf, t_gr = observe(integ_true, adf, gr, args.frames, args.dt, dev)
    want = float(sw_true.lam[CROSS[0]].detach())
    system, sw, integ = build(dev)
    for p in (sw.epsilon, sw.sigma):
        p.requires_grad_(False)
    opt = torch.optim.Adam([sw.lam], lr=args.lr)
    tie = torch.zeros(2, 2, 2, device=dev)
    for idx in CROSS:
        tie[idx] = 1.0
    hist = []
    for epoch in range(args.epochs):
        opt.zero_grad()
        a, g = observe(integ, adf, gr, args.frames, args.dt, dev)
        loss = (a - t_adf).pow(2).sum() + (g - t_gr).pow(2).mean()
        loss.backward()
        with torch.no_grad():                                           # only the two cross entries move, and they move together
            sw.lam.grad.copy_(tie * sum(sw.lam.grad[idx] for idx in CROSS))
        opt.step()
        hist.append((float(loss.detach()),) + tuple(float(sw.lam[idx].detach()) for idx in CROSS))
        print("epoch %3d  loss %.3e  lam[0,1,1] %.3f  lam[1,0,0] %.3f  (target %.3f)" % ((epoch,) + hist[-1] + (want,)), flush=True)
    return hist


if __name__ == "__main__":
    main()
