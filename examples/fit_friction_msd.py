#!/usr/bin/env python
"""Fit the friction of a Langevin thermostat to a transport property: a Lennard-Jones fluid whose `gamma` is trained so that
the diffusion coefficient of its mean-squared displacement meets a target -- the one a known `gamma` produces.  Every pass
starts from the same state and uses the same seed (common random numbers), so the loss is a smooth, deterministic function of
gamma and its gradient is the exact discrete adjoint of the BAOAB map (md.Langevin).

    python examples/fit_friction_msd.py --epochs 40
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(gamma, dev, trainable, seed):
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials
    from mdgrad_amd.md import Langevin
    from mdgrad_amd.system import System, FaceCenteredCubic
    system = System(FaceCenteredCubic("H", (3, 3, 3), 1.6), device=dev)
    system.set_temperature(1.0, rng=np.random.default_rng(0))
    pair = PairPotentials(system, P.LennardJones(1.0, 1.0), cutoff=2.5)
    for p in pair.parameters():
        p.requires_grad_(False)                   # only the friction is fitted
    integ = Langevin(pair, system, T=1.0, gamma=gamma, seed=seed, trainable_gamma=trainable).to(dev)
    return system, integ


def diffusion(system, integ, y0, t, dt, seed, t_range):
    """D of one trajectory from y0 with the noise stream (seed, step 0); positions are not wrapped inside a call."""
    from mdgrad_amd.observable import msd, diffusion_coefficient
    from mdgrad_amd.sovlers import odeint_adjoint
    integ.reseed(seed, 0)
    _, q_t = odeint_adjoint(integ, tuple(x.clone() for x in y0), t, method="baoab")
    m = msd(system, t_range=t_range)(q_t)
    return diffusion_coefficient(m, dt, fit_range=(t_range // 4, t_range))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--dt", type=float, default=0.005)
    ap.add_argument("--gamma-true", type=float, default=4.0)
    ap.add_argument("--gamma-start", type=float, default=1.0)
    ap.add_argument("--lr", type=float, default=0.15)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    dev = args.device
    t = torch.Tensor([args.dt * k for k in range(args.frames)]).to(dev)
    t_range = args.frames // 2
    system, integ_true = build(args.gamma_true, dev, False, args.seed)
    y0 = integ_true.get_inital_states(wrap=True)
    with torch.no_grad():
        D_target = float(diffusion(system, integ_true, y0, t, args.dt, args.seed, t_range))
    system, integ = build(args.gamma_start, dev, True, args.seed)
    opt = torch.optim.Adam([integ.gamma], lr=args.lr)
    hist = []
    for epoch in range(args.epochs):
        opt.zero_grad()
        D = diffusion(system, integ, y0, t, args.dt, args.seed, t_range)
        loss = (D / D_target - 1.0).pow(2)
        loss.backward()
        hist.append((float(loss.detach()), float(integ.gamma.detach()), float(D.detach())))
        print("epoch %3d  loss %.3e  gamma %.4f  D %.5f  (target D %.5f at gamma %.3f)"
              % ((epoch,) + hist[-1] + (D_target, args.gamma_true)), flush=True)
        opt.step()
        with torch.no_grad():
            integ.gamma.clamp_(min=1e-3)          # a trainable friction has to stay positive
    print("start gamma %.4f  final gamma %.4f  target gamma %.4f  final loss %.3e"
          % (args.gamma_start, float(integ.gamma.detach()), args.gamma_true, hist[-1][0]))
    return hist


if __name__ == "__main__":
    main()
