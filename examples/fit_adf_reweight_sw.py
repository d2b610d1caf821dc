#!/usr/bin/env python
"""Fit the three-body strength lam of monatomic (mW) water to a target angle distribution by trajectory reweighting (DiffTRe,
Thaler and Zavadlav 2021; mdgrad_amd/reweight.py) -- the counterpart of examples/fit_adf_sw.py WITHOUT a backward pass through
the dynamics: no adjoint launch runs anywhere.

    sample      R replicas of the 64-molecule box, stacked into one system, at the current parameters under torch.no_grad()
                (NoseHooverChain, one thermostat chain per replica)
    reweight    w_f ~ exp(-(U_theta(x_f) - U_ref(x_f)) / kT) over the stored frames (thermo.StillingerWeberEnergy: one
                list-free launch that also emits dU/d(epsilon, sigma, lam); the backward pass is their weighted sum)
    observable  adf = angle_distribution.normalise(rw.average(adf.per_frame(q_ref))): the per-frame rows are computed once per
                sample; --rdf-weight adds the reweighted g(r) (rdf.per_frame) to the loss
    resample    from the last frame of the previous sample, when the effective sample size drops below --n-eff of the frames

    python examples/fit_adf_reweight_sw.py --replicas 16 --epochs 30
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
LAM_TRUE = 23.15
BASIS = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75],
                  [.75, .75, .25]])


def build(lam, dev, R, seed=0):
    """R replicas of the jittered 64-molecule diamond box (each its own jitter and velocities) as one stacked system, the mW
    model at `lam` and its Nose-Hoover integrator."""
    from mdgrad_amd import units
    from mdgrad_amd.interface import StillingerWeber, Stack
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.system import System
    rng = np.random.default_rng(seed)
    lat = np.array([(np.array([i, j, k]) + b) * A0 for i in range(2) for j in range(2) for k in range(2) for b in BASIS])
    kT = units.kB * KT
    system = System(positions=lat, cell=np.array([2 * A0] * 3), masses=np.full(64, 18.015), device=dev).replicate(R)
    system.set_positions(np.mod(np.tile(lat, (R, 1)) + rng.normal(0, 0.15, (R * 64, 3)), 2 * A0))
    system.set_velocities(rng.normal(0, np.sqrt(kT / 18.015), (R * 64, 3)))
    sw = StillingerWeber.mW(system, lam=lam)
    integ = NoseHooverChain(Stack({"sw": sw}), system, T=kT, num_chains=3, Q=100.0, adjoint=True).to(dev)
    return system, sw, integ, kT


def sample(integ, state, frames, dt, burn):
    """`frames` steps from `state` at the integrator's current parameters, without autograd.  Returns the frames after `burn`
    [frames - burn, R N, 3] (replica-stacked: the observables give a trailing R) and the last state, positions wrapped back
    into the cell."""
    from mdgrad_amd.sovlers import odeint_adjoint
    t = torch.Tensor([dt * i for i in range(frames)]).to(state[0].device)
    with torch.no_grad():
        v_t, q_t, pv_t = odeint_adjoint(integ, tuple(s.clone() for s in state), t, method="NH_verlet")
        last = (v_t[-1].contiguous(), torch.remainder(q_t[-1], 2 * A0).contiguous(), pv_t[-1].contiguous())
        return torch.remainder(q_t[burn:], 2 * A0).contiguous(), last


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--frames", type=int, default=60, help="MD steps (= stored frames) per sample")
    ap.add_argument("--burn", type=int, default=20, help="frames of every sample left out of the averages")
    ap.add_argument("--dt", type=float, default=0.25, help="in Angstrom sqrt(amu / eV): 0.25 is about 2.5 fs")
    ap.add_argument("--lam0", type=float, default=18.0)
    ap.add_argument("--lr", type=float, default=0.3)
    ap.add_argument("--n-eff", type=float, default=0.9, help="resample when n_eff falls below this fraction of the frames")
    ap.add_argument("--rdf-weight", type=float, default=0.0, help="weight of the reweighted g(r) in the loss (0: angles alone)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from mdgrad_amd.observable import angle_distribution, rdf
    from mdgrad_amd.reweight import Reweighting
    from mdgrad_amd.thermo import StillingerWeberEnergy
    dev, R = args.device, args.replicas
    # target: the distributions of the published lam
    system, _, integ_true, kT = build(LAM_TRUE, dev, R, 999 + args.seed)
    adf = angle_distribution(system, nbins=32, angle_range=(0.0, math.pi), cutoff=3.5, keep_angles=False)
    gr = rdf(system, nbins=64, r_range=(2.0, 5.5)) if args.rdf_weight else None
    q_true, _ = sample(integ_true, integ_true.get_inital_states(wrap=True), args.frames, args.dt, args.burn)
    with torch.no_grad():
        adf_target = adf.normalise(adf.per_frame(q_true).sum((0, 1)))
        g_target = gr.normalise(gr.per_frame(q_true).sum((0, 1)))[2] if gr is not None else None
    # start from a less tetrahedral liquid
    system, sw, integ, kT = build(args.lam0, dev, R, args.seed)
    for p in (sw.epsilon, sw.sigma):
        p.requires_grad_(False)               # the angle distribution is what lam controls
    energy = StillingerWeberEnergy(system, sw)
    q_ref, state = sample(integ, integ.get_inital_states(wrap=True), args.frames, args.dt, args.burn)
    rw = Reweighting(energy, kT, q_ref)

    def rows_of(q):
        with torch.no_grad():                 # once per sample, no autograd
            return adf.per_frame(q), (gr.per_frame(q) if gr is not None else None)
    a_rows, g_rows = rows_of(q_ref)
    opt = torch.optim.Adam([sw.lam], lr=args.lr)
    hist, resamples = [], 0
    for epoch in range(args.epochs):
        opt.zero_grad()
        w = rw.weights()
        loss = (adf.normalise(rw.average(a_rows, w)) - adf_target).pow(2).sum()
        if gr is not None:
            loss = loss + args.rdf_weight * (gr.normalise(rw.average(g_rows, w))[2] - g_target).pow(2).mean()
        loss.backward()                       # through the weights alone: a weighted sum of the dU/dtheta the launch emitted
        opt.step()
        n_eff = rw.n_eff(w)                   # of the weights this step's loss was formed with
        with torch.no_grad():
            stale = rw.stale(args.n_eff)      # at the parameters just stepped to
        if stale:
            q_ref, state = sample(integ, state, args.frames, args.dt, args.burn)
            rw.resample(q_ref)
            a_rows, g_rows = rows_of(q_ref)
            resamples += 1
        # (loss, lam, n_eff, resamples so far)
        hist.append((float(loss.detach()), float(sw.lam.detach()), n_eff, resamples))
        print("epoch %3d  loss %.3e  lam %.3f  n_eff %.1f / %d  resamples %d" % ((epoch,) + hist[-1][:3] + (rw.n_frames, resamples)),
              flush=True)
    return hist


if __name__ == "__main__":
    main()
