#!/usr/bin/env python
"""Fit the preferred angle h of Tersoff silicon to a target angle distribution by trajectory reweighting (DiffTRe, Thaler and
Zavadlav 2021; mdgrad_amd/reweight.py) -- the counterpart of examples/fit_adf_tersoff.py WITHOUT a backward pass through the
dynamics: no adjoint launch runs anywhere.  With --multi: the Si-C attraction B[0, 1] = B[1, 0] of Tersoff's silicon carbide
(gradients tied) to a target RDF, the counterpart of examples/fit_rdf_sic.py.

    sample      R replicas of the 64-atom box, stacked into one system, at the current parameters under torch.no_grad()
                (NoseHooverChain, one thermostat chain per replica; --thermostat langevin: BAOAB steps instead)
    reweight    w_f ~ exp(-(U_theta(x_f) - U_ref(x_f)) / kT) over the stored frames (thermo.TersoffEnergy: one list-free
                launch that also emits dU/d(A, B, h); the backward pass is their weighted sum)
    observable  angle_distribution.normalise(rw.average(adf.per_frame(q_ref))), with --multi the g(r) of rdf.per_frame: the
                per-frame rows are computed once per sample
    resample    from the last frame of the previous sample, when the effective sample size drops below --n-eff of the frames

    python examples/fit_adf_reweight_tersoff.py --replicas 16 --epochs 30
    python examples/fit_adf_reweight_tersoff.py --multi --replicas 16 --epochs 30

On an MI355X at the defaults: h -0.45 -> -0.570 after 30 epochs (-0.582 at epoch 20; target -0.59825; loss 2.3e-04 -> 7.9e-06,
3 resamples); --multi: B[0, 1] 375.4 -> 394.7 (target 395.1; loss 6.4e-04 -> 1.8e-04, 1 resample).  The samples are short
(80 resp. 120 frames of 16 replicas), so the last few percent are sampling noise.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H_TRUE = -0.59825   # Tersoff 1988
BASIS = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75],
                  [.75, .75, .25]])
# (temperature in K, cubic lattice constant in Angstrom): silicon, zincblende SiC
SETUP = {False: (1200.0, 5.432), True: (1500.0, 4.36)}
MASS = (28.0855, 12.011)


def build(value, dev, R, multi, thermostat="nhc", gamma=0.05, seed=0):
    """R replicas of the jittered 64-atom box (each its own jitter and velocities) as one stacked system, the model -- silicon
    with h = `value`, or SiC with B[0, 1] = B[1, 0] at `value` times the published entry -- and its integrator."""
    from mdgrad_amd import units
    from mdgrad_amd.interface import Stack, Tersoff, TersoffMulti
    from mdgrad_amd.md import Langevin, NoseHooverChain
    from mdgrad_amd.system import System
    T, a0 = SETUP[multi]
    rng = np.random.default_rng(seed)
    lat = np.array([(np.array([i, j, k]) + b) * a0 for i in range(2) for j in range(2) for k in range(2) for b in BASIS])
    types = (np.arange(64) % 8 >= 4).astype(np.int64)                  # --multi: 0 = Si on the fcc sites, 1 = C on the others
    mass = np.where(types == 0, MASS[0], MASS[1]) if multi else np.full(64, MASS[0])
    kT = units.kB * T
    system = System(positions=lat, cell=np.array([2 * a0] * 3), masses=mass, device=dev).replicate(R)
    system.set_positions(np.mod(np.tile(lat, (R, 1)) + rng.normal(0, 0.08, (R * 64, 3)), 2 * a0))
    system.set_velocities(rng.normal(0, 1, (R * 64, 3)) * np.sqrt(kT / np.tile(mass, R))[:, None])
    if multi:
        ts = TersoffMulti.silicon_carbide(system, types)
        with torch.no_grad():
            ts.B[0, 1] *= value
            ts.B[1, 0] *= value
    else:
        ts = Tersoff.silicon(system, h=value)
    stack = Stack({"tersoff": ts})
    if thermostat == "langevin":
        integ = Langevin(stack, system, T=kT, gamma=gamma, seed=seed).to(dev)
    else:
        integ = NoseHooverChain(stack, system, T=kT, num_chains=3, Q=100.0, adjoint=True).to(dev)
    return system, ts, integ, kT


def sample(integ, state, frames, dt, burn, box, thermostat="nhc"):
    """`frames` steps from `state` at the integrator's current parameters, without autograd.  Returns the frames after `burn`
    [frames - burn, R N, 3] (replica-stacked: the observables give a trailing R) and the last state, positions wrapped back
    into the cell."""
    from mdgrad_amd.sovlers import odeint_adjoint
    t = torch.Tensor([dt * i for i in range(frames)]).to(state[0].device)
    with torch.no_grad():
        out = odeint_adjoint(integ, tuple(s.clone() for s in state), t, method="baoab" if thermostat == "langevin" else "NH_verlet")
        q_t = out[1]
        last = tuple(s[-1].contiguous() if k != 1 else torch.remainder(s[-1], box).contiguous() for k, s in enumerate(out))
        return torch.remainder(q_t[burn:], box).contiguous(), last


def first_state(integ, thermostat):
    state = tuple(integ.get_inital_states(wrap=True))
    return state[:2] if thermostat == "langevin" else state


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--frames", type=int, default=None, help="MD steps (= stored frames) per sample (default 120; --multi: 200)")
    ap.add_argument("--burn", type=int, default=None,
                    help="frames of every sample left out of the averages (default 40; --multi: 80)")
    ap.add_argument("--dt", type=float, default=None,
                    help="in Angstrom sqrt(amu / eV): 0.1 is about 1 fs (default 0.2; --multi: 0.1, carbon is light)")
    ap.add_argument("--multi", action="store_true", help="fit B[0, 1] = B[1, 0] of SiC (TersoffMulti) to the RDF instead")
    ap.add_argument("--h0", type=float, default=-0.45, help="the preferred angle the silicon fit starts from")
    ap.add_argument("--scale0", type=float, default=0.95, help="--multi: B[0, 1] = B[1, 0] start at this multiple of the published value")
    ap.add_argument("--lr", type=float, default=None, help="Adam step (default 0.01 for h, 0.7 for B)")
    ap.add_argument("--n-eff", type=float, default=0.9, help="resample when n_eff falls below this fraction of the frames")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--thermostat", choices=("nhc", "langevin"), default="nhc",
                    help="the sampler: NoseHooverChain, or Langevin (BAOAB)")
    ap.add_argument("--gamma", type=float, default=0.05, help="friction of --thermostat langevin")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from mdgrad_amd.observable import angle_distribution, rdf
    from mdgrad_amd.reweight import Reweighting
    from mdgrad_amd.thermo import TersoffEnergy
    dev, R, multi, th = args.device, args.replicas, args.multi, args.thermostat
    for name, value in (("frames", (120, 200)), ("burn", (40, 80)), ("dt", (0.2, 0.1)), ("lr", (0.01, 0.7))):
        if getattr(args, name) is None:
            setattr(args, name, value[multi])
    box = 2 * SETUP[multi][1]
    draw = lambda integ, state: sample(integ, state, args.frames, args.dt, args.burn, box, th)         # noqa: E731
    # target: the distribution of the published set
    system, ts_true, integ_true, kT = build(1.0 if multi else H_TRUE, dev, R, multi, th, args.gamma, 999 + args.seed)
    if multi:
        obs = rdf(system, nbins=48, r_range=(1.4, 4.2))
        curve = lambda rows: obs.normalise(rows)[2]                                                 # noqa: E731
        true = float(ts_true.B[0, 1].detach())
    else:
        obs = angle_distribution(system, nbins=32, angle_range=(0.0, math.pi), cutoff=2.8, keep_angles=False)
        curve = obs.normalise
        true = H_TRUE
    q_true, _ = draw(integ_true, first_state(integ_true, th))
    with torch.no_grad():
        target = curve(obs.per_frame(q_true).sum((0, 1)))
    # start from a wrong parameter; only that parameter trains
    system, ts, integ, kT = build(args.scale0 if multi else args.h0, dev, R, multi, th, args.gamma, args.seed)
    trained = ts.B if multi else ts.h
    for p in (ts.A, ts.B, ts.h):
        p.requires_grad_(p is trained)
    tie = torch.zeros(2, 2, device=dev)
    tie[0, 1] = tie[1, 0] = 1.0
    energy = TersoffEnergy(system, ts)
    q_ref, state = draw(integ, first_state(integ, th))
    rw = Reweighting(energy, kT, q_ref)

    def rows_of(q):
        with torch.no_grad():                 # once per sample, no autograd
            return obs.per_frame(q)
    rows = rows_of(q_ref)
    opt = torch.optim.Adam([trained], lr=args.lr)
    value = lambda: float((ts.B[0, 1] if multi else ts.h).detach())                                 # noqa: E731
    hist, resamples = [], 0
    for epoch in range(args.epochs):
        opt.zero_grad()
        w = rw.weights()
        diff = curve(rw.average(rows, w)) - target
        loss = diff.pow(2).mean() if multi else diff.pow(2).sum()
        loss.backward()                       # through the weights alone: a weighted sum of the dU/dtheta the launch emitted
        if multi:
            with torch.no_grad():             # only the Si-C entries move, and they move together
                ts.B.grad.copy_(tie * (ts.B.grad[0, 1] + ts.B.grad[1, 0]))
        opt.step()
        n_eff = rw.n_eff(w)                   # of the weights this step's loss was formed with
        with torch.no_grad():
            stale = rw.stale(args.n_eff)      # at the parameters just stepped to
        if stale:
            q_ref, state = draw(integ, state)
            rw.resample(q_ref)
            rows = rows_of(q_ref)
            resamples += 1
        # (loss, h or B[0, 1], n_eff, resamples so far)
        hist.append((float(loss.detach()), value(), n_eff, resamples))
        print("epoch %3d  loss %.3e  %s %.5f (target %.5f)  n_eff %.1f / %d  resamples %d"
              % (epoch, hist[-1][0], "B[0,1]" if multi else "h", hist[-1][1], true, n_eff, rw.n_frames, resamples), flush=True)
    return hist


if __name__ == "__main__":
    main()
