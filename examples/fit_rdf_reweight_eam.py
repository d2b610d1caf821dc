#!/usr/bin/env python
"""Fit an embedded-atom model of copper to a target RDF by trajectory reweighting (DiffTRe, Thaler and Zavadlav 2021;
mdgrad_amd/reweight.py) -- the counterpart of examples/fit_rdf_sc.py WITHOUT a backward pass through the dynamics: no adjoint
launch runs anywhere.  The same copper box (3 x 3 x 3 fcc cells at 1000 K), the same target (the RDF of the published
Sutton-Chen constants) and the same loss.

    sample      R replicas of the 108-atom box, stacked into one system, at the current parameters under torch.no_grad()
                (NoseHooverChain, one thermostat chain per replica)
    reweight    w_f ~ exp(-(U_theta(x_f) - U_ref(x_f)) / kT) over the stored frames (thermo.EAMEnergy: one list-free launch;
                for the Sutton-Chen form it also emits dU/d(epsilon, a, c) and the backward pass is their weighted sum, for
                the tabulated form the backward pass is one more walk with a fixed-point scatter into the nodes)
    observable  g(r) = rdf.normalise(rw.average(rdf.per_frame(q_ref))): the per-frame rows are computed once per sample
    resample    from the last frame of the previous sample, when the effective sample size drops below --n-eff of the frames

Default: the Sutton-Chen form, starting 5 % off in epsilon and a; a comes back towards 3.61 (at fixed volume the RDF of a
solid constrains the stiffness, which a dominates; at the default step an epoch moves a by 0.011, enough to drop n_eff below
0.9 F, so this mode resamples after nearly every epoch -- a smaller --lr or --n-eff reuses a sample longer).
--tabulated: the same start as tables (EAM.from_sutton_chen) with the embedding nodes trainable -- a few hundred parameters
fitted to the same target from the same forward launches; the claim there is a falling loss, not recovered constants.

    python examples/fit_rdf_reweight_eam.py --replicas 16 --epochs 30
    python examples/fit_rdf_reweight_eam.py --tabulated
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


def build(eps, a, dev, R, seed=0, tabulated=False, nodes=256):
    """R replicas of the jittered 108-atom copper box (each its own jitter and velocities) as one stacked system, the model at
    (eps, a) -- SuttonChen, or its tabulated twin with trainable embedding nodes -- and its Nose-Hoover integrator."""
    from mdgrad_amd import units
    from mdgrad_amd.interface import EAM, SuttonChen, Stack
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.system import System
    rng = np.random.default_rng(seed)
    lat = np.array([(np.array([i, j, k]) + b) * A0 for i in range(3) for j in range(3) for k in range(3) for b in BASIS])
    kT = units.kB * KT
    system = System(positions=lat, cell=np.array([3 * A0] * 3), masses=np.full(108, 63.546), device=dev).replicate(R)
    system.set_positions(np.mod(np.tile(lat, (R, 1)) + rng.normal(0, 0.1, (R * 108, 3)), 3 * A0))
    system.set_velocities(rng.normal(0, np.sqrt(kT / 63.546), (R * 108, 3)))
    if tabulated:
        model = EAM.from_sutton_chen(system, (eps, a, C, N, M), cutoff=CUTOFF, n_r=nodes, n_rho=nodes, trainable=("embed",))
    else:
        model = SuttonChen(system, eps, a, C, N, M, CUTOFF)
    integ = NoseHooverChain(Stack({"eam": model}), system, T=kT, num_chains=3, Q=100.0, adjoint=True).to(dev)
    return system, model, integ, kT


def sample(integ, state, frames, dt, burn):
    """`frames` steps from `state` at the integrator's current parameters, without autograd.  Returns the frames after `burn`
    [frames - burn, R N, 3] (replica-stacked: the observables give a trailing R) and the last state, positions wrapped back
    into the cell."""
    from mdgrad_amd.sovlers import odeint_adjoint
    t = torch.Tensor([dt * i for i in range(frames)]).to(state[0].device)
    with torch.no_grad():
        v_t, q_t, pv_t = odeint_adjoint(integ, tuple(s.clone() for s in state), t, method="NH_verlet")
        last = (v_t[-1].contiguous(), torch.remainder(q_t[-1], 3 * A0).contiguous(), pv_t[-1].contiguous())
        return torch.remainder(q_t[burn:], 3 * A0).contiguous(), last


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--frames", type=int, default=60, help="MD steps (= stored frames) per sample")
    ap.add_argument("--burn", type=int, default=20, help="frames of every sample left out of the averages")
    ap.add_argument("--dt", type=float, default=0.5, help="in Angstrom sqrt(amu / eV): 0.5 is about 5 fs")
    ap.add_argument("--off", type=float, default=0.05, help="relative error of the starting epsilon (above) and a (below)")
    ap.add_argument("--lr", type=float, default=0.003, help="Adam step, relative to the scale of each parameter")
    ap.add_argument("--n-eff", type=float, default=0.9, help="resample when n_eff falls below this fraction of the frames")
    ap.add_argument("--tabulated", action="store_true", help="fit the embedding nodes of the tabulated twin instead of (epsilon, a)")
    ap.add_argument("--nodes", type=int, default=256, help="nodes per table of --tabulated")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.reweight import Reweighting
    from mdgrad_amd.thermo import EAMEnergy
    dev, R = args.device, args.replicas
    # target: the RDF of the published constants
    system, _, integ_true, kT = build(EPS, A, dev, R, 999 + args.seed)
    obs = rdf(system, nbins=64, r_range=(2.0, CUTOFF))
    q_true, _ = sample(integ_true, integ_true.get_inital_states(wrap=True), args.frames, args.dt, args.burn)
    with torch.no_grad():
        g_target = obs.normalise(obs.per_frame(q_true).sum((0, 1)))[2]
    # start 5 % off in both
    system, model, integ, kT = build(EPS * (1 + args.off), A * (1 - args.off), dev, R, args.seed, args.tabulated, args.nodes)
    if args.tabulated:
        start = model.embed_nodes.detach().clone()
        opt = torch.optim.Adam([model.embed_nodes], lr=args.lr * EPS * C)
    else:
        model.c.requires_grad_(False)         # c and epsilon enter the cohesion together; the fit is over (epsilon, a)
        opt = torch.optim.Adam([{"params": [model.epsilon], "lr": args.lr * EPS}, {"params": [model.a], "lr": args.lr * A}])
    energy = EAMEnergy(system, model)
    q_ref, state = sample(integ, integ.get_inital_states(wrap=True), args.frames, args.dt, args.burn)
    rw = Reweighting(energy, kT, q_ref)
    with torch.no_grad():
        rows = obs.per_frame(q_ref)           # [T, R, nbins]: once per sample, no autograd
    hist, resamples = [], 0
    for epoch in range(args.epochs):
        opt.zero_grad()
        w = rw.weights()
        loss = (obs.normalise(rw.average(rows, w))[2] - g_target).pow(2).mean()
        loss.backward()                       # through the weights alone: no pair is visited for (epsilon, a), one walk for the nodes
        opt.step()
        n_eff = rw.n_eff(w)                   # of the weights this step's loss was formed with
        with torch.no_grad():
            stale = rw.stale(args.n_eff)      # at the parameters just stepped to
        if stale:
            q_ref, state = sample(integ, state, args.frames, args.dt, args.burn)
            rw.resample(q_ref)
            with torch.no_grad():
                rows = obs.per_frame(q_ref)
            resamples += 1
        if args.tabulated:
            # (loss, largest change of an embedding node entry so far, n_eff, resamples so far)
            hist.append((float(loss.detach()), float((model.embed_nodes.detach() - start).abs().max()), n_eff, resamples))
            print("epoch %3d  loss %.3e  max |d embed| %.3e  n_eff %.1f / %d  resamples %d"
                  % ((epoch,) + hist[-1][:3] + (rw.n_frames, resamples)), flush=True)
        else:
            # (loss, epsilon, a, n_eff, resamples so far)
            hist.append((float(loss.detach()), float(model.epsilon.detach()), float(model.a.detach()), n_eff, resamples))
            print("epoch %3d  loss %.3e  epsilon %.5e  a %.4f  n_eff %.1f / %d  resamples %d"
                  % ((epoch,) + hist[-1][:4] + (rw.n_frames, resamples)), flush=True)
    return hist


if __name__ == "__main__":
    main()
