#!/usr/bin/env python
"""Learn a neural pair potential from a target RDF by trajectory reweighting (DiffTRe, Thaler and Zavadlav 2021;
mdgrad_amd/reweight.py): the loop of examples/fit_rdf_reweight.py with the model of examples/fit_rdf_pairmlp.py (pairMLP + a
soft repulsive LJFamily prior in a Stack).  No adjoint launch runs anywhere.

    sample      R replica trajectories at the current parameters through the fused TABULATED forward kernels (the integrator
                tabulates phi'/r of the Stack), under torch.no_grad()
    reweight    w_f ~ exp(-(U_theta(x_f) - U_ref(x_f)) / kT) over the stored frames; U from thermo.TabulatedEnergy: the prior
                exactly, the MLP from a table of phi re-made at every step, one batched launch each; the backward pass is one
                nodes-only launch whose node gradient autograd carries into the MLP
    observable  g(r) = rdf.normalise(rw.average(rdf.per_frame(q_ref))): the per-frame rows are computed once per sample
    resample    from the last frame of the previous sample, when the effective sample size drops below --n-eff of the frames

    python examples/fit_rdf_reweight_pairmlp.py --replicas 64 --epochs 60
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CELL, KT, CUT = 4.8, 1.0, 2.5


def build(pair_models, dev, seed=0):
    """(system, integrator) of the 108-atom liquid for a dict of pair modules"""
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NoseHooverChain
    from mdgrad_amd.system import System, FaceCenteredCubic
    system = System(FaceCenteredCubic("H", (3, 3, 3), 1.6), device=dev)
    system.set_temperature(KT, rng=np.random.default_rng(seed))
    model = Stack({k: PairPotentials(system, m, cutoff=CUT) for k, m in pair_models.items()})
    return system, NoseHooverChain(model, system, T=KT, num_chains=5, Q=50.0).to(dev)


def learned_model():
    """the pairMLP and the frozen prior of examples/fit_rdf_pairmlp.py"""
    from mdgrad_amd import potentials as P
    torch.manual_seed(0)
    mlp = P.pairMLP(n_gauss=25, r_start=0.0, r_end=2.5, n_layers=2, n_width=64, nonlinear="ELU")
    with torch.no_grad():
        mlp.layers[-1].weight.mul_(0.1)                                     # start close to the prior alone
    prior = P.LJFamily(epsilon=2.0, sigma=0.9, rep_pow=6, attr_pow=3)
    for p in prior.parameters():
        p.requires_grad_(False)
    return mlp, prior


def initial_state(system, R, seed, dev):
    """R replicas: jittered lattice, Maxwell-Boltzmann velocities, thermostat chains at rest"""
    rng = np.random.default_rng(seed)
    lat = system.get_positions()
    pos = np.mod(lat[None] + rng.uniform(-0.05, 0.05, (R,) + lat.shape), CELL).astype(np.float32)
    vel = rng.normal(0, np.sqrt(KT / 1.008), pos.shape).astype(np.float32)
    return torch.from_numpy(vel).to(dev), torch.from_numpy(pos).to(dev), torch.zeros(R, 5, device=dev)


def sample(integ, state, frames, dt, burn):
    """One fused forward launch from `state` at the integrator's current parameters, without autograd.  Returns the frames
    after `burn` [R, frames - burn, N, 3] and the last state (positions wrapped back into the cell)."""
    from mdgrad_amd import ops
    dev = state[0].device
    t = torch.Tensor([dt * i for i in range(frames)]).to(dev)
    spec = integ.fused_spec("NH_verlet")
    assert spec is not None, "expected a fused forward path"
    with torch.no_grad():
        v_t, q_t, pv_t = ops.fused_traj(state[0], state[1], state[2], t, spec.flat_params(), spec)
        last = (v_t[:, -1].contiguous(), torch.remainder(q_t[:, -1], CELL).contiguous(), pv_t[:, -1].contiguous())
        return q_t[:, burn:].contiguous(), last


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--frames", type=int, default=60, help="MD steps (= stored frames) per sample")
    ap.add_argument("--burn", type=int, default=20, help="frames of every sample left out of the averages")
    ap.add_argument("--dt", type=float, default=0.005)
    ap.add_argument("--lr", type=float, default=3e-3)
    ap.add_argument("--n-eff", type=float, default=0.9, help="resample when n_eff falls below this fraction of the frames")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from mdgrad_amd import potentials as P
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.reweight import Reweighting
    from mdgrad_amd.thermo import TabulatedEnergy
    dev, R = args.device, args.replicas
    # target: RDF of the "true" liquid, Lennard-Jones(1, 1) at T = 1
    system, integ_true = build({"lj": P.LennardJones(1.0, 1.0)}, dev, 999 + args.seed)
    obs = rdf(system, nbins=100, r_range=(0.75, 2.5))
    q_true, _ = sample(integ_true, initial_state(system, R, 999 + args.seed, dev), args.frames, args.dt, args.burn)
    with torch.no_grad():
        g_target = obs.normalise(obs.per_frame(q_true).sum((0, 1)))[2]
    # the learned model: sampled through its force table, reweighted through its energy table
    mlp, prior = learned_model()
    system, integ = build({"pairnn": mlp, "pair": prior}, dev, args.seed)
    assert getattr(integ.fused_spec("NH_verlet"), "table", False), "expected the tabulated fused path"
    energy = TabulatedEnergy(system, integ.model)
    q_ref, state = sample(integ, initial_state(system, R, 100 + args.seed, dev), args.frames, args.dt, args.burn)
    rw = Reweighting(energy, KT, q_ref)
    with torch.no_grad():
        rows = obs.per_frame(q_ref)                      # [R, T, nbins]: once per sample, no autograd
    opt = torch.optim.Adam(mlp.parameters(), lr=args.lr)
    hist, resamples = [], 0
    for epoch in range(args.epochs):
        opt.zero_grad()
        w = rw.weights()
        g = obs.normalise(rw.average(rows, w))[2]
        loss = (g - g_target).pow(2).mean()
        loss.backward()                                  # through the weights alone: one nodes-only launch, then the tabulation
        opt.step()
        n_eff = rw.n_eff(w)                              # of the weights this step's loss was formed with
        with torch.no_grad():
            stale = rw.stale(args.n_eff)                 # at the parameters just stepped to
        if stale:
            q_ref, state = sample(integ, state, args.frames, args.dt, args.burn)
            rw.resample(q_ref)
            with torch.no_grad():
                rows = obs.per_frame(q_ref)
            resamples += 1
        hist.append((float(loss.detach()), n_eff, resamples))                # (loss, n_eff, resamples so far)
        print("epoch %3d  loss %.5f  n_eff %.1f / %d  resamples %d" % ((epoch,) + hist[-1][:2] + (rw.n_frames, resamples)), flush=True)
    return hist


if __name__ == "__main__":
    main()
