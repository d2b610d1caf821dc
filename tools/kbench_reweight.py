"""Times the kernels behind trajectory reweighting on the headline's frames (R replicas x T frames x 108 atoms, LJ 12-6, cutoff
2.5): thermo.PotentialEnergy forward, its parameters-only and full backward passes (csrc/energy.hip), rdf.per_frame forward and
backward (csrc/rdf_frames.hip), Pressure.virial forward and backward (csrc/virial.hip), and the kernels of
thermo.TabulatedEnergy (csrc/energy_table.hip through ops.EnergyTableFn: forward, backward to the nodes only, backward with
positions) for a small pairMLP tabulated once on 2 048 nodes -- all four per-frame families on the same frames.  HIP events
after warm-up; the variants alternate inside every repetition and min / median / max over the repetitions
are printed, so the run-to-run spread stands next to every difference.  Then one outer step of examples/fit_rdf_reweight.py
(with and without a resample) next to one of examples/fit_rdf_lj.py at equal replicas and steps (--no-fits leaves that out).

    python tools/kbench_reweight.py [--replicas 16384] [--frames 50] [--reps 7] [--fit-replicas 4096] [--no-fits]"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdgrad_amd import _lib, ops, potentials  # noqa: E402
from mdgrad_amd.interface import PairPotentials  # noqa: E402
from mdgrad_amd.observable import rdf  # noqa: E402
from mdgrad_amd.reweight import Reweighting  # noqa: E402
from mdgrad_amd.system import System, FaceCenteredCubic  # noqa: E402
from mdgrad_amd.thermo import PotentialEnergy, Pressure, TabulatedEnergy  # noqa: E402

DEV = "cuda:0"


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def kernels(R, T, reps, warmup):
    system = System(FaceCenteredCubic("H", (3, 3, 3), 1.6), device=DEV)
    F = R * T
    lat = torch.tensor(system.get_positions(), dtype=torch.float32, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    q = torch.remainder(lat + 0.05 * torch.randn(F, 108, 3, device=DEV, generator=g), 4.8)
    mdl = potentials.LennardJones(1.0, 1.0).to(DEV)
    pair = PairPotentials(system, mdl, cutoff=2.5)
    energy, press, obs = PotentialEnergy(system, pair), Pressure(system, pair), rdf(system, nbins=100, r_range=(0.75, 2.5))
    gU = torch.rand(F, device=DEV, generator=g) + 0.5
    gR = torch.randn(F, 100, device=DEV, generator=g)
    ps = [mdl.sigma, mdl.epsilon]
    # the tabulated family: the table of a small pairMLP, made once (the tabulation is torch autograd, not a kernel)
    mlp = potentials.pairMLP(n_gauss=8, r_start=0.5, r_end=2.5, n_layers=1, n_width=8, nonlinear="ELU").to(DEV)
    tab = TabulatedEnergy.from_terms(system, [(mlp, 2.5)], nodes=2048, check_range=False)
    table = tab.tabulate(0).detach().requires_grad_(True)
    u0, du, nodes = tab.grid(0)
    cell = _lib.make_cell(system.get_cell())

    def tabulated(x):
        return ops.EnergyTableFn.apply(x, table, cell, nodes, u0, du, 2.5, None)

    def graph(fn, positions):
        qq = q.detach().requires_grad_(positions)
        return qq, fn(qq)

    def bwd_of(fn, up, positions, leaves=ps):
        """a closure that times ONLY the backward pass: the forward runs outside the events"""
        def run():
            qq, out = graph(fn, positions)
            torch.cuda.synchronize()
            return event_ms(lambda: torch.autograd.grad((out * up).sum(), ([qq] if positions else []) + leaves))
        return run

    def fwd_of(fn):
        def run():
            with torch.no_grad():
                return event_ms(lambda: fn(q))
        return run

    variants = [("energy forward", fwd_of(energy)), ("virial forward", fwd_of(press.virial)),
                ("energy backward, parameters only", bwd_of(energy, gU, False)),
                ("energy backward, full rows", bwd_of(energy, gU, True)),
                ("virial backward", bwd_of(press.virial, gU, True)),
                ("rdf.per_frame forward", fwd_of(obs.per_frame)), ("rdf.per_frame backward", bwd_of(obs.per_frame, gR, True, [])),
                ("tabulated energy forward", fwd_of(tabulated)),
                ("tabulated energy backward, nodes only", bwd_of(tabulated, gU, False, [table])),
                ("tabulated energy backward, full rows", bwd_of(tabulated, gU, True, [table]))]
    ms = {name: [] for name, _ in variants}
    for rep in range(warmup + reps):
        for name, run in variants:                       # alternating: every repetition times every variant once
            t = run()
            if rep >= warmup:
                ms[name].append(t)
    print("%d replicas x %d frames x 108 atoms = %d frames, %d repetitions (min / median / max ms, ns per frame at the median)"
          % (R, T, F, reps), flush=True)
    for name, _ in variants:
        v = np.array(ms[name])
        print("  %-36s %9.3f / %9.3f / %9.3f ms   %8.1f ns/frame" % (name, v.min(), np.median(v), v.max(), 1e6 * np.median(v) / F),
              flush=True)


def load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fits(R, frames, reps, warmup):
    """one outer step of each example at R replicas and `frames` steps: host clock around a step that ends in a synchronise"""
    import time
    rw_ex, lj_ex = load("fit_rdf_reweight"), load("fit_rdf_lj")

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    # reweighting: sample + reference energies + per-frame rows (a resample), and the step on stored frames
    system, model, integ = rw_ex.build(0.92, 0.8, DEV)
    obs = rdf(system, nbins=100, r_range=(0.75, 2.5))
    energy = PotentialEnergy(system, integ.model)
    state = rw_ex.initial_state(system, R, 100, DEV)
    box = {}

    def resample():
        q_ref, box["state"] = rw_ex.sample(integ, box.get("state", state), frames, 0.005, 20)
        box["rw"] = Reweighting(energy, rw_ex.KT, q_ref)
        with torch.no_grad():
            box["rows"] = obs.per_frame(q_ref)

    g_target = None
    opt = torch.optim.Adam(integ.parameters(), lr=1e-4)

    def step():
        opt.zero_grad()
        w = box["rw"].weights()
        g = obs.normalise(box["rw"].average(box["rows"], w))[2]
        loss = (g - g_target).pow(2).mean()
        loss.backward()
        opt.step()
        box["rw"].stale()

    resample()
    with torch.no_grad():
        g_target = obs.normalise(box["rows"].sum((0, 1)))[2] * 1.01
    t_res, t_step = [], []
    for rep in range(warmup + reps):
        a, b = clock(resample), clock(step)
        if rep >= warmup:
            t_res.append(a), t_step.append(b)
    # the adjoint route: forward launch + rdf + adjoint launch
    system2, model2, integ2 = lj_ex.build(0.92, 0.8, DEV)
    obs2 = rdf(system2, nbins=100, r_range=(0.75, 2.5))
    opt2 = torch.optim.Adam(integ2.parameters(), lr=1e-4)
    gt2 = g_target.detach()

    def adjoint_step():
        opt2.zero_grad()
        v_t, q_t, pv_t = lj_ex.trajectories(system2, integ2, R, frames, 0.005, 100, DEV)
        loss = (obs2(q_t[:, 20:])[2] - gt2).pow(2).mean()
        loss.backward()
        opt2.step()

    t_adj = []
    for rep in range(warmup + reps):
        c = clock(adjoint_step)
        if rep >= warmup:
            t_adj.append(c)
    print("one outer step at %d replicas x %d steps (min / median / max ms over %d repetitions)" % (R, frames, reps))
    for name, v in (("fit_rdf_reweight: step on stored frames", t_step), ("fit_rdf_reweight: resample (sample + U_ref + rows)", t_res),
                    ("fit_rdf_lj: forward + rdf + adjoint", t_adj)):
        v = np.array(v)
        print("  %-52s %9.3f / %9.3f / %9.3f ms" % (name, v.min(), np.median(v), v.max()), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=16384)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fit-replicas", type=int, default=4096)
    ap.add_argument("--fit-frames", type=int, default=60)
    ap.add_argument("--no-fits", action="store_true", help="time the kernels only, not the outer steps of the examples")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_reweight: no HIP device -- timings are taken on the GPU only")
    print("device:", torch.cuda.get_device_name(0), flush=True)
    kernels(args.replicas, args.frames, args.reps, args.warmup)
    if not args.no_fits:
        fits(args.fit_replicas, args.fit_frames, max(3, args.reps // 2), 1)
