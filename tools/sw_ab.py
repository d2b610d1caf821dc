"""A/B of two checkouts on the Stillinger-Weber terms (StillingerWeber / ops.sw_eval, StillingerWeberMulti /
ops.sw_multi_eval, thermo.StillingerWeberEnergy): one SHA-256 per output on seeded inputs -- the three launch levels with and
without `into=`, the per-atom parameter rows, autograd's gradients in xyz and in (epsilon, sigma, lam), the double backward,
force and force_vjp -- for 64 atoms of jittered diamond, a 37-atom gas with an empty row and three replicas of 16; S = 1, two
identical sets, two unlike sets, asymmetric tables and three species; 1 and 5 frames and a batch with an overflowing row.  Only
public classes and ops entry points are used, so the same file runs in a checkout from before a change of the layers under
them; the package imported is the one of the checkout the file lies in.

    python <checkout A>/tools/sw_ab.py > a.txt ; python <checkout B>/tools/sw_ab.py > b.txt ; diff a.txt b.txt

Every sum of these kernels runs in a fixed order, so equal bits are the expectation, not luck: a line that differs is a
changed operation, a changed order or a factor applied elsewhere.  The first word of a line names the kernel (K23, K28, K34)."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdgrad_amd import ops  # noqa: E402
from mdgrad_amd.interface import StillingerWeber, StillingerWeberMulti  # noqa: E402
from mdgrad_amd.system import System  # noqa: E402
from mdgrad_amd.thermo import StillingerWeberEnergy  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
BASIS = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75], [.75, .75, .25]])
SI = StillingerWeberMulti.PUBLISHED["silicon"]
OTHER = dict(epsilon=1.8, sigma=2.2, lam=25.0, gamma=1.1)
THIRD = dict(epsilon=2.5, sigma=1.9, lam=18.0, a=1.9)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:24]


def diamond64(seed, jitter=0.3, a0=5.431):
    g = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    x = (g[:, None, :] + BASIS[None]).reshape(-1, 3) * a0
    L = np.full(3, 2 * a0)
    return np.mod(x + np.random.default_rng(seed).normal(0, jitter, x.shape), L).astype(F32), L.astype(F32)


def gas(n, box, corner, seed, dmin=2.0):
    """n - 3 atoms in a corner of the box (minimum separation dmin), one atom far from everything and two that see only each other"""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n - 3:
        p = rng.uniform(0, corner, 3)
        if all(np.linalg.norm(p - q) >= dmin for q in pts):
            pts.append(p)
    far = box - np.array([3.0, 3.5, 4.0])
    return np.array(pts + [far, [far[0], 4.0, far[2] - 1.0], [far[0], 4.0, far[2] + 1.3]]).astype(F32), box.astype(F32)


def geometries():
    """name -> (system, positions [N, 3], atoms per replica)"""
    out = {}
    x, L = diamond64(64)
    out["si64"] = (System(positions=x, cell=L, masses=np.full(64, 28.0855), device=DEV), x, 64)
    x, L = gas(37, np.array([14.0, 15.0, 16.0]), 7.5, 37)
    out["gas37"] = (System(positions=x, cell=L, masses=np.full(37, 28.0855), device=DEV), x, 37)
    box = np.array([8.0, 8.0, 8.5])
    rng = np.random.default_rng(16)
    base = []
    while len(base) < 16:
        p = rng.uniform(0, 1, 3) * box
        if all(np.linalg.norm((p - q) - np.rint((p - q) / box) * box) >= 2.0 for q in base):
            base.append(p)
    base = np.array(base).astype(F32)
    x = np.concatenate([np.mod(base + rng.normal(0, 0.1, base.shape), box) for _ in range(3)]).astype(F32)
    out["3x16"] = (System(positions=base, cell=box.astype(F32), masses=np.full(16, 28.0855), device=DEV).replicate(3), x, 16)
    return out


def multi_modules(system, n):
    """name -> StillingerWeberMulti on n atoms per replica"""
    rng = np.random.default_rng(n)
    ty2, ty3 = rng.integers(0, 2, n).astype(np.int32), rng.integers(0, 3, n).astype(np.int32)
    out = {"S=1": StillingerWeberMulti(system, np.zeros(n, dtype=np.int32), [SI]),
           "S=2 identical": StillingerWeberMulti(system, ty2, [SI, SI]),
           "S=2 unlike": StillingerWeberMulti(system, ty2, [SI, OTHER]),
           "S=3": StillingerWeberMulti(system, ty3, [SI, OTHER, THIRD])}
    pair, triplet = StillingerWeberMulti.mix([SI, OTHER])
    pair = {k: np.array(v) for k, v in pair.items()}
    pair["sigma"][0, 1], pair["sigma"][1, 0] = 2.05, 2.15                    # unlike supports of the two directed bonds
    pair["epsilon"][0, 1], pair["gamma"][1, 0], pair["p"][1, 0] = 1.7, 1.3, 5.0
    triplet = {k: np.array(v) for k, v in triplet.items()}
    triplet["lam"][0, 0, 1], triplet["epsilon3"][1, 0, 1] = 17.0, 2.3
    out["asymmetric"] = StillingerWeberMulti.from_tables(system, ty2, pair, triplet)
    return out


def launches(tag, run, x, w, rng):
    """the three levels of an ops entry point `run(**kw)`, plain and with into="""
    out = []
    o = run(energy=True, grad=False)
    out.append(("L0 energy", o["energy"]))
    o = run(energy=True, grad=True, want_theta=True)
    out += [("L1 energy", o["energy"]), ("L1 grad", o["grad"]), ("L1 pth", o["pth"]), ("L1 theta_sum", ops.theta_sum(o["pth"]))]
    o = run(w=w, energy=False, grad=True, want_theta=True)
    out += [("L2 grad", o["grad"]), ("L2 hw", o["hw"]), ("L2 pthw", o["pthw"]), ("L2 theta_sum", ops.theta_sum(o["pthw"]))]
    bufs = tuple(torch.as_tensor(rng.normal(0, 1, x.shape).astype(F32), device=DEV) for _ in range(2))
    o = run(energy=True, grad=True, into=(bufs[0], None), scale=-0.75)
    out += [("L1 into energy", o["energy"]), ("L1 into grad", bufs[0].clone())]
    o = run(w=w, energy=False, grad=True, into=bufs, scale=1.25)
    out += [("L2 into grad", bufs[0]), ("L2 into hw", bufs[1])]
    return [(tag, k, v) for k, v in out]


def module_outputs(tag, mod, x, w, rng):
    """everything the module hands out at x with the direction w"""
    params = (mod.epsilon, mod.sigma, mod.lam)
    xr = x.clone().requires_grad_(True)
    U = mod(xr)
    g = torch.autograd.grad(U, (xr,) + params, create_graph=True)
    h = torch.autograd.grad((g[0] * w).sum(), (xr,) + params)
    out = [("energy", U), ("dU/dx", g[0])] + [("dU/d" + n, t) for n, t in zip(("epsilon", "sigma", "lam"), g[1:])]
    out += [("H w", h[0])] + [("d(w.dU/dx)/d" + n, t) for n, t in zip(("epsilon", "sigma", "lam"), h[1:])]
    out.append(("force", mod.force(x)))
    F, dq, gth = mod.force_vjp(x, w)
    out += [("force_vjp F", F), ("force_vjp dq", dq)] + [("force_vjp theta %d" % k, t) for k, t in enumerate(gth)]
    bufs = tuple(torch.as_tensor(rng.normal(0, 1, x.shape).astype(F32), device=DEV) for _ in range(2))
    F, dq, gth = mod.force_vjp(x, w, into=bufs)
    out += [("force_vjp into F", F), ("force_vjp into dq", dq)] + [("force_vjp into theta %d" % k, t) for k, t in enumerate(gth)]
    return [(tag, k, v) for k, v in out]


def frame_outputs():
    """K34: U[f] and its parameter gradients for 1 and 5 frames of 64 atoms and for a batch of 128 atoms whose middle frame
    holds a row beyond the cap"""
    out = []
    frames = np.stack([diamond64(64 + s)[0] for s in range(5)])
    L = diamond64(64)[1]
    ok = np.concatenate([frames[0], np.mod(frames[0] + 1.1, L)]).astype(F32)
    bad = ok.copy()
    bad[:70] = (np.array([5.0, 5.0, 5.0]) + np.random.default_rng(3).normal(0, 0.5, (70, 3))).astype(F32)
    for tag, q in (("F=1", frames[:1]), ("F=5", frames), ("F=3 overflow", np.stack([ok, bad, ok]))):
        system = System(positions=q[0], cell=L, masses=np.full(q.shape[1], 28.0855), device=DEV)
        model = StillingerWeber.silicon(system)
        energy = StillingerWeberEnergy(system, model)
        U = energy(torch.as_tensor(q, device=DEV))
        gU = torch.as_tensor(np.random.default_rng(q.shape[0]).normal(0, 1, q.shape[0]).astype(F32), device=DEV)
        gth = torch.autograd.grad((U * gU).sum(), (model.epsilon, model.sigma, model.lam))
        out += [("K34 " + tag, "U", U.detach()), ("K34 " + tag, "without parameter gradient", energy(torch.as_tensor(q, device=DEV)).detach())]
        out += [("K34 " + tag, "d(sum g U)/d" + n, t) for n, t in zip(("epsilon", "sigma", "lam"), gth)]
        with torch.no_grad():
            out.append(("K34 " + tag, "U under no_grad", energy(torch.as_tensor(q, device=DEV))))
    return out


def main():
    lines = []
    for gname, (system, x32, n) in geometries().items():
        x = torch.as_tensor(x32, device=DEV)
        rng = np.random.default_rng(len(gname) + n)
        w = torch.as_tensor(rng.normal(0, 1, x32.shape).astype(F32), device=DEV)
        one = StillingerWeber.silicon(system)
        one._reset_topology(x)
        tag = "K23 %-5s one species" % gname
        lines += launches(tag, lambda **kw: ops.sw_eval(one._ell, x, one._consts, one._theta(), **kw), x, w, rng)
        lines += module_outputs(tag, one, x, w, rng)
        for mname, mod in multi_modules(system, n).items():
            mod._reset_topology(x)
            tag = "K28 %-5s %-13s" % (gname, mname)
            lines += launches(tag, lambda **kw: ops.sw_multi_eval(mod._ell, x, mod.types, mod.n_species, mod._tables(), **kw), x, w, rng)
            lines += module_outputs(tag, mod, x, w, rng)
    lines += frame_outputs()
    torch.cuda.synchronize()
    for tag, what, t in lines:
        print("%s  %-28s %s" % (tag, what, sha(t)))


if __name__ == "__main__":
    main()
