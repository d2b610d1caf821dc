"""thermo.EAMEnergy without a GPU: the host / float64 path (the model's torch restatement frame by frame) against the float64
definitions of tests/eam_table_ref.py (interface.EAM) and tests/eam_ref.py (interface.SuttonChen), the shapes it accepts, its
refusals, and the covariance identity of reweight.Reweighting with it on the host.

Tolerances: float64 torch against the float64 reference, 1e-12 relative to the frame's energy (the parameters are float32 in
the modules and are handed to the references as the modules hold them); the gradient of a reweighted RDF against
reweight_ref.gradient fed with the references' float64 dU/dtheta, 1e-6 of the largest entry of that parameter block (the bound
tests/test_gpu_reweight_sw.py puts on its float64 host path).

Observed: energies 0 (EAM) and 1.9e-16 (SuttonChen) relative; reweighted-RDF gradient 1.9e-08 (embed_nodes) and 3.3e-08 /
4.4e-08 / 1.8e-08 (epsilon, a, c): the float32 rounding of the parameters' gradient, made once after the sum over the frames."""
import numpy as np
import pytest
import torch

import eam_ref as SC
import eam_table_ref as R
import reweight_ref as RW

N, RC, RMIN = 108, 5.2, 1.8
CU = SC.PUBLISHED["copper"]


def _cpu_system(pos, cell, mass=63.546):
    from mdgrad_amd.system import System
    return System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
                  masses=np.full(len(pos), mass), device="cpu")


def _frames(n, first_seed=108):
    xs = [SC.jittered_fcc(3, 3.61, 0.15, first_seed + s) for s in range(n)]
    return np.stack([x for x, _ in xs]), xs[0][1]


def _sutton_chen(system, shift="force", **kw):
    from mdgrad_amd.interface import SuttonChen
    from mdgrad_amd.thermo import EAMEnergy
    eps, a, c, n, m = CU
    model = SuttonChen(system, eps, a, c, n, m, RC, shift=shift, **kw)
    return model, EAMEnergy(system, model)


def _tabulated(system, n=64, **kw):
    from mdgrad_amd.interface import EAM
    from mdgrad_amd.thermo import EAMEnergy
    model = EAM.from_sutton_chen(system, "copper", cutoff=RC, r_min=RMIN, n_r=n, n_rho=n, **kw)
    return model, EAMEnergy(system, model)


def _sc_reference(model, x, cell, derivatives=False):
    th = [float(p.detach()) for p in (model.epsilon, model.a, model.c)]
    k = SC.consts(model.n, model.m, model.cutoff, model.shift)
    lst = SC.pairs(x, cell, model.cutoff)
    if derivatives:
        return SC.evaluate(x, th, lst, cell, k)
    return float(SC.energy(torch.tensor(x).double(), torch.tensor(th, dtype=torch.float64), lst, cell, k))


def _table_reference(model, x, cell, derivatives=False):
    lst = R.pairs(x, cell, model.cutoff)
    types, g = model.types.cpu().long()[:x.shape[0]], R.grid_of(model)
    if derivatives:
        return R.evaluate(x, R.tables_of(model), lst, cell, types, g, pin=model.pin_cutoff)
    return float(R.energy(torch.tensor(x).double(), R.tables_of(model), lst, cell, types, g))


@pytest.mark.parametrize("kind", ["table", "table-two-species", "sc-force", "sc-none"])
def test_float64_host_frames_equal_the_reference_per_frame(kind):
    frames, cell = _frames(3)
    system = _cpu_system(frames[0], cell)
    if kind == "table":
        model, energy = _tabulated(system)
        ref = _table_reference
    elif kind == "table-two-species":
        from mdgrad_amd.interface import EAM
        from mdgrad_amd.thermo import EAMEnergy
        from test_gpu_eam_table import _functions
        model = EAM.from_functions(system, np.arange(N) % 2, *_functions(2.55), RC, 2.3, (8.0, 30.0), 48, 40, pin_cutoff=False)
        energy, ref = EAMEnergy(system, model), _table_reference
    else:
        model, energy = _sutton_chen(system, shift=kind[3:])
        ref = _sc_reference
    want = np.array([ref(model, x, cell) for x in frames])
    q = torch.tensor(frames).double().requires_grad_(True)
    U = energy(q)
    assert U.shape == (3,) and U.dtype == torch.float64
    err = np.abs(U.detach().numpy() - want) / np.abs(want)
    print("EAMEnergy float64 host (%s): largest relative error %.3e (allowed 1e-12)" % (kind, err.max()))
    assert err.max() <= 1e-12
    assert len(set(np.round(want, 6))) == 3, "three different frames"
    # differentiable in the frames and the parameters; U[f] is what the model gives for the frame
    p = model.embed_nodes if kind.startswith("table") else model.a
    gq, gp = torch.autograd.grad(U.sum(), (q, p))
    assert gq.shape == q.shape and bool(torch.isfinite(gq).all()) and float(gq.abs().max()) > 0 and float(gp.abs().max()) > 0
    for f in range(3):
        assert float(model(q[f].detach()).detach()) == float(U[f].detach())
    assert model._n_rep == 1


@pytest.mark.parametrize("kind", ["table", "sc"])
def test_shapes(kind):
    frames, cell = _frames(4, first_seed=120)
    make = _tabulated if kind == "table" else _sutton_chen
    model, energy = make(_cpu_system(frames[0], cell))
    q = torch.tensor(frames).double()
    with torch.no_grad():
        U = energy(q)
    assert energy(q[2]).shape == () and float(energy(q[2]).detach()) == float(U[2].detach())                      # [N, 3]
    assert U.shape == (4,)                                                                       # [T, N, 3]
    two = energy(q.reshape(2, 2, N, 3))                                                          # [R, T, N, 3]
    assert two.shape == (2, 2) and torch.equal(two.reshape(4), U)
    st = energy(torch.cat([q[:2], q[2:]], dim=1))                                                # [T, 2 N, 3]: q[t], q[t + 2]
    assert st.shape == (2, 2) and torch.equal(st[:, 0], U[:2]) and torch.equal(st[:, 1], U[2:])
    # a replicated system: the model sees k replicas, the observable one frame at a time
    rep = _cpu_system(frames[0], cell).replicate(2)
    m2, e2 = make(rep)
    st2 = e2(torch.cat([q[:2], q[2:]], dim=1))
    assert st2.shape == (2, 2) and torch.allclose(st2, st, rtol=1e-14, atol=0) and m2._n_rep == 2
    with pytest.raises(ValueError, match="k \\* 108"):
        energy(torch.zeros(3, 50, 3))
    # float32 host frames take the same path in float32
    assert energy(q.float()).dtype == torch.float32


def test_refusals():
    from mdgrad_amd.interface import PairPotentials, Stack, StillingerWeber, SuttonChen, Tersoff
    from mdgrad_amd.thermo import EAMEnergy
    frames, cell = _frames(1)
    system = _cpu_system(frames[0], cell)
    eps, a, c, n, m = CU
    for cls in (Stack, StillingerWeber, Tersoff, PairPotentials):          # (the refusal looks at the type alone)
        with pytest.raises(NotImplementedError, match="interface.EAM or an interface.SuttonChen; got %s" % cls.__name__):
            EAMEnergy(system, cls.__new__(cls))
    with pytest.raises(NotImplementedError, match="StillingerWeberEnergy"):
        EAMEnergy(system, StillingerWeber.__new__(StillingerWeber))
    model, _ = _sutton_chen(system)
    tabulated, _ = _tabulated(system)
    tric = _cpu_system(frames[0], np.array([[10.83, 0, 0], [0.5, 10.83, 0], [0, 0, 10.83]]))
    with pytest.raises(ValueError, match="diagonal"):
        EAMEnergy(tric, SuttonChen(tric, eps, a, c, n, m, RC))
    big = _cpu_system(np.random.default_rng(0).uniform(0, 30.0, (1025, 3)), np.full(3, 30.0))
    with pytest.raises(ValueError, match="1024 atoms"):
        EAMEnergy(big, SuttonChen(big, eps, a, c, n, m, RC))
    fewer = _cpu_system(frames[0][:107], cell)
    for mdl in (model, tabulated):
        with pytest.raises(ValueError, match="built for 108 atoms per replica, the system holds 107"):
            EAMEnergy(fewer, mdl)
        # the strict minimum image of the frame kernels needs rc <= L / 2 of the system the frames belong to
        small = _cpu_system(np.mod(frames[0], 10.0), np.full(3, 10.0))
        with pytest.raises(ValueError, match="half the shortest cell length"):
            EAMEnergy(small, mdl)


def _reweighted_rdf_gradient(system, energy, params, frames, kT):
    """[nbins, P]: the gradient of the reweighted per-frame RDF rows with respect to the flattened `params`, and the rows"""
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.reweight import Reweighting
    q = torch.tensor(frames).double()
    obs = rdf(system, nbins=24, r_range=(2.0, RC))
    rw = Reweighting(energy, kT, q)
    with torch.no_grad():
        rows = obs.per_frame(q)
    avg = rw.average(rows)
    G = torch.stack([torch.cat([g.reshape(-1) for g in torch.autograd.grad(avg[b], params, retain_graph=True)])
                     for b in range(avg.shape[0])])
    assert torch.equal(rw.weights().detach(), torch.full((len(frames),), 1.0 / len(frames), dtype=torch.float64))
    return G.numpy(), rows.numpy()


def test_reweighting_gradient_on_the_host_is_the_covariance_identity():
    kT, F = 0.0862, 10
    frames, cell = _frames(F, first_seed=300)
    w = np.full(F, 1.0 / F)
    # tabulated: d/d embed_nodes
    system = _cpu_system(frames[0], cell)
    model, energy = _tabulated(system, trainable=("embed",))
    G, rows = _reweighted_rdf_gradient(system, energy, [model.embed_nodes], frames, kT)
    n_embed = model.embed_nodes.numel()
    dU = np.stack([_table_reference(model, x, cell, True)["gtab"].numpy()[-n_embed:] for x in frames])
    want = RW.gradient(w, rows, dU, kT)
    err = np.abs(G - want).max() / np.abs(want).max()
    print("reweighted RDF on the host, d/d embed_nodes: %.3e of the largest entry (allowed 1e-6)" % err)
    assert np.abs(want).max() > 0 and err <= 1e-6
    # Sutton-Chen: d/d(epsilon, a, c)
    model, energy = _sutton_chen(system)
    G, rows = _reweighted_rdf_gradient(system, energy, [model.epsilon, model.a, model.c], frames, kT)
    dU = np.stack([_sc_reference(model, x, cell, True)["dth"].numpy() for x in frames])
    want = RW.gradient(w, rows, dU, kT)
    for k, name in enumerate(("epsilon", "a", "c")):
        err = np.abs(G[:, k] - want[:, k]).max() / np.abs(want[:, k]).max()
        print("reweighted RDF on the host, d/d%-8s %.3e of the largest entry (allowed 1e-6)" % (name, err))
        assert err <= 1e-6
