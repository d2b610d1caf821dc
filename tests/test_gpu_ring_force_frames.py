"""The wave-per-replica adjoint with the forward pass's stored forces (TrajArgs::f_t, mdg_traj_*_ft) against the same adjoint
rebuilding them (f_t = NULL): the forward's LEVEL 1 sweep sums the force of a frame in the order of the adjoint's LEVEL 2
sweep, so adj_v0, adj_q0, adj_pv0, adj_theta -- and, with the fused RDF observable, its frame gradient inside adj_q0 -- are
the same bits.  Also: keeping the forces does not change the forward trajectory."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_parity import T, mk_system, DEV

pytestmark = pytest.mark.gpu

CASES = [
    ("lj126", "nhc", 108, True),           # the headline: LJ 12-6, NHC, 108 atoms, RDF fused into the kernels
    ("lj126", "nve", 108, True),
    ("lj126", "nhc", 107, False),          # odd N: the last lane holds one atom
    ("lj126", "nve", 55, False),
    ("lj126_masked2", "nhc", 108, False),  # two masked LJ 12-6 terms: one shared sweep (ring_sweep_lj_multi)
    ("ljfam_masked2", "nve", 107, False),  # two masked LJ 8-4 terms: one pair_eval sweep per term
    ("morse", "nhc", 108, False),          # pair_eval kind
    ("morse", "nve", 107, False),
]


def _integrator(form, ensemble, n_atoms):
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NVE, NoseHooverChain
    g = load_golden("nhc_traj_lj")
    pos0, vel0, mass = g["pos"][:n_atoms], g["vel"][:n_atoms], g["mass"][:n_atoms]
    system = mk_system(pos0, g["cell"], vel0, mass)
    A_, B_ = list(range(0, n_atoms, 2)), list(range(1, n_atoms, 2))
    if form == "lj126":
        terms = {"pair": PairPotentials(system, P.LennardJones(1.0, 1.0), cutoff=2.5)}
    elif form == "lj126_masked2":
        terms = {"aa": PairPotentials(system, P.LennardJones(1.0, 1.0), cutoff=2.5, index_tuple=(A_, A_)),
                 "ab": PairPotentials(system, P.LennardJones(0.9, 0.8), cutoff=2.2, index_tuple=(A_, B_))}
    elif form == "ljfam_masked2":
        terms = {"aa": PairPotentials(system, P.LJFamily(epsilon=1.1, sigma=0.95, rep_pow=8, attr_pow=4), cutoff=2.5,
                                      index_tuple=(A_, A_)),
                 "ab": PairPotentials(system, P.LJFamily(epsilon=0.9, sigma=0.9, rep_pow=8, attr_pow=4), cutoff=2.0,
                                      index_tuple=(A_, B_))}
    else:
        terms = {"pair": PairPotentials(system, P.ModifiedMorse(a=1.5, phi=1.0), cutoff=2.5)}
    nhc = ensemble == "nhc"
    integ = (NoseHooverChain(Stack(terms), system, T=1.0, num_chains=5, Q=50.0) if nhc else NVE(Stack(terms), system)).to(DEV)
    return g, pos0, integ, nhc


def _rdf_fuse(lib, prm, spec):
    from mdgrad_amd import _lib
    nbins, lo, hi = 100, 0.75, 2.5
    mu = torch.linspace(lo, hi, nbins, device=DEV)
    sp = (hi - lo) / (nbins - 1)
    fuse = _lib.MdgRdfFuse(mu=mu.data_ptr(), nbins=nbins, coeff=-0.5 / sp ** 2, mu0=lo, spacing=sp, cutoff=hi + 0.5,
                           frame_start=0, frame_stride=1)
    assert lib.mdg_traj_rdf_supported(C.byref(prm), C.byref(spec.cell_struct), C.byref(spec.terms), C.byref(fuse))
    return fuse, mu


@pytest.mark.parametrize("form,ensemble,n_atoms,rdf", CASES)
def test_ring_adjoint_with_stored_forces_is_bitwise_the_rebuilt_one(form, ensemble, n_atoms, rdf):
    from mdgrad_amd import _lib
    lib = _lib.load()
    g, pos0, integ, nhc = _integrator(form, ensemble, n_atoms)
    R, nT = 6, 9
    spec = integ.fused_spec("NH_verlet" if nhc else "verlet")
    assert spec is not None and not spec.large
    spec.block = 64
    prm = spec.params(R, nT)
    cs, terms = spec.cell_struct, spec.terms
    assert lib.mdg_traj_ring_taken(C.byref(prm), C.byref(cs), C.byref(terms)), "the wave-per-replica kernels must run"
    rng = np.random.default_rng(n_atoms + len(form))
    pos = np.mod(pos0[None] + rng.normal(0, 0.02, (R,) + pos0.shape), g["cell"]).astype(np.float32)
    vel = rng.normal(0, 0.5, pos.shape).astype(np.float32)
    v0, q0 = T(vel, DEV).contiguous(), T(pos, DEV).contiguous()
    Cn = len(spec.Q)
    pv0 = torch.zeros(R, Cn, device=DEV) if nhc else None
    t = torch.Tensor([0.004 * i for i in range(nT)]).to(DEV)
    theta = spec.flat_params().detach().contiguous()
    P, ptr, st = C.byref, _lib.ptr, _lib.stream_ptr(DEV)
    fuse = mu = None
    if rdf:
        fuse, mu = _rdf_fuse(lib, prm, spec)

    def forward(keep):
        v_t, q_t = torch.empty(R, nT, n_atoms, 3, device=DEV), torch.empty(R, nT, n_atoms, 3, device=DEV)
        pv_t = torch.empty(R, nT, Cn, device=DEV) if nhc else None
        f_t = torch.full((R, nT, n_atoms, 3), float("nan"), device=DEV) if keep else None
        bad = torch.zeros(R, dtype=torch.int32, device=DEV)
        raw = torch.empty(100, device=DEV)
        if rdf:
            _lib.check(lib.mdg_traj_fwd_small_rdf_ft(P(prm), P(cs), P(terms), ptr(theta), ptr(spec.mass), ptr(t), ptr(v0),
                                                     ptr(q0), ptr(pv0), ptr(v_t), ptr(q_t), ptr(pv_t), ptr(f_t), ptr(bad),
                                                     P(fuse), ptr(raw), st), "fwd_rdf_ft")
        else:
            _lib.check(lib.mdg_traj_fwd_small_ft(P(prm), P(cs), P(terms), ptr(theta), ptr(spec.mass), ptr(t), ptr(v0),
                                                 ptr(q0), ptr(pv0), ptr(v_t), ptr(q_t), ptr(pv_t), ptr(f_t), ptr(bad), st),
                       "fwd_ft")
        torch.cuda.synchronize()
        assert int(bad.abs().sum()) == 0
        return v_t, q_t, pv_t, f_t, raw

    v_t, q_t, pv_t, f_t, raw = forward(True)
    ref = forward(False)
    for a, b, nm in ((v_t, ref[0], "v_t"), (q_t, ref[1], "q_t"), (pv_t, ref[2], "pv_t"), (raw, ref[4], "rdf histogram")):
        if a is not None and (nm != "rdf histogram" or rdf):
            assert torch.equal(a, b), "keeping the forces changed the forward pass: " + nm
    assert bool(torch.isfinite(f_t[:, 1:]).all()), "every frame's force 1..T-1 is written"
    assert bool(torch.isnan(f_t[:, 0]).all()), "frame 0 is not written"
    gen = torch.Generator(device=DEV).manual_seed(3)
    gv = torch.randn(v_t.shape, device=DEV, generator=gen) * 1e-2
    gq = torch.randn(q_t.shape, device=DEV, generator=gen) * 1e-2
    gp = torch.randn(pv_t.shape, device=DEV, generator=gen) * 1e-2 if nhc else None
    g_raw = torch.randn(100, device=DEV, generator=gen) * 1e-3
    KT = spec.n_theta_total

    def adjoint(ft):
        adj = [torch.empty(R, n_atoms, 3, device=DEV), torch.empty(R, n_atoms, 3, device=DEV),
               torch.empty(R, Cn, device=DEV) if nhc else None, torch.zeros(R, KT, device=DEV)]
        args = [P(prm), P(cs), P(terms), ptr(theta), ptr(spec.mass), ptr(t), ptr(v_t), ptr(q_t), ptr(pv_t), ptr(ft),
                ptr(gv), ptr(gq), ptr(gp), ptr(adj[0]), ptr(adj[1]), ptr(adj[2]), ptr(adj[3])]
        if rdf:
            _lib.check(lib.mdg_traj_adj_small_rdf_ft(*args, P(fuse), ptr(g_raw), st), "adj_rdf_ft")
        else:
            _lib.check(lib.mdg_traj_adj_small_ft(*args, st), "adj_ft")
        torch.cuda.synchronize()
        return adj

    new, old = adjoint(f_t), adjoint(None)
    for a, b, nm in zip(new, old, ("adj_v0", "adj_q0" + (" (with the RDF frame gradient)" if rdf else ""), "adj_pv0",
                                   "adj_theta")):
        if a is None:
            continue
        assert bool(torch.isfinite(a).all()), nm
        assert torch.equal(a, b), "%s: stored forces vs rebuilt, max |diff| %.3e" % (nm, float((a - b).abs().max()))
    assert float(new[1].abs().max()) > 0 and (KT == 0 or float(new[3].abs().max()) > 0)
    if rdf:
        # the observable's frame gradient is really in adj_q0: without g_raw's contribution the result moves
        keep = g_raw.clone()
        g_raw.zero_()
        assert not torch.equal(adjoint(f_t)[1], new[1])
        g_raw.copy_(keep)
    del mu


def test_fused_traj_keeps_forces_only_on_the_ring_path():
    """ops.FusedTrajFn allocates the per-frame forces where the wave-per-replica kernels run, not on the workgroup path."""
    from mdgrad_amd import ops
    g, pos0, integ, nhc = _integrator("lj126", "nhc", 108)
    R, nT = 4, 5
    t = torch.Tensor([0.004 * i for i in range(nT)]).to(DEV)
    rng = np.random.default_rng(2)
    pos = np.mod(pos0[None] + rng.normal(0, 0.02, (R,) + pos0.shape), g["cell"]).astype(np.float32)
    vel = rng.normal(0, 0.5, pos.shape).astype(np.float32)
    grads = {}
    for block in (64, 128):
        spec = integ.fused_spec("NH_verlet")
        spec.block = block
        v0, q0 = T(vel, DEV).requires_grad_(True), T(pos, DEV).requires_grad_(True)
        pv0 = torch.zeros(R, 5, device=DEV, requires_grad=True)
        out = ops.FusedTrajFn.apply(v0, q0, pv0, t, spec.flat_params(), spec)
        ctx = out[0].grad_fn
        assert (getattr(ctx, "f_t", None) is not None) == (block == 64)
        (out[1][:, -1].pow(2).mean() + out[0].pow(2).mean()).backward()
        grads[block] = (v0.grad.clone(), q0.grad.clone())
    for a, b in zip(grads[64], grads[128]):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) + 1e-7
