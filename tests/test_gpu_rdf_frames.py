"""observable.rdf.per_frame on the GPU (csrc/rdf_frames.hip, ops.RdfFramesFn): every row and its gradient against
tests/rdf_ref.py called one frame at a time.

Error measures and tolerance exactly as tests/test_gpu_rdf_ref.py: forward |raw_k - ref64_k| / max_k ref64 of the frame; backward
|g - ref64| per atom and component over the atom's scale A (not below rdf_ref.scale_floor; an atom with A = 0 must hold exact
zeros).  Per frame, on the CPU: floor = the kernel's model -- the 2R + 1 centres around the nearest one, ("reach", R) with
R = ops.rdf_frames_reach -- in float32 against the same model in float64, at least 2^-24; model_gap = the float64 model against
the exact float64 sum; allowed = MARGIN x floor + model_gap, MARGIN = 10.  Nothing comes from the kernel.

Upstream rows differ per frame: the forms of rdf_ref (linspace(-1, 1), one-hot first / last bin) in turn, scaled by f + 1, row 1
zero (that frame gets exact zeros).  Frames carry no fragile pair at the observable's cutoff_boundary (rdf_ref.draw_frames).

(Every case prints floor, model_gap, allowed and the kernel's figure; MDG_TEST_REPORT=<file> collects them.)"""
import numpy as np
import pytest
import torch

import rdf_ref as R
from test_rdf_frames_host import BOX, _report, frames_for, inputs, observable, references, upstream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 10.0


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def base_of(n):
    """(lattice positions, box): the RDF golden's 108-atom lattice in the 4.8 cell up to 108 atoms, the first n sites of
    rdf_ref._liquid (216 sites for 129 atoms, 1 000 for 1 000) in its own cell beyond"""
    if n <= 108:
        return None, BOX
    pos, box = R._liquid(6 if n <= 216 else 10, 61)
    return pos[:n], box


CASES = [  # (atoms, frames, nbins, width in spacings or None, masked)
    (2, 3, 100, None, False), (3, 5, 2, None, False), (107, 3, 100, None, False), (107, 5, 100, None, True),
    (108, 257, 100, None, False), (108, 1, 1000, None, False), (108, 3, 100, 5.0, False), (129, 3, 100, 5.0, False),
    (129, 5, 1000, None, True), (1000, 1, 100, None, False),
]


def setup(n, F, nbins, width, masked):
    from mdgrad_amd import ops
    base, box = base_of(n)
    it = (list(range(0, (5 * n) // 12)), list(range((5 * n) // 12, n))) if masked else None
    probe = observable(n, nbins=nbins, device=DEV, box=box)
    obs = observable(n, nbins=nbins, width=None if width is None else width * probe.spacing, index_tuple=it, device=DEV, box=box)
    frames = frames_for(obs, n, F, index_tuple=it, base=base, box=box)
    return obs, frames, it, box, ("reach", ops.rdf_frames_reach(obs.spacing, obs.coeff))


def run(obs, frames, g):
    q = T(frames).requires_grad_(True)
    raw = obs.per_frame(q)
    (gq,) = torch.autograd.grad((raw * T(g)).sum(), q)
    return raw.detach(), gq


@pytest.mark.parametrize("n,F,nbins,width,masked", CASES)
def test_rows_and_gradients_against_the_reference(n, F, nbins, width, masked):
    obs, frames, it, box, model = setup(n, F, nbins, width, masked)
    g = upstream(F, nbins)
    exact = references(frames, obs, g, it, box=box)
    m64 = references(frames, obs, g, it, model=model, box=box)
    m32 = references(frames, obs, g, it, dtype=np.float32, model=model, box=box)
    raw, gq = run(obs, frames, g)
    assert raw.shape == (F, nbins) and torch.isfinite(raw).all() and torch.isfinite(gq).all()
    raw, gq = raw.cpu().numpy(), gq.cpu().numpy()
    what = "N=%d F=%d nbins=%d width=%s%s R=%d" % (n, F, nbins, width or 1, " masked" if masked else "", model[1])
    bad, worst, budget = [], {}, []
    for f in range(F):
        ref = exact[f]
        peak = ref.raw.max()
        if peak == 0:                                                       # no pair in reach of a centre: exact zeros
            assert (raw[f] == 0).all() and (gq[f] == 0).all()
            continue
        floor = max(float(np.abs(m32[f].raw.astype(np.float64) - m64[f].raw).max() / peak), R.ULP)
        gap = R.forward_error(m64[f].raw, ref)
        figs = [("raw", R.forward_error(raw[f], ref), floor, gap)]
        budget.append((MARGIN * floor + gap, peak))
        if np.abs(g[f]).max() > 0:
            a_min = R.scale_floor(g[f], obs.coeff)
            scale = (ref.A + a_min)[..., None]
            bfloor = max(float((np.abs(m32[f].g_xyz.astype(np.float64) - m64[f].g_xyz) / scale).max()), R.ULP)
            bgap = float((np.abs(m64[f].g_xyz - ref.g_xyz) / scale).max())
            ref1 = ref._replace(g_xyz=ref.g_xyz[None], A=ref.A[None])
            figs.append(("g_xyz", R.backward_error(gq[f][None], ref1, 0, a_min), bfloor, bgap))
        else:
            assert (gq[f] == 0).all(), "a zero upstream row must give exact zeros"
        for q, v, fl, gp in figs:
            allowed = MARGIN * fl + gp
            if q not in worst or v / allowed > worst[q][0] / worst[q][3]:
                worst[q] = (v, fl, gp, allowed, f)
            if not v <= allowed:
                bad.append((f, q, v, allowed))
    for q, (v, fl, gp, allowed, f) in worst.items():
        _report("%-52s %-6s worst frame %3d  floor %.3e  model_gap %.3e  allowed %.3e  kernel %.3e%s" % (
            what, q, f, fl, gp, allowed, v, "" if v <= allowed else "   <-- FAILS"))
    assert not bad, "%s: %s" % (what, bad[:6])
    # normalise(sum of the rows) is the reference's normalised sum: every row is within allowed_f peak_f per bin, so the sum
    # within E = sum_f of that, its total S within nbins E, and count_k = sum_k / S within E / S + count_k nbins E / S
    tot = sum(r.raw for r in exact)
    S = tot.sum()
    if S > 0:
        E = sum(a * p for a, p in budget)
        count = obs.normalise(T(raw).sum(0))[0].cpu().numpy().astype(np.float64)
        bound = E / S + (tot / S) * nbins * E / S + 2.0 ** -22 * (tot / S)      # (+ the float32 sum over frames and division)
        assert (np.abs(count - tot / S) <= bound).all()


def test_shapes_and_stacked_replicas():
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.system import System
    n = 48
    obs = observable(n, device=DEV)
    q = T(frames_for(obs, n, 4))
    raw = obs.per_frame(q)
    assert raw.shape == (4, 100)
    assert torch.equal(obs.per_frame(q[2]), raw[2]) and torch.equal(obs.per_frame(q.reshape(2, 2, n, 3)).reshape(4, 100), raw)
    rep = System(positions=np.zeros((n, 3)), cell=BOX.astype(np.float64), masses=np.ones(n), device=DEV).replicate(2)
    st = rdf(rep, nbins=100, r_range=(0.75, 2.5)).per_frame(torch.cat([q[:2], q[2:]], dim=1))
    assert st.shape == (2, 2, 100) and torch.equal(st[:, 0], raw[:2]) and torch.equal(st[:, 1], raw[2:])
    sl = torch.cat([q, q, q])[::3]                                          # a strided view
    assert not sl.is_contiguous() and torch.equal(obs.per_frame(sl), obs.per_frame(sl.contiguous()))
    # float64 device positions take the torch restatement with the exact sum
    r64 = obs.per_frame(q.double())
    assert r64.dtype == torch.float64 and torch.allclose(r64.float(), raw, rtol=0, atol=1e-5 * float(raw.max()))


@pytest.mark.parametrize("n,F,nbins", [(108, 64, 100), (107, 5, 1000), (300, 3, 100)])
def test_bitwise_repeatable(n, F, nbins):
    base, box = (None, BOX) if n <= 108 else (R._liquid(7, 3)[0][:n], R._liquid(7, 3)[1])
    obs = observable(n, nbins=nbins, device=DEV, box=box)
    rng = np.random.default_rng(2)
    from conftest import load_golden
    base = load_golden("rdf")["xyz"][0][:n] if base is None else base
    frames = np.mod(base[None] + rng.normal(0, 0.05, (F,) + base.shape), box).astype(np.float32)
    g = upstream(F, nbins)
    a, b = run(obs, frames, g), run(obs, frames, g)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[0].max()) > 0


def test_torch_ops_equal_the_ctypes_path():
    from mdgrad_amd import _torch_ops
    ns = _torch_ops.get()
    assert ns is not None
    n, F = 107, 5
    it = (list(range(0, 40)), list(range(40, n)))
    obs = observable(n, index_tuple=it, device=DEV)
    frames = frames_for(obs, n, F, index_tuple=it)
    g = upstream(F, obs.nbins)
    raw, gq = run(obs, frames, g)
    cell = _torch_ops.cell_args(obs._cell_struct)
    raw_t = ns.rdf_frames_fwd(T(frames), cell, obs.cutoff_boundary, obs._mask, obs.offsets, obs.spacing, obs.coeff)
    gq_t = ns.rdf_frames_bwd(T(frames), cell, obs.cutoff_boundary, obs._mask, obs.offsets, obs.spacing, obs.coeff, T(g))
    assert torch.equal(raw_t, raw) and torch.equal(gq_t, gq)
    with pytest.raises(RuntimeError, match="g_raw"):
        ns.rdf_frames_bwd(T(frames), cell, obs.cutoff_boundary, obs._mask, obs.offsets, obs.spacing, obs.coeff, T(g[:2]))


def test_limits_are_refused():
    with pytest.raises(ValueError, match="1024 atoms"):
        observable(1025, device=DEV, box=np.full(3, 12.0)).per_frame(torch.zeros(1, 1025, 3, device=DEV))
    with pytest.raises(ValueError, match="nbins"):
        observable(8, nbins=1025, device=DEV).per_frame(torch.zeros(1, 8, 3, device=DEV))
    obs = observable(8, device=DEV)
    q = torch.rand(2, 8, 3, device=DEV).requires_grad_(True)
    (gq,) = torch.autograd.grad(obs.per_frame(q).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):
        gq.pow(2).sum().backward()
