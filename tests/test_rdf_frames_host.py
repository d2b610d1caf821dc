"""observable.rdf.per_frame / rdf.normalise without a GPU: the torch restatement (host / float64 positions, the exact sum) row by
row against tests/rdf_ref.py called one frame at a time, the normalised sum against the reference's, the index_tuple mask, the
limits, and the C entry points' argument checks.

Tolerance: float64 torch against the float64 reference in rdf_ref's error measures (forward: of the largest bin; backward: of
the atom's scale A) <= 1e-12.  The frames carry no fragile pair at the observable's cutoff_boundary (rdf_ref.draw_frames
redraws a frame that has one), so the reference is exact on them and no case is left out."""
import os

import numpy as np
import pytest
import torch

import rdf_ref as R
from conftest import load_golden

TOL64 = 1e-12
BOX = np.full(3, 4.8, np.float32)


def _report(line):
    print(line)
    if os.environ.get("MDG_TEST_REPORT"):
        with open(os.environ["MDG_TEST_REPORT"], "a") as fh:
            fh.write(line + "\n")


def observable(n_atoms, nbins=100, r_range=(0.75, 2.5), width=None, index_tuple=None, device="cpu", box=BOX):
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.system import System
    system = System(positions=np.zeros((n_atoms, 3)), cell=np.asarray(box, np.float64), masses=np.ones(n_atoms), device=device)
    return rdf(system, nbins=nbins, r_range=r_range, index_tuple=index_tuple, width=width)


def inputs(obs):
    """what a kernel receives from the observable: (centres, coeff, cutoff)"""
    return obs.offsets.detach().cpu().numpy(), obs.coeff, obs.cutoff_boundary


def frames_for(obs, n_atoms, n_frames, seed=13, index_tuple=None, base=None, box=BOX):
    mu, coeff, cut = inputs(obs)
    base = load_golden("rdf")["xyz"][0][:n_atoms] if base is None else base
    frames, _ = R.draw_frames(base, box, n_frames, seed,
                              lambda fr: R.fragile_pairs(fr, box, mu, coeff, cut, index_tuple=index_tuple))
    assert len(R.fragile_pairs(frames, box, mu, coeff, cut, index_tuple=index_tuple)) == 0
    return frames


def upstream(n_frames, nbins):
    """rows that differ per frame: the forms of rdf_ref (linspace, one-hot first / last) in turn, scaled by f + 1; row 1 zero"""
    g = np.zeros((n_frames, nbins), np.float32)
    for f in range(n_frames):
        form = R.FORMS[f % 3]
        g[f] = np.linspace(-1, 1, nbins, dtype=np.float32) if form == "linspace" else 0.0
        if form == "first":
            g[f, 0] = 1.0
        if form == "last":
            g[f, -1] = 1.0
        g[f] *= f + 1
    if n_frames > 1:
        g[1] = 0.0
    return g


def references(frames, obs, g, index_tuple=None, dtype=np.float64, model=None, box=BOX):
    mu, coeff, cut = inputs(obs)
    return [R.rdf_reference(frames[f:f + 1], box, mu, coeff, cut, g[f], index_tuple=index_tuple, dtype=dtype, model=model)
            for f in range(len(frames))]


@pytest.mark.parametrize("masked", [False, True], ids=["all pairs", "index_tuple"])
def test_rows_and_gradients_against_the_reference(masked):
    n, F = 48, 3
    it = (list(range(0, 20)), list(range(20, n))) if masked else None
    obs = observable(n, index_tuple=it)
    frames = frames_for(obs, n, F, index_tuple=it)
    g = upstream(F, obs.nbins)
    refs = references(frames, obs, g, it)
    q = torch.as_tensor(frames, dtype=torch.float64).requires_grad_(True)
    raw = obs.per_frame(q)
    assert raw.shape == (F, obs.nbins) and raw.dtype == torch.float64
    (gq,) = torch.autograd.grad((raw * torch.as_tensor(g, dtype=torch.float64)).sum(), q)
    for f, ref in enumerate(refs):
        a_min = R.scale_floor(g[f], obs.coeff) or 1.0                       # (a zero row: A = 0 everywhere, exact zeros wanted)
        ref1 = ref._replace(g_xyz=ref.g_xyz[None], A=ref.A[None])
        ef = R.forward_error(raw[f].detach().numpy(), ref)
        eb = R.backward_error(gq[f].numpy()[None], ref1, 0, a_min)
        _report("rdf.per_frame float64 host%s frame %d  allowed %.1e  raw %.3e  g_xyz %.3e" % (" masked" if masked else "", f, TOL64, ef, eb))
        assert ef <= TOL64 and eb <= TOL64
    assert float(gq[1].abs().max()) == 0.0                                   # (the zero upstream row)
    if masked:                                                              # the mask is honoured: it changes the rows
        full = observable(n).per_frame(q.detach())
        assert float((full - raw.detach()).min()) >= -1e-9 and float((full - raw.detach()).max()) > 1.0
    # the normalised sum of the rows = the reference's sum over the frames, normalised like rdf.forward
    mu, coeff, cut = inputs(obs)
    tot = R.rdf_reference(frames, BOX, mu, coeff, cut, index_tuple=it).raw
    assert np.abs(sum(r.raw for r in refs) - tot).max() <= TOL64 * tot.max()
    count, bins, gr = obs.normalise(raw.detach().sum(0))
    want = tot / tot.sum()
    assert bins is obs.bins
    assert np.abs(count.numpy() - want).max() <= TOL64 * want.max()
    vol = obs.vol_bins.double().numpy() / obs.V
    assert np.abs(gr.numpy() - want / vol).max() <= TOL64 * (want / vol).max()
    # ... and of every row at once
    c_rows = obs.normalise(raw.detach())[0]
    assert c_rows.shape == raw.shape and torch.allclose(c_rows.sum(-1), torch.ones(F, dtype=torch.float64), rtol=1e-14, atol=0)


def test_float32_host_path_and_shapes():
    n = 48
    obs = observable(n)
    frames = frames_for(obs, n, 4)
    q = torch.as_tensor(frames)
    raw = obs.per_frame(q)
    assert raw.shape == (4, 100) and raw.dtype == torch.float32
    zero = np.zeros((4, 100), np.float32)
    refs, refs32 = references(frames, obs, zero), references(frames, obs, zero, dtype=np.float32)
    for f in range(4):                   # within MARGIN = 10 x the float32 floor of the formula (the reference's own float32 run)
        floor = max(R.forward_error(refs32[f].raw, refs[f]), R.ULP)
        err = R.forward_error(raw[f].numpy(), refs[f])
        _report("rdf.per_frame float32 host frame %d  floor %.3e  allowed %.3e  figure %.3e" % (f, floor, 10 * floor, err))
        assert err <= 10 * floor
    assert obs.per_frame(q[2]).shape == (100,) and torch.equal(obs.per_frame(q[2]), raw[2])
    two = obs.per_frame(q.reshape(2, 2, n, 3))
    assert two.shape == (2, 2, 100) and torch.equal(two.reshape(4, 100), raw)
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.system import System
    rep = System(positions=np.zeros((n, 3)), cell=BOX.astype(np.float64), masses=np.ones(n), device="cpu").replicate(2)
    obs2 = rdf(rep, nbins=100, r_range=(0.75, 2.5))
    st = obs2.per_frame(torch.cat([q[:2], q[2:]], dim=1))                   # [2, 2 N, 3]: frame t holds q[t], q[t + 2]
    assert st.shape == (2, 2, 100) and torch.equal(st[:, 0], raw[:2]) and torch.equal(st[:, 1], raw[2:])
    with pytest.raises(ValueError, match="k \\* 48"):
        obs.per_frame(torch.zeros(3, 50, 3))


def test_limits_are_refused():
    with pytest.raises(ValueError, match="1024 atoms"):
        observable(1025, box=np.full(3, 12.0)).per_frame(torch.zeros(1, 1025, 3))
    with pytest.raises(ValueError, match="nbins"):
        observable(8, nbins=1025).per_frame(torch.zeros(1, 8, 3))


def test_reach_of_the_kernel_follows_the_width():
    """R = ceil(5.3 / (s spacing)), s = sqrt(-coeff log2 e): 7 centres either side at the default width, 32 at five spacings"""
    from mdgrad_amd import ops
    obs = observable(8)
    assert ops.rdf_frames_reach(obs.spacing, obs.coeff) == 7
    wide = observable(8, width=5 * obs.spacing)
    assert ops.rdf_frames_reach(wide.spacing, wide.coeff) == 32
    # a dropped term is <= 2^-28.1 of a peak term: the nearest dropped centre is at least (R + 1/2) spacings away
    for o in (obs, wide):
        Rr = ops.rdf_frames_reach(o.spacing, o.coeff)
        assert np.exp(o.coeff * ((Rr + 0.5) * o.spacing) ** 2) <= 2.0 ** -28.1


def test_library_validates_rdf_frames_arguments():
    import ctypes as C
    from mdgrad_amd import _lib
    lib = _lib.load()
    cell, tric = _lib.make_cell([5.0, 5.0, 5.0]), _lib.make_cell([[5.0, 0, 0], [1.0, 5.0, 0], [0, 0, 5.0]])
    buf = C.c_void_p(256)                # never dereferenced: every call below fails its checks

    def fwd(n_frames=2, n_atoms=8, c=cell, cutoff=3.0, mu=buf, spacing=0.02, coeff=-1000.0, nbins=100, raw=buf, pos=buf):
        return lib.mdg_rdf_frames_fwd(pos, n_frames, n_atoms, C.byref(c), cutoff, None, mu, spacing, coeff, nbins, raw, None)

    def bwd(g_raw=buf, g_xyz=buf):
        return lib.mdg_rdf_frames_bwd(buf, 2, 8, C.byref(cell), 3.0, None, buf, 0.02, -1000.0, 100, g_raw, g_xyz, None)

    for call, word in ((lambda: fwd(c=tric), "diagonal"), (lambda: fwd(n_frames=0), "empty"), (lambda: fwd(n_atoms=1025), "atoms"),
                       (lambda: fwd(nbins=1), "nbins"), (lambda: fwd(nbins=1025), "nbins"), (lambda: fwd(coeff=0.5), "coeff"),
                       (lambda: fwd(spacing=0.0), "spacing"), (lambda: fwd(cutoff=0.0), "cutoff"), (lambda: fwd(mu=None), "null"),
                       (lambda: fwd(pos=None), "null"), (lambda: fwd(raw=None), "null"), (lambda: bwd(g_raw=None), "null"),
                       (lambda: bwd(g_xyz=None), "null")):
        rc = call()
        assert rc == -1 and word in lib.mdg_last_error().decode(), (rc, word, lib.mdg_last_error())
