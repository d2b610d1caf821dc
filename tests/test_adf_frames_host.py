"""observable.angle_distribution.per_frame / normalise without a GPU: the torch restatement (host / float64 positions, the exact
sum over every centre) against an independent float64 loop over the triplets, the normalised sum against forward's definition,
the index_tuple selection, the shapes, and the argument checks of the C entry points of K35 (csrc/adf.hip).

Tolerance: float64 torch against the float64 loop, 1e-12 of the largest bin."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_gpu_adf import lj_frames

TOL64 = 1e-12
N = 32


def observable(cell, nbins=60, cutoff=1.5, index_tuple=None, width=None, n_rep=None):
    from mdgrad_amd.observable import angle_distribution
    from mdgrad_amd.system import System
    s = System(positions=np.zeros((N, 3)), cell=np.asarray(cell, np.float64), masses=np.ones(N), device="cpu")
    s = s.replicate(n_rep) if n_rep else s
    return angle_distribution(s, nbins, (0.0, math.pi), cutoff=cutoff, index_tuple=index_tuple, width=width, keep_angles=False)


def loop_histogram(frame, L, cutoff, mu, coeff, selected=None):
    """raw[b] = sum over centres j and unordered pairs (i, k) of its neighbours of 2 exp(coeff (theta - mu_b)^2): neighbours by
    the strict minimum image and 0 < d < cutoff, bond vectors re-imaged with -[b >= L/2] + [b < -L/2], theta = atan2(|u x v|, u.v)."""
    x = np.asarray(frame, np.float64)
    L = np.asarray(L, np.float32).astype(np.float64)             # (the observable holds the cell in float32)
    raw = np.zeros(len(mu))
    for j in range(len(x)):
        nb = []
        for i in range(len(x)):
            if i == j or (selected is not None and not selected(i, j)):
                continue
            d = x[i] - x[j]
            s = d / L
            d = d + (-(s > 0.5).astype(float) + (s < -0.5).astype(float)) * L
            if 0.0 < (d ** 2).sum() < cutoff ** 2:
                b = x[i] - x[j]
                nb.append(b + (-(b >= 0.5 * L).astype(float) + (b < -0.5 * L).astype(float)) * L)
        for p in range(len(nb)):
            for q in range(p + 1, len(nb)):
                th = math.atan2(np.linalg.norm(np.cross(nb[p], nb[q])), float(nb[p] @ nb[q]))
                raw += 2.0 * np.exp(coeff * (th - mu) ** 2)
    return raw


def test_rows_sum_to_the_all_triplet_histogram_and_normalise_is_forwards_tail():
    frames, cell = lj_frames(3, 41, size=2)
    obs = observable(cell)
    mu = obs.smear.offsets.double().numpy()
    q = torch.tensor(frames).double().requires_grad_(True)
    raw = obs.per_frame(q)
    assert raw.shape == (3, 60) and raw.dtype == torch.float64
    want = np.stack([loop_histogram(f, cell, obs.cutoff, mu, obs.coeff) for f in frames])
    err = np.abs(raw.detach().numpy() - want).max() / want.max()
    print("angle_distribution.per_frame float64 host: largest error / largest bin %.3e (allowed %.0e)" % (err, TOL64))
    assert err <= TOL64 and want.max() > 10.0
    assert np.abs(raw.detach().numpy()[0] - want[1]).max() > 1e-3 * want.max(), "the frames differ"
    total = want.sum(0)
    assert np.abs(raw.detach().sum(0).numpy() - total).max() <= TOL64 * total.max()
    # forward's definition: count = raw / raw.sum()
    count = obs.normalise(raw.detach().sum(0))
    assert np.abs(count.numpy() - total / total.sum()).max() <= TOL64 * (total / total.sum()).max()
    rows = obs.normalise(raw.detach())
    assert rows.shape == raw.shape and torch.allclose(rows.sum(-1), torch.ones(3, dtype=torch.float64), rtol=1e-14, atol=0)
    # differentiable; a zero upstream row gives a zero gradient
    g = torch.tensor(np.random.default_rng(2).normal(0, 1, (3, 60)))
    g[1] = 0.0
    (gq,) = torch.autograd.grad((raw * g).sum(), q)
    assert bool(torch.isfinite(gq).all()) and float(gq[0].abs().max()) > 0 and float(gq[1].abs().max()) == 0.0
    # ... and agrees with central differences of the loop along one direction
    w = np.random.default_rng(3).normal(0, 1, frames[0].shape)
    h = 1e-6
    fd = ((loop_histogram(frames[0] + h * w, cell, obs.cutoff, mu, obs.coeff)
           - loop_histogram(frames[0] - h * w, cell, obs.cutoff, mu, obs.coeff)) / (2 * h) * g[0].numpy()).sum()
    an = float((gq[0].numpy() * w).sum())
    assert abs(an - fd) <= 1e-6 * max(abs(fd), 1.0), (an, fd)


def test_index_tuple_selection_is_honoured():
    frames, cell = lj_frames(2, 42, size=2)
    idx = (list(range(0, N, 3)), list(range(N)))
    obs = observable(cell, nbins=48, cutoff=1.8, index_tuple=idx, width=0.08)
    mu = obs.smear.offsets.double().numpy()
    first = set(idx[0])
    raw = obs.per_frame(torch.tensor(frames).double())
    want = np.stack([loop_histogram(f, cell, obs.cutoff, mu, obs.coeff, lambda i, j: i in first or j in first) for f in frames])
    assert np.abs(raw.numpy() - want).max() <= TOL64 * want.max()
    full = observable(cell, nbins=48, cutoff=1.8, width=0.08).per_frame(torch.tensor(frames).double())
    assert float((full - raw).min()) >= -1e-9 and float((full - raw).max()) > 1.0


def test_shapes_and_float32_host_path():
    frames, cell = lj_frames(4, 43, size=2)
    obs = observable(cell)
    q = torch.tensor(frames)
    raw = obs.per_frame(q)
    assert raw.shape == (4, 60) and raw.dtype == torch.float32
    r64 = obs.per_frame(q.double())
    assert float((raw.double() - r64).abs().max()) <= 1e-4 * float(r64.max())
    assert obs.per_frame(q[2]).shape == (60,) and torch.equal(obs.per_frame(q[2]), raw[2])
    two = obs.per_frame(q.reshape(2, 2, N, 3))
    assert two.shape == (2, 2, 60) and torch.equal(two.reshape(4, 60), raw)
    st = observable(cell, n_rep=2).per_frame(torch.cat([q[:2], q[2:]], dim=1))            # [2, 2 N, 3]: q[t], q[t + 2]
    assert st.shape == (2, 2, 60) and torch.equal(st[:, 0], raw[:2]) and torch.equal(st[:, 1], raw[2:])
    with pytest.raises(ValueError, match="k \\* 32"):
        obs.per_frame(torch.zeros(3, 50, 3))


def test_library_validates_adf_frames_arguments():
    from mdgrad_amd import _lib
    lib = _lib.load()
    cell, tric = _lib.make_cell([5.0, 5.0, 5.0]), _lib.make_cell([[5.0, 0, 0], [1.0, 5.0, 0], [0, 0, 5.0]])
    buf = C.c_void_p(256)                # never dereferenced: every call below fails its checks

    def fwd(n_frames=2, n_atoms=8, c=cell, cutoff=1.5, col=buf, cnt=buf, max_nbr=8, mu=buf, spacing=0.05, coeff=-200.0, nbins=60,
            raw=buf, pos=buf):
        return lib.mdg_adf_frames_fwd(pos, n_frames, n_atoms, C.byref(c), cutoff, col, cnt, max_nbr, mu, spacing, coeff, nbins, raw,
                                      None)

    def bwd(g_raw=buf, g_xyz=buf, nbins=60, c=cell):
        return lib.mdg_adf_frames_bwd(buf, 2, 8, C.byref(c), 1.5, buf, buf, 8, buf, 0.05, -200.0, nbins, g_raw, g_xyz, None)

    for call, word in ((lambda: fwd(c=tric), "diagonal"), (lambda: fwd(n_frames=0), "empty"), (lambda: fwd(n_atoms=0), "empty"),
                       (lambda: fwd(max_nbr=0), "empty"), (lambda: fwd(nbins=0), "nbins"), (lambda: fwd(nbins=4097), "nbins"),
                       (lambda: fwd(coeff=0.5), "coeff"), (lambda: fwd(spacing=0.0), "distinct"), (lambda: fwd(cutoff=0.0), "cutoff"),
                       (lambda: fwd(mu=None), "null"), (lambda: fwd(pos=None), "null"), (lambda: fwd(col=None), "null"),
                       (lambda: fwd(raw=None), "null output"), (lambda: bwd(g_raw=None), "null g_raw"),
                       (lambda: bwd(g_xyz=None), "null g_raw"), (lambda: bwd(c=tric), "diagonal"), (lambda: bwd(nbins=0), "nbins")):
        rc = call()
        assert rc == -1 and word in lib.mdg_last_error().decode(), (rc, word, lib.mdg_last_error())
