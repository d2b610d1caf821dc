"""K35: the bond-angle histogram of every frame (observable.angle_distribution.per_frame, ops.AdfFramesFn, mdg_adf_frames_fwd /
_bwd, csrc/adf.hip) against the independent float64 implementation of tests/test_gpu_adf.py (ref64) run frame by frame, and
against the summed histogram of K14 (ops.AdfRawFn).

Tolerances: those tests/test_gpu_adf.py uses for the same arithmetic -- 2e-6 of the largest bin of the frame for the rows, 1e-4
of the largest gradient component for d(sum g_raw[f, b] raw[f, b])/dx, 1e-6 of the largest bin for the rows summed over the
frames against AdfRawFn (the fixed-point scales of the two differ).  Fixtures: lj_frames of that file, 108 atoms and the
32-atom (size 2) box, 1, 3 and 130 frames.  The float64 references are computed once per fixture and shared."""
import math

import numpy as np
import pytest
import torch

from test_gpu_adf import DEV, close, lj_frames, ref64, system_of

pytestmark = pytest.mark.gpu
NBINS = 90


def observable(frames, cell, cutoff, nbins=NBINS, **kw):
    from mdgrad_amd.observable import angle_distribution
    return angle_distribution(system_of(frames[0], cell), nbins, (0.0, math.pi), cutoff=cutoff, keep_angles=False, **kw)


class Case:
    def __init__(self, size, n_frames, seed, cutoff, mask_idx=None, **kw):
        self.frames, self.cell = lj_frames(n_frames, seed, size=size)
        self.N = self.frames.shape[1]
        self.obs = observable(self.frames, self.cell, cutoff, index_tuple=mask_idx, **kw)
        self.g_raw = torch.tensor(np.random.default_rng(seed + 1).normal(0, 1, (n_frames, self.obs.nbins)), dtype=torch.float32,
                                  device=DEV)
        if n_frames > 1:
            self.g_raw[1] = 0.0
        from mdgrad_amd import ops
        self.mask = None if mask_idx is None else ops.build_mask(self.N, mask_idx, None, DEV)
        mu = self.obs.smear.offsets.double()
        refs = [ref64(self.frames[f:f + 1], self.cell, self.obs.cutoff, mu, self.obs.coeff, self.mask, self.g_raw[f].double())
                for f in range(n_frames)]
        self.raw64 = torch.stack([r for r, _ in refs])
        self.grad64 = torch.cat([g for _, g in refs])

    def run(self):
        x = torch.tensor(self.frames, device=DEV, requires_grad=True)
        raw = self.obs.per_frame(x)
        (gx,) = torch.autograd.grad((raw * self.g_raw).sum(), x)
        return raw.detach(), gx


def check(case, tag):
    raw, gx = case.run()
    assert raw.shape == case.raw64.shape and raw.dtype == torch.float32
    for f in range(raw.shape[0]):
        close(raw[f], case.raw64[f], 0, 2e-6 * float(case.raw64[f].abs().max()), "%s frame %d rows vs f64" % (tag, f))
    close(gx, case.grad64, 0, 1e-4 * float(case.grad64.abs().max()), tag + " grad vs f64")
    worst = max(float((raw[f].double() - case.raw64[f]).abs().max() / case.raw64[f].abs().max()) for f in range(raw.shape[0]))
    print("%-40s rows: largest err / largest bin %.3e (allowed 2e-6); grad: %.3e of the largest component (allowed 1e-4)"
          % (tag, worst, float((gx.double() - case.grad64).abs().max() / case.grad64.abs().max())))
    if raw.shape[0] > 1:
        assert float(gx[1].abs().max()) == 0.0, "a zero g_raw row gives a zero gradient"
        assert float(gx[0].abs().max()) > 0.0
    return raw, gx


@pytest.fixture(scope="module")
def lj108():
    return Case(3, 130, 51, 1.5)


@pytest.mark.parametrize("size,n_frames", [(3, 1), (3, 3), (2, 1), (2, 3), (2, 130)])
def test_rows_and_gradient_against_float64(size, n_frames):
    check(Case(size, n_frames, 40 + size + n_frames, 1.5 if size == 3 else 1.4), "lj%d F=%d" % (4 * size ** 3, n_frames))


def test_130_frames_of_108_atoms_and_their_sum_against_the_summed_kernel(lj108):
    from mdgrad_amd import ops
    raw, gx = check(lj108, "lj108 F=130")
    obs = lj108.obs
    total = ops.AdfRawFn.apply(torch.tensor(lj108.frames, device=DEV), obs.smear.offsets, obs.coeff, obs.cutoff, obs._cell_struct,
                               obs._mask, obs.spacing)
    close(raw.double().sum(0), total, 0, 1e-6 * float(total.abs().max()), "rows summed over the frames vs AdfRawFn")
    # normalise(sum of rows) = forward's count
    _, count, _ = obs(torch.tensor(lj108.frames, device=DEV))
    close(obs.normalise(raw.double().sum(0)), count, 0, 2e-6 * float(count.max()), "normalise(sum of rows) vs forward")
    # shapes: one frame, [R, T, N, 3]
    x = torch.tensor(lj108.frames[:4], device=DEV)
    assert torch.equal(obs.per_frame(x[2]), raw[2]) and torch.equal(obs.per_frame(x.reshape(2, 2, 108, 3)).reshape(4, -1), raw[:4])


def test_bitwise_reproducible_and_chunked(lj108, monkeypatch):
    from mdgrad_amd import ops
    r1, g1 = lj108.run()
    r2, g2 = lj108.run()
    assert torch.equal(r1, r2) and torch.equal(g1, g2)
    monkeypatch.setattr(ops, "ADF_CHUNK_FRAMES", 27)            # 5 chunks, the last one short
    r3, g3 = lj108.run()
    assert torch.equal(r3, r1) and torch.equal(g3, g1)


def test_a_non_finite_frame_gives_a_nan_row_and_leaves_the_others(lj108):
    """The kernel's rule, at the entry point: the list is searched on the finite frames (the list builders drop an atom with a
    non-finite coordinate, so through per_frame no angle of it is ever formed), then one coordinate of frame 2 is made NaN."""
    import ctypes as C
    from mdgrad_amd import _lib, ops
    obs, lib = lj108.obs, _lib.load()
    x = torch.tensor(lj108.frames[:5], device=DEV).reshape(-1, 3).contiguous()
    ell = ops.build_ell(x, obs._cell_struct, obs.cutoff, None, group=108)
    mu = obs.smear.offsets.float().contiguous()

    def rows(pos):
        raw = torch.empty(5, obs.nbins, device=DEV)
        _lib.check(lib.mdg_adf_frames_fwd(_lib.ptr(pos), 5, 108, C.byref(obs._cell_struct), float(obs.cutoff), _lib.ptr(ell.col),
                                          _lib.ptr(ell.cnt), ell.max_nbr, _lib.ptr(mu), float(obs.spacing), float(obs.coeff),
                                          obs.nbins, _lib.ptr(raw), _lib.stream_ptr(pos.device)), "mdg_adf_frames_fwd")
        return raw
    good = rows(x)
    assert torch.equal(good, lj108.run()[0][:5])
    bad = x.clone()
    bad[2 * 108 + 7, 1] = float("nan")
    raw = rows(bad)
    assert bool(torch.isnan(raw[2]).all())
    keep = [0, 1, 3, 4]
    assert torch.equal(raw[keep], good[keep]) and bool(torch.isfinite(good).all())


def test_masked_mixture():
    idx = (list(range(0, 108, 3)), list(range(108)))
    case = Case(3, 3, 61, 1.8, mask_idx=idx, nbins=72, width=0.08)
    raw, _ = check(case, "lj108 masked")
    full = observable(case.frames, case.cell, 1.8, nbins=72, width=0.08).per_frame(torch.tensor(case.frames, device=DEV))
    assert float((full - raw).max()) > 1.0
