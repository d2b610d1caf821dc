"""Intermediate scattering functions without a GPU: pins on the float64 definition of the tests (tests/isf_ref.py),
relaxation / relaxation_time, what the constructor and the library refuse before any launch, and the compiled kernels'
resources read from the gfx950 code object that build() made (as tests/test_msd_host.py does for K17)."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from isf_ref import isf64, random_walk
from sk_ref import sk64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mdgrad_amd", "csrc", "isf.hip")
OBJ = os.path.join(ROOT, "mdgrad_amd", "lib", "obj", "isf.hip.o")
READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
ISF_VGPRS = 128           # 256-thread workgroups: four waves per SIMD stay possible up to here (docs/KERNELS.md)


def host_system(n_atoms, cell=(5.0, 5.0, 5.0), dim=3):
    from mdgrad_amd.system import System
    pos = np.random.default_rng(0).uniform(0, 5.0, (n_atoms, 3))
    return System(positions=pos, cell=np.asarray(cell, dtype=np.float64), masses=np.full(n_atoms, 1.008), device="cpu", dim=dim)


def vectors(cell, nbins, k_range, max_per_bin=None):
    from mdgrad_amd.observable import sk_vectors
    n, seg, kabs, _ = sk_vectors(np.asarray(cell, dtype=np.float32).astype(np.float64), nbins, k_range, 3, max_per_bin)
    return n, seg, kabs


# ---------------------------------------------------------------------------------------------- (a) the reference itself
def test_reference_on_ballistic_motion():
    """x = x0 + v t with float32-exact inputs: F_s[k, tau] = sum_i w_i^2 cos(k.v_i tau) / W2."""
    rng = np.random.default_rng(1)
    N, T, L = 7, 12, 12
    cell = np.array([8.0, 4.0, 16.0], dtype=np.float32)
    x0 = rng.integers(-40, 40, (1, N, 3)).astype(np.float64)
    v = rng.integers(-6, 7, (N, 3)).astype(np.float64) / 8
    x = x0 + v[None] * np.arange(T)[:, None, None]
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    n, seg, _ = vectors(cell, 5, (0.5, 4.0), 6)
    k = 2 * np.pi * n / cell.astype(np.float64)
    w = (rng.integers(1, 9, N) / 4).astype(np.float32)
    for weights in (None, w):
        w2 = np.ones(N) if weights is None else weights.astype(np.float64) ** 2
        for stride in (1, 3):
            r = isf64(x, cell, n, seg, L, stride, weights, coherent=False)
            tau = np.arange(L, dtype=np.float64)
            want = (w2[None, :, None] * np.cos((k @ v.T)[:, :, None] * tau)).sum(1) / w2.sum()          # [M, L]
            assert np.abs(r["Fsk"] - want).max() <= 1e-12


def test_reference_identities():
    """N = 1: F = F_s.  origin_stride = 1: F[:, 0] is the frame mean of S.  F_s[:, 0] = 1.  Shifts by whole cells change
    nothing.  The gradient is bounded by gabs and vanishes for atoms of weight 0."""
    cell = np.array([4.0, 8.0, 4.0], dtype=np.float32)                  # exact in float32, as are the shifts below
    n, seg, _ = vectors(cell, 6, (1.0, 6.0), 5)
    x1 = (np.round(random_walk(9, 1, seed=2, step=0.4, spread=8.0) * 256) / 256).astype(np.float32)
    r = isf64(x1, cell, n, seg, 9, 2)
    assert np.abs(r["F"] - r["Fs"]).max() <= 1e-14 and np.abs(r["g"] - r["gs"]).max() <= 1e-12
    x = (np.round(random_walk(10, 11, seed=3, step=0.4, spread=8.0) * 256) / 256).astype(np.float32)
    w = np.random.default_rng(4).uniform(0.25, 2, 11).astype(np.float32)
    w[3] = 0.0
    G = np.random.default_rng(5).uniform(-1, 1, (6, 7))
    for weights in (None, w):
        r = isf64(x, cell, n, seg, 7, 1, weights, G)
        S = sk64(x, cell, n, seg, weights)[0]                                # [T, B]
        assert np.abs(r["F"][:, 0] - S.mean(0)).max() <= 1e-12
        assert np.abs(r["Fs"][:, 0] - 1.0).max() <= 1e-14
        rng = np.random.default_rng(6)
        shift = rng.integers(-7, 8, x.shape).astype(np.float64) * cell.astype(np.float64)
        xs = x.astype(np.float64) + shift
        assert np.array_equal(xs.astype(np.float32).astype(np.float64), xs)
        rs = isf64(xs, cell, n, seg, 7, 1, weights, G)
        assert np.abs(rs["F"] - r["F"]).max() <= 1e-9 and np.abs(rs["Fs"] - r["Fs"]).max() <= 1e-9
        assert (np.abs(r["gs"]) <= r["gabs"] * (1 + 1e-12) + 1e-300).all()
        if weights is not None:
            assert (r["g"][:, 3] == 0).all() and (r["gs"][:, 3] == 0).all() and (r["gabs"][:, 3] == 0).all()
    # origin_stride = s against the explicit loop over the origins (one vector, self part)
    k = 2 * np.pi * n / cell.astype(np.float64)
    xd = x.astype(np.float64)
    for s in (1, 3, 11):
        r = isf64(x, cell, n, seg, 7, s, coherent=False)
        for tau in range(7):
            t0s = [t0 for t0 in range(0, 10, s) if t0 + tau < 10]
            assert len(t0s) == (9 - tau) // s + 1
            want = np.mean([np.cos((xd[t0 + tau] - xd[t0]) @ k[0]).mean() for t0 in t0s])
            assert abs(r["Fsk"][0, tau] - want) <= 1e-13


WALK = dict(T=16, N=4096, seed=11, sigma=0.3, cell=(10.0, 10.0, 10.0), nbins=4, k_range=(0.5, 3.2), max_per_bin=3)


def walk_expected(kabs, seg, L, sigma):
    """exp(-k^2 sigma^2 tau / 2) of every vector, averaged over each bin."""
    tau = np.arange(L, dtype=np.float64)
    per_vec = np.exp(-0.5 * (kabs[:, None] * sigma) ** 2 * tau[None])
    return np.stack([per_vec[seg[b]:seg[b + 1]].mean(0) for b in range(len(seg) - 1)])


def test_reference_random_walk_decays_as_a_gaussian():
    """4 096 walkers with Gaussian steps of sigma per component: F_s(k, tau) = exp(-k^2 sigma^2 tau / 2) within 0.05, more than
    3 standard errors 1 / sqrt(4096) of a single origin."""
    W = WALK
    cell = np.asarray(W["cell"], dtype=np.float32)
    n, seg, kabs = vectors(cell, W["nbins"], W["k_range"], W["max_per_bin"])
    assert (np.diff(seg) > 0).all()
    x = random_walk(W["T"], W["N"], W["seed"], step=W["sigma"])
    r = isf64(x, cell, n, seg, W["T"], 1, coherent=False)
    err = np.abs(r["Fs"] - walk_expected(kabs, seg, W["T"], W["sigma"])).max()
    print("largest |F_s - exp(-k^2 sigma^2 tau / 2)| %.4f" % err)
    assert err < 0.05


# ---------------------------------------------------------------------------------------------- (b) relaxation helpers
def test_relaxation_and_relaxation_time():
    """phi = exp(-tau dt / tau0): the chord between two lags lies above the convex curve by at most dt^2 phi'' / 8 <=
    dt^2 phi(a) / (8 tau0^2), and |phi'| >= phi(b) / tau0 = phi(a) exp(-dt / tau0) / tau0 on the interval, so the interpolated
    crossing is late by at most dt^2 exp(dt / tau0) / (8 tau0)."""
    from mdgrad_amd.observable import relaxation, relaxation_time
    dt, L = 0.1, 40
    tau = torch.arange(L, dtype=torch.float64)
    tau0 = torch.tensor([1.33, 0.75, 2.95], dtype=torch.float64)        # (none crosses exactly at a lag)
    phi = torch.exp(-tau[None] * dt / tau0[:, None])
    phi = torch.cat([phi, torch.ones(1, L, dtype=torch.float64), 0.2 * torch.ones(1, L, dtype=torch.float64)]).requires_grad_(True)
    t = relaxation_time(phi, dt)
    assert t.shape == (5,)
    for i in range(3):
        bound = dt * dt * math.exp(dt / float(tau0[i])) / (8 * float(tau0[i]))
        late = float(t[i].detach()) - float(tau0[i])
        assert 0 <= late <= bound, (late, bound)
    assert math.isinf(float(t[3].detach())) and float(t[4].detach()) == 0.0
    t[:3].sum().backward()
    g = phi.grad
    assert torch.isfinite(g).all() and (g[3:] == 0).all()
    for i in range(3):
        assert int((g[i] != 0).sum()) == 2                                  # the two lags around the crossing
    # another level, a leading batch shape, and a float32 row
    t2 = relaxation_time(phi.detach()[:3].reshape(3, 1, L), dt, level=0.5)
    assert t2.shape == (3, 1) and torch.allclose(t2.reshape(-1), tau0 * math.log(2.0), atol=2e-3, rtol=0)
    assert relaxation_time(phi.detach()[0].float(), dt).dtype == torch.float32
    F = torch.tensor([[2.0, 1.0, 0.5], [0.0, 0.0, 0.0], [-4.0, 2.0, 1.0]], requires_grad=True)
    r = relaxation(F)
    assert torch.equal(r.detach(), torch.tensor([[1.0, 0.5, 0.25], [0.0, 0.0, 0.0], [1.0, -0.5, -0.25]]))
    r.sum().backward()
    assert torch.isfinite(F.grad).all() and (F.grad[1] == 0).all()


# ---------------------------------------------------------------------------------------------- (c) the constructor
def test_constructor_and_shape_validation():
    from mdgrad_amd.observable import intermediate_scattering as isf, isf_max_lags
    from mdgrad_amd import _lib
    ISF_MAX_LAGS = isf_max_lags()
    assert ISF_MAX_LAGS == _lib.load().mdg_isf_max_lags()
    s = host_system(12)
    tric = host_system(12, cell=[[5.0, 0, 0], [0.6, 5.0, 0], [0, 0, 5.0]])
    with pytest.raises(ValueError, match="diagonal"):
        isf(tric, 4, (1.0, 8.0), 4)
    for bad in (0, -1, 1025, 2.5):
        with pytest.raises(ValueError, match="nbins"):
            isf(s, bad, (1.0, 8.0), 4)
    for kr in ((8.0, 1.0), (1.0, 1.0), (0.0, 8.0), (-1.0, 8.0)):
        with pytest.raises(ValueError, match="k_range"):
            isf(s, 4, kr, 4)
    with pytest.raises(ValueError, match="no wave vector"):
        isf(s, 4, (0.1, 1.0), 4)
    for bad in (0, -3, ISF_MAX_LAGS + 1, 2.0):
        with pytest.raises(ValueError, match="t_range"):
            isf(s, 4, (1.0, 8.0), bad)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="origin_stride"):
            isf(s, 4, (1.0, 8.0), 4, origin_stride=bad)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="max_per_bin"):
            isf(s, 4, (1.0, 8.0), 4, max_per_bin=bad)
    with pytest.raises(ValueError, match="kind"):
        isf(s, 4, (1.0, 8.0), 4, kind="distinct")
    with pytest.raises(ValueError, match="weights.*12"):
        isf(s, 4, (1.0, 8.0), 4, weights=np.ones(11))
    with pytest.raises(ValueError, match="weights.*zero"):
        isf(s, 4, (1.0, 8.0), 4, weights=np.zeros(12))
    with pytest.raises(ValueError, match="weights.*finite"):
        isf(s, 4, (1.0, 8.0), 4, weights=[1.0] * 11 + [float("nan")])
    with pytest.raises(ValueError, match="index_tuple"):
        isf(s, 4, (1.0, 8.0), 4, index_tuple=[0, 12])
    with pytest.raises(ValueError, match="index_tuple"):
        isf(s, 4, (1.0, 8.0), 4, index_tuple=[])
    with pytest.raises(ValueError, match="weights.*zero"):
        isf(s, 4, (1.0, 8.0), 4, index_tuple=[0, 1], weights=[0.0, 0.0] + [1.0] * 10)
    assert isf(s, 4, (1.0, 8.0), 4).weights is None
    assert isf(s, 4, (1.0, 8.0), 4, index_tuple=[1, 3]).weights.tolist() == [0, 1, 0, 1] + [0] * 8
    assert isf(s, 4, (1.0, 8.0), 4, index_tuple=([1, 3], [3, 5])).weights.tolist() == [0, 1, 0, 1, 0, 1] + [0] * 6
    assert isf(s, 4, (1.0, 8.0), 4, index_tuple=[0], weights=-np.arange(12.0) - 2).weights.tolist() == [-2.0] + [0] * 11
    from mdgrad_amd.observable import structure_factor
    obs, ref = isf(s, 6, (1.0, 8.0), 5, kind="self", max_per_bin=7, origin_stride=2), structure_factor(s, 6, (1.0, 8.0), max_per_bin=7)
    assert torch.equal(obs.kvecs, ref.kvecs) and torch.equal(obs.n_vectors, ref.n_vectors) and torch.equal(obs.bins, ref.bins)
    assert torch.equal(obs.k, ref.k)
    with pytest.raises(ValueError, match="t_range = 5 exceeds the 4 frames"):
        obs.per_replica(torch.zeros(4, 12, 3))
    with pytest.raises(ValueError, match="k \\* 12"):
        obs.per_replica(torch.zeros(6, 13, 3))
    with pytest.raises(ValueError):
        obs.per_replica(torch.zeros(12, 3))
    with pytest.raises(RuntimeError, match="HIP device"):             # no CPU implementation behind it
        obs(torch.zeros(6, 12, 3))
    for shape, lead in (((6, 12, 3), ()), ((2, 6, 12, 3), (2,)), ((6, 36, 3), (3,)), ((2, 6, 36, 3), (2, 3))):
        x, got = obs._batch(torch.zeros(shape))
        assert x.dim() == 4 and x.shape[1] == 6 and got == lead


# ---------------------------------------------------------------------------------------------- (d) the library
def test_library_validates_isf_arguments():
    """Argument errors return -1 with a message, before anything is launched (no device needed)."""
    import ctypes as C
    from mdgrad_amd import _lib
    lib = _lib.load()
    cell, tric = _lib.make_cell([5.0, 5.0, 5.0]), _lib.make_cell([[5.0, 0, 0], [1.0, 5.0, 0], [0, 0, 5.0]])
    neg = _lib.make_cell([5.0, 5.0, 5.0])
    neg.h[4] = -5.0
    buf = C.c_void_p(256)                # never dereferenced: every call below fails its checks
    max_lags = lib.mdg_isf_max_lags()

    def fwd(kind=1, x=buf, n_batch=2, n_frames=10, n_cols=24, group=12, rep0=0, n_reps=2, c=cell, norm=12.0, kvec=buf, n_vecs=16,
            seg=buf, n_bins=4, n_lags=5, stride=1, F=buf, ws=buf):
        return lib.mdg_isf_fwd(kind, x, n_batch, n_frames, n_cols, group, rep0, n_reps, C.byref(c), None, norm, kvec, n_vecs, seg,
                               n_bins, n_lags, stride, F, ws, None)

    def bwd(kind=0, x=buf, n_frames=10, n_cols=24, n_lags=5, stride=1, norm=12.0, c=cell, gF=buf, gx=buf, ws=buf):
        return lib.mdg_isf_bwd(kind, x, 2, n_frames, n_cols, 12, 0, 2, C.byref(c), None, norm, buf, 16, buf, 4, n_lags, stride, gF,
                               gx, ws, None)

    for call, word in ((lambda: fwd(x=None), "null"), (lambda: fwd(kvec=None), "null"), (lambda: fwd(seg=None), "null"),
                       (lambda: fwd(F=None), "null"), (lambda: fwd(ws=None), "null"), (lambda: fwd(kind=0, F=None), "null"),
                       (lambda: bwd(x=None), "null"), (lambda: bwd(gF=None), "null"), (lambda: bwd(gx=None), "null"),
                       (lambda: bwd(ws=None), "null"), (lambda: bwd(kind=1, gx=None), "null"),
                       (lambda: fwd(kind=2), "kind"), (lambda: bwd(kind=-1), "kind"),
                       (lambda: fwd(n_batch=0), "empty"), (lambda: fwd(n_frames=0), "empty"), (lambda: fwd(group=0), "empty"),
                       (lambda: fwd(n_cols=25), "multiple"), (lambda: bwd(n_cols=25), "multiple"),
                       (lambda: fwd(rep0=1), "replicas"), (lambda: fwd(n_reps=0), "replicas"), (lambda: fwd(rep0=-1), "replicas"),
                       (lambda: fwd(kind=0, n_cols=32769, group=32769, n_reps=1), "atoms"),
                       (lambda: fwd(n_lags=11), "lags"), (lambda: bwd(n_lags=11), "lags"), (lambda: fwd(n_lags=0), "lags"),
                       (lambda: fwd(n_frames=2000, n_lags=max_lags + 1), "lags"),
                       (lambda: bwd(n_frames=2000, n_lags=max_lags + 1), "lags"),
                       (lambda: fwd(stride=0), "origin_stride"), (lambda: bwd(stride=-1), "origin_stride"),
                       (lambda: fwd(n_vecs=0), "vectors"), (lambda: fwd(n_vecs=65537), "vectors"),
                       (lambda: fwd(n_bins=0), "bins"), (lambda: fwd(n_bins=1025), "bins"),
                       (lambda: fwd(c=tric), "diagonal"), (lambda: bwd(c=tric), "diagonal"), (lambda: fwd(c=neg), "positive"),
                       (lambda: fwd(norm=0.0), "norm"), (lambda: bwd(norm=-1.0), "norm")):
        rc = call()
        assert rc == -1 and word in lib.mdg_last_error().decode(), (rc, word, lib.mdg_last_error())
    src = open(SRC).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    tile, window = 1 << const("ISF_TILE_SHIFT"), const("ISF_WINDOW")
    assert lib.mdg_isf_tile_atoms() == tile == 16 and lib.mdg_isf_window() == window == 8
    # the lag limit: what 64 KiB hold at one wave's worth (64) of pairs: a ring of L - 1 + window slots of 2 x 64 floats, an
    # accumulator per (lag, pair), the window's atoms in turns (window x 16 x 8 floats) and 4 vectors
    fits = lambda L: 4 * ((L - 1 + window) * 128 + L * 64 + window * tile * 8 + 16) <= 65536
    assert fits(max_lags) and not fits(max_lags + 1) and max_lags == 75
    # self: one partial per (row, vector, lag, atom tile); coherent: rho partials [rows T, atom blocks, M] float2 and behind
    # them the larger of [rows, L, M] double and [rows T, M] float2
    assert lib.mdg_isf_workspace(1, 16384, 64, 108, 200, 25) == 16384 * 200 * 25 * 7
    assert lib.mdg_isf_workspace(0, 16384, 64, 108, 200, 25) == 2 * 16384 * 200 * (64 * 1 + 64)
    assert lib.mdg_isf_workspace(0, 3, 5, 1025, 17, 5) == 2 * 3 * 17 * (5 * 2 + 5)
    assert lib.mdg_isf_workspace(1, 3, 5, 17, 1, 1) == 3 * 2
    assert lib.mdg_isf_workspace(1, 0, 5, 17, 1, 1) == 0 and lib.mdg_isf_workspace(0, 1, 100, 12, 4, max_lags + 1) == 0


# ---------------------------------------------------------------------------------------------- (e) the code object
def _kernels(tmp_path):
    if not os.path.exists(OBJ):
        from mdgrad_amd.build import build_library
        build_library(verbose=False)
    data = open(OBJ, "rb").read()
    o = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert o >= 0, "no offload bundle in %s" % OBJ
    n = struct.unpack_from("<Q", data, o + 24)[0]
    p, co = o + 32, None
    for _ in range(n):
        off, size, il = struct.unpack_from("<QQQ", data, p)
        p += 24
        ident = data[p:p + il].decode()
        p += il
        if ident.endswith("gfx950"):
            co = tmp_path / "isf_gfx950.co"
            co.write_bytes(data[o + off:o + off + size])
    assert co is not None, "no gfx950 code object in the bundle"
    out = subprocess.run([READELF, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    res = {}
    for blk in out.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if name and vg and ps:
            res[name.group(1)] = (int(vg.group(1)), int(ps.group(1)))
    return res


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf of the ROCm toolchain is needed")
def test_isf_kernels_use_no_scratch_and_stay_under_the_register_bound(tmp_path):
    ks = _kernels(tmp_path)
    names = sorted(ks)
    for stem in ("isf_rho_kernel", "isf_corr_kernel", "isf_bins_kernel", "isf_coef_kernel", "isf_sweep_kernel",
                 "isf_self_fwd_kernel", "isf_self_finish_kernel", "isf_self_bwd_kernel"):
        assert any(stem in n for n in names), "kernel %s is missing from isf.hip.o: %s" % (stem, names)
    for n, (vgprs, scratch) in ks.items():
        print("%-60s %3d VGPRs, scratch %d" % (n, vgprs, scratch))
        assert scratch == 0, "%s uses %d B of scratch per lane" % (n, scratch)
        assert vgprs <= ISF_VGPRS, "%s: %d VGPRs" % (n, vgprs)


def test_isf_source_has_no_floating_point_atomics_and_shares_the_phase_code():
    src = open(SRC).read()
    assert "atomic" not in src.lower() and "asm" not in src
    sk = open(os.path.join(ROOT, "mdgrad_amd", "csrc", "sk.hip")).read()
    for text in (src, sk):
        assert '#include "sk_phase.hpp"' in text
        for helper in ("void turns(", "void load_atom(", "float phase(", "void sincos_turns(", "void rho_sweep(", "void grad_chunk(",
                       "float4 load_n(", "int bin_of("):
            assert helper not in text, "%s is defined outside sk_phase.hpp" % helper
