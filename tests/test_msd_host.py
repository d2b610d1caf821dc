"""MSD observable without a GPU: pins on the float64 definition of the tests (tests/msd_ref.py), diffusion_coefficient, what
the constructor and the library refuse before any launch, and the compiled kernels' resources read from the gfx950 code object
that build() made (as tests/test_sk_host.py does for K16)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from msd_ref import msd64, random_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mdgrad_amd", "csrc", "msd.hip")
OBJ = os.path.join(ROOT, "mdgrad_amd", "lib", "obj", "msd.hip.o")
READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
MSD_VGPRS = 128           # 256-thread workgroups: four waves per SIMD and more stay possible up to here (docs/KERNELS.md)


def host_system(n_atoms, dim=3):
    from mdgrad_amd.system import System
    pos = np.random.default_rng(0).uniform(0, 5.0, (n_atoms, 3))
    return System(positions=pos, cell=np.array([5.0, 5.0, 5.0]), masses=np.full(n_atoms, 1.008), device="cpu", dim=dim)


# ---------------------------------------------------------------------------------------------- (a) the reference itself
def test_reference_on_ballistic_motion():
    """x = x0 + v t: M2[tau] = <w |v|^2> tau^2, M4[tau] = <w |v|^4> tau^4 (float32-exact inputs: small integers and halves)."""
    rng = np.random.default_rng(1)
    N, T, L = 7, 12, 12
    x0 = rng.integers(-40, 40, (1, N, 3)).astype(np.float64)
    v = rng.integers(-6, 7, (N, 3)).astype(np.float64) / 2
    x = x0 + v[None] * np.arange(T)[:, None, None]
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    w = rng.uniform(0.5, 2.0, N).astype(np.float32)
    v2 = (v * v).sum(1)
    for weights in (None, w):
        wd = np.ones(N) if weights is None else weights.astype(np.float64)
        for stride in (1, 3):
            M2, M4, _, _ = msd64(x, L, stride, weights)
            tau = np.arange(L, dtype=np.float64)
            e2, e4 = (wd * v2).sum() / wd.sum() * tau ** 2, (wd * v2 * v2).sum() / wd.sum() * tau ** 4
            assert np.abs(M2 - e2).max() <= 1e-12 * e2.max() and np.abs(M4 - e4).max() <= 1e-12 * e4.max()
            assert np.all(np.abs(M2[1:] - e2[1:]) <= 1e-12 * e2[1:]) and np.all(np.abs(M4[1:] - e4[1:]) <= 1e-12 * e4[1:])
            assert M2[0] == 0.0 and M4[0] == 0.0


def test_reference_translation_stride_and_lag_zero():
    x = (np.round(random_walk(20, 9, seed=2, drift=4.0) * 1024) / 1024).astype(np.float32)      # multiples of 2^-10 below 64
    w = np.random.default_rng(3).uniform(0, 1, 9).astype(np.float32)
    w[4] = 0.0
    M2, M4, gx, gabs = msd64(x, 20, 1, w)
    assert M2[0] == 0.0 and M4[0] == 0.0 and (M2[1:] > 0).all()
    # a rigid translation of all frames: the shifted coordinates are still exact in float32, so nothing may move at all
    shifted = x.astype(np.float64) + np.array([64.0, -128.0, 32.0])
    assert np.array_equal(shifted.astype(np.float32).astype(np.float64), shifted)
    M2s, M4s, gxs, _ = msd64(shifted, 20, 1, w)
    assert np.array_equal(M2s, M2) and np.array_equal(M4s, M4) and np.array_equal(gxs, gx)
    # origin_stride = s against the explicit loop over the origins
    for s in (1, 2, 3, 7, 21):
        A2, A4, _, _ = msd64(x, 20, s, w)
        wd = w.astype(np.float64)
        xd = x.astype(np.float64)
        for tau in range(20):
            acc2 = acc4 = 0.0
            n = 0
            for t0 in range(0, 20, s):
                if t0 + tau < 20:
                    d2 = ((xd[t0 + tau] - xd[t0]) ** 2).sum(1)
                    acc2 += (wd * d2).sum()
                    acc4 += (wd * d2 * d2).sum()
                    n += 1
            assert n == (19 - tau) // s + 1
            assert abs(A2[tau] - acc2 / (n * wd.sum())) <= 1e-12 * max(acc2, 1.0)
            assert abs(A4[tau] - acc4 / (n * wd.sum())) <= 1e-12 * max(acc4, 1.0)
    # the gradient of a translation-invariant function sums to zero over the frames' common shift; gabs bounds |gx|
    assert np.abs(gx.sum(0).sum(0)).max() <= 1e-12 * gabs.sum()
    assert (np.abs(gx) <= gabs * (1 + 1e-12) + 1e-300).all()
    assert (gx[:, w == 0] == 0).all()


def test_reference_random_walk_is_gaussian():
    """4 096 walkers x 64 frames of a seeded Gaussian walk: alpha_2 = 3 M4 / (5 M2^2) - 1 stays within 0.1 of 0."""
    x = random_walk(64, 4096, seed=11)
    M2, M4, _, _ = msd64(x, 64)
    a2 = 3 * M4[1:] / (5 * M2[1:] ** 2) - 1
    print("largest |alpha_2| %.4f, M2[1] %.4f (3 expected)" % (np.abs(a2).max(), M2[1]))
    assert np.abs(a2).max() < 0.1
    assert abs(M2[1] - 3.0) < 0.05


# ---------------------------------------------------------------------------------------------- (b) diffusion_coefficient
def test_diffusion_coefficient():
    from mdgrad_amd.observable import diffusion_coefficient
    D, dt, L = 0.37, 0.005, 40
    tau = torch.arange(L, dtype=torch.float64)
    m = (6 * D * tau * dt).requires_grad_(True)
    for fr in ((5, 30), (0, L), None, (10, None), (L - 2, L)):
        got = diffusion_coefficient(m, dt, fit_range=fr) if fr is not None else diffusion_coefficient(m, dt)
        assert abs(float(got.detach()) - D) <= 1e-12 * D, fr
    assert abs(float(diffusion_coefficient(4 * D * tau * dt, dt, (3, 20), dim=2)) - D) <= 1e-12
    # d D / d m = the least-squares weights (tau - mean) / (dt sum (tau - mean)^2) / (2 dim) inside the range, 0 outside
    a, b = 5, 30
    (g,) = torch.autograd.grad(diffusion_coefficient(m, dt, (a, b)), m)
    c = tau[a:b] - tau[a:b].mean()
    want = torch.zeros(L, dtype=torch.float64)
    want[a:b] = c / (c.pow(2).sum() * dt) / 6
    assert torch.allclose(g, want, rtol=1e-13, atol=0)
    # a leading batch shape, and an offset does not move the slope
    mb = torch.stack([6 * 0.1 * tau * dt + 1.0, 6 * 0.2 * tau * dt - 2.0]).reshape(2, 1, L)
    out = diffusion_coefficient(mb, dt, (1, L))
    assert out.shape == (2, 1) and torch.allclose(out.reshape(-1), torch.tensor([0.1, 0.2], dtype=torch.float64), rtol=1e-11)
    for fr in ((3, 4), (7, 7), (9, 2), (L - 1, L + 5)):
        with pytest.raises(ValueError, match="fit_range"):
            diffusion_coefficient(m, dt, fit_range=fr)


# ---------------------------------------------------------------------------------------------- (c) the constructor
def test_constructor_validation():
    from mdgrad_amd.observable import msd
    s = host_system(12)
    for bad in (0, -3, 1025):
        with pytest.raises(ValueError, match="t_range"):
            msd(s, bad)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="origin_stride"):
            msd(s, 4, origin_stride=bad)
    with pytest.raises(ValueError, match="weights.*12"):
        msd(s, 4, weights=np.ones(11))
    for bad in ([1.0] * 11 + [float("nan")], [1.0] * 11 + [float("inf")], [1.0] * 11 + [-0.5]):
        with pytest.raises(ValueError, match="weights.*finite and non-negative"):
            msd(s, 4, weights=bad)
    with pytest.raises(ValueError, match="weights.*zero"):
        msd(s, 4, weights=np.zeros(12))
    with pytest.raises(ValueError, match="index_tuple"):
        msd(s, 4, index_tuple=[0, 12])
    with pytest.raises(ValueError, match="index_tuple"):
        msd(s, 4, index_tuple=[])
    with pytest.raises(ValueError, match="weights.*zero"):
        msd(s, 4, index_tuple=[0, 1], weights=[0.0, 0.0] + [1.0] * 10)
    assert msd(s, 4).weights is None
    assert msd(s, 4, index_tuple=[1, 3]).weights.tolist() == [0, 1, 0, 1] + [0] * 8
    assert msd(s, 4, index_tuple=([1, 3], [3, 5])).weights.tolist() == [0, 1, 0, 1, 0, 1] + [0] * 6
    assert msd(s, 4, index_tuple=[0], weights=np.arange(12.0) + 2).weights.tolist() == [2.0] + [0] * 11
    obs = msd(s, 5, origin_stride=2, fourth_moment=False)
    with pytest.raises(ValueError, match="t_range = 5 exceeds the 4 frames"):
        obs.per_replica(torch.zeros(4, 12, 3))
    with pytest.raises(ValueError, match="k \\* 12"):
        obs.per_replica(torch.zeros(6, 13, 3))
    with pytest.raises(ValueError):
        obs.per_replica(torch.zeros(12, 3))
    with pytest.raises(ValueError, match="fourth_moment"):
        obs.moments(torch.zeros(6, 12, 3))
    with pytest.raises(RuntimeError, match="HIP device"):             # no CPU implementation behind it
        obs(torch.zeros(6, 12, 3))
    for shape, lead in (((6, 12, 3), ()), ((2, 6, 12, 3), (2,)), ((6, 36, 3), (3,)), ((2, 6, 36, 3), (2, 3))):
        x, got = obs._batch(torch.zeros(shape))
        assert x.dim() == 4 and x.shape[1] == 6 and got == lead


# ---------------------------------------------------------------------------------------------- (d) the library
def test_library_validates_msd_arguments():
    """Argument errors return -1 with a message, before anything is launched (no device needed)."""
    import ctypes as C
    from mdgrad_amd import _lib
    lib = _lib.load()
    buf = C.c_void_p(256)                # never dereferenced: every call below fails its checks

    def fwd(x=buf, n_batch=2, n_frames=10, n_cols=24, group=12, n_lags=5, stride=1, out2=buf, ws=buf):
        return lib.mdg_msd_fwd(x, n_batch, n_frames, n_cols, group, None, n_lags, stride, out2, None, ws, None)

    def bwd(x=buf, n_frames=10, n_cols=24, group=12, n_lags=5, stride=1, g2=buf, gx=buf, ws=buf):
        return lib.mdg_msd_bwd(x, 2, n_frames, n_cols, group, None, n_lags, stride, g2, None, gx, ws, None)

    for call, word in ((lambda: fwd(x=None), "null"), (lambda: fwd(out2=None), "null"), (lambda: fwd(ws=None), "null"),
                       (lambda: bwd(x=None), "null"), (lambda: bwd(g2=None), "null"), (lambda: bwd(gx=None), "null"),
                       (lambda: bwd(ws=None), "null"),
                       (lambda: fwd(n_lags=11), "lags"), (lambda: bwd(n_lags=11), "lags"), (lambda: fwd(n_lags=0), "lags"),
                       (lambda: fwd(n_frames=2000, n_lags=1025), "lags"),
                       (lambda: fwd(n_cols=25), "multiple"), (lambda: bwd(n_cols=25), "multiple"),
                       (lambda: fwd(group=0), "empty"), (lambda: fwd(n_batch=0), "empty"), (lambda: fwd(n_frames=0), "empty"),
                       (lambda: fwd(stride=0), "origin_stride"), (lambda: bwd(stride=-1), "origin_stride")):
        rc = call()
        assert rc == -1 and word in lib.mdg_last_error().decode(), (rc, word, lib.mdg_last_error())
    tile = lib.mdg_msd_tile_atoms()
    assert tile == 16 and lib.mdg_msd_window() == 16 and lib.mdg_msd_max_lags() == 1024
    # head (sum of the weights) + one partial per (row, lag, atom tile) and moment
    assert lib.mdg_msd_workspace(16384, 108, 108, 25, 0) == 2 + 16384 * 25 * 7
    assert lib.mdg_msd_workspace(2, 3 * 17, 17, 4, 1) == 2 + 2 * (2 * 3) * 4 * 2
    assert lib.mdg_msd_workspace(1, 64, 64, 1024, 1) == 2 + 2 * 1024 * 32          # the atom tile shrinks to 2 at the lag limit
    assert lib.mdg_msd_workspace(1, 25, 12, 4, 0) == 0 and lib.mdg_msd_workspace(1, 24, 12, 1025, 0) == 0


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
            co = tmp_path / "msd_gfx950.co"
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
def test_msd_kernels_use_no_scratch_and_stay_under_the_register_bound(tmp_path):
    ks = _kernels(tmp_path)
    names = sorted(ks)
    for stem in ("msd_fwd_kernelILb0E", "msd_fwd_kernelILb1E", "msd_bwd_kernelILb0E", "msd_bwd_kernelILb1E", "msd_finish_kernel",
                 "msd_wsum_kernel"):
        assert any(stem in n for n in names), "kernel %s is missing from msd.hip.o: %s" % (stem, names)
    for n, (vgprs, scratch) in ks.items():
        print("%-60s %3d VGPRs, scratch %d" % (n, vgprs, scratch))
        assert scratch == 0, "%s uses %d B of scratch per lane" % (n, scratch)
        assert vgprs <= MSD_VGPRS, "%s: %d VGPRs" % (n, vgprs)


def test_msd_source_has_no_floating_point_atomics():
    assert "atomic" not in open(SRC).read().lower()
