"""Structure factor observable without a GPU: the float64 definition of the tests (tests/sk_ref.py) on the perfect lattice, the
wave-vector set of structure_factor.__init__, what the constructor and the library refuse before any launch, and the compiled
kernels' resources read from the gfx950 code object that build() made (as tests/test_pressure_host.py does for K15)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_golden
from sk_ref import sk64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mdgrad_amd", "csrc", "sk.hip")
OBJ = os.path.join(ROOT, "mdgrad_amd", "lib", "obj", "sk.hip.o")
READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
WAVE_VGPRS = 128          # wave-per-frame kernels: four waves per SIMD (44 forward, 69 backward at the time of writing)


def fcc(size=3, a=1.6):
    base = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
    pos = np.array([(np.array([i, j, k]) + b) * a for i in range(size) for j in range(size) for k in range(size) for b in base])
    return pos, np.array([a * size] * 3)


def host_system(pos, cell, dim=3):
    from mdgrad_amd.system import System
    return System(positions=np.asarray(pos, dtype=np.float64), cell=np.asarray(cell, dtype=np.float64),
                  masses=np.full(len(pos), 1.008), device="cpu", dim=dim)


def in_half_space(n):
    return (n[:, 0] > 0) | ((n[:, 0] == 0) & ((n[:, 1] > 0) | ((n[:, 1] == 0) & (n[:, 2] > 0))))


def test_float64_definition_on_the_perfect_lattice():
    """S = 108 at exactly the 32 half-space vectors below k = 16 with n = 3 (h, k, l), h k l all even or all odd, and nothing
    (< 1e-9) at the other 3 812: pins the tests' own reference."""
    from mdgrad_amd.observable import sk_vectors
    pos, cell = fcc()
    n, seg, kabs, _ = sk_vectors(cell, 30, (1.0, 16.0))
    assert len(n) == 3844
    one = np.arange(len(n) + 1)                                        # every vector its own bin
    S, Sk, _ = sk64(pos.astype(np.float32)[None], cell, n, one)
    hkl = n // 3
    bragg = (n % 3 == 0).all(1) & ((hkl % 2 == 0).all(1) | (hkl % 2 == 1).all(1))
    print("Bragg vectors %d, max |S - 108| there %.3e, max S elsewhere %.3e" % (bragg.sum(), np.abs(Sk[0, bragg] - 108).max(),
                                                                                  Sk[0, ~bragg].max()))
    assert bragg.sum() == 32 and (~bragg).sum() == 3812
    assert np.abs(Sk[0, bragg] - 108.0).max() < 1e-9 and Sk[0, ~bragg].max() < 1e-9
    assert np.array_equal(S[0], Sk[0])


def test_vector_set():
    from mdgrad_amd.observable import structure_factor
    pos, cell = fcc()
    obs = structure_factor(host_system(pos, cell), 30, (1.0, 16.0))
    n, cnt = obs.kvecs.numpy(), obs.n_vectors.numpy()
    assert n.shape == (3844, 3) and cnt.sum() == 3844
    assert cnt[:6].tolist() == [3, 6, 4, 15, 12, 21] and cnt[-2:].tolist() == [312, 355]
    assert in_half_space(n).all() and len({tuple(v) for v in n} & {tuple(-v) for v in n}) == 0
    edges = obs.bins.numpy()
    assert np.allclose(edges, np.linspace(1.0, 16.0, 31), rtol=0, atol=1e-12)
    L = np.float32(4.8).astype(np.float64)
    kabs = 2 * np.pi * np.sqrt((n * n).sum(1)) / L
    seg = np.concatenate([[0], np.cumsum(cnt)])
    for b in range(30):
        kb, nb = kabs[seg[b]:seg[b + 1]], n[seg[b]:seg[b + 1]]
        assert ((kb >= edges[b]) & (kb < edges[b + 1])).all()
        keys = [((v * v).sum(), v[0], v[1], v[2]) for v in nb]
        assert keys == sorted(keys), "bin %d is not ordered by (|n|^2, nx, ny, nz)" % b
        assert np.isclose(float(obs.k[b]), kb.mean(), rtol=1e-6)
    # every half-space vector of the shell is there: count them independently
    r = np.arange(-13, 14)
    g = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    kg = 2 * np.pi * np.sqrt((g * g).sum(1)) / L
    assert (in_half_space(g) & (kg >= 1.0) & (kg < 16.0)).sum() == 3844

    thin = structure_factor(host_system(pos, cell), 30, (1.0, 16.0), max_per_bin=8)
    assert thin.n_vectors.tolist() == np.minimum(cnt, 8).tolist()
    seg8 = np.concatenate([[0], np.cumsum(thin.n_vectors.numpy())])
    for b in range(30):
        assert np.array_equal(thin.kvecs.numpy()[seg8[b]:seg8[b + 1]], n[seg[b]:seg[b] + min(8, cnt[b])])

    box = np.array([4.8, 6.0, 7.2])
    ortho = structure_factor(host_system(pos, box), 12, (1.0, 7.0))
    no, co = ortho.kvecs.numpy(), ortho.n_vectors.numpy()
    ko = 2 * np.pi * np.sqrt(((no / box.astype(np.float32).astype(np.float64)) ** 2).sum(1))
    bo = np.repeat(np.arange(12), co)
    eo = ortho.bins.numpy()
    assert ((ko >= eo[bo]) & (ko < eo[bo + 1])).all() and in_half_space(no).all()
    r = np.arange(-9, 10)
    g = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    kg = 2 * np.pi * np.sqrt(((g / box.astype(np.float32).astype(np.float64)) ** 2).sum(1))
    assert (in_half_space(g) & (kg >= 1.0) & (kg < 7.0)).sum() == len(no)

    flat = structure_factor(host_system(pos, cell, dim=2), 10, (1.0, 8.0))
    assert (flat.kvecs[:, 2] == 0).all() and len(flat.kvecs) > 0

    gap = structure_factor(host_system(pos, cell), 4, (0.2, 2.2))        # first bin [0.2, 0.7): below 2 pi / L = 1.309
    assert gap.n_vectors[0] == 0 and np.isclose(float(gap.k[0]), 0.45)


def test_constructor_validation():
    from mdgrad_amd.observable import structure_factor
    pos, cell = fcc()
    s = host_system(pos, cell)
    tric = host_system(pos, np.array([[4.8, 0, 0], [0.6, 4.8, 0], [0, 0, 4.8]]))
    with pytest.raises(ValueError, match="diagonal"):
        structure_factor(tric, 10, (1.0, 8.0))
    for kr in ((8.0, 1.0), (1.0, 1.0), (0.0, 8.0), (-1.0, 8.0)):
        with pytest.raises(ValueError, match="k_range"):
            structure_factor(s, 10, kr)
    with pytest.raises(ValueError, match="no wave vector"):
        structure_factor(s, 4, (0.1, 1.0))
    big, big_cell = fcc(3, 16.0)                                         # L = 48: ~5e5 half-space vectors below k = 8
    with pytest.raises(ValueError, match="max_per_bin"):
        structure_factor(host_system(big, big_cell), 10, (1.0, 8.0))
    assert len(structure_factor(host_system(big, big_cell), 10, (1.0, 8.0), max_per_bin=4).kvecs) == 40
    with pytest.raises(ValueError, match="weights"):
        structure_factor(s, 10, (1.0, 8.0), weights=np.ones(107))
    with pytest.raises(ValueError, match="zero"):
        structure_factor(s, 10, (1.0, 8.0), weights=np.zeros(108))
    with pytest.raises(ValueError, match="nbins"):
        structure_factor(s, 0, (1.0, 8.0))
    obs = structure_factor(s, 10, (1.0, 8.0), weights=np.linspace(0.5, 2, 108))
    assert np.isclose(obs._norm, (np.linspace(0.5, 2, 108).astype(np.float32).astype(np.float64) ** 2).sum())
    with pytest.raises(ValueError, match="k \\* 108"):
        obs.per_frame(torch.zeros(2, 100, 3))
    with pytest.raises(ValueError):
        obs.per_frame(torch.zeros(108, 2))
    with pytest.raises(ValueError):
        obs.per_frame(torch.zeros(3))
    x, lead = obs._frames(torch.zeros(5, 2, 216, 3))
    assert x.shape == (20, 108, 3) and lead == (5, 2, 2)
    x, lead = obs._frames(torch.zeros(108, 3))
    assert x.shape == (1, 108, 3) and lead == ()


def test_library_validates_sk_arguments():
    """Argument errors return -1 with a message, before anything is launched (no device needed)."""
    import ctypes as C
    from mdgrad_amd import _lib
    lib = _lib.load()
    cell, tric = _lib.make_cell([5.0, 5.0, 5.0]), _lib.make_cell([[5.0, 0, 0], [1.0, 5.0, 0], [0, 0, 5.0]])
    buf = C.c_void_p(256)                # never dereferenced: every call below fails its checks

    def fwd(n_frames=2, n_atoms=8, c=cell, norm=8.0, kvec=buf, n_vecs=16, seg=buf, n_bins=4, S=buf, ws=buf):
        return lib.mdg_sk_fwd(buf, n_frames, n_atoms, C.byref(c), None, norm, kvec, n_vecs, seg, n_bins, S, ws, None)

    def bwd(gS=buf, g_pos=buf):
        return lib.mdg_sk_bwd(buf, 2, 8, C.byref(cell), None, 8.0, buf, 16, buf, 4, gS, g_pos, buf, None)

    for call, word in ((lambda: fwd(c=tric), "diagonal"), (lambda: fwd(n_frames=0), "empty"), (lambda: fwd(n_atoms=0), "empty"),
                       (lambda: fwd(n_atoms=32769), "atoms"), (lambda: fwd(n_frames=1 << 24), "frames"),
                       (lambda: fwd(n_vecs=0), "vectors"), (lambda: fwd(n_vecs=65537), "vectors"),
                       (lambda: fwd(n_bins=0), "bins"), (lambda: fwd(n_bins=1025), "bins"), (lambda: fwd(norm=0.0), "norm"),
                       (lambda: fwd(kvec=None), "null"), (lambda: fwd(seg=None), "null"), (lambda: fwd(S=None), "null"),
                       (lambda: fwd(ws=None), "null"), (lambda: bwd(gS=None), "null"), (lambda: bwd(g_pos=None), "null")):
        rc = call()
        assert rc == -1 and word in lib.mdg_last_error().decode(), (rc, word, lib.mdg_last_error())
    assert lib.mdg_sk_workspace(8192, 108, 3844) == 1                      # whole frames in LDS: nothing to keep
    assert lib.mdg_sk_workspace(3, 1024, 500) == 1
    assert lib.mdg_sk_workspace(64, 4096, 1920) == 2 * 64 * 1920 * (4 + 1)  # partials of 4 atom blocks + the coefficients
    assert lib.mdg_sk_workspace(2, 1025, 7) == 2 * 2 * 7 * 3


def test_fixtures_are_consistent():
    from mdgrad_amd.observable import sk_vectors
    p1 = load_golden("pressure_p1")
    for name in ("sk_s1", "sk_s2"):
        g = load_golden(name)
        assert g["S64"].dtype == np.float64 and g["dS_dq"].dtype == np.float64 and g["S64"].shape == (3, 30)
        mpb = int(g["max_per_bin"]) or None
        n, seg, _, _ = sk_vectors(g["cell"].astype(np.float64), 30, tuple(g["k_range"]), 3, mpb)
        assert np.array_equal(np.diff(seg), g["n_vectors"])
        S, _, gq = sk64(g["xyz"], g["cell"], n, seg, g["weights"] if "weights" in g else None, g["gS"])
        assert np.abs(S - g["S64"]).max() < 1e-11 and np.abs(gq - g["dS_dq"]).max() < 1e-9 * np.abs(gq).max()
        # S is invariant under a translation of the frame: the per-atom gradients of a frame sum to zero
        assert np.abs(g["dS_dq"].sum(1)).max() <= 1e-10 * np.abs(g["dS_dq"]).max()
    assert np.array_equal(load_golden("sk_s1")["xyz"], p1["xyz"]) and load_golden("sk_s1")["n_vectors"].sum() == 3844
    assert load_golden("sk_s2")["n_vectors"].max() == 16
    g3 = load_golden("sk_s3")
    assert g3["S_t"].shape == (21, 18) and g3["q_t"].shape == (21, 108, 3)
    assert np.isclose(float(g3["loss"][0]), ((g3["S_t"].mean(0) - 1.0) ** 2).sum(), rtol=1e-12)


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
            co = tmp_path / "sk_gfx950.co"
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
def test_sk_kernels_use_no_scratch_and_the_wave_kernels_keep_four_waves(tmp_path):
    ks = _kernels(tmp_path)
    names = sorted(ks)
    for stem in ("sk_frame_kernelILi64ELb0E", "sk_frame_kernelILi64ELb1E", "sk_frame_kernelILi256ELb0E",
                 "sk_frame_kernelILi256ELb1E", "sk_tile_rho_kernel", "sk_tile_bins_kernel", "sk_tile_coef_kernel",
                 "sk_tile_bwd_kernel"):
        assert any(stem in n for n in names), "kernel %s is missing from sk.hip.o: %s" % (stem, names)
    for n, (vgprs, scratch) in ks.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (n, scratch)
        if "sk_frame_kernelILi64E" in n:
            assert vgprs <= WAVE_VGPRS, "%s: %d VGPRs" % (n, vgprs)


def test_sk_source_has_no_floating_point_atomics():
    src = open(SRC).read()
    assert "atomic" not in src.lower()
