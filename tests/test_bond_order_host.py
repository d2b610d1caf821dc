"""Bond-orientational order without a GPU: the float64 definition of the tests (tests/bond_order_ref.py) against Steinhardt's
values, its invariances and its gradient; the measured rounding constants of the kernels' harmonic recurrences; a float32
rehearsal of the GPU tests' bounds; what the constructor and the library refuse before any launch; and the compiled kernels'
resources read from the gfx950 code object that build() made (as tests/test_msd_host.py does for K17)."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import bond_order_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "mdgrad_amd", "lib", "obj", "bond_order.hip.o")
READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")


def host_system(n_atoms, cell=(5.0, 5.0, 5.0)):
    from mdgrad_amd.system import System
    pos = np.random.default_rng(0).uniform(0, 5.0, (n_atoms, 3))
    return System(positions=pos, cell=np.array(cell), masses=np.full(n_atoms, 1.008), device="cpu")


# ---------------------------------------------------------------------------------------------- (a) the reference itself
@pytest.mark.parametrize("name", sorted(R.LATTICES))
def test_known_values_of_perfect_shells(name):
    """Steinhardt's q_l of the perfect shells to 1e-5; q_1 = q_2 = 0 for all of them, q_3 = 0 for the centrosymmetric ones."""
    kind, reps, rc, ri, vals = R.LATTICES[name]
    pos, box = R.lattice(kind, reps)
    want = {1: 0.0, 2: 0.0}
    want.update(vals)
    if name not in ("hcp", "tetrahedral"):
        want[3] = 0.0
    ls = sorted(want)
    for chunk in (ls[:4], ls[4:]):
        if not chunk:
            continue
        ref = R.bond_order64(pos, box, rc, ri, chunk)
        assert (ref["cnt"] == R.SHELL[name]).all() and np.abs(ref["n"] - R.SHELL[name]).max() < 1e-12
        for k, l in enumerate(chunk):
            print("%-12s q_%-2d %.6f (expected %.5f)" % (name, l, ref["q"][0, k], want[l]))
            assert np.abs(ref["q"][:, k] - want[l]).max() <= 1e-5, (name, l, ref["q"][:, k])
            if name not in ("hcp", "tetrahedral"):                      # one sublattice: Q_l = q_l
                assert abs(ref["Q"][k] - want[l]) <= 1e-5


def cluster(n, seed):
    """float32 [n, 3] on a grid of 2^-14 around the middle of a box of 50: nothing crosses the boundary."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n:
        p = rng.uniform(-1.4, 1.4, 3)
        if all(np.linalg.norm(p - o) >= 0.6 for o in pts):
            pts.append(p)
    return (np.round((np.asarray(pts) + 25.0) * 2 ** 14) / 2 ** 14).astype(np.float32)


def test_reference_is_rotation_invariant():
    x = cluster(14, 1).astype(np.float64) - 25.0
    rot, _ = np.linalg.qr(np.random.default_rng(2).normal(size=(3, 3)))
    a = R.bond_order64(x + 25.0, [50.0] * 3, 1.6, 1.3, (3, 4, 6, 12))
    # (the rotated positions are rounded to float32 again: 50 x 2^-24 = 3e-6 in x, far below what a real dependence would show)
    b = R.bond_order64(x @ rot.T + 25.0, [50.0] * 3, 1.6, 1.3, (3, 4, 6, 12))
    assert (a["cnt"] == b["cnt"]).all() and a["cnt"].min() >= 1
    assert np.abs(a["q"] - b["q"]).max() < 2e-4 and np.abs(a["Q"] - b["Q"]).max() < 2e-4
    assert np.abs(a["q"] - b["q"]).max() > 0                    # (and they are not the same numbers by accident)


def test_reference_gradient_against_central_differences():
    x = cluster(10, 3)
    ls, h, N = (3, 4, 6), 2.0 ** -11, 10
    rng = np.random.default_rng(4)
    G, H, Cm = rng.uniform(-1, 1, (N, 3)).astype(np.float32), rng.uniform(-1, 1, 3).astype(np.float32), rng.uniform(-1, 1, (3, N, N)).astype(np.float32)
    G64, H64, C64 = G.astype(np.float64), H.astype(np.float64), Cm.astype(np.float64)

    def loss(xx):
        r = R.bond_order64(xx, [50.0] * 3, 1.6, 1.3, ls)
        return (G64 * r["q"]).sum() + (H64 * r["Q"]).sum() + (C64 * r["S"]).sum()

    ref = R.bond_order64(x, [50.0] * 3, 1.6, 1.3, ls, G=G, H=H, C=Cm)
    assert not ref["below"].any() and ref["cnt"].min() >= 1
    worst = 0.0
    for i in range(N):
        for c in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, c] += h
            xm[i, c] -= h
            assert xp[i, c] - xm[i, c] == 2 * h                 # exact in float32: the grid of 2^-14
            fd = (loss(xp) - loss(xm)) / (2 * h)
            worst = max(worst, abs(fd - ref["gx"][i, c]))
    scale = np.abs(ref["gx"]).max()
    print("central differences: largest deviation %.3e of largest |g| %.3e" % (worst, scale))
    assert worst <= 2e-4 * scale                                 # h^2 / 6 f''' with f''' / f' ~ l^2 / r^2 ~ 50 .. 100
    assert (np.abs(ref["gx"]).max(1) <= ref["gabs"] * (1 + 1e-9)).all()


# ---------------------------------------------------------------------------------------------- (b) the kernels' recurrences
@pytest.mark.parametrize("l", range(1, 13))
def test_recurrences_in_float64_satisfy_the_addition_theorem_and_their_float32_constants(l):
    u = R.directions(400, seed=l)
    Y, D = R.harmonics(u, l, np.float64)
    s = u.astype(np.float64) / np.linalg.norm(u.astype(np.float64), axis=1, keepdims=True)
    P = R.legendre(l, torch.as_tensor(s @ s.T))[l].numpy()
    assert np.abs(4 * math.pi / (2 * l + 1) * Y @ Y.T - P).max() < 1e-11
    assert np.abs((D * s[:, None, :]).sum(-1)).max() < 1e-9                      # the gradient is tangential
    # sum_m |grad Y_lm|^2 = l (l+1) (2l+1) / (4 pi), and a finite difference along a tangent
    assert np.abs((D * D).sum((1, 2)) / (l * (l + 1) * (2 * l + 1) / (4 * math.pi)) - 1).max() < 1e-10
    t = np.cross(s, np.eye(3)[np.argmin(np.abs(s), axis=1)])
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    h = 1e-5
    Yp, _ = R.harmonics(s + h * t, l, np.float64)
    Ym, _ = R.harmonics(s - h * t, l, np.float64)
    assert np.abs((Yp - Ym) / (2 * h) - (D * t[:, None, :]).sum(-1)).max() < 1e-6 * l ** 3
    # parity, which the backward kernel uses for the end role
    Yn, _ = R.harmonics(-s, l, np.float64)
    assert np.abs(Yn - (-1) ** l * Y).max() < 1e-12
    kv, kg = R.measure_kappa(l)
    print("l %2d: measured kappa %.1f (x 4 = %.1f, table %d), kappa_g %.1f (x 4 = %.1f, table %d)" % (
        l, kv, 4 * kv, R.KAPPA[l], kg, 4 * kg, R.KAPPA_G[l]))
    assert 4 * kv <= R.KAPPA[l] and 4 * kg <= R.KAPPA_G[l]


def _compose32(A, n, ls):
    """(q, Q, S) from float32 moments with the module's own float32 composition."""
    from mdgrad_amd.observable import bond_order
    obs = bond_order(host_system(len(n)), ls=ls, cutoff=1.0)
    At, nt = torch.as_tensor(A), torch.as_tensor(n)
    q, Q = obs._invariants(At, nt), obs._invariants(At.sum(0), nt.sum(0))
    S = torch.stack([4.0 * math.pi / (2 * l + 1) * (At[:, None, a:b] * At[None, :, a:b]).sum(-1)
                     for l, a, b in zip(obs.ls, obs.offsets_l[:-1], obs.offsets_l[1:])])
    return q.double().numpy(), Q.double().numpy(), S.double().numpy()


def test_float32_transcription_stays_inside_the_bounds_of_the_gpu_tests():
    """The numpy float32 transcription of the kernels' forward against the reference on the configurations of the GPU tests:
    the bounds hold there before any GPU is involved; the floor is at least 16 times the bound of q_l; and the seeds are
    good: no atom of the disordered configuration at or below the floor, two atoms of the sparse one without a neighbour."""
    from mdgrad_amd.observable import BOND_ORDER_Q_FLOOR
    D = R.DISORDERED
    cases = [("disordered", R.disordered(1)[0], D["box"], D["cutoff"], D["r_in"], D["ls"]),
             ("sparse", R.sparse9(), R.SPARSE["box"], R.SPARSE["cutoff"], R.SPARSE["r_in"], R.SPARSE["ls"]),
             ("switching", R.switching(), R.SWITCHING["box"], R.SWITCHING["cutoff"], R.SWITCHING["r_in"], R.SWITCHING["ls"])]
    for name, (kind, reps, rc, ri, vals) in R.LATTICES.items():
        pos, box = R.lattice(kind, reps)
        cases.append((name, pos.astype(np.float32), box, rc, ri, tuple(sorted(vals))))
    for name, x, box, rc, ri, ls in cases:
        box = np.broadcast_to(np.asarray(box, dtype=np.float64), (3,))
        ref = R.bond_order64(x, box, rc, ri, ls)
        A, n = R.moments32(x, box, rc, ri, ls)
        q, Q, S = _compose32(A, n, ls)
        fq, fQ = (np.abs(q - ref["q"]) / ref["tol_q"]).max(), (np.abs(Q - ref["Q"]) / ref["tol_Q"]).max()
        fS = (np.abs(S - ref["S"]) / (ref["tol_S"] + 1e-300)).max()
        print("%-12s float32 transcription: q %.3f, Q %.3f, S %.3f of the bound; largest bound of q %.2e" % (name, fq, fQ, fS, ref["tol_q"].max()))
        assert fq <= 1 and fQ <= 1 and fS <= 1
        assert 16 * ref["tol_q"].max() <= BOND_ORDER_Q_FLOOR
        if name == "disordered":
            assert not ref["below"].any() and ref["q"].min() > 0.1 and len(x) % 64 != 0
        if name == "sparse":
            assert (ref["n"] == 0).sum() == 2 and (q[ref["n"] == 0] == 0).all()


# ---------------------------------------------------------------------------------------------- (c) the constructor
def test_constructor_validation():
    from mdgrad_amd.observable import bond_order, bond_order_distribution
    from mdgrad_amd.system import System
    s = host_system(12)
    for bad in ((), (1, 2, 3, 4, 5), (4, 4), (0,), (13,), (4.5,), (-2, 6)):
        with pytest.raises(ValueError, match="ls"):
            bond_order(s, ls=bad, cutoff=1.5)
    with pytest.raises(ValueError, match="cutoff"):
        bond_order(s)
    for bad in (2.5, 3.0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="cutoff"):
            bond_order(s, cutoff=bad)
    with pytest.raises(ValueError, match="cutoff"):
        bond_order(host_system(12, (5.0, 4.0, 5.0)), cutoff=2.2)              # half the SHORTEST length
    for bad in (0.0, -0.1, 1.5, 2.0):
        with pytest.raises(ValueError, match="r_in"):
            bond_order(s, cutoff=1.5, r_in=bad)
    tri = System(positions=np.zeros((4, 3)), cell=np.array([[5.0, 0, 0], [1.0, 5.0, 0], [0, 0, 5.0]]), masses=np.ones(4), device="cpu")
    with pytest.raises(ValueError, match="diagonal"):
        bond_order(tri, cutoff=1.5)
    with pytest.raises(ValueError, match="width"):
        bond_order_distribution(s, 6, 10, (0.0, 1.0), 1.5, width=0.0)
    with pytest.raises(ValueError, match="nbins"):
        bond_order_distribution(s, 6, 0, (0.0, 1.0), 1.5)
    with pytest.raises(ValueError, match="ls"):
        bond_order_distribution(s, 13, 10, (0.0, 1.0), 1.5)
    obs = bond_order(s, cutoff=2.0)
    assert obs.ls == (4, 6) and obs.n_components == 22 and abs(obs.r_in - 1.7) < 1e-12 and obs.offsets_l == (0, 9, 22)
    d = bond_order_distribution(s, 6, 10, (0.0, 1.0), 1.5)
    assert d.ls == (6,) and d.bins.shape == (11,) and abs(d.width - 1.0 / 9) < 1e-6
    with pytest.raises(ValueError, match="k \\* 12"):
        obs.per_atom(torch.zeros(2, 13, 3))
    with pytest.raises(RuntimeError, match="HIP device"):         # no CPU implementation behind it
        obs(torch.zeros(2, 12, 3))


# ---------------------------------------------------------------------------------------------- (d) the library
def test_library_validates_bond_order_arguments():
    """Argument errors return -1 with a message before anything is launched (no device needed); a refused ls comes first."""
    import ctypes as C
    from mdgrad_amd import _lib
    lib = _lib.load()
    buf = C.c_void_p(256)                # never dereferenced: every call below fails its checks
    cell = _lib.make_cell(torch.tensor([5.0, 5.0, 5.0]))

    def arr(*ls):
        return (C.c_int32 * max(len(ls), 1))(*ls)

    def fwd(ls, n_l=None, pos=None, A=None):
        return lib.mdg_bond_order_fwd(pos, 2, 12, C.byref(cell), 1.5, 1.2, None, None, 8, arr(*ls), len(ls) if n_l is None else n_l, A, None, None)

    def bwd(ls, n_l=None):
        return lib.mdg_bond_order_bwd(None, 2, 12, C.byref(cell), 1.5, 1.2, None, None, 8, arr(*ls), len(ls) if n_l is None else n_l, None,
                                      None, None, None)

    for call, word in ((lambda: fwd((4, 6), n_l=0), "n_l"), (lambda: fwd((1, 2, 3, 4, 5)), "n_l"), (lambda: bwd((4,), n_l=-1), "n_l"),
                       (lambda: fwd((0,)), "[1, 12]"), (lambda: fwd((4, 13)), "[1, 12]"), (lambda: bwd((-3, 4)), "[1, 12]"),
                       (lambda: fwd((4, 6, 4)), "distinct"), (lambda: bwd((12, 12)), "distinct"),
                       (lambda: fwd((4, 6)), "null"), (lambda: bwd((4, 6)), "null"),
                       (lambda: fwd((4, 6), pos=buf, A=buf), "null")):
        rc = call()
        assert rc == -1 and word in lib.mdg_last_error().decode(), (rc, word, lib.mdg_last_error())
    assert lib.mdg_bond_order_components(arr(4, 6), 2) == 22 and lib.mdg_bond_order_components(arr(1, 2, 3, 12), 4) == 40
    assert lib.mdg_bond_order_components(arr(4, 4), 2) == 0 and lib.mdg_bond_order_components(arr(4), 0) == 0


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
            co = tmp_path / "bond_order_gfx950.co"
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
def test_bond_order_kernels_use_no_scratch(tmp_path):
    ks = _kernels(tmp_path)
    for stem in ("bond_order_fwd_kernel", "bond_order_bwd_kernel"):
        assert any(stem in n for n in ks), "kernel %s is missing from bond_order.hip.o: %s" % (stem, sorted(ks))
    for n, (vgprs, scratch) in ks.items():
        print("%-70s %3d VGPRs, scratch %d" % (n, vgprs, scratch))
        assert scratch == 0, "%s uses %d B of scratch per lane" % (n, scratch)
        assert vgprs <= 128, "%s: %d VGPRs (four waves per SIMD need <= 128)" % (n, vgprs)
