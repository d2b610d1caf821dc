"""Pressure observable without a GPU: the fixtures' internal consistency (tests/golden/make_pressure_goldens.py), the
constructor's validation, and the compiled virial kernels' resources read from the gfx950 code object that build() made
(as tests/test_ring_register_budget.py does for the trajectory kernels)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mdgrad_amd", "csrc", "virial.hip")
OBJ = os.path.join(ROOT, "mdgrad_amd", "lib", "obj", "virial.hip.o")
READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")

FWD_BOUND = 1e-5          # the ceiling of the kernels' forward tolerance: the reference's own float32 must pass it
WAVE_VGPRS = 128          # wave-per-frame kernels: four waves per SIMD (49 at the time of writing)
P1_FORMS = ["lj", "ljfam_8_4", "lj69", "exvol12", "exvol10", "morse_pos", "morse_neg", "buck"]


def _cases():
    g1, g2 = load_golden("pressure_p1"), load_golden("pressure_p2")
    return [(n, g1, n + "_") for n in P1_FORMS] + [("stack", g2, "")]


def test_fixtures_are_consistent():
    for name, g, pre in _cases():
        W32, W64, S, K, P = (g[pre + k].astype(np.float64) for k in ("W32", "W64", "S", "K", "P"))
        assert (S > 0).all() and (np.abs(W64) <= S * (1 + 1e-12)).all(), name
        assert (np.abs(W32 - W64) <= FWD_BOUND * S).all(), "%s: float32 reference off its float64 value" % name
        dV = int(g["dim"]) * float(np.prod(g["cell"].astype(np.float64)))
        assert np.allclose(P, (K + W32) / dV, rtol=1e-6, atol=0), name               # (float32 arithmetic of the script)
        assert np.allclose(K, (float(g["mass"]) * g["vel"].astype(np.float64) ** 2).sum((1, 2)), rtol=1e-6, atol=0), name
        assert g[pre + "dW_dq"].shape == g["xyz"].shape and np.isfinite(g[pre + "dW_dq"]).all(), name
        # W is invariant under a translation of the frame: the per-atom gradients of a frame sum to zero
        assert np.abs(g[pre + "dW_dq"].astype(np.float64).sum(1)).max() <= 1e-5 * np.abs(g[pre + "dW_dq"]).max(), name
    g3 = load_golden("pressure_p3")
    assert g3["P_t"].shape == (int(g3["n_steps"]),)
    assert np.isclose(float(g3["loss"][0]), ((g3["P_t"].astype(np.float64) - float(g3["target"])) ** 2).sum(), rtol=1e-5)


def test_constructor_validation():
    """What Pressure refuses before any kernel runs: the model classes (md._pair_terms_of) and the frame shapes."""
    import torch
    from mdgrad_amd import md, thermo
    assert md._pair_terms_of(torch.nn.Linear(2, 2)) is None
    assert callable(thermo.Pressure) and "Yukawa" in thermo._FORMS and "ModifiedMorse" in thermo._FORMS
    obs = thermo.Pressure.__new__(thermo.Pressure)
    torch.nn.Module.__init__(obs)
    obs.natoms = 4
    with pytest.raises(ValueError, match="k \\* 4"):
        obs._frames(torch.zeros(2, 6, 3), "q")
    with pytest.raises(ValueError):
        obs._frames(torch.zeros(4, 2), "q")
    with pytest.raises(ValueError):
        obs._frames(torch.zeros(3), "q")
    x, lead = obs._frames(torch.zeros(5, 2, 8, 3), "q")
    assert x.shape == (20, 4, 3) and lead == (5, 2, 2)
    x, lead = obs._frames(torch.zeros(4, 3), "q")
    assert x.shape == (1, 4, 3) and lead == ()
    with pytest.raises(ValueError, match="agree"):
        obs.forward(torch.zeros(2, 4, 3), torch.zeros(3, 4, 3))


def test_library_validates_virial_arguments():
    """Argument errors return -1 with a message, before anything is launched (no device needed)."""
    import ctypes as C
    from mdgrad_amd import _lib, ops
    lib = _lib.load()
    cell, tric = _lib.make_cell([5.0, 5.0, 5.0]), _lib.make_cell([[5.0, 0, 0], [1.0, 5.0, 0], [0, 0, 5.0]])
    lj = ops.make_term(dict(kind=_lib.PAIR_LJ, p=12, q=6, c=1.0), 2.5, 0, 2)
    one = ops.make_terms([lj], 2)
    buf = C.c_void_p(256)                # never dereferenced: every call below fails its checks

    def fwd(n_frames=2, n_atoms=8, c=cell, terms=one, theta=buf):
        return lib.mdg_virial_fwd(buf, n_frames, n_atoms, C.byref(c), C.byref(terms), theta, buf, buf, None)

    table = ops.make_terms([ops.make_term(dict(kind=4, p=8), 2.5, 0, 16)], 16)
    shifted = ops.make_terms([ops.make_term(dict(kind=_lib.PAIR_LJ, p=12, q=6), 2.5, 1, 2)], 2)
    for call, word in ((lambda: fwd(c=tric), "diagonal"), (lambda: fwd(n_frames=0), "empty"),
                       (lambda: fwd(n_atoms=40000), "atoms"), (lambda: fwd(theta=None), "theta"),
                       (lambda: fwd(terms=ops.make_terms([], 0)), "terms"), (lambda: fwd(terms=table), "built-in"),
                       (lambda: fwd(terms=shifted), "offset"),
                       (lambda: lib.mdg_virial_bwd(buf, 2, 8, C.byref(cell), C.byref(one), buf, None, buf, buf, buf, None), "null")):
        rc = call()
        assert rc == -1 and word in lib.mdg_last_error().decode(), (rc, word, lib.mdg_last_error())
    assert lib.mdg_virial_workspace(8192, 108, 2) == 8192 * 2
    assert lib.mdg_virial_workspace(64, 4096, 2) == 64 * 16 * 9          # 16 i-blocks x 9 shells of tiles > 64 * 16 * 2
    assert lib.mdg_virial_workspace(3, 108, 0) == 1


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
            co = tmp_path / "virial_gfx950.co"
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
def test_virial_kernels_use_no_scratch_and_the_wave_kernels_keep_four_waves(tmp_path):
    ks = _kernels(tmp_path)
    names = sorted(ks)
    # the instantiations of csrc/frame_pairs.hpp for VirialVisit: value (0) and full rows (2), a wave / a workgroup per frame
    wave = [n for n in names if "fp_frame_kernel" in n and "VirialVisitELi64E" in n]
    assert len(wave) == 2, names
    for stem in ("VirialVisitELi64ELi0E", "VirialVisitELi64ELi2E", "VirialVisitELi256ELi0E", "VirialVisitELi256ELi2E",
                 "fp_tile_once_kernel", "fp_tile_rows_kernel", "fp_row_sum_kernel", "fp_col_sum_kernel"):
        assert any(stem in n for n in names), "kernel %s is missing from virial.hip.o: %s" % (stem, names)
    for n, (vgprs, scratch) in ks.items():
        print("%-110s %3d VGPRs, %d B scratch" % (n, vgprs, scratch))
        assert scratch == 0, "%s uses %d B of scratch per lane" % (n, scratch)
        if n in wave:
            assert vgprs <= WAVE_VGPRS, "%s: %d VGPRs" % (n, vgprs)


def test_virial_source_has_no_floating_point_atomics():
    for path in (SRC, os.path.join(os.path.dirname(SRC), "frame_pairs.hpp")):        # the policy, and the sweeps it runs on
        src = open(path).read()
        code = "\n".join(line.split("//")[0] for line in src.splitlines())
        assert "unsafeAtomicAdd" not in code and "atomicAdd" not in code and "atomic" not in code.lower(), path
