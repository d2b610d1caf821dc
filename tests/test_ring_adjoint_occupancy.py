"""Occupancy of the headline ring adjoint, read from the gfx950 code object that build() compiled (no GPU): the LJ 12-6
adjoint that reads the forward's per-frame forces -- with and without the fused RDF -- fits three waves per SIMD: at most 168
registers (512 / 3, allocated in blocks of 8; on gfx950 the accumulation registers share the file, so they count), and no
scratch: the state that is live across a sweep is parked in LDS by hand, a spill into the ring loop is what cost 9 % of the pass
when the allocator was left to reach the count on its own.  The forward kernels stay at four waves per SIMD.  The fused
adjoint's workgroup of four waves asks for one table + four wave slabs of LDS; three such workgroups fit the CU's 160 KB."""
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "mdgrad_amd", "lib", "obj", "traj_small.hip.o")
READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")

FWD_VGPRS = 128           # 4 waves per SIMD (512 / 128)
ADJ_FT_VGPRS = 168        # 3 waves per SIMD (512 / 3 = 170.7, blocks of 8)


def _gfx950_code_object(tmp_path):
    if not os.path.exists(OBJ):
        from mdgrad_amd.build import build_library
        build_library(verbose=False)
    data = open(OBJ, "rb").read()
    o = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert o >= 0, "no offload bundle in %s" % OBJ
    n = struct.unpack_from("<Q", data, o + 24)[0]
    p = o + 32
    for _ in range(n):
        off, size, il = struct.unpack_from("<QQQ", data, p)
        p += 24
        ident = data[p:p + il].decode()
        p += il
        if ident.endswith("gfx950"):
            co = tmp_path / "traj_small_gfx950.co"
            co.write_bytes(data[o + off:o + off + size])
            return str(co)
    raise AssertionError("no gfx950 code object in the bundle")


def _kernels(tmp_path):
    """name -> (.vgpr_count, .agpr_count, .private_segment_fixed_size)"""
    out = subprocess.run([READELF, "--notes", _gfx950_code_object(tmp_path)], capture_output=True, text=True, check=True).stdout
    res = {}
    for blk in out.split("  - .agpr_count:")[1:]:
        ag = re.match(r"\s*(\d+)", blk)
        name = re.search(r"\.name:\s+(\S+)", blk)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if ag and name and vg and ps:
            res[name.group(1)] = (int(vg.group(1)), int(ag.group(1)), int(ps.group(1)))
    return res


def _ring(rdf, ft=None):
    # <RDF, KIND_LJ126 = 16, MASK = false, NT = 1[, FT]> of the anonymous namespace
    tail = "" if ft is None else ("Lb1E" if ft else "Lb0E")
    pre = "traj_adj_ring_kernel" if ft is not None else "traj_fwd_ring_kernel"
    return "_ZN12_GLOBAL__N_1%d%sILb%dELi16ELb0ELi1E%sEEvNS_8TrajArgsENS_11RingRdfArgsE" % (len(pre), pre, int(rdf), tail)


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf of the ROCm toolchain is needed")
def test_headline_ring_adjoint_fits_three_waves_per_simd(tmp_path):
    ks = _kernels(tmp_path)
    for rdf in (True, False):
        vg, ag, scratch = ks[_ring(rdf, ft=True)]
        print("adjoint ring kernel, stored forces (rdf=%s): %d VGPRs, %d AGPRs, %d B scratch" % (rdf, vg, ag, scratch))
        assert vg <= ADJ_FT_VGPRS and ag == 0 and scratch == 0, \
            "adjoint ring kernel, stored forces (rdf=%s): %d VGPRs, %d AGPRs, %d B scratch" % (rdf, vg, ag, scratch)


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf of the ROCm toolchain is needed")
def test_forward_ring_kernels_keep_four_waves_per_simd(tmp_path):
    ks = _kernels(tmp_path)
    for rdf in (True, False):
        vg, ag, scratch = ks[_ring(rdf)]
        print("forward ring kernel (rdf=%s): %d VGPRs, %d AGPRs, %d B scratch" % (rdf, vg, ag, scratch))
        assert vg <= FWD_VGPRS and ag == 0 and scratch == 0, \
            "forward ring kernel (rdf=%s): %d VGPRs, %d AGPRs, %d B scratch" % (rdf, vg, ag, scratch)


def test_three_fused_adjoint_workgroups_fit_the_cu():
    """The launch's own arithmetic (csrc/traj_small.hip, csrc/traj_ring.hpp), restated: a workgroup of RING_RDF_ADJ_WAVES = 4
    waves holds the derivative table (16 B per cell) and, per wave, the ring buffers (6 rows) + RING_PARK_VECS = 4 parked
    vectors (3 rows each) of 64 f32x2.  Three workgroups -- twelve waves -- must fit 160 KB at the headline's table of 14 KB
    (100 bins), with room for the allocation granule."""
    src = open(os.path.join(ROOT, "mdgrad_amd", "csrc", "traj_ring.hpp")).read()
    waves = int(re.search(r"constexpr int RING_RDF_ADJ_WAVES = (\d+);", src).group(1))
    vecs = int(re.search(r"constexpr int RING_PARK_VECS = (\d+);", src).group(1))
    per_wave = (6 + 3 * vecs) * 64 * 8
    assert waves == 4, "one wave per SIMD"
    wg = 14 * 1024 + waves * per_wave
    assert 3 * (wg + 2048) <= 160 * 1024, "%d B per workgroup: three do not fit 160 KB" % wg
