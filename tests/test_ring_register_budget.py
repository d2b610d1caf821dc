"""Register budget of the headline wave-per-replica kernels, read from the gfx950 code object that build() compiled (no GPU):
the LJ 12-6 forward (with and without the fused RDF) stays at <= 128 VGPRs -- four waves per SIMD --, the adjoint that reads
the forward's per-frame forces stays within ADJ_FT_VGPRS, and none of them uses scratch.  A change that silently costs
occupancy fails here.  (rocprof's `vgpr` column is not the allocated count: the kernel descriptor's .vgpr_count is.)"""
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "mdgrad_amd", "lib", "obj", "traj_small.hip.o")
READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")

FWD_VGPRS = 128           # 4 waves per SIMD (512 / 128)
ADJ_FT_VGPRS = 224        # the adjoint with stored forces: 220 at the time of writing (2 waves per SIMD)


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
    out = subprocess.run([READELF, "--notes", _gfx950_code_object(tmp_path)], capture_output=True, text=True, check=True).stdout
    res = {}
    for blk in out.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if name and vg and ps:
            res[name.group(1)] = (int(vg.group(1)), int(ps.group(1)))
    return res


def _ring(rdf, ft=None):
    # <RDF, KIND_LJ126 = 16, MASK = false, NT = 1[, FT]> of the anonymous namespace
    tail = "" if ft is None else ("Lb1E" if ft else "Lb0E")
    pre = "traj_adj_ring_kernel" if ft is not None else "traj_fwd_ring_kernel"
    return "_ZN12_GLOBAL__N_1%d%sILb%dELi16ELb0ELi1E%sEEvNS_8TrajArgsENS_11RingRdfArgsE" % (len(pre), pre, int(rdf), tail)


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf of the ROCm toolchain is needed")
def test_headline_ring_kernels_keep_their_register_budget(tmp_path):
    ks = _kernels(tmp_path)
    for rdf in (True, False):
        fwd = ks[_ring(rdf)]
        assert fwd[0] <= FWD_VGPRS and fwd[1] == 0, "forward ring kernel (rdf=%s): %d VGPRs, %d B scratch" % (rdf, *fwd)
        adj = ks[_ring(rdf, ft=True)]
        assert adj[0] <= ADJ_FT_VGPRS and adj[1] == 0, "adjoint ring kernel, stored forces (rdf=%s): %d VGPRs, %d B scratch" % (
            rdf, *adj)
        old = ks[_ring(rdf, ft=False)]
        assert old[1] == 0, "adjoint ring kernel (rdf=%s) spills to scratch" % rdf
