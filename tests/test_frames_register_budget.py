"""Register budget of the per-frame many-body energy kernels (csrc/sw_frames.hip, csrc/eam_frames.hip, csrc/tersoff_frames.hip
and the parameter reducer csrc/frames_reduce.hip), read from the gfx950 code objects that build() compiled (no GPU): every
kernel of the four translation units stays at <= 128 VGPRs -- four waves per SIMD -- and uses no scratch.  The kernels share
the scaffold of csrc/frame_atoms.hpp, so a change there that silently costs one of them occupancy fails here.  (The widest at
the time of writing: the multi-species Tersoff kernel with the parameter derivative, 106.)"""
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDIR = os.path.join(ROOT, "mdgrad_amd", "lib", "obj")
READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")

UNITS = ("sw_frames", "eam_frames", "tersoff_frames", "frames_reduce")
MAX_VGPRS = 128           # 4 waves per SIMD (512 / 128)
# the kernels each unit must hold (a renamed kernel is not a passed check)
EXPECT = {"sw_frames": ("sw_frames_kernel",), "eam_frames": ("etf_fwd_kernel", "etf_nodes_kernel", "eam_frames_kernel"),
          "tersoff_frames": ("tersoff_frames_kernel",), "frames_reduce": ("frames_theta_reduce_kernel",)}


def _gfx950_code_object(unit, tmp_path):
    obj = os.path.join(OBJDIR, unit + ".hip.o")
    if not os.path.exists(obj):
        from mdgrad_amd.build import build_library
        build_library(verbose=False)
    data = open(obj, "rb").read()
    o = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert o >= 0, "no offload bundle in %s" % obj
    n = struct.unpack_from("<Q", data, o + 8 + 16)[0]
    p = o + 32
    for _ in range(n):
        off, size, il = struct.unpack_from("<QQQ", data, p)
        p += 24
        ident = data[p:p + il].decode()
        p += il
        if ident.endswith("gfx950"):
            co = tmp_path / (unit + "_gfx950.co")
            co.write_bytes(data[o + off:o + off + size])
            return str(co)
    raise AssertionError("no gfx950 code object in the bundle of %s" % obj)


def _kernels(unit, tmp_path):
    """{kernel symbol: (VGPRs, bytes of scratch)} of a unit's code object"""
    out = subprocess.run([READELF, "--notes", _gfx950_code_object(unit, tmp_path)], capture_output=True, text=True, check=True).stdout
    res = {}
    for blk in out.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        assert name and vg and ps, "unreadable kernel note in %s:\n%s" % (unit, blk)
        res[name.group(1)] = (int(vg.group(1)), int(ps.group(1)))
    return res


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf of the ROCm toolchain is needed")
@pytest.mark.parametrize("unit", UNITS)
def test_frame_kernels_keep_four_waves_per_simd_and_no_scratch(unit, tmp_path):
    ks = _kernels(unit, tmp_path)
    for stem in EXPECT[unit]:
        assert any(stem in k for k in ks), "%s holds no %s (kernels: %s)" % (unit, stem, sorted(ks))
    for k, (vgprs, scratch) in sorted(ks.items()):
        assert scratch == 0, "%s: %s uses %d B of scratch" % (unit, k, scratch)
        assert vgprs <= MAX_VGPRS, "%s: %s takes %d VGPRs (> %d: fewer than four waves per SIMD)" % (unit, k, vgprs, MAX_VGPRS)
