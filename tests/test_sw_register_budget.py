"""Register budget of the Stillinger-Weber list kernels (csrc/sw.hip, csrc/sw_multi.hip: the two views of the one kernel
template of csrc/sw_core.hpp), read from the gfx950 code objects that build() compiled (no GPU): no scratch, and every
instantiation stays at the occupancy step the two separate kernels had before they were folded into the core -- 8 / 6 / 4
waves per SIMD for the one-species view at LEVEL 0 / 1 / 2, 8 / 4 / 3 for the table view.  The level is the integer template
argument in the kernel's symbol.  (At the time of writing: 46 / 80 / 119 and 50 / 108 / 166 VGPRs.)"""
import os
import re

import pytest

from test_frames_register_budget import READELF, _kernels

# unit -> (the view its kernels are instantiated with, VGPR ceiling per LEVEL): 512 / 64 = 8, 512 / 80 = 6, 512 / 128 = 4,
# 512 / 168 = 3 waves per SIMD
BUDGET = {"sw": ("SwOneView", {0: 64, 1: 80, 2: 128}), "sw_multi": ("SwTableView", {0: 64, 1: 128, 2: 168})}


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf of the ROCm toolchain is needed")
@pytest.mark.parametrize("unit", sorted(BUDGET))
def test_sw_list_kernels_keep_their_occupancy_and_no_scratch(unit, tmp_path):
    view, ceiling = BUDGET[unit]
    ks = _kernels(unit, tmp_path)
    seen = {}
    for k, (vgprs, scratch) in sorted(ks.items()):
        assert scratch == 0, "%s: %s uses %d B of scratch" % (unit, k, scratch)
        m = re.search(r"sw_kernelINS_\d+%sELi(\d)E" % view, k)
        if m:
            seen[int(m.group(1))] = (k, vgprs)
    assert sorted(seen) == [0, 1, 2], "%s holds no sw_kernel<%s, 0 / 1 / 2> (kernels: %s)" % (unit, view, sorted(ks))
    for level, (k, vgprs) in sorted(seen.items()):
        assert vgprs <= ceiling[level], "%s: %s takes %d VGPRs (> %d: a wave per SIMD less than before)" % (unit, k, vgprs, ceiling[level])
