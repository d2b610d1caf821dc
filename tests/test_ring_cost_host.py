"""Instruction cost of the ring loops of the two headline kernels, read from the gfx950 code object that build() compiled (no
GPU; tools/ring_isa_count.py does the reading): the FULL loops -- the ones the headline runs -- hold no more VALU instructions
than profiles/ring_cost_isa.txt records for this tree, the loops that evaluate the fused RDF derivative table keep its two
cubics scalar (at most two v_mov_b32 per iteration: the one that joins each pair of results into a register pair; the
SLP-packed form needed thirteen), and the visitor address of every ring loop costs at most four VALU instructions."""
import os
import re

import pytest

import conftest  # noqa: F401  (the repository root on sys.path)
from tools import ring_isa_count as isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "ring_cost_isa.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(isa.OBJDUMP), reason="llvm-objdump of the ROCm toolchain is needed")


@pytest.fixture(scope="module")
def loops():
    if not os.path.exists(isa.OBJ):
        from mdgrad_amd.build import build_library
        build_library(verbose=False)
    return {k: [(body,) + isa.classify(body) for body in v] for k, v in isa.ring_loops().items()}


def _recorded_full():
    """{kernel: [VALU of each FULL loop, in address order]} of the `## result` table of profiles/ring_cost_isa.txt"""
    txt = open(RECORD).read()
    txt = txt[txt.index("## result"):]
    res, cur = {}, None
    for ln in txt.splitlines():
        if ln.startswith("== "):
            cur = ln[3:].strip()
            res[cur] = []
        m = re.match(r"^(\d+)\s+(\d+)\s.*\bfull=1\b", ln)
        if m and cur:
            res[cur].append(int(m.group(2)))
    return res


def test_full_loops_hold_no_more_valu_than_recorded(loops):
    rec = _recorded_full()
    assert sorted(rec) == sorted(isa.KERNELS) and all(rec.values()), "no FULL rows in %s" % RECORD
    for k in isa.KERNELS:
        got = [c["VALU"] for _, c, f in loops[k] if f["full"]]
        print("%s: FULL loops VALU %s, recorded %s" % (k, got, rec[k]))
        assert len(got) == len(rec[k]), "%s: %d FULL loops, %d recorded" % (k, len(got), len(rec[k]))
        assert all(a <= b for a, b in zip(got, rec[k])), "%s: FULL loops VALU %s against the recorded %s" % (k, got, rec[k])


def test_rdf_first_evaluation_loops_keep_the_cubic_scalar(loops):
    k = "adjoint <RDF, LJ 12-6, FT>"
    first = [(c, f) for _, c, f in loops[k] if f["b128"] and f["bperm"] == 12]      # LEVEL 3 / RDF 2: gj and rj travel
    assert len(first) >= 3, "general, near and FULL"
    for c, f in first:
        assert f["mov"] <= 2, "a first-evaluation loop of %d VALU holds %d v_mov_b32" % (c["VALU"], f["mov"])


def test_visitor_address_costs_at_most_four_valu(loops):
    n = 0
    for k in isa.KERNELS:
        for body, c, f in loops[k]:
            if f["bperm"] not in (6, 12) or f["addr"] == 0:
                continue                   # (not a ring step: what it reads from LDS sits at loop-invariant addresses)
            n += 1
            assert f["addr"] <= 4, "%s, loop of %d VALU: %d VALU produce the visitor address" % (k, c["VALU"], f["addr"])
    assert n >= 39, "%d ring loops found" % n
