"""Per-iteration instruction counts of the ring loops (`#pragma unroll 1` in ring_sweep, csrc/traj_ring.hpp) of the headline
ring kernels, from the gfx950 code object that build() compiled (no GPU).

    python tools/ring_isa_count.py [traj_small.hip.o] > table

A ring loop is an innermost loop (a backward conditional branch with no other backward branch inside) that holds
ds_bpermute_b32.  The sweep variant is read off the loop's LDS traffic:

    bpermute  ds_read_b128  ds_add_u32   variant
       12         yes           -        adjoint LEVEL 3 / RDF 2 (gj + rj travel, table lookups)
        6          -            -        adjoint LEVEL 3 / RDF 0 (the same evaluation at a frame the observable skips) or
                                         forward LEVEL 1 / RDF 0 (fj travels) -- told apart by the kernel
       12          -            -        adjoint LEVEL 2 / RDF 0 (fj + gj travel)
        6          -           yes       forward LEVEL 1 / RDF 1 (fj travels, histogram atomics)

and NEAR / general minimum image by v_rndne_f32 (the general form rounds; the window form compares), FULL (no per-pair
existence flags: the even-N specialisation) by the order in the kernel, which is the order of the branches in ring_force: the
listing prints every loop in address order with its features and leaves the naming to the reader where two loops share a row.
Columns: VALU (all vector ALU, VOPC included), VOPC (v_cmp*), SALU, DS (LDS instructions, bpermute included), total."""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "mdgrad_amd", "lib", "obj", "traj_small.hip.o")
OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")
KERNELS = {
    "adjoint <RDF, LJ 12-6, FT>": "traj_adj_ring_kernelILb1ELi16ELb0ELi1ELb1EE",
    "forward <RDF, LJ 12-6>": "traj_fwd_ring_kernelILb1ELi16ELb0ELi1EE",
}


def code_object(obj, out):
    data = open(obj, "rb").read()
    o = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    n = struct.unpack_from("<Q", data, o + 24)[0]
    p = o + 32
    for _ in range(n):
        off, size, il = struct.unpack_from("<QQQ", data, p)
        p += 24
        ident = data[p:p + il].decode()
        p += il
        if ident.endswith("gfx950"):
            open(out, "wb").write(data[o + off:o + off + size])
            return out
    raise SystemExit("no gfx950 code object in %s" % obj)


def kernel_bodies(co):
    txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--symbolize-operands", co], capture_output=True, text=True,
                         check=True).stdout
    cur, res = None, {}
    for ln in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", ln)
        if m and not re.match(r"L\d+$", m.group(1)):
            cur = next((k for k, v in KERNELS.items() if v in m.group(1)), None)
            if cur:
                res[cur] = []
            continue
        if cur:
            res[cur].append(ln)
    return res


def loops(lines):
    """innermost loops: (first, last) indices into the instruction list"""
    ins, label_at = [], {}
    for ln in lines:
        m = re.match(r"^[0-9a-f]* ?<(L\d+)>:", ln)
        if m:
            label_at[m.group(1)] = len(ins)
            continue
        s = ln.split("//")[0].strip()
        if s:
            ins.append(s)
    back = []
    for i, s in enumerate(ins):
        m = re.match(r"s_cbranch_\w+ (L\d+)", s)
        if m and label_at.get(m.group(1), len(ins)) <= i:
            back.append((label_at[m.group(1)], i))
    inner = [(a, b) for a, b in back if not any((c, d) != (a, b) and a <= c and d <= b for c, d in back)]
    return ins, inner


def classify(body):
    op = [s.split()[0] for s in body]
    c = {"VALU": sum(o.startswith("v_") for o in op), "VOPC": sum(o.startswith("v_cmp") for o in op),
         "SALU": sum(o.startswith("s_") and not o.startswith(("s_waitcnt", "s_nop", "s_cbranch", "s_branch")) for o in op),
         "DS": sum(o.startswith("ds_") for o in op), "total": len(op)}
    f = {"bperm": op.count("ds_bpermute_b32"), "b128": "ds_read_b128" in op, "add": "ds_add_u32" in op,
         "rndne": any(o.startswith("v_rndne") for o in op), "cndmask": sum(o.startswith("v_cndmask") for o in op),
         "pk": sum(o.startswith("v_pk_") for o in op)}
    return c, f


def main():
    obj = sys.argv[1] if len(sys.argv) > 1 else OBJ
    with tempfile.TemporaryDirectory() as td:
        bodies = kernel_bodies(code_object(obj, os.path.join(td, "k.co")))
    for k in KERNELS:
        print("== %s" % k)
        ins, inner = loops(bodies[k])
        print("%-6s %5s %5s %5s %4s %6s   %s" % ("loop", "VALU", "VOPC", "SALU", "DS", "total", "features"))
        n = 0
        for a, b in inner:
            c, f = classify(ins[a:b + 1])
            if not f["bperm"]:
                continue
            n += 1
            print("%-6d %5d %5d %5d %4d %6d   bpermute=%d table=%d hist=%d image=%s v_cndmask=%d v_pk=%d" % (
                n, c["VALU"], c["VOPC"], c["SALU"], c["DS"], c["total"], f["bperm"], f["b128"], f["add"],
                "general" if f["rndne"] else "near", f["cndmask"], f["pk"]))


if __name__ == "__main__":
    main()
