"""Per-iteration instruction counts of the ring loops (`#pragma unroll 1` in ring_sweep, csrc/traj_ring.hpp) of the headline
ring kernels, from the gfx950 code object that build() compiled (no GPU).

    python tools/ring_isa_count.py [traj_small.hip.o] > table
    python tools/ring_isa_count.py --opcodes 19 [traj_small.hip.o]     # + the opcode histogram of loop 19 of each kernel
    python tools/ring_isa_count.py --opcodes all --listing [...]       # every loop's histogram and its instructions

A ring loop is an innermost loop (a backward conditional branch with no other backward branch inside) that holds
ds_bpermute_b32.  The sweep variant is read off the loop's LDS traffic:

    bpermute  ds_read_b128  ds_add_u32   variant
       12         yes           -        adjoint LEVEL 3 / RDF 2 (gj + rj travel, table lookups)
        6          -            -        adjoint LEVEL 3 / RDF 0 (the same evaluation at a frame the observable skips) or
                                         forward LEVEL 1 / RDF 0 (fj travels) -- told apart by the kernel
       12          -            -        adjoint LEVEL 2 / RDF 0 (fj + gj travel)
        6          -           yes       forward LEVEL 1 / RDF 1 (fj travels, histogram atomics)

and NEAR / general minimum image by v_rndne_f32 (the general form rounds; the window form compares), FULL (no per-pair
existence flags: the even-N specialisation) by its compares (full=1: only the visitor address, the cutoff tests and the
observable's range tests are left): the listing prints every loop in address order with its features and leaves the naming to
the reader where two loops share a row.  v_mov: v_mov_b32 in the loop; addr: the VALU instructions that produce the address of the first visitor read (address_valu).
Columns: VALU (all vector ALU, VOPC included), VOPC (v_cmp*), SALU, DS (LDS instructions, bpermute included), total, and
cycles: the loop's VALU instructions weighted with the measured issue cost of each form (cycles per wave-instruction and
SIMD, tools/micro/valu_rate.hip: profiles/r05_valu_rate.txt for the packed forms, v_rcp and plain v_fma,
profiles/valu_rate_plain.txt for moves, selects, integer adds, compares, conversions, v_fract, v_med3 and v_sqrt; a form
neither file has a row for takes v_fma_f32's cost).  The cycles are those of one wave with the pipe to itself: the cost
model of docs/KERNELS.md, not a measurement of the loop."""
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


RATE_FILES = [os.path.join(ROOT, "profiles", "r05_valu_rate.txt"), os.path.join(ROOT, "profiles", "valu_rate_plain.txt")]
INT_PREFIXES = ("v_add_u32", "v_add_co", "v_addc", "v_sub_u32", "v_subrev_u32", "v_sub_co", "v_subrev_co", "v_add3", "v_lshl", "v_lshr",
                "v_ashr", "v_and", "v_or", "v_xor", "v_bfe", "v_bfi", "v_mad_u32", "v_mad_i32", "v_mul_u32", "v_mul_i32", "v_mul_lo",
                "v_min_u32", "v_max_u32", "v_min_i32", "v_max_i32", "v_not")


def rates(files=None):
    """{row name: cycles per wave-instruction}; the first file that has a row wins (within a file: its first section)"""
    out = {}
    for f in files or RATE_FILES:
        if not os.path.exists(f):
            continue
        for ln in open(f):
            m = re.match(r"^(\S.*?)\s+[\d.]+ ms\s+([\d.]+) cycles per wave-instruction", ln)
            if m and m.group(1) not in out:
                out[m.group(1)] = float(m.group(2))
    return out


def weight(op, r):
    """cost of one VALU opcode from the rows of rates()"""
    plain = r.get("v_fma_f32", 4.0)
    for pre, row in (("v_pk_fma_f32", "v_pk_fma_f32"), ("v_pk_mul_f32", "v_pk_mul_f32"), ("v_pk_add_f32", "v_pk_add_f32"),
                     ("v_rcp_f32", "v_rcp_f32"), ("v_sqrt_f32", "v_sqrt_f32"), ("v_rndne_f32", "v_rndne + v_med3"),
                     ("v_med3_f32", "v_med3_f32"), ("v_mov_b32", "v_mov_b32"), ("v_cndmask_b32", "v_cndmask_b32"),
                     ("v_cvt_", "v_cvt_i32_f32"), ("v_fract_f32", "v_fract_f32"), ("v_cmp", "v_cmp_lt_u32")):
        if op.startswith(pre):
            return r.get(row, plain)
    if op.startswith(INT_PREFIXES):
        return r.get("v_add_u32", plain)
    return plain


def cycles(body, r):
    return sum(weight(s.split()[0], r) for s in body if s.startswith("v_"))


def histogram(body):
    h = {}
    for s in body:
        o = s.split()[0]
        h[o] = h.get(o, 0) + 1
    return sorted(h.items(), key=lambda kv: (-kv[1], kv[0]))


def ring_loops(obj=None):
    """{kernel: [instructions of each ring loop, in address order]} of the two headline instantiations"""
    with tempfile.TemporaryDirectory() as td:
        bodies = kernel_bodies(code_object(obj or OBJ, os.path.join(td, "k.co")))
    res = {}
    for k in KERNELS:
        ins, inner = loops(bodies[k])
        res[k] = [ins[a:b + 1] for a, b in inner if any(s.startswith("ds_bpermute_b32") for s in ins[a:b + 1])]
    return res


def classify(body):
    op = [s.split()[0] for s in body]
    c = {"VALU": sum(o.startswith("v_") for o in op), "VOPC": sum(o.startswith("v_cmp") for o in op),
         "SALU": sum(o.startswith("s_") and not o.startswith(("s_waitcnt", "s_nop", "s_cbranch", "s_branch")) for o in op),
         "DS": sum(o.startswith("ds_") for o in op), "total": len(op)}
    f = {"bperm": op.count("ds_bpermute_b32"), "b128": "ds_read_b128" in op, "add": "ds_add_u32" in op,
         "rndne": any(o.startswith("v_rndne") for o in op), "cndmask": sum(o.startswith("v_cndmask") for o in op),
         "pk": sum(o.startswith("v_pk_") for o in op)}
    # FULL: the window form without existence flags -- what is left of the compares is the visitor address (1), the two
    # cutoff tests of each of the two operations where forces or H.w are evaluated (4: the loops with v_rcp_f32) and, with the
    # fused observable, its two range tests per operation (4)
    f["full"] = (not f["rndne"] and f["bperm"] in (6, 12)
                 and c["VOPC"] == 1 + (4 if "v_rcp_f32_e32" in op else 0) + (4 if f["b128"] or f["add"] else 0))
    f["mov"] = sum(o.startswith("v_mov_b32") for o in op)
    f["addr"] = address_valu(body)
    return c, f


def _regs(tok):
    """registers named by one operand: v7 -> {v7}, v[4:7] -> {v4..v7}, s[2:3] -> {s2, s3}, vcc"""
    m = re.match(r"^([vs])\[(\d+):(\d+)\]$", tok)
    if m:
        return {"%s%d" % (m.group(1), n) for n in range(int(m.group(2)), int(m.group(3)) + 1)}
    if re.match(r"^[vs]\d+$", tok) or tok in ("vcc", "scc"):
        return {tok}
    return set()


def address_valu(body):
    """VALU instructions per iteration that the visitor address costs: the ones in the loop that (transitively) produce the
    address register of the loop's first read of a visitor row (ds_read_b64 / ds_read2st64_b64).  The walk goes backwards
    from the read, once round the loop (the compiler rotates some loops: the read need not come first); a register with no
    definition in the loop is loop-invariant and ends its branch."""
    first = next((i for i, s in enumerate(body) if s.split()[0].startswith(("ds_read_b64", "ds_read2st64_b64", "ds_read2_b64"))), None)
    if first is None:
        return 0
    ops = [t.strip() for t in body[first].split(None, 1)[1].split(",")]
    need, n = _regs(ops[1].split()[0]), 0
    for step in range(1, len(body)):
        s = body[(first - step) % len(body)]
        o, _, rest = s.partition(" ")
        toks = [t.strip().split()[0] for t in rest.split(",") if t.strip()]
        if not toks or o.startswith(("s_waitcnt", "s_nop", "s_cbranch", "s_branch", "ds_write", "ds_add")):
            continue
        dst = _regs(toks[0])
        if o.startswith(("s_add_", "s_sub_", "s_cmp")):
            dst |= {"scc"}
        if not (dst & need):
            continue
        need -= dst
        for t in toks[1:]:
            need |= _regs(t)
        if o.startswith("v_"):
            n += 1
    return n


def main():
    args = sys.argv[1:]
    want, listing = None, False
    if "--listing" in args:
        listing = True
        args.remove("--listing")
    if "--opcodes" in args:
        i = args.index("--opcodes")
        want = args[i + 1]
        del args[i:i + 2]
    obj = args[0] if args else OBJ
    r = rates()
    all_loops = ring_loops(obj)
    for k in KERNELS:
        print("== %s" % k)
        print("%-6s %5s %5s %5s %4s %6s %7s   %s" % ("loop", "VALU", "VOPC", "SALU", "DS", "total", "cycles", "features"))
        for n, body in enumerate(all_loops[k], 1):
            c, f = classify(body)
            print("%-6d %5d %5d %5d %4d %6d %7.0f   bpermute=%d table=%d hist=%d image=%s full=%d v_cndmask=%d v_pk=%d v_mov=%d addr=%d" % (
                n, c["VALU"], c["VOPC"], c["SALU"], c["DS"], c["total"], cycles(body, r), f["bperm"], f["b128"], f["add"],
                "general" if f["rndne"] else "near", f["full"], f["cndmask"], f["pk"], f["mov"], f["addr"]))
        for n, body in enumerate(all_loops[k], 1):
            if want is None or (want != "all" and int(want) != n):
                continue
            print("-- loop %d: opcode, count, cycles each" % n)
            for o, cnt in histogram(body):
                print("   %-24s %4d %s" % (o, cnt, ("%6.2f" % weight(o, r)) if o.startswith("v_") else ""))
            if listing:
                for s_ in body:
                    print("      " + s_)


if __name__ == "__main__":
    main()
