#!/usr/bin/env python3
"""Static record of k1's instruction stream, from the built library's disassembly: registers and
spills of the product kernel (k16_fwd_bwd_kernel<16, 2, 8, 1>: cfg3 fp16x3 training), the counts of
the instructions its chunk loop is made of, and how the LDS-DMA pieces and the slab stores are
addressed (a scalar base, or a per-lane 64-bit address the wave had to build).

  python scripts/k16_loop_report.py [LIB.so ...] [--kernel REGEX] [--json]

With several libraries (a parent build and the working tree's) the table has one column per library.
k1 pays for every instruction of a wave's stream, so the counts are whole-kernel
static counts, the same way for every column; the fully unrolled hidden passes dominate them.
A report (DESIGN.md sections 3 and 9) and the source of tests/test_k16_addressing.py's figures."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import isa_check  # noqa: E402

K1 = r"k16_fwd_bwd_kernelILi16ELi2ELi8ELi1ELb0EEEv"   # the plain object's product instantiation
KR = r"kr_fwd_kernelILi16ELb0EEEv"

_SADDR = re.compile(r"^s\[\d+:\d+\]$")


def is_lds_dma(ins):
    return "load_lds" in ins.mn or (ins.mn.startswith("buffer_load") and " lds" in ins.ops)


def is_slab_store(ins):
    """The slab stores are the kernel's nontemporal 12- and 16-byte stores."""
    return ins.mn in ("global_store_dwordx3", "global_store_dwordx4", "buffer_store_dwordx3",
                      "buffer_store_dwordx4") and re.search(r"\bnt\b", ins.ops) is not None


def scalar_base(ins):
    """The instruction takes its base address from scalar registers: the SGPR-base form of a global_*
    instruction (vOffset, [vData,] s[base:base+1]) or a buffer_* instruction (a descriptor)."""
    if ins.mn.startswith("buffer_"):
        return True
    ops = [o.strip().split()[0] for o in ins.ops.split(",") if o.strip()]
    return any(_SADDR.match(o) for o in ops)


def vadd64(ins):
    """64-bit vector address arithmetic: v_lshl_add_u64, or a v_add_co / v_addc_co carry pair (each
    instruction of the pair counts)."""
    return ins.mn.startswith(("v_lshl_add_u64", "v_add_co_u32", "v_addc_co_u32"))


def kernel_meta(lib):
    """{kernel name: (vgprs, sgprs, spilled vgprs, spilled sgprs, scratch bytes)} from the code objects'
    metadata notes."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in isa_check.extract_code_objects(lib, d):
            r = subprocess.run([f"{isa_check.LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True)
            name = None
            cur = {}
            for line in r.stdout.splitlines():
                m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)", line)
                if not m:
                    continue
                k, v = m.group(1), m.group(2)
                if k == "name" and not v.endswith(".kd") and v.startswith("_Z"):
                    name = v
                if k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                         "private_segment_fixed_size", "symbol"):
                    cur[k] = v
                if k == "symbol":
                    sym = v[:-3] if v.endswith(".kd") else v
                    out[sym] = cur
                    cur = {}
    return out


def record(insts, meta):
    c = dict(instructions=len(insts))
    c["mfma"] = sum(i.mfma for i in insts)
    c["ds_read_b128"] = sum(i.mn == "ds_read_b128" for i in insts)
    dma = [i for i in insts if is_lds_dma(i)]
    st = [i for i in insts if is_slab_store(i)]
    c["lds_dma"] = len(dma)
    c["lds_dma_scalar_base"] = sum(scalar_base(i) for i in dma)
    c["slab_stores"] = len(st)
    c["slab_stores_scalar_base"] = sum(scalar_base(i) for i in st)
    c["s_waitcnt"] = sum(i.mn == "s_waitcnt" for i in insts)
    c["s_nop"] = sum(i.mn == "s_nop" for i in insts)
    c["v_lshl_add_u64"] = sum(i.mn.startswith("v_lshl_add_u64") for i in insts)
    c["v_add_co/v_addc_co"] = sum(i.mn.startswith(("v_add_co_u32", "v_addc_co_u32")) for i in insts)
    c["vector_add64"] = sum(vadd64(i) for i in insts)
    c["s_cmp_lg_u64"] = sum(i.mn == "s_cmp_lg_u64" for i in insts)
    c["s_cselect"] = sum(i.mn.startswith("s_cselect") for i in insts)
    c["valu"] = sum(i.valu for i in insts)
    c["salu"] = sum(i.mn.startswith("s_") and i.mn not in ("s_waitcnt", "s_nop", "s_barrier") and
                    not i.mn.startswith(("s_load", "s_buffer_load", "s_branch", "s_cbranch")) for i in insts)
    c["m0_from_cselect"] = len(m0_fed_by_cselect(insts))
    for k, f in (("vgprs", "vgpr_count"), ("sgprs", "sgpr_count"), ("vgpr_spills", "vgpr_spill_count"),
                 ("sgpr_spills", "sgpr_spill_count"), ("scratch_bytes", "private_segment_fixed_size")):
        c[k] = int(meta[f]) if meta and f in meta else None
    return c


def m0_fed_by_cselect(insts):
    """M0 writes whose source scalar register was last written (in the straight line before it) by
    an s_cselect: the null test of a generic -> LDS pointer cast."""
    out = []
    for i, ins in enumerate(insts):
        if not (ins.mn.startswith("s_") and ins.ops.strip().startswith("m0")):
            continue
        srcs = {r for r in isa_check.regs_of(",".join(ins.ops.split(",")[1:])) if r[0] == "s"}
        for p in reversed(insts[max(0, i - 8):i]):
            if p.mn.startswith(("s_branch", "s_cbranch")):
                break
            opl = [o.strip() for o in p.ops.split(",")]
            dst = isa_check.regs_of(opl[0]) if opl and p.mn.startswith("s_") else frozenset()
            if dst & srcs:
                if p.mn.startswith("s_cselect"):
                    out.append(ins)
                break
    return out


def report(lib, kernel_re):
    asm = isa_check.disassemble_all(lib)
    meta = kernel_meta(lib)
    out = {}
    for name, insts in isa_check.parse_kernels(asm, kernel_re).items():
        out[name] = record(insts, meta.get(name))
    return out


ROWS = ("vgprs", "sgprs", "vgpr_spills", "sgpr_spills", "scratch_bytes", "instructions", "mfma", "ds_read_b128",
        "lds_dma", "lds_dma_scalar_base", "slab_stores", "slab_stores_scalar_base", "s_waitcnt", "s_nop",
        "v_lshl_add_u64", "v_add_co/v_addc_co", "vector_add64", "s_cmp_lg_u64", "s_cselect", "m0_from_cselect",
        "valu", "salu")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", default=[os.path.join(os.path.dirname(HERE), "loma-nerf_amd", "lib",
                                                             "libloma_nerf.so")])
    ap.add_argument("--kernel", default=K1)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    reps = {os.path.basename(p): report(p, a.kernel) for p in a.libs}
    if a.json:
        print(json.dumps(reps, indent=1))
        return
    names = sorted({n for r in reps.values() for n in r})
    for n in names:
        print(n)
        print("  " + "".ljust(26) + "".join(os.path.basename(p)[:24].rjust(26) for p in a.libs))
        for row in ROWS:
            print("  " + row.ljust(26) + "".join(str(reps[os.path.basename(p)].get(n, {}).get(row, "-")).rjust(26)
                                                for p in a.libs))


if __name__ == "__main__":
    main()
