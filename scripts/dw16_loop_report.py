#!/usr/bin/env python3
"""Static record of the dW kernel's half-block loops, from the built library's disassembly: for every
innermost loop of the kernel that holds MFMAs, the instruction counts by kind per iteration, the
scratch operations inside it (the FULL 2 x 4 loop of the hidden layers must have none) and how its
LDS waits sit relative to the reads they wait for.

  python scripts/dw16_loop_report.py [LIB.so | OBJ.o] [--kernel REGEX] [--near N] [--json]

A loop is the span between a backward branch's target and the branch; only the loops with the most
MFMAs per iteration are listed, which are the hidden layers' 2 x 4 loops (three half-blocks per
iteration), and of those the one with the fewest branches is marked as the FULL loop (the non-FULL
variant tests the layer's tile counts). An LDS wait "follows its read"
when the newest LDS read before it is at most N (default 12) instructions away: a wait that close
exposes the LDS round trip, whatever else is in flight.
Both selections are heuristics (the text output says so): the FULL loop is picked by branch count,
and a scratch operation is recognised as scratch_* or as a buffer_* ... offen access through the
scratch descriptor s[0:3] -- the kernel's own A-slab buffer loads use another descriptor today.
A report, not a test."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import isa_check  # noqa: E402


def kind_of(ins):
    mn = ins.mn
    if ins.mfma:
        return "mfma"
    if mn == "s_waitcnt":
        return "s_waitcnt"
    if mn == "s_barrier":
        return "s_barrier"
    if mn == "s_nop":
        return "s_nop"
    if mn.startswith(("s_branch", "s_cbranch")):
        return "branch"
    if "saveexec" in mn:
        return "saveexec"
    if mn.startswith("scratch_") or (mn.startswith("buffer_") and "offen" in ins.ops and "s[0:3]" in ins.ops):
        return "scratch"
    if mn.startswith("ds_read") and "_tr" in mn:
        return "ds_read_tr"
    if mn.startswith("ds_read"):
        return "ds_read"
    if mn.startswith("ds_write"):
        return "ds_write"
    if mn.startswith("ds_"):
        return "ds_other"
    if mn.startswith(("global_load", "buffer_load", "flat_load")):
        return "vmem_load"
    if mn.startswith(("global_", "buffer_", "flat_")):
        return "vmem_other"
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith("s_"):
        return "salu"
    return "other"


def loops_of(insts):
    """Innermost loops [(first, last)] as instruction index spans (backward branch target .. branch)."""
    idx = {ins.addr: i for i, ins in enumerate(insts)}
    spans = []
    for i, ins in enumerate(insts):
        if not ins.mn.startswith(("s_branch", "s_cbranch")):
            continue
        try:
            imm = int(ins.ops.split(",")[0].split()[0], 0)
        except (ValueError, IndexError):
            continue
        if imm >= 0x8000:
            imm -= 0x10000
        t = idx.get(ins.addr + ins.size + 4 * imm)
        if t is not None and t <= i:
            spans.append((t, i))
    return [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]


def loop_record(insts, first, last, near):
    counts = {}
    lds_waits = near_waits = 0
    since_read = None   # instructions since the newest LDS read
    for ins in insts[first:last + 1]:
        k = kind_of(ins)
        counts[k] = counts.get(k, 0) + 1
        if k in ("ds_read", "ds_read_tr"):
            since_read = 0
            continue
        if since_read is not None:
            since_read += 1
        if k == "s_waitcnt" and ins.wait is not None and ins.wait[1] < 15 and since_read is not None:
            lds_waits += 1
            near_waits += since_read <= near
    return {"first": f"{insts[first].addr:#x}", "instructions": last - first + 1, "counts": dict(sorted(counts.items())),
            "scratch_ops": counts.get("scratch", 0), "lds_waits": lds_waits, "lds_waits_near_read": near_waits}


def report(lib, kernel_re, near):
    out = {}
    for name, insts in isa_check.parse_kernels(isa_check.disassemble_all(lib), kernel_re).items():
        recs = [loop_record(insts, a, b, near) for a, b in loops_of(insts)]
        recs = [r for r in recs if r["counts"].get("mfma")]
        if recs:
            # the 2 x 4 loops: the most MFMAs per iteration (the smaller shapes' loops and the
            # exceptional-row pass have fewer)
            top = max(r["counts"]["mfma"] for r in recs)
            recs = [r for r in recs if r["counts"]["mfma"] == top]
            min(recs, key=lambda r: r["counts"].get("branch", 0))["full_2x4"] = True
        out[name] = recs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", nargs="?", default=os.path.join(os.path.dirname(HERE), "loma-nerf_amd", "lib", "libloma_nerf.so"))
    ap.add_argument("--kernel", default=r"dw16_kernel.*Li2E")
    ap.add_argument("--near", type=int, default=12)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    rep = report(a.lib, a.kernel, a.near)
    if a.json:
        print(json.dumps(rep, indent=1))
        return
    print("heuristics: the FULL loop is the one with the fewest branches among the loops with the most MFMAs; "
          "scratch operations are scratch_* and buffer_* ... offen on the descriptor s[0:3] (the kernel's own "
          "buffer loads use another descriptor today: check the listing if the scratch count is not 0)")
    for name, recs in rep.items():
        print(name)
        for r in recs:
            tag = "FULL 2x4 loop" if r.get("full_2x4") else "loop"
            print(f"  {tag} at {r['first']}: {r['instructions']} instructions, scratch ops {r['scratch_ops']}, "
                  f"LDS waits {r['lds_waits']} ({r['lds_waits_near_read']} within {a.near} of the newest read)")
            print("    " + " ".join(f"{k}={v}" for k, v in r["counts"].items()))


if __name__ == "__main__":
    main()
