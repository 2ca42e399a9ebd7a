"""k1's and kr's LDS-DMA and slab-store addressing, read back from the built library's disassembly
(CPU only; scripts/k16_loop_report.py does the counting).

The product kernel k16_fwd_bwd_kernel<16, 2, 8, 1> (cfg3 fp16x3 training) and kr_fwd_kernel<16> take every
LDS-DMA piece and every nontemporal slab store from a scalar base (lnerf_wave_addr.h): no per-lane 64-bit
address is built for them, and no generic -> LDS pointer cast (its null test ends in an s_cselect) feeds M0.
The figures of the build before that change are the record tests/golden/k16_loop_report_parent.json
(`scripts/k16_loop_report.py PARENT.so --kernel ... --json` on the parent commit's library; DESIGN.md
section 3 quotes the same table)."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, "loma-nerf_amd", "lib", "libloma_nerf.so")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KERNELS = ("k1", "kr")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB):
        pytest.skip("libloma_nerf.so not built (python -c 'import __graft_entry__ as g; g.build()')")
    import isa_check
    import k16_loop_report as rep
    asm = isa_check.disassemble_all(LIB)
    meta = rep.kernel_meta(LIB)
    out = {}
    for key, rx in (("k1", rep.K1), ("kr", rep.KR)):
        ks = isa_check.parse_kernels(asm, rx)
        assert len(ks) == 1, (rx, list(ks))
        name, insts = next(iter(ks.items()))
        out[key] = (name, insts, rep.record(insts, meta.get(name)))
    return out


@pytest.fixture(scope="module")
def parent():
    import k16_loop_report as rep
    import re
    recs = json.load(open(os.path.join(HERE, "golden", "k16_loop_report_parent.json")))
    recs = next(iter(recs.values()))
    out = {}
    for key, rx in (("k1", rep.K1), ("kr", rep.KR)):
        (rec,) = [r for n, r in recs.items() if re.search(rx, n)]
        out[key] = rec
    return out


@pytest.mark.parametrize("k", KERNELS)
def test_no_spills_and_no_more_registers_than_the_parent(built, parent, k):
    name, _, rec = built[k]
    assert rec["vgprs"] is not None, f"no metadata for {name}"
    assert rec["vgpr_spills"] == 0 and rec["sgpr_spills"] == 0, rec
    assert rec["scratch_bytes"] <= parent[k]["scratch_bytes"], rec
    assert rec["vgprs"] <= parent[k]["vgprs"], (rec["vgprs"], parent[k]["vgprs"])


@pytest.mark.parametrize("k", KERNELS)
def test_every_lds_dma_and_slab_store_takes_a_scalar_base(built, k):
    import k16_loop_report as rep
    _, insts, rec = built[k]
    assert rec["lds_dma"] > 0
    if k == "k1":
        assert rec["slab_stores"] > 0
    bad = [f"{i.addr:#x} {i.mn} {i.ops.strip()}" for i in insts
           if (rep.is_lds_dma(i) or rep.is_slab_store(i)) and not rep.scalar_base(i)]
    assert not bad, "\n".join(bad[:10])
    # the same transfers as before: not one instruction more or fewer
    assert rec["lds_dma"] == rec["lds_dma_scalar_base"] and rec["slab_stores"] == rec["slab_stores_scalar_base"]


@pytest.mark.parametrize("k", KERNELS)
def test_same_transfers_as_the_parent(built, parent, k):
    rec = built[k][2]
    for what in ("lds_dma", "slab_stores", "mfma", "ds_read_b128"):
        assert rec[what] == parent[k][what], (what, rec[what], parent[k][what])


@pytest.mark.parametrize("k", KERNELS)
def test_no_m0_write_fed_by_a_cselect(built, k):
    import k16_loop_report as rep
    _, insts, _ = built[k]
    bad = [f"{i.addr:#x} {i.mn} {i.ops.strip()}" for i in rep.m0_fed_by_cselect(insts)]
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("k", KERNELS)
def test_vector_64bit_adds_fell_by_the_transfers(built, parent, k):
    """One 64-bit vector add per LDS-DMA piece and per slab store carried no information: the kernel's
    count is lower than the parent's by at least its LDS-DMA instructions plus its slab stores."""
    rec = built[k][2]
    drop = parent[k]["vector_add64"] - rec["vector_add64"]
    assert drop >= rec["lds_dma"] + rec["slab_stores"], (parent[k]["vector_add64"], rec["vector_add64"], rec["lds_dma"],
                                                         rec["slab_stores"])


@pytest.mark.parametrize("k", KERNELS)
def test_scalar_base_is_not_fresh_from_the_vector_unit(built, k):
    """The LDS-DMA sits in inline asm, where the compiler pads no hazard: a vector-memory instruction may
    read a scalar register a VALU instruction wrote (v_readfirstlane, v_readlane, v_cmp) only 5 wait states
    later. Looks back over the straight line before every LDS-DMA (a branch ends the search: its target's
    history is unknown, and the bases come out of scalar adds issued with the piece)."""
    import isa_check
    import k16_loop_report as rep
    _, insts, _ = built[k]
    bad = []
    for n, ins in enumerate(insts):
        if not rep.is_lds_dma(ins):
            continue
        ops = [o.strip().split()[0] for o in ins.ops.split(",")]
        base = set()
        for o in ops[1:]:
            base |= {r for r in isa_check.regs_of(o) if r[0] == "s"}
        states = 0
        for p in reversed(insts[max(0, n - 8):n]):
            if p.mn.startswith(("s_branch", "s_cbranch")) or states >= 5:
                break
            if p.valu and p.ops.strip():
                dst = isa_check.regs_of(p.ops.split(",")[0])
                if dst & base:
                    bad.append(f"{ins.addr:#x} {ins.mn} {ins.ops.strip()} <- {p.addr:#x} {p.mn} {p.ops.strip()}")
            states += p.states
    assert not bad, "\n".join(bad[:10])
