"""The dW kernel's hidden-layer loop, read back from the built library's disassembly (CPU only;
scripts/dw16_loop_report.py and scripts/isa_check.py do the reading).

hb_loop3<2, 2, 4, true, true> inside dw16_kernel<2> (cfg3 fp16x3 training: the FULL 2 x 4 loop, three
half-blocks per iteration) does its 72 MFMAs on 12 slab loads without touching scratch; its db sums
are plain f32 adds (no packed VALU instruction: a v_pk_add_f32 beside MFMAs costs more than the two
v_add_f32 it replaces), and the wave-uniform addresses of a step's loads advance by scalar adds (no
scalar multiply and no 64-bit shift is left in the loop). The kernel takes no more vector registers
and spills no more of them than the build before that change, whose figures are the record
tests/golden/dw16_loop_parent.json (`scripts/dw16_loop_report.py` and `scripts/kernel_resources.py`
on the parent commit's library; profiles/dw16_loop_parent.json is the same record)."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, "loma-nerf_amd", "lib", "libloma_nerf.so")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KERNEL = r"dw16_kernel.*Li2E"


@pytest.fixture(scope="module")
def built():
    """(the FULL 2 x 4 loop's instructions, its record, the kernel's resource figures)"""
    if not os.path.exists(LIB):
        pytest.skip("libloma_nerf.so not built (python -c 'import __graft_entry__ as g; g.build()')")
    import dw16_loop_report as rep
    import isa_check
    import kernel_resources
    ks = isa_check.parse_kernels(isa_check.disassemble_all(LIB), KERNEL)
    assert len(ks) == 1, list(ks)
    name, insts = next(iter(ks.items()))
    spans = rep.loops_of(insts)
    recs = [(rep.loop_record(insts, a, b, 12), a, b) for a, b in spans]
    top = max(r["counts"].get("mfma", 0) for r, _, _ in recs)
    # the report's own choice: of the loops with the most MFMAs the one with the fewest branches
    rec, a, b = min((x for x in recs if x[0]["counts"].get("mfma", 0) == top),
                    key=lambda x: x[0]["counts"].get("branch", 0))
    res = kernel_resources.resources(LIB, KERNEL)
    assert name in res, list(res)
    return insts[a:b + 1], rec, res[name]


@pytest.fixture(scope="module")
def parent():
    return json.load(open(os.path.join(HERE, "golden", "dw16_loop_parent.json")))


def test_same_matrix_work_and_slab_loads_per_iteration(built):
    _, rec, _ = built
    c = rec["counts"]
    assert c.get("mfma") == 72 and c.get("ds_read_tr") == 72 and c.get("vmem_load") == 12, c


def test_no_scratch_operation_in_the_loop(built):
    loop, rec, _ = built
    assert rec["scratch_ops"] == 0, rec
    assert not [i for i in loop if i.mn.startswith("scratch_")]


def test_no_packed_valu_in_the_loop(built):
    loop, _, _ = built
    bad = [f"{i.addr:#x} {i.mn} {i.ops.strip()}" for i in loop if i.mn.startswith("v_pk_")]
    assert not bad, "\n".join(bad)


def test_no_scalar_multiply_or_wide_shift_in_the_loop(built):
    loop, _, _ = built
    bad = [f"{i.addr:#x} {i.mn} {i.ops.strip()}" for i in loop if i.mn.startswith("s_mul_") or i.mn == "s_lshl_b64"]
    assert not bad, "\n".join(bad)


def test_no_more_registers_or_spills_than_the_parent(built, parent):
    _, _, res = built
    was = parent["resources"]
    assert res["vgpr_count"] <= was["vgpr_count"], (res, was)
    assert res["vgpr_spill_count"] <= was["vgpr_spill_count"], (res, was)
