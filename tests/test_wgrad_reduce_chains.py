"""The scalar chain in front of the first vector-memory instruction of the weight-gradient
and reduction kernels (tools/load_chains.py --args) on the built library: a pin against the
compiler quietly taking the kernel arguments in several dependent trips again, not a
performance claim.

profiles/wgrad_reduce_args_isa.txt records the scalar-load waits for the parent tree and for
this one.  The built library must not exceed this tree's counts, and this tree's counts must
be below the parent's.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import load_chains  # noqa: E402

MULTI = ("wgrad_multi_kernel<0>", "wgrad_multi_kernel<1>")
REDUCE = ("reduce_kernel<0, 0>", "reduce_kernel<0, 1>", "reduce_kernel<1, 0>", "reduce_kernel<1, 1>")


def recorded(section):
    """{kernel: scalar-load waits before the first vector-memory instruction} of one section."""
    text = open(os.path.join(ROOT, "profiles", "wgrad_reduce_args_isa.txt")).read()
    body = text.split(f"== {section}")[1].split("\n== ")[0]
    out = {}
    for line in body.splitlines():
        m = re.match(r"(\w+(?:<[^>]*>)?)\s+(\d+)\s+(\d+)\s+(\d+)\s+\|", line)
        if m:
            out[m.group(1)] = int(m.group(2))
    return out


@pytest.fixture(scope="module")
def rows(lib_built):
    return load_chains.report_args(load_chains.disassemble(lib_built), r"^(wgrad_multi_kernel|reduce_kernel)")


def test_finds_the_shipped_instantiations(rows):
    assert sorted(rows) == sorted(MULTI + REDUCE)
    for r in rows.values():
        assert r["arg_loads"] >= r["arg_waits"] >= 1 and r["insts_to_vmem"] > r["arg_loads"]


def test_argument_waits_do_not_grow(rows):
    new = recorded("new tree")
    assert set(MULTI + REDUCE) <= set(new)
    for k in MULTI + REDUCE:
        assert rows[k]["arg_waits"] <= new[k], (k, rows[k], new[k])


def test_new_tree_is_below_the_parent():
    new, parent = recorded("new tree"), recorded("parent")
    for k in MULTI:     # the parent has one kernel for both grids
        assert new[k] < parent["wgrad_multi_kernel"], (k, new[k], parent["wgrad_multi_kernel"])
    for k in REDUCE:
        assert new[k] < parent[k], (k, new[k], parent[k])
    # the block-index grid: one trip to the kernel arguments before the first LDS-DMA
    assert new["wgrad_multi_kernel<1>"] == 1


def test_argument_waits_on_a_synthetic_stream():
    insts = ["s_load_dwordx16 s[8:23], s[0:1], 0x0", "s_load_dwordx2 s[2:3], s[0:1], 0x40",
             "s_waitcnt lgkmcnt(0)",                      # one trip for two loads
             "s_waitcnt lgkmcnt(0)",                      # no scalar load since: no new trip
             "ds_write_b32 v1, v2", "s_waitcnt lgkmcnt(0)",   # an LDS wait is not an argument trip
             "v_writelane_b32 v62, s4, 0",
             "s_buffer_load_dword s4, s[8:11], 0x0", "s_waitcnt vmcnt(0) lgkmcnt(0)",
             "s_load_dword s5, s[0:1], 0x4", "s_waitcnt vmcnt(0)",      # not an lgkmcnt wait
             "global_load_lds_dwordx4 v[4:5], off",       # the first vector-memory instruction
             "s_load_dword s6, s[0:1], 0x8", "s_waitcnt lgkmcnt(0)", "v_writelane_b32 v62, s6, 1",
             "global_store_dword v[0:1], v2, off"]
    r = load_chains.arg_waits(insts)
    assert (r["arg_waits"], r["arg_loads"], r["insts_to_vmem"], r["writelanes"]) == (2, 4, 11, 2)
    # a store or an atomic ends the front as a load does; without any, the whole stream counts
    assert load_chains.arg_waits(insts[:3] + ["global_store_dword v[0:1], v2, off"] + insts[7:9])["arg_waits"] == 1
    assert load_chains.arg_waits(insts[:3] + ["global_atomic_add_f32 v0, v1, s[2:3]"] + insts[7:9])["arg_waits"] == 1
    assert load_chains.arg_waits(insts[:11])["arg_waits"] == 2
    assert load_chains.short_name("_ZN3snd12_GLOBAL__N_118wgrad_multi_kernelILb1EEEvNS0_11WgMultiPackE") == \
        "wgrad_multi_kernel<1>"
    regs = load_chains.registers("\t.amdhsa_kernel _Zk\n\t\t.amdhsa_next_free_vgpr 63\n\t\t.amdhsa_next_free_sgpr 72\n")
    assert regs == {"_Zk": {"v": 63, "s": 72}}
