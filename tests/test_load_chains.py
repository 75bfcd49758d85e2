"""tools/load_chains.py on the built library: a pin against silent regressions of the
load-then-wait kind, not a performance claim.

The compiler decides where a load is waited for; a harmless-looking edit (a select on a
loaded value, a load inside a per-element branch) can put a wait behind every single load
again.  profiles/load_chains_isa.txt records, for the three shipped instantiations of the
C2 step's chain kernels, the number of s_waitcnt vmcnt before the first barrier that follow
one or two loads -- for the parent tree and for this one.  The built library must not
exceed this tree's recorded counts.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import load_chains  # noqa: E402

KERNELS = ("enc_front_kernel<2>", "head_fwd_kernel<64, 2, 4>", "head_bwd_kernel<128, 1, 2, 3>")


def recorded(section):
    """{kernel: short waits before the first barrier} of one section of the profile."""
    text = open(os.path.join(ROOT, "profiles", "load_chains_isa.txt")).read()
    body = text.split(f"== {section}")[1].split("\n== ")[0]
    out = {}
    for line in body.splitlines():
        m = re.match(r"(\S+<[^>]*>)\s+(\d+)\s+(\d+)\s+(\d+)\s+\|", line)
        if m:
            out[m.group(1)] = int(m.group(3))
    return out


@pytest.fixture(scope="module")
def rows(lib_built):
    return load_chains.report(load_chains.disassemble(lib_built), load_chains.DEFAULT)


def test_finds_the_shipped_instantiations(rows):
    assert sorted(rows) == sorted(KERNELS)
    for k in KERNELS:
        r = rows[k]
        assert r["barriers"] >= 2 and r["loads_pre"] > 0 and r["waits_pre"] >= r["short_pre"]


def test_short_waits_before_the_first_barrier_do_not_grow(rows):
    new, parent = recorded("new tree"), recorded("parent")
    assert set(KERNELS) <= set(new) and set(KERNELS) <= set(parent)
    for k in KERNELS:
        assert rows[k]["short_pre"] <= new[k], (k, rows[k], new[k], "parent", parent[k])


def test_counts_on_a_synthetic_stream():
    insts = ["global_load_dword v1, v[2:3], off", "s_waitcnt vmcnt(0)",
             "global_load_dword v1, v[2:3], off", "buffer_load_dwordx4 v[4:7], v1, s[0:3], 0 offen",
             "global_load_lds_dwordx4 v[2:3], off", "s_waitcnt vmcnt(1)", "s_waitcnt lgkmcnt(0)",
             "s_barrier", "global_load_dword v1, v[2:3], off", "s_waitcnt vmcnt(0) lgkmcnt(0)"]
    r = load_chains.chains(insts)
    assert (r["waits_pre"], r["short_pre"], r["loads_pre"]) == (2, 1, 4)
    assert (r["waits"], r["short"], r["loads"], r["barriers"]) == (3, 2, 5, 1)
    # a second wait on the same group of loads is no new trip
    assert load_chains.chains(insts[2:5] + ["s_waitcnt vmcnt(2)", "s_waitcnt vmcnt(0)"])["short"] == 0
    assert load_chains.chains(insts[:1] + ["s_waitcnt vmcnt(0)", "s_waitcnt vmcnt(0)"])["short"] == 1
    assert load_chains.short_name("_ZN3snd12_GLOBAL__N_115head_fwd_kernelILi64ELi2ELi4EEEvNS_11HeadFwdArgsE") == \
        "head_fwd_kernel<64, 2, 4>"
