"""tools/load_chains.py on the two shipped 128-row instantiations of the fused decoder
chains: a pin against silent regressions of the load-then-wait kind, not a performance claim.

Both kernels' time is one tile's dependent chain, so a vmcnt wait that follows one or two
loads is a memory round trip paid in full.  profiles/dec_tail_isa.txt records the short
waits over the whole kernel for the parent tree (13 and 16) and for this one; the built
library must not exceed this tree's counts, and those must be below the parent's.  Only
loads, waits and barriers are read.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import load_chains  # noqa: E402

KERNELS = ("dec_fwd_kernel<128, 16, 0>", "dec_bwd_kernel<128, 16, 0>")
PARENT = {"dec_fwd_kernel<128, 16, 0>": 13, "dec_bwd_kernel<128, 16, 0>": 16}


def recorded(section):
    """{kernel: short waits over the whole kernel} of one section of the profile."""
    text = open(os.path.join(ROOT, "profiles", "dec_tail_isa.txt")).read()
    body = text.split(f"== {section}")[1].split("\n== ")[0]
    out = {}
    for line in body.splitlines():
        m = re.match(r"(\S+<[^>]*>)\s+\d+\s+\d+\s+\d+\s+\|\s+\d+\s+(\d+)\s+\d+\s+\d+", line)
        if m:
            out[m.group(1)] = int(m.group(2))
    return out


@pytest.fixture(scope="module")
def rows(lib_built):
    pattern = "|".join(re.escape(k) for k in KERNELS)
    return load_chains.report(load_chains.disassemble(lib_built), pattern)


def test_finds_the_shipped_instantiations(rows):
    assert sorted(rows) == sorted(KERNELS)
    for k in KERNELS:
        assert rows[k]["barriers"] >= 6 and rows[k]["loads"] > 0 and rows[k]["waits"] >= rows[k]["short"]


def test_short_waits_do_not_grow(rows):
    new, parent = recorded("new tree"), recorded("parent")
    assert parent == PARENT
    for k in KERNELS:
        assert new[k] < parent[k], (k, new[k], parent[k])
        assert rows[k]["short"] <= new[k], (k, rows[k], new[k], "parent", parent[k])
