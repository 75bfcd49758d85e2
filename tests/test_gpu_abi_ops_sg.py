"""snd_sg_prep, snd_sg_workspace, snd_sg_layer_fwd and snd_sg_layer_bwd at the C ABI on the
guarded operands of tests/abi_ops_sg.py: raw pointers into NaN-patterned guard bands, a
workspace of exactly snd_sg_workspace bytes, strided x / dx, the split-K weight gradients at
R = 4105 and 8225.  The three calls of a case run on one workspace (the backward needs the
forward's), then ``sg_verify`` checks every output against the float64 reference and every
guard.  Ratios are printed as "ABI_RATIO <op> <case> <output> <ratio>" (DESIGN.md §3).
"""
import ctypes

import numpy as np
import pytest
import torch

import abi_ops_sg as S
from test_gpu_abi_ops import ERR_ARG, Device, ids, lib, ok, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def graph(d, c, _lib, n_rows=None):
    return _lib.SGGraph(d.p("rowptr"), d.p("colidx"), c.R if n_rows is None else n_rows, c.N, d.p("edge_lr"),
                        d.p("edge_q"), d.p("edge_rev"), d.p("node_deg"), d.p("node_e"))


def layer_fwd(L, S_, g, d, c, ldx=None, bn_act=None, out="out"):
    return L.snd_sg_layer_fwd(ctypes.byref(g), d.p("x"), d.ld("x") if ldx is None else ldx, c.F, *c.hidden, d.p("params"),
                              c.bn_act if bn_act is None else bn_act, d.p("y"), d.p(out), d.p("ws"), S_)


@pytest.mark.parametrize("bn_act", [0, 1], ids=["plain", "bn_act"])
@pytest.mark.parametrize("case", S.SG_CASES, ids=ids(S.SG_CASES))
def test_sg_prep_layer_fwd_bwd(case, bn_act):
    L, S_, _lib = lib()
    c = S.sg_setup(case, bn_act)                                 # asserts the kink conditions on the CPU
    assert L.snd_sg_param_count(c.F, *c.hidden) == c.prm.size
    assert L.snd_sg_workspace(c.R, c.F, *c.hidden) == 4 * c.geo.floats == 4 * c.bufs["ws"].width
    if case[0] == "strided":                                     # base pointers 4 bytes past 16-byte alignment
        assert all(c.bufs[k].off % 4 == 1 for k in ("x", "dx", "params", "grads"))
    d = Device(c)
    g = graph(d, c, _lib)
    ok(L.snd_sg_prep(ctypes.byref(g), d.p("rel"), d.p("n_unmatched"), S_), "snd_sg_prep")
    ok(layer_fwd(L, S_, g, d, c), "snd_sg_layer_fwd")
    ok(L.snd_sg_layer_bwd(ctypes.byref(g), d.p("x"), d.ld("x"), c.F, *c.hidden, d.p("params"), bn_act, d.p("y"),
                          d.p("dout"), d.p("dx"), d.ld("dx", c.F), d.p("grads"), d.p("ws"), S_), "snd_sg_layer_bwd")
    report("sg_layer", case[0] + ("_bn_act" if bn_act else ""), S.sg_verify(c, d.back()))


# ---------------------------------------------------------------- error returns
def rejected(rc, d, entry):
    """SND_ERR_ARG, a message naming the entry point, and every buffer as it was."""
    _, _, _lib = lib()
    assert rc == ERR_ARG, rc
    assert entry in _lib.last_error(), _lib.last_error()
    after = d.back()
    for k, b in d.c.bufs.items():
        assert np.array_equal(after[k].view(np.uint8), b.arr.view(np.uint8)), f"{k} changed by a rejected call"


def test_sg_layer_fwd_rejects_a_short_ldx():
    L, S_, _lib = lib()
    c = S.sg_setup(S.sg_case("strided"), 1)
    d = Device(c)
    rejected(layer_fwd(L, S_, graph(d, c, _lib), d, c, ldx=c.F - 1), d, "snd_sg_layer_fwd")


def test_sg_layer_fwd_rejects_bn_act_without_out():
    L, S_, _lib = lib()
    c = S.sg_setup(S.sg_case("strided"), 1)
    d = Device(c)
    rejected(layer_fwd(L, S_, graph(d, c, _lib), d, c, bn_act=1, out="no such buffer"), d, "snd_sg_layer_fwd")


def test_sg_prep_rejects_rows_not_a_multiple_of_the_graph():
    L, S_, _lib = lib()
    c = S.sg_setup(S.sg_case("strided"), 0)                      # 60 rows of 6 per graph; claim 59
    d = Device(c)
    g = graph(d, c, _lib, n_rows=c.R - 1)
    rejected(L.snd_sg_prep(ctypes.byref(g), d.p("rel"), d.p("n_unmatched"), S_), d, "snd_sg_prep")
