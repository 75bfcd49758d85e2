"""``snd_e2e_decode`` (ABI 22) at the C ABI on the guarded operands of
tests/disent_infer_ref.py: z with a leading dimension, every weight, a NaN-patterned margin,
a pattern-filled adjacency between guard bytes and a workspace of exactly the queried size.

Per case: one call, then the margin against the float64 reference within its bar (the
derived rule capped by the fp32 conditioning idiom, ``margin_bar``), the adjacency exact (the
setup redraws operands until every off-diagonal |margin| is over the bar, and holds both
classes), every guard intact; margin = NULL gives the same adjacency; a second run is
bitwise equal.  ``disent.structure_decode`` then agrees with the ``correct`` count of the
training route ``disent.structure_decoder`` on the same operands, and one call captured in a
HIP graph replays to the eager result.  Ratios are printed as
"ABI_RATIO e2e_decode <case> margin <ratio>" (DESIGN.md §3).
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import disent_infer_ref as IR
from abi_ops import vec
from test_gpu_abi_ops import Device, ids, lib, ok, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


_SETUPS = {}


def setup(case):
    """One float64 reference per case, shared by the tests of this file."""
    if case[0] not in _SETUPS:
        _SETUPS[case[0]] = IR.decode_setup(case)
    return _SETUPS[case[0]]


def run(L, S, _lib, c, d, adj, need, margin=True):
    n = len(c.layers)
    arr = (_lib.E2ELayer * n)(*[_lib.E2ELayer(d.p(f"l{i}_gamma"), d.p(f"l{i}_beta"), d.p(f"l{i}_w"), d.p(f"l{i}_b"),
                                              int(c.hidden[i])) for i in range(n)])
    return L.snd_e2e_decode(d.p("z"), c.ldz, c.B, c.N, c.D, arr, n, d.p("head_gamma"), d.p("head_beta"),
                            d.p("head_w"), d.p("head_b"), adj.data_ptr() + c.adj_off, d.p("margin") if margin else None,
                            d.p("ws"), need, S)


@pytest.mark.parametrize("case", IR.DECODE_CASES, ids=ids(IR.DECODE_CASES))
def test_e2e_decode(case):
    L, S, _lib = lib()
    c = setup(case)
    couts = (ctypes.c_int * len(c.hidden))(*c.hidden)
    need = L.snd_e2e_decode_workspace(c.B, c.N, c.D, couts, len(c.hidden))
    assert need > 0 and need % 4 == 0
    if c.N > 1:
        assert need <= IR.workspace_limit(c.B, c.N, c.D, c.hidden)
    c.bufs["ws"] = vec(need // 4, offset=c.off, name="ws")          # exactly the queried size
    d = Device(c)
    adj = torch.from_numpy(c.adj0).cuda()
    ok(run(L, S, _lib, c, d, adj, need), "snd_e2e_decode")
    after, adj1 = d.back(), adj.cpu().numpy()                       # ws: any value inside, its guards checked
    report("e2e_decode", case[0], IR.decode_verify(c, after, adj1))
    # a second run: bitwise equal
    ok(run(L, S, _lib, c, d, adj, need), "snd_e2e_decode")
    again, adj2 = d.back(), adj.cpu().numpy()
    assert np.array_equal(again["margin"].view(np.uint32), after["margin"].view(np.uint32)), "margin differs between runs"
    assert np.array_equal(adj2, adj1), "adj differs between runs"
    # margin = NULL: the same adjacency, the margin buffer untouched
    d2 = Device(c)
    adj3 = torch.from_numpy(c.adj0).cuda()
    ok(run(L, S, _lib, c, d2, adj3, need, margin=False), "snd_e2e_decode")
    after3 = d2.back()
    assert np.array_equal(adj3.cpu().numpy(), adj1), "adj differs without the margin"
    assert np.array_equal(after3["margin"].view(np.uint32), c.bufs["margin"].arr.view(np.uint32))


@pytest.mark.parametrize("case", IR.DECODE_CASES[:3], ids=ids(IR.DECODE_CASES[:3]))
def test_structure_decode_counts_what_the_training_route_counts(case):
    """The same operands through ``structure_decode`` and through ``structure_decoder`` (pair
    tensor, e2e, BN passes, head + CE): #(adj == A) equals the training route's ``correct``
    to within the number of entries under the bar, which the setup makes zero."""
    from snd_vae_amd import disent
    c = setup(case)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    layers = [{k: t(v).reshape(np.shape(v)) for k, v in l.items()} for l in c.layers]
    head = {k: t(v) for k, v in c.head.items()}
    rng = np.random.default_rng(3)
    A = (rng.random((c.B, c.N, c.N)) < 0.4).astype(np.float32)
    z = t(c.z)
    adj, margin = disent.structure_decode(z, layers, head, want_margin=True)
    assert adj.dtype == torch.uint8 and tuple(adj.shape) == (c.B, c.N, c.N)
    assert torch.equal(adj, disent.structure_decode(z, layers, head))
    correct = disent.structure_decoder(z, t(A), layers, head)[1]
    under = int((np.abs(c.ref.margin[c.offd]) <= c.ref.bound[c.offd]).sum())
    assert under == 0
    assert abs(float((adj.cpu().numpy() == A).sum()) - correct) <= under
    assert np.array_equal(adj.cpu().numpy(), (c.ref.margin > 0).astype(np.uint8))
    assert np.array_equal(adj.cpu().numpy(), (margin.cpu().numpy() > 0).astype(np.uint8))


def test_decode_rejects_a_short_workspace_and_a_short_ldz_on_device_operands():
    """The error returns leave every device buffer as it was."""
    from test_gpu_abi_ops_sg import rejected
    L, S, _lib = lib()
    c = copy.copy(setup(IR.DECODE_CASES[0]))
    c.bufs = dict(c.bufs)
    couts = (ctypes.c_int * len(c.hidden))(*c.hidden)
    need = L.snd_e2e_decode_workspace(c.B, c.N, c.D, couts, len(c.hidden))
    c.bufs["ws"] = vec(need // 4, name="ws")
    d = Device(c)
    adj = torch.from_numpy(c.adj0).cuda()
    rejected(run(L, S, _lib, c, d, adj, need - 4), d, "snd_e2e_decode")
    c.ldz = c.D - 1
    rejected(run(L, S, _lib, c, d, adj, need), d, "snd_e2e_decode")
    assert np.array_equal(adj.cpu().numpy(), c.adj0)


def test_decode_is_capturable_in_a_graph():
    """No host synchronisation and no allocation inside: one call captured in a HIP graph
    (a linear chain of kernels) replays to the eager result bit for bit."""
    L, _, _lib = lib()
    c = setup(IR.DECODE_CASES[0])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    z = t(c.z)
    layers = [{k: t(v) for k, v in l.items()} for l in c.layers]
    head = {k: t(v) for k, v in c.head.items()}
    n = len(layers)
    couts = (ctypes.c_int * n)(*c.hidden)
    arr = (_lib.E2ELayer * n)(*[_lib.E2ELayer(l["gamma"].data_ptr(), l["beta"].data_ptr(), l["w"].data_ptr(),
                                              l["b"].data_ptr(), int(co)) for l, co in zip(layers, c.hidden)])
    need = L.snd_e2e_decode_workspace(c.B, c.N, c.D, couts, n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    adj = torch.zeros(c.B, c.N, c.N, dtype=torch.uint8, device="cuda")
    margin = torch.zeros(c.B, c.N, c.N, device="cuda")

    def call(stream):
        ok(L.snd_e2e_decode(z.data_ptr(), c.D, c.B, c.N, c.D, arr, n, head["gamma"].data_ptr(), head["beta"].data_ptr(),
                            head["w"].data_ptr(), head["b"].data_ptr(), adj.data_ptr(), margin.data_ptr(),
                            ws.data_ptr(), need, _lib.stream_ptr(stream)), "snd_e2e_decode")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        call(side)
        side.synchronize()
        eager = (adj.clone(), margin.clone())
        with torch.cuda.graph(g, stream=side):
            call(side)
    torch.cuda.current_stream().wait_stream(side)
    adj.zero_()
    margin.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(adj, eager[0]) and torch.equal(margin, eager[1])
    assert np.array_equal(adj.cpu().numpy(), (c.ref.margin > 0).astype(np.uint8))
