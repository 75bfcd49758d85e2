"""``snd_e2e_train`` (ABI 24) at the C ABI on guarded operands, as tests/test_gpu_e2e_decode.py
builds them: z and dz with a leading dimension, every weight and every gradient between
guard bands, a workspace of exactly the queried size.

Per case: CE within rel 1e-5 of the float64 oracle (autograd on the literal pair-tensor
model) and ``correct`` exact; dz, every layer block and the head block within 1e-4 of the
block's max-abs (the bars tests/test_gpu_disent.py::test_structure_decoder sets for the
direct engine); every guard untouched; a second call bitwise equal; a captured graph's
replay bitwise equal to the eager call.

A relu mask that flips under fp32 rounding changes a gradient by a whole term, so the
operands must sit off the kinks; asserted on the reference alone: no float64 BN
pre-activation of any layer or the head lies closer to zero than 10x the largest
|float32 literal - float64| of that stage, and likewise no off-diagonal |l1 - l0| (so
``correct`` is an exact count).  No exclusions.  The seeds below were picked on the CPU so
that this holds (every seed in 0..19 does for the small cases; 0, 14, 15 do for ``ref``).
Two cases beyond the issue's table reach the kernels' remaining shape-dependent paths: more
than 32 graphs (weight-gradient slabs of several graphs, a short last one) and a wide, large-N
shape (j chunks, channel chunks, 4-row tiles); they meet the same assertions.
"""
import ctypes

import numpy as np
import pytest
import torch

import e2e_train_ref as TR
from abi_ops import check_guards, guarded, vec
from oracle import ref_disent as RD
from test_gpu_abi_ops import Device, ids, lib, ok

pytestmark = pytest.mark.gpu

# (id, B, N, D, hidden, pointer offset in floats, extra ldz / lddz, seed, beta_far of e2e_train_ref.operands)
CASES = (
    ("n7", 2, 7, 3, (5, 4), 0, 0, 0, 0.0),
    ("n8_wide", 1, 8, 5, (33, 32), 0, 0, 0, 0.0),      # even N; a width past a 32-lane tile; the head at its limit
    ("one_layer", 2, 6, 4, (6,), 0, 0, 0, 0.0),        # layer 0 feeds the head: no general layer
    ("three", 2, 5, 2, (9, 7, 5), 0, 0, 0, 0.0),
    ("n1", 2, 1, 3, (4, 3), 0, 0, 0, 0.0),
    ("n2", 1, 2, 3, (4, 3), 0, 0, 0, 0.0),
    ("tail", 6, 5, 3, (5, 4), 0, 0, 0, 0.0),           # a graph-group tail of layer 0's 4-graph workgroups
    ("off1", 2, 7, 3, (5, 4), 1, 3, 0, 0.0),           # every pointer 4 bytes off 16-byte alignment, ldz = lddz = d + 3
    ("ref", 2, 25, 40, (50, 20), 0, 0, 0, 0.0),        # the synthetic2 widths
    # beyond the issue's table: the shape-dependent paths of the new kernels
    ("b33", 33, 3, 2, (3, 2), 0, 0, 0, 0.0),           # 17 weight-gradient slabs of 2 graphs, the last with 1
    # layer 1 (36 -> 260): the data gradient's channel chunks (260 > 92).  Layer 2 (260 -> 4): the weight
    # gradient's j chunks (47 < 48 rows staged) and a second block of (c, 4 o) tiles, the data gradient on
    # 4-row tiles.  Its 700 000 pre-activations cannot all miss zero by chance: whole channels on or off
    ("wide", 1, 48, 2, (36, 260, 4), 0, 0, 0, 1.0),
)
KEYS = ("gamma", "beta", "w", "b")


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


_SETUPS = {}


def setup(case):
    """Operands, guarded buffers and one float64 reference per case, shared by the tests."""
    if case[0] in _SETUPS:
        return _SETUPS[case[0]]
    name, B, N, D, hidden, off, ldx, seed, beta_far = case
    c = TR.operands(B, N, D, hidden, seed, beta_far)
    c.off, c.ldz = off, D + ldx
    for stage, (lo, err) in enumerate(TR.kink_margins(c)):
        assert lo > 10.0 * err, f"{name}: BN stage {stage} has a pre-activation {lo:.3e} within 10 x {err:.3e}"
    lo, err = TR.argmax_margin(c)
    assert lo > 10.0 * err, f"{name}: an argmax within 10 x {err:.3e} of a tie ({lo:.3e})"
    c.ref = RD.structure_decoder_grads(c.z, c.adj, c.layers, c.head)
    c.bufs = {"z": guarded(B * N, D, ld=c.ldz, offset=off, data=c.z, name="z"),
              "adj": vec(B * N * N, offset=off, data=c.adj, name="adj"),
              "dz": guarded(B * N, D, ld=c.ldz, offset=off, name="dz"),
              "out": vec(2, dtype="f64", offset=off, name="out")}
    for i, l in enumerate(c.layers):
        for k in KEYS:
            c.bufs[f"l{i}_{k}"] = vec(l[k].size, offset=off, data=l[k], name=f"l{i}_{k}")
            c.bufs[f"g{i}_{k}"] = vec(l[k].size, offset=off, name=f"g{i}_{k}")
    for k in KEYS:
        c.bufs[f"head_{k}"] = vec(c.head[k].size, offset=off, data=c.head[k], name=f"head_{k}")
        c.bufs[f"ghead_{k}"] = vec(c.head[k].size, offset=off, name=f"ghead_{k}")
    _SETUPS[case[0]] = c
    return c


def run(L, S, _lib, c, d, need):
    n = len(c.layers)
    arr = (_lib.E2ELayer * n)(*[_lib.E2ELayer(*[d.p(f"l{i}_{k}") for k in KEYS], int(c.hidden[i])) for i in range(n)])
    garr = (_lib.E2ELayerGrad * n)(*[_lib.E2ELayerGrad(*[d.p(f"g{i}_{k}") for k in KEYS]) for i in range(n)])
    return L.snd_e2e_train(d.p("z"), c.ldz, d.p("adj"), c.B, c.N, c.D, arr, n, d.p("head_gamma"), d.p("head_beta"),
                           d.p("head_w"), d.p("head_b"), d.p("dz"), c.ldz, garr, d.p("ghead_gamma"),
                           d.p("ghead_beta"), d.p("ghead_w"), d.p("ghead_b"), d.p("out"), d.p("ws"), need, S)


def outputs(c, after):
    """(out[2], dz, layer grads, head grads) of the device state ``after``."""
    v = lambda k: c.bufs[k].values(after[k])
    lg = [{k: v(f"g{i}_{k}").reshape(np.shape(l[k])) for k in KEYS} for i, l in enumerate(c.layers)]
    hg = {k: v(f"ghead_{k}").reshape(np.shape(c.head[k])) for k in KEYS}
    return c.bufs["out"].block(after["out"]).reshape(-1), v("dz").reshape(c.z.shape), lg, hg


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a if k != "ws")


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_e2e_train(case):
    L, S, _lib = lib()
    c = setup(case)
    couts = (ctypes.c_int * len(c.hidden))(*c.hidden)
    need = L.snd_e2e_train_workspace(c.B, c.N, c.D, couts, len(c.hidden))
    assert need > 0 and need % 4 == 0
    c.bufs["ws"] = vec(need // 4, offset=c.off, name="ws")          # exactly the queried size
    d = Device(c)
    ok(run(L, S, _lib, c, d, need), "snd_e2e_train")
    after = d.back()
    out, dz, lg, hg = outputs(c, after)
    rce, rcorrect, rdz, rlg, rhg = c.ref
    M = c.B * c.N * c.N
    errs = TR.block_errors((dz, lg, hg), (rdz, rlg, rhg))
    print(f"E2E_TRAIN {case[0]} ce_rel {abs(out[0] / M - rce) / abs(rce):.3e} correct {out[1]:.0f} ref {rcorrect:.0f} "
          + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert abs(out[0] / M - rce) <= 1e-5 * abs(rce)
    assert out[1] == rcorrect
    for k, e in errs.items():
        assert e < 1e-4, (k, e)
    check_guards(c, after)                                           # ws: any value inside, its guards checked
    # a second run: bitwise equal
    ok(run(L, S, _lib, c, d, need), "snd_e2e_train")
    assert same_bits(after, d.back()), "two runs differ"


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_train_is_capturable_in_a_graph(case):
    """No host synchronisation and no allocation inside: one call captured in a HIP graph (a
    linear chain of kernels) replays to the eager result bit for bit."""
    L, _, _lib = lib()
    c = setup(case)
    couts = (ctypes.c_int * len(c.hidden))(*c.hidden)
    need = L.snd_e2e_train_workspace(c.B, c.N, c.D, couts, len(c.hidden))
    c.bufs["ws"] = vec(need // 4, offset=c.off, name="ws")
    d = Device(c)
    fresh = {k: t.clone() for k, t in d.t.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        ok(run(L, _lib.stream_ptr(side), _lib, c, d, need), "snd_e2e_train")
        side.synchronize()
        eager = d.back()
        with torch.cuda.graph(g, stream=side):
            ok(run(L, _lib.stream_ptr(side), _lib, c, d, need), "snd_e2e_train")
    torch.cuda.current_stream().wait_stream(side)
    for k, t in d.t.items():                                         # the outputs back to their patterns
        t.copy_(fresh[k])
    g.replay()
    replayed = d.back()
    assert same_bits(eager, replayed), "the replay differs from the eager call"
    check_guards(c, replayed)
    assert TR.block_errors(outputs(c, replayed)[1:], c.ref[2:])["dz"] < 1e-4


def test_train_rejects_a_short_workspace_on_device_operands():
    """The error returns leave every device buffer as it was."""
    from test_gpu_abi_ops_sg import rejected
    L, S, _lib = lib()
    c = setup(CASES[0])
    couts = (ctypes.c_int * len(c.hidden))(*c.hidden)
    need = L.snd_e2e_train_workspace(c.B, c.N, c.D, couts, len(c.hidden))
    c.bufs["ws"] = vec(need // 4, name="ws")
    d = Device(c)
    rejected(run(L, S, _lib, c, d, need - 4), d, "snd_e2e_train")
