"""snd_graph_stats (graph statistics of a CSR and coordinates) on the GPU, through the raw
entry point on the guarded buffers of tests/abi_ops.py: every operand, every output and the
workspace sits between NaN-pattern guards, and outputs start at the pattern, so a store
outside an output or a missed store shows.

Everything is compared exactly with tests/graph_stats_ref.py: deg, tri2, the degree and
clustering histograms and the totals are integers; the edge-length histogram is exact under
the margin rule (no edge of a case lies within 2^-21 |v| of a bin edge; asserted before any
launch, graph_stats_ref.case_coords).
"""
import numpy as np
import pytest
import torch

import abi_ops as A
import graph_stats_ref as G

pytestmark = pytest.mark.gpu

I64_PAT = np.uint64(A.PATTERN["f64"][2]).astype(np.int64)       # int64 outputs ride in 8-byte "f64" buffers
I32_PAT = np.int32(A.PATTERN["i32"][2])
ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def run_raw(c, sd=2, want_deg=True, want_tri2=True, accumulate=0, start=None, expect_rc=0, override=None):
    """One call on fresh guarded buffers.  ``start``: (hist, totals) int64 arrays the outputs
    hold before the call (default: the guard pattern).  ``override``: raw argument values that
    replace the regular ones (rejected calls).  Returns the outputs after the call, with every
    guard, padding element and input checked."""
    from snd_vae_amd import _lib
    L = _lib.lib()
    R = c.B * c.n
    bufs = {"rowptr": A.guarded(1, R + 1, None, "i32", 0, c.rp, "rowptr"),
            "colidx": A.guarded(1, len(c.ci), None, "i32", 0, c.ci, "colidx"),
            "deg": A.guarded(1, R, None, "i32", 0, None, "deg"),
            "tri2": A.guarded(1, R, None, "i32", 0, None, "tri2"),
            "hist": A.guarded(1, c.B * 3 * G.BINS, None, "f64", 0, None, "hist"),
            "totals": A.guarded(1, c.B * 4, None, "f64", 0, None, "totals")}
    scale = 0.0
    if sd is not None:
        x, scale = G.case_coords(c.name, sd)
        bufs["coords"] = A.guarded(R, sd, sd + 3, "f32", 1, x, "coords")      # base 4 bytes off 16
    if start is not None:
        bufs["hist"].block().view(np.int64)[...] = start[0].reshape(1, -1)
        bufs["totals"].block().view(np.int64)[...] = start[1].reshape(1, -1)
    wsb = L.snd_graph_stats_workspace(c.B, c.n)
    bufs["ws"] = A.guarded(1, max(wsb // 4 + 1, 4), None, "f32", 0, None, "workspace")
    dev = {k: torch.from_numpy(g.arr).cuda() for k, g in bufs.items()}
    ptr = {k: dev[k].data_ptr() + g.off * g.arr.itemsize for k, g in bufs.items()}
    args = dict(rowptr=ptr["rowptr"], colidx=ptr["colidx"], n_graphs=c.B, n=c.n, coords=ptr.get("coords"),
                ldc=0 if sd is None else sd + 3, sd=0 if sd is None else sd, len_scale=float(scale),
                deg=ptr["deg"] if want_deg else None, tri2=ptr["tri2"] if want_tri2 else None,
                hist=ptr["hist"], totals=ptr["totals"], accumulate=accumulate, workspace=ptr["ws"],
                workspace_bytes=wsb)
    args.update(override or {})
    rc = L.snd_graph_stats(*args.values(), _lib.stream_ptr())
    assert rc == expect_rc, (rc, _lib.last_error())
    err = _lib.last_error() if rc else ""
    torch.cuda.synchronize()
    after = {k: t.cpu().numpy() for k, t in dev.items()}
    for k, g in bufs.items():
        g.check_untouched(after[k])
    for k in ("rowptr", "colidx", "coords", "ws"):                           # inputs bitwise intact
        if k in bufs:
            assert np.array_equal(after[k].view(np.uint32), bufs[k].arr.view(np.uint32)), k
    i64 = lambda k: np.ascontiguousarray(bufs[k].block(after[k])).view(np.int64).ravel()
    out = {"deg": bufs["deg"].block(after["deg"]).ravel(), "tri2": bufs["tri2"].block(after["tri2"]).ravel(),
           "hist": i64("hist").reshape(c.B, 3, G.BINS), "totals": i64("totals").reshape(c.B, 4), "err": err,
           "raw": {k: after[k] for k in ("deg", "tri2", "hist", "totals")}}
    return out


def check(c, out, sd, want_deg=True, want_tri2=True, what=""):
    x, scale = G.case_coords(c.name, sd) if sd is not None else (None, None)
    ref = G.ref_stats(c.rp, c.ci, c.B, c.n, x, scale)
    got = {"hist": out["hist"], "totals": out["totals"],
           "deg": out["deg"] if want_deg else None, "tri2": out["tri2"] if want_tri2 else None}
    G.assert_stats_equal(got, ref, c.n, f"{c.name} sd={sd} {what}")
    if not want_deg:
        assert (out["deg"] == I32_PAT).all()
    if not want_tri2:
        assert (out["tri2"] == I32_PAT).all()
    if sd is None:
        assert not out["hist"][:, 2].any()
    return ref


@pytest.mark.parametrize("name", G.CASES)
def test_cases_exact(name):
    """Every case at sd = 1, 2, 3 (ldc = sd + 3, base 4 bytes off 16-byte alignment) and with
    coords = NULL; two runs bitwise equal."""
    c = G.build_case(name)
    for sd in (1, 2, 3, None):
        out = run_raw(c, sd)
        ref = check(c, out, sd)
        print(f"GSTATS {name} sd={sd} sum_deg {int(ref['totals'][:, 0].sum())} sum_tri2 "
              f"{int(ref['totals'][:, 1].sum())} max_deg {int(ref['deg'].max())}")
    again = run_raw(c, 2)
    first = run_raw(c, 2)
    for k, v in first["raw"].items():
        assert np.array_equal(v.view(np.uint8), again["raw"][k].view(np.uint8)), (name, k)


def test_cases_hold_the_conditions():
    """On the CPU: the cases hold what they are there for."""
    ref = {n: G.ref_stats(G.build_case(n).rp, G.build_case(n).ci, G.build_case(n).B, G.build_case(n).n)
           for n in G.CASES}
    assert (ref["k40"]["tri2"] == 39 * 38).all() and ref["k40"]["hist"][0, 1, 255] == 40
    assert ref["star200"]["deg"][0] == 199 and ref["star200"]["hist"][0, 1, 0] == 200
    assert ref["deg300"]["deg"].max() == 299 and ref["deg300"]["hist"][1, 0, 255] == 1
    assert not ref["empty_middle"]["totals"][1].any() and ref["empty_middle"]["totals"][[0, 2], 0].all()
    assert len(G.build_case("b1n1").ci) == 1 and not ref["b1n1"]["totals"].any()
    big = G.build_case("b2n2049")
    assert 4.0 < ref["b2n2049"]["deg"].mean() < 8.0 and ref["b2n2049"]["tri2"].any()
    assert (big.ci[:big.rp[-1]] % 2049 >= 2048).any()                     # the mask's last word
    for n in ("b3n33", "b2n70", "b2n2049", "deg300"):                         # injected entries
        c = G.build_case(n)
        rows = np.repeat(np.arange(c.B * c.n), np.diff(c.rp))
        ci = c.ci[:c.rp[-1]]
        assert (ci == rows).any() and (ci // c.n != rows // c.n).any(), n
        srt = all(np.all(np.diff(ci[c.rp[i]:c.rp[i + 1]]) > 0) for i in range(c.B * c.n))
        assert not srt, n                                                     # shuffled within rows


@pytest.mark.parametrize("want_deg,want_tri2", [(False, True), (True, False), (False, False)])
def test_null_per_node_outputs(want_deg, want_tri2):
    c = G.build_case("b2n70")
    out = run_raw(c, 2, want_deg, want_tri2)
    check(c, out, 2, want_deg, want_tri2)


def test_accumulate_adds_two_batches():
    """accumulate = 1 over two different batches of one shape is the sum of the two; with
    coords = NULL it leaves the edge-length row as it was."""
    a, b = G.build_case("b3n33"), G.build_case("empty_middle")
    ra = check(a, run_raw(a, 3), 3)
    xb, sb = G.case_coords(b.name, 3)
    rb = G.ref_stats(b.rp, b.ci, b.B, b.n, xb, sb)
    out = run_raw(b, 3, accumulate=1, start=(ra["hist"], ra["totals"]))
    assert np.array_equal(out["hist"], ra["hist"] + rb["hist"])
    assert np.array_equal(out["totals"], ra["totals"] + rb["totals"])
    assert np.array_equal(out["deg"], rb["deg"]) and np.array_equal(out["tri2"], rb["tri2"])
    out = run_raw(b, None, accumulate=1, start=(ra["hist"], ra["totals"]))
    want = ra["hist"] + rb["hist"]
    want[:, 2] = ra["hist"][:, 2]
    assert np.array_equal(out["hist"], want)
    assert np.array_equal(out["totals"], ra["totals"] + rb["totals"])


def test_rejected_calls_touch_nothing():
    """Every SND_ERR_ARG call returns the code with a message naming the entry point, and all
    buffers (outputs included: they keep the guard pattern) are bitwise intact."""
    from snd_vae_amd import _lib
    c = G.build_case("b2n70")
    nan, inf = float("nan"), float("inf")
    bad = [dict(n_graphs=0), dict(n=0), dict(n=32769), dict(sd=0), dict(sd=4), dict(ldc=1),
           dict(len_scale=nan), dict(len_scale=-1.0), dict(len_scale=inf), dict(rowptr=None),
           dict(hist=None), dict(totals=None)]
    wsb = _lib.lib().snd_graph_stats_workspace(c.B, c.n)
    if wsb:                                  # every partial sum lives in LDS today: no workspace
        bad.append(dict(workspace_bytes=wsb - 1))
    for kw in bad:
        out = run_raw(c, 2, expect_rc=ERR_ARG, override=kw)
        assert "snd_graph_stats" in out["err"], (kw, out["err"])
        assert (out["deg"] == I32_PAT).all() and (out["tri2"] == I32_PAT).all(), kw
        assert (out["hist"] == I64_PAT).all() and (out["totals"] == I64_PAT).all(), kw
    # coords = NULL: sd, ldc and len_scale are not looked at
    check(c, run_raw(c, None, override=dict(sd=9, ldc=-3, len_scale=nan)), None)
    check(c, run_raw(c, 2), 2)                # and the regular call is accepted


def test_layers_graph_stats():
    """The torch-level op: fresh and given buffers, accumulate, per_node, contiguous coords."""
    from snd_vae_amd import layers
    from snd_vae_amd.metrics import GraphStats
    c = G.build_case("b2n70")
    x, scale = G.case_coords(c.name, 2)
    max_len = float(np.sqrt(2.0))
    assert np.float32(256.0 / max_len) == scale
    ref = G.ref_stats(c.rp, c.ci, c.B, c.n, x, scale)
    rp, ci, xt = (torch.from_numpy(np.array(a)).cuda() for a in (c.rp, c.ci, x))
    hist, totals, deg, tri2 = layers.graph_stats(rp, ci, c.B, c.n, xt, max_len, per_node=True)
    got = {"hist": hist.cpu().numpy(), "totals": totals.cpu().numpy(), "deg": deg.cpu().numpy(),
           "tri2": tri2.cpu().numpy()}
    G.assert_stats_equal(got, ref, c.n, "layers")
    h2, t2 = layers.graph_stats(rp, ci, c.B, c.n, xt, max_len, hist=hist, totals=totals, accumulate=True)
    assert h2 is hist and np.array_equal(hist.cpu().numpy(), 2 * ref["hist"])
    assert np.array_equal(totals.cpu().numpy(), 2 * ref["totals"])
    layers.graph_stats(rp, ci, c.B, c.n, hist=hist, totals=totals)           # cleared, no lengths
    assert np.array_equal(hist.cpu().numpy()[:, :2], ref["hist"][:, :2]) and not hist[:, 2].any()
    gs = GraphStats(*layers.graph_stats(rp, ci, c.B, c.n, xt, max_len), c.n, max_len)
    assert gs == GraphStats(ref["hist"], ref["totals"], c.n, max_len)
    assert gs.n_edges == int(ref["totals"][:, 3].sum())
    with pytest.raises(ValueError, match="max_len"):
        layers.graph_stats(rp, ci, c.B, c.n, xt)
    with pytest.raises(ValueError, match="max_len"):
        layers.graph_stats(rp, ci, c.B, c.n, max_len=1.0)
    with pytest.raises(ValueError, match="coords"):
        layers.graph_stats(rp, ci, c.B, c.n, xt[:-1], max_len)
    with pytest.raises(ValueError, match="accumulate"):
        layers.graph_stats(rp, ci, c.B, c.n, accumulate=True)
    with pytest.raises(ValueError, match="hist"):
        layers.graph_stats(rp, ci, c.B, c.n, hist=hist[:1], totals=totals)
