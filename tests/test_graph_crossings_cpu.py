"""snd_graph_crossings without a GPU: the NumPy reference (tests/graph_crossings_ref.py) against
closed forms and against exact rational arithmetic, metrics.CrossingStats, the ABI number, the
argument rules of the entry point on host pointers (none reaches a launch) and the kernels'
resource records.
"""
import ctypes
import math
import os
import re
from math import comb

import numpy as np
import pytest

import graph_crossings_ref as X
import graph_stats_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the reference itself
def _one(pairs, xy, n=25, extra=()):
    c = X.Case(f"one_{abs(hash((tuple(map(tuple, pairs)), xy.tobytes(), tuple(extra))))}", 1, n,
               *G.csr_from_pairs(pairs, 1, n, extra=extra), xy)
    return c, X.reference(c)


def test_closed_forms():
    forms = {nm: (pairs, xy, x) for nm, pairs, xy, x in X.closed_forms()}
    assert forms["k8_circle"][2] == comb(8, 4) == 70 and forms["k34_lines"][2] == 18
    for nm, (pairs, xy, x) in forms.items():
        _, w = _one(pairs, xy)
        assert w["counts"][0, 0] == len(pairs) and w["counts"][0, 1] == x, (nm, w["counts"][0].tolist())
    _, w = _one(*forms["grid5_diagonals"][:2])
    assert w["counts"][0, 0] == 72 and w["counts"][0, 1] == 16 and w["counts"][0, 2] == 32 and w["counts"][0, 6] == 1
    assert w["hist"][0, 2, 255] == 16 and w["hist"][0, 2].sum() == 16              # every angle pi / 2
    h1 = w["hist"][0, 1]
    assert np.nonzero(h1)[0].tolist() == [0, 64, 128, 192] and h1[[0, 64, 128, 192]].tolist() == [20, 16, 20, 16]
    assert X.band_share(w["dir_vals"][0], wrap=True) == 0.0
    _, w = _one(*forms["degenerate"][:2])
    assert w["counts"][0].tolist() == [6, 0, 0, 15, 0, 1, 0]                       # one zero-length edge
    assert w["hist"][0, 1].sum() == 5
    # K8: every edge's count by its chord length: a side crosses nothing, a diameter the most
    _, w = _one(*forms["k8_circle"][:2])
    assert w["counts"][0, 3] == comb(28, 2) - 8 * comb(7, 2) and w["counts"][0, 6] == 9
    assert w["hist"][0, 0, [0, 5, 8, 9]].tolist() == [8, 8, 8, 4]


def test_the_reference_equals_exact_rational_arithmetic():
    """Random edges between points of a 9 x 9 grid (coordinates k / 8, exact in fp32): collinear
    overlaps, T-junctions and touching ends are frequent there.  Conditions 2 and 3 in rationals."""
    rng = np.random.default_rng(8)
    n, total, degenerate = 25, 0, 0
    for trial in range(12):
        xy = (rng.integers(0, 9, (n, 2)) / 8.0).astype(np.float32)
        allp = np.asarray(X._complete(n))
        pairs = allp[rng.choice(len(allp), size=60, replace=False)]
        c, w = _one(pairs, xy)
        a, b, _, _, _ = X.mutual_edges(c.rp, c.ci, 1, n, 0)
        got = set(zip(*(v.tolist() for v in X.crossing_pairs(a, b, xy))))
        want = set()
        for i in range(len(a)):
            for j in range(i + 1, len(a)):
                if len({a[i], b[i], a[j], b[j]}) < 4:
                    continue
                if X.exact_cross(xy[a[i]], xy[b[i]], xy[a[j]], xy[b[j]]):
                    want.add((i, j))
                else:                                             # how many of the refusals are degenerate
                    o = X.orient(*xy[a[i]].astype(float), *xy[b[i]].astype(float), *xy[a[j]].astype(float))
                    degenerate += int(o == 0)
        assert got == want, (trial, sorted(got ^ want)[:5])
        assert w["counts"][0, 1] == len(want)
        total += len(want)
    assert total > 1000 and degenerate > 100


def test_ignored_entries_change_only_the_one_way_count():
    rng = np.random.default_rng(21)
    B, n = 3, 20
    xy = rng.random((B * n, 2)).astype(np.float32)
    pairs = X.rgg_pairs(xy, B, n, 0.5)
    clean = X.Case("ignored_clean", B, n, *G.csr_from_pairs(pairs, B, n), xy)
    dirty = X.Case("ignored_dirty", B, n, *G.csr_from_pairs(pairs, B, n, shuffle_seed=4,
                                                            extra=X._extras(rng, B, n, pairs)), xy)
    wc, wd = X.reference(clean), X.reference(dirty)
    assert (wc["counts"][:, 4] == 0).all() and (wd["counts"][:, 4] > 0).all()
    keep = [0, 1, 2, 3, 5, 6]
    assert np.array_equal(wc["counts"][:, keep], wd["counts"][:, keep]) and (wc["counts"][:, 1] > 0).all()
    assert np.array_equal(wc["hist"], wd["hist"]) and np.array_equal(wc["work"], wd["work"])


@pytest.mark.parametrize("name", ["r33", "tile_edges", "b70_mixed", "cap_middle"])
def test_sums_of_the_reference(name):
    c = X.build_case(name)
    w = X.reference(c, X.case_work_cap(name))
    for g in range(c.B):
        lo, hi = int(c.rp[g * c.n]), int(c.rp[(g + 1) * c.n])
        ce = w["cross_out"][lo:hi]
        if w["counts"][g, 0] < 0:
            assert (ce == -1).all() and not w["hist"][g].any() and (w["counts"][g] == -1).all()
            continue
        E, x = w["counts"][g, 0], w["counts"][g, 1]
        assert ce.sum() == 2 * x and w["hist"][g, 0].sum() == E and w["hist"][g, 2].sum() == x
        assert w["hist"][g, 1].sum() == E - w["counts"][g, 5] and w["work"][g] == E * (E - 1) // 2
        assert (ce > 0).sum() == w["counts"][g, 2] and (ce.max() if len(ce) else 0) == w["counts"][g, 6]
        assert 0 <= x <= w["counts"][g, 3] <= w["work"][g]
    assert (w["cross_out"][int(c.rp[-1]):] == -7).all()
    if name == "tile_edges":
        assert w["counts"][:, 0].tolist() == [X.TILE - 1, X.TILE, X.TILE + 1, 2 * X.TILE + 1]
    if name == "cap_middle":
        assert (w["counts"][:, 0] < 0).tolist() == [False, True, False]


def test_the_band_comparison_itself():
    """assert_hist_in_band accepts the exact histogram and a value moved across an edge inside
    the band, and refuses one moved from outside it."""
    rng = np.random.default_rng(2)
    vals = rng.random(4096) * 256.0
    share = X.band_share(vals, wrap=True)
    assert 0.0005 < share < 0.006                                  # about 2 * 2^-10 of a bin: 0.2 %
    h = np.bincount(np.floor(vals).astype(int), minlength=256)
    X.assert_hist_in_band(h, vals, "exact", wrap=True)
    near = np.concatenate([vals, [17.0 + X.DELTA / 2]])
    moved = np.bincount(np.floor(np.concatenate([vals, [16.99]])).astype(int), minlength=256)
    X.assert_hist_in_band(moved, near, "inside the band")
    far = np.concatenate([vals, [17.0 + 4 * X.DELTA]])
    with pytest.raises(AssertionError, match="edge 17"):
        X.assert_hist_in_band(moved, far, "outside the band")
    wrapped = np.bincount(np.floor(np.concatenate([vals, [255.99]])).astype(int), minlength=256)
    X.assert_hist_in_band(wrapped, np.concatenate([vals, [X.DELTA / 4]]), "across 0", wrap=True)


# ---------------------------------------------------------------- metrics.CrossingStats
def _stats(names):
    from snd_vae_amd.metrics import CrossingStats
    forms = {nm: (pairs, xy) for nm, pairs, xy, _ in X.closed_forms()}
    ws = [_one(*forms[nm])[1] for nm in names]
    return CrossingStats(np.concatenate([w["counts"] for w in ws]), np.concatenate([w["hist"] for w in ws]), 25)


def test_crossing_stats_arithmetic():
    from snd_vae_amd.metrics import CROSSING_KINDS, CrossingStats, orientation_entropy, orientation_order
    grid = _stats(["grid5"])
    s = grid.summary()
    assert abs(s["orientation_entropy"] - math.log(2.0)) < 1e-14 and abs(s["orientation_order"] - 1.0) < 1e-14
    assert s["planar"] == 1.0 and s["crossings_per_edge"] == 0.0 and s["crossing_ratio"] == 0.0
    assert math.isnan(s["mean_cross_angle"]) and s["n_skipped"] == 0 and s["one_way"] == 0
    uniform = np.ones(256)
    assert abs(orientation_entropy(uniform) - math.log(32.0)) < 1e-14
    assert abs(orientation_order(orientation_entropy(uniform))) < 1e-14
    assert "Boeing" in orientation_order.__doc__ and "Boeing" in orientation_entropy.__doc__
    h = np.zeros(256)
    h[[252, 3]] = 1                                               # both within 4 fine bins of direction 0
    assert orientation_entropy(h) == 0.0

    both = _stats(["k8_circle", "grid5_diagonals", "grid5"])
    s = both.summary()
    E, x = 28 + 72 + 40, 70 + 16
    assert s["planar"] == 1 / 3 and s["crossings_per_edge"] == x / E and s["crossed_share"] == (20 + 32) / E
    ind = both.counts[:, 3].sum()
    assert s["crossing_ratio"] == x / ind
    pg = both.per_graph()
    assert pg["X"].tolist() == [70, 16, 0] and pg["planar"].tolist() == [0.0, 0.0, 1.0]
    assert abs(pg["mean_cross_angle"][1] - 255.5 * math.pi / 512) < 1e-15 and math.isnan(pg["mean_cross_angle"][2])
    p, q = 20 / 72, 16 / 72                                       # two axes of 20 edges, two diagonals of 16
    assert abs(pg["orientation_entropy"][1] + 2 * (p * math.log(p) + q * math.log(q))) < 1e-14

    for kind in CROSSING_KINDS:
        assert abs(both.mmd(both, kind)) <= 1e-15 and abs(both.kld(both, kind)) <= 1e-15
        assert both.mmd(grid, kind) >= 0.0
    assert both.mmd(grid, "crossings") > 0.01 and both.kld(grid, "orientation") > 0.1
    cmp = both.compare(grid)
    assert set(cmp) == {f"{m}_{k}" for m in ("mmd", "kld") for k in CROSSING_KINDS} | {"n_skipped", "self", "other"}
    assert cmp["self"] == both.summary() and cmp["n_skipped"] == (0, 0)
    with pytest.raises(ValueError, match="kind"):
        both.mmd(grid, "degree")
    with pytest.raises(ValueError):
        both.mmd(grid, "crossings", sigma=0.0)

    parts = [_stats([nm]) for nm in ("k8_circle", "grid5_diagonals", "grid5")]
    assert CrossingStats.concat(parts) == both and both.n_graphs == 3
    assert both != _stats(["k8_circle", "grid5", "grid5_diagonals"])
    with pytest.raises(ValueError):
        CrossingStats.concat([both, CrossingStats(both.counts, both.hist, 26)])
    with pytest.raises(ValueError):
        CrossingStats(both.counts[:, :6], both.hist, 25)

    # a skipped graph is left out and counted
    c = both.counts.copy()
    h = both.hist.copy()
    c[0], h[0] = -1, 0
    skipped = CrossingStats(c, h, 25)
    assert skipped.n_skipped == 1 and skipped.n_graphs == 3 and skipped.per_graph()["X"].tolist() == [16, 0]
    assert skipped.summary()["planar"] == 0.5 and skipped.compare(both)["n_skipped"] == (1, 0)
    assert skipped.mmd(_stats(["grid5_diagonals", "grid5"]), "crossings") <= 1e-15
    none = CrossingStats(np.full((2, 7), -1), np.zeros((2, 3, 256), np.int64), 25)
    assert math.isnan(none.summary()["planar"]) and math.isnan(none.mmd(both, "crossings"))


# ---------------------------------------------------------------- the C ABI without a device
def test_header_library_and_integration_agree_on_abi_29(lib_built):
    from snd_vae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snd_vae.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    so = ctypes.CDLL(lib_built)
    for name in ("snd_graph_crossings", "snd_graph_crossings_workspace"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(so, name) and name in doc, name
    abi = int(re.search(r"#define\s+SND_ABI_VERSION\s+(\d+)", hdr).group(1))
    stub = int(re.search(r"SND_ABI_VERSION\s*=\s*(\d+)", doc).group(1))
    assert abi == _lib.ABI_VERSION == so.snd_abi_version() == stub and abi >= 29


def test_no_spill_or_scratch_in_the_new_kernels(lib_built):
    from snd_vae_amd.build import build_info, kernel_resources
    names = ("gx_prep_kernel", "gx_plan_kernel", "gx_pairs_kernel", "gx_finish_kernel", "gx_final_kernel")
    res = {k: v for k, v in kernel_resources().items() if any(s in k for s in names)}
    assert len(res) == 5, sorted(res)
    for k, v in res.items():
        assert v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v.get("scratch", 0) == 0, (k, v)
    assert not any("gx_" in k for k in build_info().get("spills", {}))


def test_the_walk_cases_hold_more_tile_pairs_than_waves():
    """On a 256-CU device (and any smaller one) the two walk cases give every wave several items."""
    for name in X.WALK_CASES:
        c = X.build_case(name)
        w = X.reference(c, X.case_work_cap(name))
        items = sum(X.tile_pairs(e) for e in w["counts"][:, 0] if e >= 0)
        assert items > 1.3 * X.pair_waves(c.B, c.n, len(c.ci), 256), (name, items)


def test_tile_size_and_cap_are_the_kernels():
    from snd_vae_amd import layers
    hpp = open(os.path.join(ROOT, "snd_vae_amd", "csrc", "snd_gcrossings.hpp")).read()
    assert int(re.search(r"kGxTile\s*=\s*(\d+)", hpp).group(1)) == layers.CROSSINGS_TILE == X.TILE
    assert int(re.search(r"kGxMaxN\s*=\s*(\d+)", hpp).group(1)) == layers.CROSSINGS_MAX_N == X.MAX_N
    assert int(re.search(r"kGxGridPerCu\s*=\s*(\d+)", hpp).group(1)) == X.GRID_PER_CU
    prof = __import__("json").load(open(os.path.join(ROOT, "profiles", "graph_crossings_timing.json")))
    assert prof["default_work_cap"] == layers.CROSSINGS_WORK_CAP
    rate = prof["chords"]["pairs_per_second"]                     # the cap is that rate to one digit
    digit = 10 ** math.floor(math.log10(rate))
    assert layers.CROSSINGS_WORK_CAP == int(round(rate / digit)) * digit


class HostArgs:
    """A well-formed argument list over host memory.  No rule below reaches a launch, so nothing
    dereferences these pointers."""

    def __init__(self, _lib, B=2, n=10, cap=40):
        self.L = _lib.lib()
        self._lib = _lib
        self.need = self.L.snd_graph_crossings_workspace(B, n, cap)
        self.bufs = {"rowptr": np.zeros(B * n + 1, np.int32), "colidx": np.zeros(cap, np.int32),
                     "coords": np.zeros(B * n * 2, np.float32),
                     "counts": np.full(B * 7, 7, np.int64), "hist": np.full(B * 3 * 256, 7, np.int64),
                     "work": np.full(B, 7, np.int64), "cross": np.full(cap, 7, np.int32),
                     "ws": np.full(self.need // 8 + 2, 7, np.int64)}
        ws = self.bufs["ws"].ctypes.data
        ws += (-ws) % 16
        p = lambda k: self.bufs[k].ctypes.data
        self.args = dict(rowptr=p("rowptr"), colidx=p("colidx"), nnz_cap=cap, n_graphs=B, n=n, coords=p("coords"),
                         ldc=2, work_cap=1000, counts=p("counts"), hist=p("hist"), work=p("work"), cross=p("cross"),
                         ws=ws, ws_bytes=self.need)

    def call(self, **kw):
        a = dict(self.args)
        a.update(kw)
        rc = self.L.snd_graph_crossings(*a.values(), None)
        msg = self._lib.last_error() if rc else ""
        for k in ("counts", "hist", "work", "cross", "ws"):
            assert (self.bufs[k] == 7).all(), (kw, k)
        return rc, msg


def test_the_op_rejects_bad_arguments_before_any_launch(lib_built):
    from snd_vae_amd import _lib
    h = HostArgs(_lib)
    assert h.need >= 2 * 64 + 3 * 8 + 40 * 28 and h.need % 16 == 0
    bad = [dict(n_graphs=0), dict(n_graphs=-1), dict(n=0), dict(n=X.MAX_N + 1), dict(n=X.MAX_N, n_graphs=1 << 17),
           dict(nnz_cap=-1), dict(work_cap=-1), dict(ldc=1), dict(ldc=0), dict(rowptr=None), dict(coords=None),
           dict(counts=None), dict(hist=None), dict(work=None), dict(colidx=None), dict(ws_bytes=h.need - 1),
           dict(ws=None), dict(ws=h.args["ws"] + 8)]
    for kw in bad:
        rc, msg = h.call(**kw)
        assert rc == -1, (kw, rc)
        assert msg.startswith("snd_graph_crossings:"), (kw, msg)
    assert "workspace" in h.call(ws_bytes=h.need - 1)[1] and "work_cap" in h.call(work_cap=-1)[1]
    assert "colidx" in h.call(colidx=None)[1] and "n=" in h.call(n=0)[1] and "ldc" in h.call(ldc=1)[1]
    assert "aligned" in h.call(ws=h.args["ws"] + 8)[1]
    L = h.L
    assert L.snd_graph_crossings_workspace(0, 10, 40) == 0 and L.snd_graph_crossings_workspace(2, X.MAX_N + 1, 40) == 0
    assert L.snd_graph_crossings_workspace(2, 10, -1) == 0 and L.snd_graph_crossings_workspace(1 << 17, X.MAX_N, 0) == 0
    assert L.snd_graph_crossings_workspace(2, 10, 0) == 128 + 32 + 4 * 28       # the header's formula
    assert L.snd_graph_crossings_workspace(3, 10, 41) == 192 + 32 + 44 * 28


def test_layers_checks_without_a_device():
    import torch
    from snd_vae_amd import layers
    rp, ci = torch.zeros(21, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    xy = torch.zeros(20, 2)
    assert layers.CROSSINGS_WORK_CAP > 0
    for kw, match in ((dict(n_graphs=0), "n_graphs"), (dict(n=X.MAX_N + 1), "16384"), (dict(work_cap=-1), "work_cap"),
                      (dict(), "device tensor")):
        a = dict(rowptr=rp, colidx=ci, n_graphs=2, n=10, coords=xy)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            layers.graph_crossings(**a)
