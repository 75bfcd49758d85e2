"""NumPy restatement of snd_graph_crossings (include/snd_vae.h), importable without a GPU.

* ``mutual_edges``: the edges (a < b, local ids) of one graph block under snd_graph_motifs' rule,
  with the CSR position of each (the first occurrence of column b in row a) and the one-way arcs.
* ``crossing_pairs``: the predicate, vectorised in chunks: fp32 box reject on the coordinates as
  stored, then the four float64 orientations, every operation a separate NumPy call (one rounding
  each, no contraction), signs compared.
* ``reference``: counts [B, 7], hist [B, 3, 256], work [B], cross_out [len(colidx)] and, per graph,
  the continuous bin coordinates of the two angle histograms computed in float64 (``dir_vals``:
  theta 256 / pi + 1/2 folded to [0, 256); ``ang_vals``: phi 512 / pi), for the band comparison.
* ``exact_cross``: the predicate in exact rational arithmetic (``fractions``).
* ``CASES`` / ``build_case``: the GPU cases.
"""
from __future__ import annotations

from fractions import Fraction
from math import comb

import numpy as np

import graph_stats_ref as G

MAX_N = 16384                           # kGxMaxN
TILE = 64                               # kGxTile
BINS = 256
DELTA = 2.0 ** -10                      # half width of a bin edge's band, in bins
NAMES = ("E", "X", "crossed", "independent", "one_way", "zero_length", "max_c")


class Case:
    def __init__(self, name, B, n, rp, ci, xy):
        self.name, self.B, self.n = name, B, n
        self.rp = np.asarray(rp, np.int32)
        self.ci = np.asarray(ci, np.int32) if len(ci) else np.zeros(1, np.int32)    # a one-element colidx
        self.xy = np.ascontiguousarray(xy, np.float32).reshape(B * n, 2)
        for a in (self.rp, self.ci, self.xy):
            a.setflags(write=False)


# ------------------------------------------------------------------ the graph
def mutual_edges(rp, ci, B, n, g):
    """(a, b, pos, one_way, deg) of graph g: edges a < b in local ids, pos the CSR position of the
    first entry (row a, column b), the number of one-way arcs, the degrees [n]."""
    rp = np.asarray(rp, np.int64)
    lo, hi = int(rp[g * n]), int(rp[(g + 1) * n])
    rows = np.repeat(np.arange(g * n, (g + 1) * n, dtype=np.int64), np.diff(rp[g * n:(g + 1) * n + 1])) - g * n
    lc = np.asarray(ci[lo:hi], np.int64) - g * n
    ok = (lc >= 0) & (lc < n) & (lc != rows)
    idx = np.nonzero(ok)[0]
    key = rows[idx] * n + lc[idx]
    key, first = np.unique(key, return_index=True)               # the first occurrence counts
    idx = idx[first]
    r, c = key // n, key % n
    mut = np.isin(c * n + r, key)
    one_way = int((~mut).sum())
    up = mut & (c > r)
    deg = np.bincount(r[mut], minlength=n)
    return r[up], c[up], idx[up] + lo, one_way, deg


def orient(px, py, qx, qy, rx, ry):
    """(qx - px)(ry - py) - (qy - py)(rx - px) in float64, seven roundings."""
    t0 = np.multiply(np.subtract(qx, px), np.subtract(ry, py))
    t1 = np.multiply(np.subtract(qy, py), np.subtract(rx, px))
    return np.subtract(t0, t1)


def _opposite(s, t):
    return ((s > 0) & (t < 0)) | ((s < 0) & (t > 0))


def crossing_pairs(a, b, xy, chunk=512):
    """Index pairs (i < j) into the edge list whose edges cross.  xy [n, 2] float32."""
    E = len(a)
    if E < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    A, Bp = xy[a], xy[b]                                         # float32
    xmin, xmax = np.minimum(A[:, 0], Bp[:, 0]), np.maximum(A[:, 0], Bp[:, 0])
    ymin, ymax = np.minimum(A[:, 1], Bp[:, 1]), np.maximum(A[:, 1], Bp[:, 1])
    A64, B64 = A.astype(np.float64), Bp.astype(np.float64)
    out_i, out_j = [], []
    for i0 in range(0, E, chunk):
        i1 = min(E, i0 + chunk)
        s = slice(i0, i1)
        rej = ((xmax[s, None] < xmin[None, :]) | (xmax[None, :] < xmin[s, None])
               | (ymax[s, None] < ymin[None, :]) | (ymax[None, :] < ymin[s, None]))
        share = ((a[s, None] == a[None, :]) | (a[s, None] == b[None, :]) | (b[s, None] == a[None, :])
                 | (b[s, None] == b[None, :]))
        upper = np.arange(i0, i1)[:, None] < np.arange(E)[None, :]
        i, j = np.nonzero(~rej & ~share & upper)
        i += i0
        p, q, r, t = A64[i], B64[i], A64[j], B64[j]
        o1 = orient(p[:, 0], p[:, 1], q[:, 0], q[:, 1], r[:, 0], r[:, 1])
        o2 = orient(p[:, 0], p[:, 1], q[:, 0], q[:, 1], t[:, 0], t[:, 1])
        o3 = orient(r[:, 0], r[:, 1], t[:, 0], t[:, 1], p[:, 0], p[:, 1])
        o4 = orient(r[:, 0], r[:, 1], t[:, 0], t[:, 1], q[:, 0], q[:, 1])
        hit = _opposite(o1, o2) & _opposite(o3, o4)
        out_i.append(i[hit])
        out_j.append(j[hit])
    return np.concatenate(out_i), np.concatenate(out_j)


def direction_values(a, b, xy):
    """theta 256 / pi + 1/2 folded to [0, 256) of every edge of non-zero length, float64."""
    u = xy[b].astype(np.float64) - xy[a].astype(np.float64)
    u = u[(u[:, 0] != 0) | (u[:, 1] != 0)]
    neg = (u[:, 1] < 0) | ((u[:, 1] == 0) & (u[:, 0] < 0))
    u = np.where(neg[:, None], -u, u)
    t = np.arctan2(u[:, 1], u[:, 0]) * (256.0 / np.pi) + 0.5
    return np.where(t >= 256.0, t - 256.0, t)


def angle_values(a, b, xy, i, j):
    """phi 512 / pi of every crossing pair, float64."""
    u = xy[b[i]].astype(np.float64) - xy[a[i]].astype(np.float64)
    v = xy[b[j]].astype(np.float64) - xy[a[j]].astype(np.float64)
    cr = np.abs(u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0])
    dt = np.abs(u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1])
    return np.arctan2(cr, dt) * (512.0 / np.pi)


def reference(c, work_cap=None):
    """{counts, hist, work, cross_out, dir_vals, ang_vals} of a case; cross_out holds None-marker
    -7 past rowptr[B n] (untouched entries)."""
    key = (c.name, work_cap)
    if key in _ref_cache:
        return _ref_cache[key]
    B, n = c.B, c.n
    counts = np.zeros((B, 7), np.int64)
    hist = np.zeros((B, 3, BINS), np.int64)
    work = np.zeros(B, np.int64)
    cross = np.full(len(c.ci), -7, np.int32)
    cross[:int(c.rp[-1])] = 0
    dir_vals, ang_vals = [], []
    for g in range(B):
        xy = c.xy[g * n:(g + 1) * n]
        a, b, pos, one_way, deg = mutual_edges(c.rp, c.ci, B, n, g)
        E = len(a)
        work[g] = E * (E - 1) // 2
        if work_cap is not None and work[g] > work_cap:
            counts[g] = -1
            cross[int(c.rp[g * n]):int(c.rp[(g + 1) * n])] = -1
            dir_vals.append(np.zeros(0))
            ang_vals.append(np.zeros(0))
            continue
        i, j = crossing_pairs(a, b, xy)
        ce = np.bincount(np.concatenate([i, j]), minlength=E).astype(np.int64) if E else np.zeros(0, np.int64)
        zero = (xy[a, 0] == xy[b, 0]) & (xy[a, 1] == xy[b, 1])
        counts[g] = [E, len(i), int((ce > 0).sum()), work[g] - int((deg * (deg - 1) // 2).sum()), one_way,
                     int(zero.sum()), int(ce.max()) if E else 0]
        hist[g, 0] = np.bincount(np.minimum(ce, 255), minlength=BINS)
        dv = direction_values(a, b, xy)
        av = angle_values(a, b, xy, i, j)
        hist[g, 1] = np.bincount(np.floor(dv).astype(np.int64) % BINS, minlength=BINS)
        hist[g, 2] = np.bincount(np.minimum(np.floor(av).astype(np.int64), 255), minlength=BINS)
        cross[pos] = ce
        dir_vals.append(dv)
        ang_vals.append(av)
    out = {"counts": counts, "hist": hist, "work": work, "cross_out": cross, "dir_vals": dir_vals,
           "ang_vals": ang_vals}
    for v in (counts, hist, work, cross):
        v.setflags(write=False)
    _ref_cache[key] = out
    return out


_ref_cache = {}


# ------------------------------------------------------------------ the band comparison
def band_share(vals, wrap=False):
    """Share of the values within DELTA of a bin edge 1 .. 255 (and of the wrap edge 0 = 256)."""
    if not len(vals):
        return 0.0
    d = np.abs(vals - np.round(vals))
    near = (d < DELTA) & (np.round(vals) >= 1) & (np.round(vals) <= 255)
    if wrap:
        near |= (vals < DELTA) | (vals > 256.0 - DELTA)
    return float(near.mean())


def assert_hist_in_band(got, vals, what, wrap=False):
    """The device's cumulative count at every bin edge lies between the reference's counts of values
    below edge - DELTA and below edge + DELTA (atan2f is not correctly rounded).  ``wrap``: the
    histogram is circular (directions); a value within DELTA of the edge 0 = 256 may sit in
    bin 0 or bin 255."""
    got = np.asarray(got, np.int64)
    assert got.sum() == len(vals), (what, int(got.sum()), len(vals))
    cum = np.cumsum(got)[:-1]                                    # below the edges 1 .. 255
    v = np.sort(vals)
    edges = np.arange(1, BINS, dtype=np.float64)
    lo = np.searchsorted(v, edges - DELTA, side="left")
    hi = np.searchsorted(v, edges + DELTA, side="left")
    if wrap:
        lo = lo - int((vals < DELTA).sum())                      # those may have gone to bin 255
        hi = hi + int((vals > 256.0 - DELTA).sum())              # those may have come to bin 0
    bad = np.nonzero((cum < lo) | (cum > hi))[0]
    assert not len(bad), f"{what}: edge {int(bad[0]) + 1}: cumulative {int(cum[bad[0]])} not in " \
                         f"[{int(lo[bad[0]])}, {int(hi[bad[0]])}] ({len(bad)} edges)"


def assert_equal(got, want, what=""):
    """Exact parts: counts, work, cross_out, hist[0], the sums of hist[1] and hist[2]; then the
    two angle histograms per graph through the band."""
    for k in ("work", "counts"):
        g, w = np.asarray(got[k], np.int64), np.asarray(want[k], np.int64)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what} {k}: at {bad[0].tolist()} got {int(g[tuple(bad[0])])} want " \
                             f"{int(w[tuple(bad[0])])} ({len(bad)} differ; got {g[bad[0][0]].tolist()} " \
                             f"want {w[bad[0][0]].tolist()})"
    gh, wh = np.asarray(got["hist"], np.int64), want["hist"]
    assert np.array_equal(gh[:, 0], wh[:, 0]), f"{what}: hist[0]"
    assert np.array_equal(gh[:, 1:].sum(axis=2), wh[:, 1:].sum(axis=2)), f"{what}: sums of hist[1], hist[2]"
    if got.get("cross_out") is not None:
        g, w = np.asarray(got["cross_out"]), want["cross_out"]
        keep = w != -7
        bad = np.nonzero(g[keep] != w[keep])[0]
        assert not len(bad), f"{what} cross_out: entry {int(bad[0])} got {int(g[keep][bad[0]])} want " \
                             f"{int(w[keep][bad[0]])} ({len(bad)} differ)"
    for g in range(gh.shape[0]):
        if want["counts"][g, 0] < 0:
            assert not gh[g].any(), f"{what}: skipped graph {g} has hist entries"
            continue
        assert_hist_in_band(gh[g, 1], want["dir_vals"][g], f"{what} graph {g} hist[1]", wrap=True)
        assert_hist_in_band(gh[g, 2], np.minimum(want["ang_vals"][g], 255.5), f"{what} graph {g} hist[2]")


# ------------------------------------------------------------------ exact arithmetic
def exact_cross(p, q, r, t):
    """The predicate on four points with exactly representable coordinates, in rationals
    (conditions 2 and 3; the caller knows the endpoints are distinct nodes)."""
    F = lambda z: (Fraction(float(z[0])), Fraction(float(z[1])))
    p, q, r, t = F(p), F(q), F(r), F(t)
    for k in (0, 1):
        if max(p[k], q[k]) < min(r[k], t[k]) or max(r[k], t[k]) < min(p[k], q[k]):
            return False
    o = lambda a, b, c: (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    opp = lambda s, u: (s > 0 and u < 0) or (s < 0 and u > 0)
    return opp(o(p, q, r), o(p, q, t)) and opp(o(r, t, p), o(r, t, q))


# ------------------------------------------------------------------ graphs
def _complete(n, base=0):
    return [(base + i, base + j) for i in range(n) for j in range(i + 1, n)]


def grid_pairs(k, diagonals):
    p = [(r * k + q, r * k + q + 1) for r in range(k) for q in range(k - 1)]
    p += [(r * k + q, (r + 1) * k + q) for r in range(k - 1) for q in range(k)]
    if diagonals:
        p += [(r * k + q, (r + 1) * k + q + 1) for r in range(k - 1) for q in range(k - 1)]
        p += [(r * k + q + 1, (r + 1) * k + q) for r in range(k - 1) for q in range(k - 1)]
    return p


def grid_xy(k, n):
    xy = np.full((n, 2), 2.0, np.float32)                        # unused nodes far away
    for r in range(k):
        for q in range(k):
            xy[r * k + q] = (0.25 * q, 0.25 * r)                 # exact in fp32
    return xy


def circle_xy(m, n, centre=0.5, radius=0.4):
    xy = np.full((n, 2), 2.0, np.float32)
    ang = 2.0 * np.pi * np.arange(m) / m
    xy[:m, 0] = (centre + radius * np.cos(ang)).astype(np.float32)
    xy[:m, 1] = (centre + radius * np.sin(ang)).astype(np.float32)
    return xy


# (name, pairs, xy builder, expected X) of the closed-form graphs, all on n = 25 nodes
def closed_forms(n=25):
    out = []
    out.append(("k8_circle", _complete(8), circle_xy(8, n), comb(8, 4)))
    xy = np.full((n, 2), 2.0, np.float32)
    for i in range(3):
        xy[i] = (np.float32(0.1) * np.float32(i), 0.0)
    for j in range(4):
        xy[3 + j] = (np.float32(0.13) * np.float32(j), 1.0)
    out.append(("k34_lines", [(i, 3 + j) for i in range(3) for j in range(4)], xy, 18))
    out.append(("grid5_diagonals", grid_pairs(5, True), grid_xy(5, n), 16))
    out.append(("grid5", grid_pairs(5, False), grid_xy(5, n), 0))
    xy = circle_xy(24, n)
    xy[24] = (0.5, 0.5)
    out.append(("star", [(24, j) for j in range(24)], xy, 0))
    xy = np.random.default_rng(5).random((n, 2)).astype(np.float32)
    xy = xy[np.argsort(xy[:, 0])]
    out.append(("path", [(i, i + 1) for i in range(n - 1)], xy, 0))                 # x-monotone: no crossing
    xy = np.full((n, 2), 2.0, np.float32)
    xy[:4] = [(0.0, 0.0), (0.25, 0.25), (0.5, 0.5), (0.75, 0.75)]                    # a line
    xy[4:7] = [(0.0, 1.0), (1.0, 1.0), (0.5, 1.0)]                                   # 6 sits on {4, 5}
    xy[7] = (0.5, 1.5)
    xy[8], xy[9] = (0.5, 0.5), (0.0, 0.5)                                            # 8 coincides with 2
    xy[10] = xy[11] = (0.9, 0.1)                                                     # a zero-length edge
    out.append(("degenerate", [(0, 2), (1, 3), (4, 5), (6, 7), (8, 9), (10, 11)], xy, 0))
    return out


def _csr(pairs, B, n, seed=None, extra=()):
    return G.csr_from_pairs(pairs, B, n, shuffle_seed=seed, extra=extra)


def _extras(rng, B, n, pairs):
    """One-way arcs, self loops and out-of-block entries as directed extras."""
    have = {(int(i), int(j)) for i, j in pairs}
    extra = []
    for b in range(B):
        for _ in range(max(1, n // 3)):
            x, y = (int(v) for v in rng.choice(n, size=2, replace=False))
            if (b * n + min(x, y), b * n + max(x, y)) not in have:
                extra.append((b * n + x, b * n + y))
        extra += [(b * n + int(x), b * n + int(x)) for x in rng.choice(n, size=max(1, n // 4), replace=False)]
        if B > 1:
            extra.append((b * n + int(rng.integers(n)), ((b + 1) % B) * n + int(rng.integers(n))))
    return sorted(set(extra))


def rgg_pairs(xy, B, n, radius):
    out = []
    for b in range(B):
        p = xy[b * n:(b + 1) * n].astype(np.float64)
        d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        i, j = np.nonzero(np.triu(d2 < radius * radius, k=1))
        out.append(np.stack([i + b * n, j + b * n], axis=1))
    return np.concatenate(out)


def _subset_pairs(rng, n, m, base):
    allp = np.asarray(_complete(n), np.int64)
    return allp[rng.choice(len(allp), size=m, replace=False)] + base


CASES = ("closed", "r33", "tile_edges", "b70_mixed", "n1024", "n16384_sparse", "cap_middle", "cap0", "walk_one",
         "walk_batch")
WALK_CASES = ("walk_one", "walk_batch")  # more tile pairs than the all-pairs kernel has waves: a wave walks several
GRID_PER_CU = 8                         # kGxGridPerCu: four-wave workgroups of the all-pairs kernel per compute unit


def pair_waves(B, n, nnz_cap, cus):
    """The waves of the all-pairs kernel for a call (graph_crossings_pair_blocks of the host code)."""
    bound = min(nnz_cap // 2, n * (n - 1) // 2)
    T = -(-bound // TILE)
    most = GRID_PER_CU * cus
    per = min(T * (T + 1) // 2, most * 4)
    return 4 * max(1, min(most, -(-(per * B) // 4)))


def tile_pairs(E):
    """Work items of a counted graph with E edges."""
    T = -(-int(E) // TILE)
    return T * (T + 1) // 2 if E >= 2 else 0


def build_case(name):
    if name in _case_cache:
        return _case_cache[name]
    if name == "closed":
        n = 25
        forms = closed_forms(n)
        graphs = []                                                                  # (pairs, xy)
        rnd = np.random.default_rng(3).random((n, 2)).astype(np.float32)
        for k, (_, pairs, xy, _) in enumerate(forms):
            graphs.append((pairs, xy))
            if k == 0:
                graphs.append(([], rnd))                                             # an empty graph
            if k == 1:
                graphs.append(([(3, 17)], rnd))                                      # a one-edge graph
        B = len(graphs)
        pairs = [(b * n + i, b * n + j) for b, (pp, _) in enumerate(graphs) for i, j in pp]
        c = Case(name, B, n, *_csr(pairs, B, n, seed=2), np.concatenate([xy for _, xy in graphs]))
    elif name == "r33":
        B, n = 5, 33
        rng = np.random.default_rng(33)
        xy = rng.random((B * n, 2)).astype(np.float32)
        pairs = rgg_pairs(xy, B, n, 0.45)
        c = Case(name, B, n, *_csr(pairs, B, n, seed=34, extra=_extras(rng, B, n, pairs)), xy)
    elif name == "tile_edges":
        n, sizes = 40, (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
        rng = np.random.default_rng(64)
        B = len(sizes)
        pairs = np.concatenate([_subset_pairs(rng, n, m, b * n) for b, m in enumerate(sizes)])
        c = Case(name, B, n, *_csr(pairs, B, n, seed=65), rng.random((B * n, 2)).astype(np.float32))
    elif name == "b70_mixed":
        B, n = 70, 25
        rng = np.random.default_rng(70)
        full = n * (n - 1) // 2
        pairs = np.concatenate([_subset_pairs(rng, n, round(b * full / (B - 1)), b * n) for b in range(B)])
        c = Case(name, B, n, *_csr(pairs, B, n, seed=71, extra=G._injected(B, n, 72)),
                 rng.random((B * n, 2)).astype(np.float32))
    elif name == "n1024":
        B, n = 2, 1024
        rng = np.random.default_rng(1024)
        xy = rng.random((B * n, 2)).astype(np.float32)
        c = Case(name, B, n, *_csr(rgg_pairs(xy, B, n, 0.0493), B, n, seed=1025), xy)
    elif name == "n16384_sparse":
        n = MAX_N
        rng = np.random.default_rng(16384)
        ch = rng.integers(0, n, (2100, 2))
        ch = ch[ch[:, 0] != ch[:, 1]]
        ch = np.unique(np.sort(ch, axis=1), axis=0)
        # irregular angles: the chords of a regular n-gon meet at multiples of pi / n, on bin edges
        ang = np.sort(rng.random(n)) * 2.0 * np.pi
        xy = np.stack([0.5 + 0.45 * np.cos(ang), 0.5 + 0.45 * np.sin(ang)], axis=1).astype(np.float32)
        c = Case(name, 1, n, *_csr(ch, 1, n, seed=7), xy)
    elif name == "walk_one":
        # one graph of about 10^4 edges, T = 162 tiles: 13203 tile pairs for at most 8192 waves, so a wave
        # walks along a row of tiles and from one row to the next
        n = 2048
        rng = np.random.default_rng(2048)
        xy = rng.random((n, 2)).astype(np.float32)
        c = Case(name, 1, n, *_csr(rgg_pairs(xy, 1, n, 0.04), 1, n, seed=2049), xy)
    elif name == "walk_batch":
        # 2200 graphs of 0 .. 300 edges (1, 3, 6, 10 or 15 tile pairs each, about 1.1e4 in all), every
        # 9th empty and every 13th complete (over this case's work_cap): the waves' ranges cross from
        # graph to graph, over graphs without items
        B, n = 2200, 25
        rng = np.random.default_rng(1500)
        full = n * (n - 1) // 2
        sizes = [0 if b % 9 == 4 else (full if b % 13 == 6 else int(rng.integers(1, full))) for b in range(B)]
        allp = np.asarray(_complete(n), np.int64)
        pairs = np.concatenate([allp[rng.choice(full, size=m, replace=False)] + b * n for b, m in enumerate(sizes)])
        c = Case(name, B, n, *_csr(pairs, B, n, seed=1501), rng.random((B * n, 2)).astype(np.float32))
    elif name == "cap_middle":
        n = 30
        rng = np.random.default_rng(30)
        pairs = np.concatenate([_subset_pairs(rng, n, 40, 0), _subset_pairs(rng, n, 200, n),
                                _subset_pairs(rng, n, 50, 2 * n)])
        c = Case(name, 3, n, *_csr(pairs, 3, n, seed=31), rng.random((3 * n, 2)).astype(np.float32))
    elif name == "cap0":
        n = 10
        rng = np.random.default_rng(10)
        pairs = [(0, 5), (1, 6)] + [(2 * n + 3, 2 * n + 4)] + [(3 * n + i, 3 * n + j) for i, j in _complete(5)]
        c = Case(name, 4, n, *_csr(pairs, 4, n, seed=11), rng.random((4 * n, 2)).astype(np.float32))
    else:
        raise KeyError(name)
    _case_cache[name] = c
    return c


_case_cache = {}


def case_work_cap(name):
    """The work_cap a case runs with (None: none of its graphs may be skipped)."""
    if name == "cap_middle":
        return (50 * 49 // 2 + 200 * 199 // 2) // 2
    if name == "cap0":
        return 0
    if name == "walk_batch":
        return 300 * 299 // 2 - 1                               # only the complete graphs are above it
    return None
