"""Integer / float64 reference of snd_graph_stats (include/snd_vae.h), plain NumPy + scipy:
importable without a GPU.

* ``neighbour_matrix``: the block-diagonal CSR after the set / block / self-loop rules, as a
  0/1 scipy CSR matrix A (row i holds N(i)).
* ``ref_stats``: deg = A 1, tri2 = rowsum((A A^T) o A) -- |N(i) & N(j)| is (A A^T)_ij, which
  is (A A)_ij on a symmetric CSR --, the three histograms and the totals.  Edge lengths in
  float64 from the fp32 coordinates and the fp32 len_scale.
* ``ambiguous_edges``: the edges whose v = len * len_scale lies within 2^-21 |v| of an
  integer.  An fp32 evaluation rounds 2^-24 relative at the difference, the two squares,
  the sum, the square root and the scale; eight roundings are allowed.  Outside that margin
  the fp32 bin is the float64 bin, so ``settle_coords`` re-draws the coordinates of the
  nodes on such edges until none is left and the histograms are compared exactly.
* ``emulate``: the kernel's walk restated row by row (mask words, 64-entry load steps), the
  vehicle of the planted faults of tests/test_graph_stats_cpu.py; ``bins_from_rows`` is its
  per-row epilogue (degree and clustering bins, totals).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

BINS = 256
MARGIN = 2.0 ** -21


# ------------------------------------------------------------------ the rules
def valid_entries(rp, ci, B, n):
    """(row, local column) of every entry that counts: inside the row's block, no self loop."""
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)[:rp[-1]]
    rows = np.repeat(np.arange(B * n, dtype=np.int64), np.diff(rp))
    base = rows // n * n
    ok = (ci >= base) & (ci < base + n) & (ci != rows)
    return rows[ok], (ci - base)[ok]


def neighbour_matrix(rp, ci, B, n):
    rows, lc = valid_entries(rp, ci, B, n)
    R = B * n
    A = sp.csr_matrix((np.ones(len(rows), np.int64), (rows, rows // n * n + lc)), shape=(R, R))
    A.data[:] = 1                                   # a set: duplicates collapse
    A.sum_duplicates()
    A.data[:] = 1
    return A


def len_bins(v):
    return np.minimum(np.floor(v), BINS - 1).astype(np.int64)


def edge_values(A, n, coords, len_scale):
    """(i, j, v) of every entry with column > row: v = len * len_scale in float64, from the
    fp32 coordinates and the fp32 scale."""
    U = sp.triu(A, k=1).tocoo()
    x = np.asarray(coords, np.float32).astype(np.float64)
    d = x[U.row] - x[U.col]
    v = np.sqrt((d * d).sum(axis=1)) * float(np.float32(len_scale))
    return U.row.astype(np.int64), U.col.astype(np.int64), v


def cluster_bins(deg, tri2):
    """min(floor(256 tri2 / (deg (deg - 1))), 255) in exact integers; deg < 2 -> 0."""
    deg = [int(d) for d in deg]
    return np.array([0 if d < 2 else min(256 * int(t) // (d * (d - 1)), BINS - 1) for d, t in zip(deg, tri2)],
                    np.int64)


def bins_from_rows(deg, tri2, B, n, fault=None):
    """The per-row epilogue: hist rows 0 and 1 and totals[:, :3] from deg and tri2."""
    deg = np.asarray(deg, np.int64)
    tri2 = np.asarray(tri2, np.int64)
    hist = np.zeros((B, 3, BINS), np.int64)
    totals = np.zeros((B, 4), np.int64)
    if fault == "clustering_f32":
        dd = (deg * (deg - 1)).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.float32(256.0) * tri2.astype(np.float32) / dd
        cb = np.where(deg < 2, 0, np.minimum(np.floor(np.nan_to_num(q)), BINS - 1)).astype(np.int64)
    else:
        cb = cluster_bins(deg, tri2)
    g = np.arange(B * n) // n
    np.add.at(hist, (g, 0, np.minimum(deg, BINS - 1)), 1)
    np.add.at(hist, (g, 1, cb), 1)
    np.add.at(totals, (g, 0), deg)
    np.add.at(totals, (g, 1), tri2)
    np.add.at(totals, (g, 2), deg * (deg - 1))
    return hist, totals, cb


def ref_stats(rp, ci, B, n, coords=None, len_scale=None):
    """{"deg", "tri2" [B*n], "hist" [B, 3, 256], "totals" [B, 4], "cbin" [B*n]}."""
    A = neighbour_matrix(rp, ci, B, n)
    deg = np.asarray(A.sum(axis=1)).ravel().astype(np.int64)
    tri2 = np.asarray((A @ A.T).multiply(A).sum(axis=1)).ravel().astype(np.int64)
    hist, totals, cb = bins_from_rows(deg, tri2, B, n)
    U = sp.triu(A, k=1).tocoo()
    np.add.at(totals, (U.row // n, 3), 1)
    if coords is not None:
        i, _, v = edge_values(A, n, coords, len_scale)
        np.add.at(hist, (i // n, 2, len_bins(v)), 1)
    return {"deg": deg, "tri2": tri2, "hist": hist, "totals": totals, "cbin": cb}


# ------------------------------------------------------------------ the margin rule
def ambiguous_edges(rp, ci, B, n, coords, len_scale):
    """[(i, j)] (global ids, j > i) of the edges whose v is within 2^-21 |v| of an integer."""
    A = neighbour_matrix(rp, ci, B, n)
    i, j, v = edge_values(A, n, coords, len_scale)
    bad = np.abs(v - np.rint(v)) <= MARGIN * np.abs(v)
    return np.stack([i[bad], j[bad]], axis=1)


def settle_coords(rp, ci, B, n, sd, len_scale, seed, max_rounds=64):
    """fp32 coordinates [B*n, sd] in the unit box with no ambiguous edge: drawn from ``seed``,
    the nodes on ambiguous edges re-drawn until none is left."""
    rng = np.random.default_rng(seed)
    x = rng.random((B * n, sd)).astype(np.float32)
    for _ in range(max_rounds):
        bad = ambiguous_edges(rp, ci, B, n, x, len_scale)
        if len(bad) == 0:
            return x
        nodes = np.unique(bad)
        x[nodes] = rng.random((len(nodes), sd)).astype(np.float32)
    raise AssertionError(f"settle_coords: {len(bad)} ambiguous edges left after {max_rounds} rounds")


# ------------------------------------------------------------------ the kernel's walk
FAULTS = ("mask_drops_last_word", "walk_stops_at_64", "self_loop_counted", "next_block_counted",
          "length_both_directions", "clustering_f32")


def emulate(rp, ci, B, n, coords=None, len_scale=None, fault=None):
    """snd_graph_stats as graph_stats_kernel walks it: per row the mask of N(i) in 32-bit
    words, the neighbours' rows read in load steps of 64 entries and tested against the mask,
    the lengths of the entries with column > row in float32.  ``fault`` plants one of FAULTS."""
    assert fault is None or fault in FAULTS, fault
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    R = B * n
    words = n // 32 if fault == "mask_drops_last_word" else (n + 31) // 32
    deg = np.zeros(R, np.int64)
    tri2 = np.zeros(R, np.int64)
    edges = np.zeros(B, np.int64)
    lhist = np.zeros((B, BINS), np.int64)
    x = None if coords is None else np.asarray(coords, np.float32)
    scale = None if coords is None else np.float32(len_scale)

    def local(c, base, self_row):
        """(local ids, member flags) of global columns c for a row of the block at base."""
        lc = c - base
        if fault == "next_block_counted":
            ok = (lc >= 0) & (lc < 2 * n) & (c < R)
            lc = lc % n
        else:
            ok = (lc >= 0) & (lc < n)
        if fault != "self_loop_counted":
            ok &= lc != self_row
        return lc, ok

    for i in range(R):
        base, li = i // n * n, i % n
        c = ci[rp[i]:rp[i + 1]]
        lc, ok = local(c, base, li)
        mask = np.zeros(max(words, 1), np.uint32)
        inmask = ok & (lc >> 5 < words)
        np.bitwise_or.at(mask, lc[inmask] >> 5, (np.uint32(1) << (lc[inmask] & 31).astype(np.uint32)))
        deg[i] = int(ok.sum())
        for j in lc[ok]:
            row = ci[rp[base + j]:rp[base + j + 1]]
            if fault == "walk_stops_at_64":
                row = row[:64]
            for s in range(0, len(row), 64):                       # one load step
                l2, ok2 = local(row[s:s + 64], base, j)
                ok2 &= l2 >> 5 < words
                l2 = l2[ok2]
                tri2[i] += int(((mask[l2 >> 5] >> (l2 & 31).astype(np.uint32)) & 1).sum())
        up = ok if fault == "length_both_directions" else ok & (lc > li)
        edges[i // n] += int((ok & (lc > li)).sum())
        if x is not None and up.any():
            d = x[i][None, :] - x[base + lc[up]]
            s = np.zeros(d.shape[0], np.float32)
            for k in range(d.shape[1]):
                s = s + d[:, k] * d[:, k]
            v = np.sqrt(s) * scale
            np.add.at(lhist[i // n], len_bins(v.astype(np.float64)), 1)
    hist, totals, _ = bins_from_rows(deg, tri2, B, n, fault)
    hist[:, 2] = lhist
    totals[:, 3] = edges
    return {"deg": deg, "tri2": tri2, "hist": hist, "totals": totals}


def assert_stats_equal(got, want, n, what=""):
    """Exact comparison; a failure names the first row (deg, tri2) or the graph and bin."""
    for k in ("deg", "tri2"):
        if got.get(k) is None:
            continue
        g, w = np.asarray(got[k], np.int64), np.asarray(want[k], np.int64)
        bad = np.nonzero(g != w)[0]
        if len(bad):
            i = int(bad[0])
            raise AssertionError(f"{what} {k}: row {i} (graph {i // n}, node {i % n}) got {int(g[i])} want "
                                 f"{int(w[i])} ({len(bad)} rows differ)")
    names = ("degree", "clustering", "edge_length")
    g, w = np.asarray(got["hist"], np.int64), np.asarray(want["hist"], np.int64)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    if len(bad):
        b, r, k = (int(t) for t in bad[0])
        rows = ""
        if r == 1 and "cbin" in want:
            rows = f"; rows of that bin: {np.nonzero(want['cbin'] == k)[0][:4].tolist()}"
        raise AssertionError(f"{what} hist: graph {b} {names[r]} bin {k} got {int(g[b, r, k])} want "
                             f"{int(w[b, r, k])} ({len(bad)} bins differ){rows}")
    g, w = np.asarray(got["totals"], np.int64), np.asarray(want["totals"], np.int64)
    bad = np.argwhere(g != w)
    if len(bad):
        b, k = (int(t) for t in bad[0])
        raise AssertionError(f"{what} totals: graph {b} column {k} got {int(g[b, k])} want {int(w[b, k])}")


# ------------------------------------------------------------------ graphs
def csr_from_pairs(pairs, B, n, shuffle_seed=None, extra=()):
    """Block-diagonal CSR (rowptr, colidx int32) holding both directions of the undirected
    (i, j) global pairs, plus the directed ``extra`` entries (self loops, out-of-block ids,
    one-way arcs); rows ascending, or shuffled within each row by ``shuffle_seed``."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    extra = np.asarray(extra, np.int64).reshape(-1, 2)
    r = np.concatenate([pairs[:, 0], pairs[:, 1], extra[:, 0]])
    c = np.concatenate([pairs[:, 1], pairs[:, 0], extra[:, 1]])
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    rp = np.zeros(B * n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=B * n), out=rp[1:])
    if shuffle_seed is not None:
        rng = np.random.default_rng(shuffle_seed)
        for i in range(B * n):
            rng.shuffle(c[rp[i]:rp[i + 1]])
    return rp.astype(np.int32), c.astype(np.int32)


def random_pairs(B, n, mean_degree, seed):
    """Undirected G(n, p) pairs per graph (global ids, i < j, no duplicates)."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        if n < 2:
            continue
        m = rng.poisson(mean_degree * n / 2.0)
        i = rng.integers(0, n, m)
        j = rng.integers(0, n, m)
        keep = i != j
        lo, hi = np.minimum(i, j)[keep], np.maximum(i, j)[keep]
        key = np.unique(lo * n + hi)
        out.append(np.stack([key // n + b * n, key % n + b * n], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


# ------------------------------------------------------------------ the GPU cases
# The smallest shapes at which the kernel can go wrong: one node, one edge, n below / across /
# not a multiple of the mask's 32-bit word and of the 64-entry load step, more rows than one
# workgroup's four, several graphs, rows longer than 64 and than 255 entries.
CASES = ("b1n1", "b1n2", "b3n33", "b2n70", "b1n257", "b2n2049", "k40", "star200", "empty_middle", "deg300")


class Case:
    def __init__(self, name, B, n, rp, ci):
        self.name, self.B, self.n = name, B, n
        self.rp, self.ci = rp, ci if len(ci) else np.zeros(1, np.int32)     # a one-element colidx
        self.rp.setflags(write=False)
        self.ci.setflags(write=False)


def _injected(B, n, seed):
    """Self loops and (for B > 1) entries of other graphs' blocks, as directed extras."""
    rng = np.random.default_rng(seed)
    R = B * n
    loops = rng.choice(R, size=max(1, R // 7), replace=False)
    extra = [(int(i), int(i)) for i in loops]
    if B > 1:
        for i in rng.choice(R, size=max(2, R // 5), replace=False):
            other = (int(i) // n + 1 + int(rng.integers(0, B - 1))) % B
            extra.append((int(i), other * n + int(rng.integers(0, n))))
        extra += [(n - 1, n), (n, n - 1)]                                  # across the block edge
    return sorted(set(extra))


_case_cache = {}


def build_case(name):
    if name in _case_cache:
        return _case_cache[name]
    if name == "b1n1":
        c = Case(name, 1, 1, *csr_from_pairs([], 1, 1))
    elif name == "b1n2":
        c = Case(name, 1, 2, *csr_from_pairs([(0, 1)], 1, 2))
    elif name in ("b3n33", "b2n70", "b1n257", "b2n2049"):
        B, n, md = {"b3n33": (3, 33, 5.0), "b2n70": (2, 70, 8.0), "b1n257": (1, 257, 6.0),
                    "b2n2049": (2, 2049, 6.0)}[name]
        seed = 100 + n
        c = Case(name, B, n, *csr_from_pairs(random_pairs(B, n, md, seed), B, n, shuffle_seed=seed + 1,
                                              extra=_injected(B, n, seed + 2)))
    elif name == "k40":
        c = Case(name, 1, 40, *csr_from_pairs([(i, j) for i in range(40) for j in range(i + 1, 40)], 1, 40))
    elif name == "star200":
        c = Case(name, 1, 200, *csr_from_pairs([(0, j) for j in range(1, 200)], 1, 200, shuffle_seed=7))
    elif name == "empty_middle":
        p = random_pairs(3, 33, 5.0, 300)
        p = p[(p[:, 0] // 33) != 1]
        c = Case(name, 3, 33, *csr_from_pairs(p, 3, 33, shuffle_seed=301))
    elif name == "deg300":
        p = np.concatenate([random_pairs(2, 300, 6.0, 310), [(300 + 5, 300 + j) for j in range(300) if j != 5]])
        p = np.unique(np.sort(p, axis=1), axis=0)
        c = Case(name, 2, 300, *csr_from_pairs(p, 2, 300, shuffle_seed=311, extra=_injected(2, 300, 312)))
    else:
        raise KeyError(name)
    _case_cache[name] = c
    return c


_coord_cache = {}


def case_coords(name, sd):
    """(fp32 coordinates [B*n, sd] without an ambiguous edge, fp32 len_scale = 256 / sqrt(sd))."""
    key = (name, sd)
    if key not in _coord_cache:
        c = build_case(name)
        scale = np.float32(256.0 / np.sqrt(float(sd)))
        x = settle_coords(c.rp, c.ci, c.B, c.n, sd, scale, seed=1000 * sd + len(name) + c.n)
        assert len(ambiguous_edges(c.rp, c.ci, c.B, c.n, x, scale)) == 0
        x.setflags(write=False)
        _coord_cache[key] = (x, scale)
    return _coord_cache[key]
