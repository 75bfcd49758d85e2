"""Integer reference of snd_graph_motifs (include/snd_vae.h), plain NumPy + scipy: importable
without a GPU.

* ``brute_census`` / ``brute_orbits``: every 3- and 4-subset of the nodes of one graph
  (n <= 14) classified by the edge count and degree sequence of its induced subgraph; the
  edge rule is restated with Python loops over the CSR, independent of the scipy route.
* ``route_census``: the counting route of the header on scipy.sparse matrices (degrees,
  codegrees M M, per-edge triangles (M M) o M, 4-cliques as the triangles among the higher
  neighbours of every node), then the primed-to-induced conversion.  ``fault`` plants one of
  FAULTS.
* ``work``: the header's formula on the CSR rows.
* ``reference``: census [B, 10] and work [B] of a batch, with the work_cap rule.
* ``CASES`` / ``build_case``: the GPU cases.
"""
from __future__ import annotations

from itertools import combinations
from math import comb

import numpy as np
import scipy.sparse as sp

import graph_stats_ref as G

MAX_N = 16384                           # kGmMaxN
LDS_THRESHOLD = 7280                    # four waves per workgroup up to here, one above
NAMES = ("E", "P2", "T", "P3", "S3", "C4", "TT", "D", "K4", "one_way")
FAULTS = ("conversion_constant", "diagonal_counted", "one_way_counted", "next_block_counted")


# ------------------------------------------------------------------ brute force
def dense_mutual(rp, ci, B, n, g):
    """(mutual adjacency [n, n] bool, one-way arcs) of graph g, by the rule's own words."""
    rp = np.asarray(rp, np.int64)
    arc = np.zeros((n, n), bool)
    for li in range(n):
        i = g * n + li
        for e in range(rp[i], rp[i + 1]):
            c = int(ci[e])
            if g * n <= c < (g + 1) * n and c != i:
                arc[li, c - g * n] = True
    m = arc & arc.T
    return m, int(arc.sum() - m.sum())


def _kind4(sub):
    """Index into NAMES of the connected induced 4-node subgraph with adjacency ``sub``, or -1;
    and the orbit of each of its nodes."""
    deg = sub.sum(axis=1)
    e, key = int(deg.sum()) // 2, tuple(sorted(deg.tolist()))
    if e == 3 and key == (1, 1, 2, 2):
        return 3, [4 if d == 1 else 5 for d in deg]
    if e == 3 and key == (1, 1, 1, 3):
        return 4, [6 if d == 1 else 7 for d in deg]
    if e == 4 and key == (2, 2, 2, 2):
        return 5, [8] * 4
    if e == 4 and key == (1, 2, 2, 3):
        return 6, [{1: 9, 2: 10, 3: 11}[int(d)] for d in deg]
    if e == 5:
        return 7, [12 if d == 2 else 13 for d in deg]
    if e == 6:
        return 8, [14] * 4
    return -1, None


def brute_orbits(m):
    """(census[:9], per-node orbit table [n, 15]) of the bool adjacency m, n <= 14."""
    n = m.shape[0]
    assert n <= 14
    cen = np.zeros(9, np.int64)
    orb = np.zeros((n, 15), np.int64)
    for i, j in combinations(range(n), 2):
        if m[i, j]:
            cen[0] += 1
            orb[i, 0] += 1
            orb[j, 0] += 1
    for s in combinations(range(n), 3):
        sub = m[np.ix_(s, s)]
        deg = sub.sum(axis=1)
        e = int(deg.sum()) // 2
        if e == 2:
            cen[1] += 1
            for node, d in zip(s, deg):
                orb[node, 2 if d == 2 else 1] += 1
        elif e == 3:
            cen[2] += 1
            for node in s:
                orb[node, 3] += 1
    for s in combinations(range(n), 4):
        k, o = _kind4(m[np.ix_(s, s)])
        if k >= 0:
            cen[k] += 1
            for node, ob in zip(s, o):
                orb[node, ob] += 1
    return cen, orb


def brute_census(rp, ci, B, n):
    out = np.zeros((B, 10), np.int64)
    for g in range(B):
        m, one = dense_mutual(rp, ci, B, n, g)
        out[g, :9] = brute_orbits(m)[0]
        out[g, 9] = one
    return out


def orbit_sums(census):
    """[..., 15]: the fifteen orbit counts summed over a graph's nodes, from census[..., :9]."""
    c = np.asarray(census, np.int64)
    E, P2, T, P3, S3, C4, TT, D, K4 = (c[..., k] for k in range(9))
    return np.stack([2 * E, 2 * P2, P2, 3 * T, 2 * P3, 2 * P3, 3 * S3, S3, 4 * C4, TT, 2 * TT, TT, 2 * D, 2 * D,
                     4 * K4], axis=-1)


# ------------------------------------------------------------------ the counting route
def arc_matrix(rp, ci, B, n, fault=None):
    """0/1 CSR matrix of the arcs that count (row i holds N(i)), a set."""
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)[:rp[-1]]
    R = B * n
    rows = np.repeat(np.arange(R, dtype=np.int64), np.diff(rp))
    base = rows // n * n
    lc = ci - base
    if fault == "next_block_counted":
        ok = (lc >= 0) & (lc < 2 * n) & (ci < R)
        lc = lc % n
    else:
        ok = (lc >= 0) & (lc < n)
    if fault != "diagonal_counted":
        ok &= lc != rows - base
    A = sp.csr_matrix((np.ones(int(ok.sum()), np.int64), (rows[ok], (base + lc)[ok])), shape=(R, R))
    A.sum_duplicates()
    A.data[:] = 1
    return A


def _k4(M):
    """4-cliques of the symmetric 0/1 matrix M: the triangles among the higher neighbours of
    every node (each clique at its smallest node)."""
    M = M.tocsr()
    U = sp.triu(M, k=1).tocsr()
    total = 0
    for u in np.nonzero(np.diff(U.indptr) >= 3)[0]:
        nb = U.indices[U.indptr[u]:U.indptr[u + 1]]
        S = M[nb][:, nb]
        if len(nb) <= 2048:
            S = S.toarray().astype(np.float64)              # counts < 2^53: exact
            total += int(round(((S @ S) * S).sum())) // 6
        else:
            total += int((S @ S).multiply(S).sum()) // 6
    return total


def route_graph(M, fault=None):
    """census[:9] of one graph from its symmetric 0/1 matrix M by the header's route."""
    M = M.tocsr().astype(np.int64)
    d = np.asarray(M.sum(axis=1)).ravel().astype(np.int64)
    C = (M @ M).tocsr()                                     # c(u, w); the diagonal holds d
    t = C.multiply(M).tocsr()                               # t(u, v) on the edges
    T = int(t.sum()) // 6
    tv = np.asarray(t.sum(axis=1)).ravel().astype(np.int64) // 2
    E = int(d.sum()) // 2
    W = int((d * (d - 1) // 2).sum())
    S3p = int((d * (d - 1) * (d - 2) // 6).sum())
    P3p = int((d - 1) @ (M @ (d - 1))) // 2 - 3 * T
    TTp = int((tv * (d - 2)).sum())
    cu = sp.triu(C, k=1).data.astype(np.int64)
    C4p = int((cu * (cu - 1) // 2).sum()) // 2
    tu = sp.triu(t, k=1).data.astype(np.int64)
    Dp = int((tu * (tu - 1) // 2).sum())
    K4 = _k4(M)
    D = Dp - (5 if fault == "conversion_constant" else 6) * K4
    C4 = C4p - D - 3 * K4
    TT = TTp - 4 * D - 12 * K4
    S3 = S3p - TT - 2 * D - 4 * K4
    P3 = P3p - 2 * TT - 4 * C4 - 6 * D - 12 * K4
    return np.array([E, W - 3 * T, T, P3, S3, C4, TT, D, K4], np.int64)


def route_census(rp, ci, B, n, fault=None):
    """[B, 10] by the counting route: mutual-edge rule, nine counts, one-way arcs."""
    A = arc_matrix(rp, ci, B, n, fault)
    M = (A + A.T if fault == "one_way_counted" else A.multiply(A.T)).tocsr()
    M.data[:] = 1
    out = np.zeros((B, 10), np.int64)
    for g in range(B):
        s = slice(g * n, (g + 1) * n)
        Mg = M[s][:, s]
        out[g, :9] = route_graph(Mg, fault)
        out[g, 9] = int(A[s].nnz) - int(A[s].multiply(A.T[s]).nnz)
    return out


def work(rp, ci, B, n):
    """work[b] = sum_i 9 l_i + 4 a_i + c_i (the header's formula; duplicates count)."""
    rp = np.asarray(rp, np.int64)
    ln = np.diff(rp)
    rows, lc = G.valid_entries(rp, ci, B, n)
    lj = ln[rows // n * n + lc]
    per = 4 * lj + np.where(lc > rows % n, lj * np.minimum(ln[rows], lj), 0)
    out = np.zeros(B, np.int64)
    np.add.at(out, rows // n, per)
    out += 9 * ln.reshape(B, n).sum(axis=1)
    return out


def reference(c, work_cap=None):
    """(census [B, 10], work [B]) of a case; graphs with work > work_cap are -1."""
    key = (c.name, "full")
    if key not in _ref_cache:
        _ref_cache[key] = (route_census(c.rp, c.ci, c.B, c.n), work(c.rp, c.ci, c.B, c.n))
    cen, wk = _ref_cache[key]
    cen = cen.copy()
    if work_cap is not None:
        cen[wk > work_cap] = -1
    return cen, wk.copy()


_ref_cache = {}


def assert_census(got_census, got_work, want_census, want_work, what=""):
    g, w = np.asarray(got_work, np.int64), np.asarray(want_work, np.int64)
    bad = np.nonzero(g != w)[0]
    assert not len(bad), f"{what} work: graph {int(bad[0])} got {int(g[bad[0]])} want {int(w[bad[0]])}"
    g, w = np.asarray(got_census, np.int64), np.asarray(want_census, np.int64)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    if len(bad):
        b, k = (int(x) for x in bad[0])
        raise AssertionError(f"{what} census: graph {b} {NAMES[k]} got {int(g[b, k])} want {int(w[b, k])} "
                             f"({len(bad)} entries differ; got row {g[b].tolist()} want {w[b].tolist()})")


# ------------------------------------------------------------------ graphs
def random_csr(B, n, p, seed, extras=True):
    """G(n, p) per graph, both directions, plus (``extras``) self loops, out-of-block entries and
    one-way arcs; rows shuffled."""
    rng = np.random.default_rng(seed)
    pairs, extra = [], []
    for b in range(B):
        up = np.triu(rng.random((n, n)) < p, k=1)
        i, j = np.nonzero(up)
        pairs += [(b * n + int(x), b * n + int(y)) for x, y in zip(i, j)]
        if extras and n >= 2:
            for _ in range(max(1, n // 3)):
                x, y = (int(v) for v in rng.choice(n, size=2, replace=False))
                if not up[min(x, y), max(x, y)]:
                    extra.append((b * n + x, b * n + y))                  # a one-way arc
            extra += [(b * n + int(x), b * n + int(x)) for x in rng.choice(n, size=max(1, n // 4), replace=False)]
            if B > 1:
                extra.append((b * n + int(rng.integers(n)), ((b + 1) % B) * n + int(rng.integers(n))))
    return G.csr_from_pairs(pairs, B, n, shuffle_seed=seed + 1, extra=sorted(set(extra)))


def _complete(n, base=0):
    return [(base + i, base + j) for i in range(n) for j in range(i + 1, n)]


def _sparse_pairs(n, mean_degree, seed):
    return G.random_pairs(1, n, mean_degree, seed)


# The smallest shapes at which the kernels can go wrong: one to four nodes, the complete graphs
# whose counts are binomials, the 32-bit mask word and the 64-entry load step from below and
# above, rows longer than 64 and 255 entries, several workgroups per graph, the LDS-layout
# threshold (four waves per workgroup up to n = 7280, one above), the largest n, 70 graphs.
CASES = ("n1", "n2", "n3", "k4", "k5", "empty", "ring50", "path50", "lattice12", "star200", "deg300", "k40",
         "r33", "r64", "r65", "r257", "n7279", "n7280", "n7281", "n16384", "b70_mixed", "unsorted", "injected",
         "one_way", "duplicates", "isolated", "k200_middle", "cap0")


def build_case(name):
    if name in _case_cache:
        return _case_cache[name]
    C, csr = G.Case, G.csr_from_pairs
    if name == "n1":
        c = C(name, 2, 1, *csr([], 2, 1, extra=[(0, 0), (1, 0)]))
    elif name == "n2":
        c = C(name, 3, 2, *csr([(0, 1)], 3, 2, extra=[(2, 3)]))              # an edge, a one-way arc, nothing
    elif name == "n3":
        c = C(name, 2, 3, *csr([(0, 1), (1, 2), (0, 2), (3, 4), (4, 5)], 2, 3))   # a triangle and a 2-path
    elif name in ("k4", "k5", "k40"):
        n = int(name[1:])
        c = C(name, 1, n, *csr(_complete(n), 1, n, shuffle_seed=n))
    elif name == "empty":
        c = C(name, 2, 10, *csr([], 2, 10))
    elif name == "ring50":
        c = C(name, 1, 50, *csr([(i, (i + 1) % 50) for i in range(50)], 1, 50))
    elif name == "path50":
        c = C(name, 1, 50, *csr([(i, i + 1) for i in range(49)], 1, 50))
    elif name == "lattice12":
        k = 12
        p = [(r * k + q, r * k + q + 1) for r in range(k) for q in range(k - 1)]
        p += [(r * k + q, (r + 1) * k + q) for r in range(k - 1) for q in range(k)]
        c = C(name, 1, k * k, *csr(p, 1, k * k, shuffle_seed=12))
    elif name == "star200":
        c = C(name, 1, 200, *csr([(0, j) for j in range(1, 200)], 1, 200, shuffle_seed=7))
    elif name == "deg300":
        g = G.build_case("deg300")
        c = C(name, g.B, g.n, np.array(g.rp), np.array(g.ci))
    elif name in ("r33", "r64", "r65", "r257"):
        n = int(name[1:])
        B, p = {33: (3, 0.3), 64: (2, 0.2), 65: (2, 0.2), 257: (1, 0.05)}[n]
        c = C(name, B, n, *random_csr(B, n, p, 500 + n))
    elif name in ("n7279", "n7280", "n7281"):
        n = int(name[1:])
        c = C(name, 1, n, *csr(_sparse_pairs(n, 5.0, n), 1, n, shuffle_seed=n + 1))
    elif name == "n16384":
        n = MAX_N
        rng = np.random.default_rng(16384)
        p = [(i, (i + 1) % n) for i in range(n)] + [(i, (i + 2) % n) for i in range(0, n, 3)]
        ch = rng.integers(0, n, (3000, 2))
        p += [(int(x), int(y)) for x, y in ch if abs(int(x) - int(y)) > 2]
        p = np.unique(np.sort(np.asarray(p, np.int64), axis=1), axis=0)
        c = C(name, 1, n, *csr(p, 1, n, shuffle_seed=5))
    elif name == "b70_mixed":
        B, n = 70, 20
        parts = []
        for b in range(B):
            kind = b % 5
            if kind == 0:
                pr = _complete(n)
            elif kind == 1:
                pr = [(i, (i + 1) % n) for i in range(n)]
            elif kind == 2:
                pr = []
            else:
                up = np.triu(np.random.default_rng(700 + b).random((n, n)) < (0.15 if kind == 3 else 0.6), k=1)
                pr = list(zip(*(x.tolist() for x in np.nonzero(up))))
            parts += [(b * n + i, b * n + j) for i, j in pr]
        c = C(name, B, n, *csr(parts, B, n, shuffle_seed=70, extra=G._injected(B, n, 71)))
    elif name == "unsorted":
        c = C(name, 2, 100, *random_csr(2, 100, 0.15, 900, extras=False))
        assert any(np.any(np.diff(c.ci[s:e]) < 0) for s, e in zip(c.rp[:-1], c.rp[1:]))
    elif name == "injected":
        B, n = 3, 33
        c = C(name, B, n, *csr(G.random_pairs(B, n, 6.0, 910), B, n, shuffle_seed=911, extra=G._injected(B, n, 912)))
    elif name == "one_way":
        c = C(name, 2, 40, *random_csr(2, 40, 0.25, 920))
    elif name == "duplicates":                                               # the first occurrence counts
        pr = G.random_pairs(2, 50, 8.0, 940)
        extra = [(int(i), int(j)) for i, j in pr[:60]] + [(int(j), int(i)) for i, j in pr[:30]]
        extra += [(int(i), int(j)) for i, j in pr[:15]] + [(3, 4), (3, 4), (60, 61), (60, 61)]
        c = C(name, 2, 50, *csr(pr, 2, 50, shuffle_seed=941, extra=extra))
        assert any(len(set(c.ci[s:e].tolist())) < e - s for s, e in zip(c.rp[:-1], c.rp[1:]))
    elif name == "isolated":
        n = 300
        c = C(name, 1, n, *csr([(30 * i, 30 * j) for i in range(10) for j in range(i + 1, 10) if (i + j) % 3], 1, n))
    elif name == "k200_middle":
        n = 200
        p = np.concatenate([G.random_pairs(1, n, 6.0, 930), np.asarray(_complete(n, n)),
                            G.random_pairs(1, n, 6.0, 931) + 2 * n])
        c = C(name, 3, n, *csr(p, 3, n, shuffle_seed=932))
    elif name == "cap0":
        n = 10
        c = C(name, 3, n, *csr(_complete(4) + _complete(5, 2 * n), 3, n))
    else:
        raise KeyError(name)
    _case_cache[name] = c
    return c


_case_cache = {}


def case_work_cap(name):
    """The work_cap a case runs with (None: none of its graphs may be skipped)."""
    c = build_case(name)
    if name == "k200_middle":
        wk = work(c.rp, c.ci, c.B, c.n)
        assert max(wk[0], wk[2]) < wk[1]
        return int(max(wk[0], wk[2]) + wk[1]) // 2
    if name == "cap0":
        return 0
    return None


def known_counts(name):
    """Closed forms the reference itself must give: {graph: {NAMES entry: value}}."""
    if name in ("k4", "k5", "k40"):
        n = int(name[1:])
        return {0: {"E": comb(n, 2), "T": comb(n, 3), "K4": comb(n, 4), "P2": 0, "P3": 0, "S3": 0, "C4": 0,
                    "TT": 0, "D": 0}}
    if name == "lattice12":
        return {0: {"C4": 121, "T": 0, "E": 264, "K4": 0, "D": 0, "TT": 0}}
    if name == "star200":
        return {0: {"S3": comb(199, 3), "P2": comb(199, 2), "E": 199, "T": 0, "P3": 0}}
    if name == "ring50":
        return {0: {"E": 50, "P2": 50, "P3": 50, "T": 0, "C4": 0, "S3": 0}}
    if name == "path50":
        return {0: {"E": 49, "P2": 48, "P3": 47, "T": 0, "C4": 0, "S3": 0}}
    if name == "k200_middle":
        return {1: {"K4": comb(200, 4), "T": comb(200, 3), "E": comb(200, 2)}}
    return {}
