"""Reference of snd_graph_paths (include/snd_vae.h), plain NumPy + scipy: importable without a
GPU.  It reuses the edge rule (``neighbour_matrix``), ``csr_from_pairs``, ``random_pairs`` and
``Case`` of tests/graph_stats_ref.py.

* ``reference``: the float64 side.  comp from ``connected_components(directed=False)`` relabelled
  to the smallest member, hops from ``shortest_path(unweighted=True)``, routes from ``dijkstra``
  with predecessors on float64 lengths of the fp32 coordinates.
* ``emulate``: the kernel's fixed point in float32, d[s] = 0, d[v] = min_u fl(d[u] + len(u, v)),
  len formed in float32 as the kernel forms it (difference, square, sum in coordinate order,
  square root, each rounded once).  Bellman-Ford over all sources at once, the arcs relaxed in a
  chosen order; ``dijkstra32`` is the float32 Dijkstra with predecessors of one source.  The
  two are bitwise equal whatever the order (tests/test_graph_paths_cpu.py): fl(. + w) is
  monotone and w >= 0, so the least fixed point is unique.  ``emulate`` is also the vehicle of
  the planted FAULTS.

The route bound (derived, not measured).  u = 2^-24.  An edge length in fp32 is
sqrt(sum_k fl(fl(x_k - y_k)^2)): the difference carries u, its square 2u + u, the sum of up to
three squares 2u more, the square root halves that and adds u: <= 3.5 u relative.  A sum of K
such lengths, added one at a time, carries at most (K - 1) u more.  So along ANY path of K
edges, |fl-length - true length| <= (K + 2.5) u (1 + O(K u)) true length.
Now route32 <= fl-length of the float64-optimal path (K64 edges) <= route64 (1 + (K64 + 2.5) u),
and route32 is the fl-length of an fp32-optimal path (K32 edges) whose true length is >=
route64, so route32 >= route64 (1 - (K32 + 2.5) u).  With K = max(K64, K32):

    |route32 - route64| <= (K + 6) 2^-23 route64          (ROUTE_SLACK = 6, twice over the need)

K64 is read off scipy's predecessors; K32 is the fewest edges of a path that is tight in fp32
(d[v] == fl(d[u] + len) bitwise along it), the one that gives the smallest valid bound.

The histogram rule.  The detour bin value is v = (route / e - 1) scale.  In fp32 e carries 3.5 u,
the quotient u, the subtraction u of the quotient, the scaling u: the value the kernel floors is
within m = scale (route64 / e64) (K + 10) 2^-23 of v64.  A pair is AMBIGUOUS when floor(v64 - m)
and floor(v64 + m), both clamped to [0, 255], differ: v64 within m of an integer >= 1 (values
near 0 clamp to bin 0 either way, values past 255 to bin 255).  The comparison is an envelope:
for every graph and bin, definite <= got <= definite + ambiguous-that-could-land-there, and each
row sums to its pair count exactly.  CONDITION, asserted on the CPU before any launch
(``reference``): at most 1 % of a case's pairs are ambiguous (AMBIGUOUS_CAP).  The hop
histogram, comp, hops and totals are integers and compared exactly.
"""
from __future__ import annotations

import heapq

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components, dijkstra, shortest_path

import graph_stats_ref as G

BINS = 256
ROUTE_SLACK = 6
BIN_SLACK = 10
EPS23 = 2.0 ** -23
AMBIGUOUS_CAP = 0.01
DETOUR_SCALE = np.float32(64.0)
NAMES = ("hops", "detour")

FAULTS = ("bfs_stops_at_64", "self_loop_followed", "next_block_followed", "source_counted",
          "unreachable_binned", "one_sweep_only", "weighted_path_hops", "detour_without_minus_one",
          "components_directed_only")


def sources(n, src_step):
    return np.arange(0, n, src_step, dtype=np.int64)


# ------------------------------------------------------------------ arcs
def graph_arcs(rp, ci, B, n, g, fault=None):
    """(u, v) local ids of graph g's arcs after the edge rule, in CSR order (duplicates kept:
    they change nothing)."""
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    lo, hi = rp[g * n], rp[(g + 1) * n]
    rows = np.repeat(np.arange(g * n, (g + 1) * n, dtype=np.int64), np.diff(rp[g * n:(g + 1) * n + 1]))
    c = ci[lo:hi]
    if fault == "bfs_stops_at_64":
        pos = np.arange(lo, hi) - rp[rows]
        rows, c = rows[pos < 64], c[pos < 64]
    lc = c - g * n
    if fault == "next_block_followed":
        ok = (lc >= 0) & (lc < 2 * n) & (c < B * n)
        lc = lc % n
    else:
        ok = (lc >= 0) & (lc < n)
    ok &= lc != rows - g * n
    return (rows - g * n)[ok], lc[ok]


def self_loops(rp, ci, n, g):
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(g * n, (g + 1) * n, dtype=np.int64), np.diff(rp[g * n:(g + 1) * n + 1]))
    c = np.asarray(ci, np.int64)[rp[g * n]:rp[(g + 1) * n]]
    return np.unique(rows[c == rows]) - g * n


def lengths32(x, u, v):
    """The kernel's edge length: float32, one rounding per operation, coordinates in order."""
    x = np.asarray(x, np.float32)
    s = np.zeros(len(u), np.float32)
    for k in range(x.shape[1]):
        d = x[u, k] - x[v, k]
        s = s + d * d
    return np.sqrt(s)


def lengths64(x, u, v):
    x = np.asarray(x, np.float32).astype(np.float64)
    d = x[u] - x[v]
    return np.sqrt((d * d).sum(axis=1))


# ------------------------------------------------------------------ float32 fixed point
def _sorted_by_target(u, v, idx):
    order = np.argsort(v[idx], kind="stable")
    return u[idx][order], v[idx][order], idx[order]


def _relax_min(d, vs, cand):
    """d[t] = min(d[t], min of the candidates of t) for [n, S] arrays; ``vs`` (ascending) names
    each candidate row's target.  Returns the targets at which anything fell."""
    if not len(vs):
        return vs
    starts = np.nonzero(np.r_[True, vs[1:] != vs[:-1]])[0]
    best = np.minimum.reduceat(cand, starts, axis=0)
    tg = vs[starts]
    old = d[tg]
    new = np.minimum(old, best)
    d[tg] = new
    return tg[(new < old).any(axis=1)]


def bellman_ford32(n, u, v, w, src, order_seed=None, chunks=1, max_sweeps=None):
    """Least fixed point of d[s] = 0, d[v] = min fl(d[u] + w) in float32 for every source of
    ``src``: [S, n].  The arcs are permuted by ``order_seed`` and relaxed in ``chunks`` groups
    one after the other within a sweep (1: Jacobi, and only the arcs out of nodes that fell in
    the sweep before are looked at, which changes no value)."""
    S = len(src)
    d = np.full((n, S), np.inf, np.float32)
    d[src, np.arange(S)] = 0.0
    perm = np.arange(len(u)) if order_seed is None else np.random.default_rng(order_seed).permutation(len(u))
    parts = [_sorted_by_target(u, v, p) for p in np.array_split(perm, chunks)]
    active = np.zeros(n, bool)
    active[src] = True
    sweeps = 0
    while True:
        fell = np.zeros(n, bool)
        for us, vs, idx in parts:
            m = active[us] if chunks == 1 else np.ones(len(us), bool)
            cand = (d[us[m]] + w[idx[m]][:, None]).astype(np.float32)
            fell[_relax_min(d, vs[m], cand)] = True
        sweeps += 1
        if not fell.any() or (max_sweeps is not None and sweeps >= max_sweeps):
            return np.ascontiguousarray(d.T)
        active = fell


def tight_edge_count(n, u, v, w, src, d):
    """Fewest edges of a path from the source that is tight in float32: [S, n] (0 at the source,
    -1 where unreachable)."""
    S = len(src)
    big = np.int64(1) << 40
    k = np.full((n, S), big, np.int64)
    k[src, np.arange(S)] = 0
    us, vs, idx = _sorted_by_target(u, v, np.arange(len(u)))
    dT = np.ascontiguousarray(d.T)
    active = np.zeros(n, bool)
    active[src] = True
    while active.any():
        m = active[us]
        a, b, e = us[m], vs[m], idx[m]
        tight = ((dT[a] + w[e][:, None]).astype(np.float32) == dT[b]) & np.isfinite(dT[b])
        fell = _relax_min(k, b, np.where(tight, k[a] + 1, big))
        active = np.zeros(n, bool)
        active[fell] = True
    return np.ascontiguousarray(np.where(k >= big, -1, k).T)


def dijkstra32(n, u, v, w, s):
    """Float32 Dijkstra of one source with predecessors: (d [n] float32, edges [n] of the path it
    found, -1 where unreachable)."""
    adj = [[] for _ in range(n)]
    for a, b, x in zip(u.tolist(), v.tolist(), w):
        adj[a].append((b, np.float32(x)))
    d = np.full(n, np.inf, np.float32)
    pred = np.full(n, -1, np.int64)
    d[s] = 0.0
    done = np.zeros(n, bool)
    heap = [(np.float32(0.0), int(s))]
    while heap:
        du, a = heapq.heappop(heap)
        if done[a]:
            continue
        done[a] = True
        for b, x in adj[a]:
            c = np.float32(du + x)
            if c < d[b]:
                d[b], pred[b] = c, a
                heapq.heappush(heap, (c, b))
    edges = np.full(n, -1, np.int64)
    edges[s] = 0
    for t in range(n):
        chain = []
        while edges[t] < 0 and pred[t] >= 0:
            chain.append(t)
            t = pred[t]
        for back in reversed(chain):
            edges[back] = edges[pred[back]] + 1
    return d, edges


def bfs_hops(n, u, v, src):
    """[S, n] arc counts from every source, -1 where unreachable."""
    S = len(src)
    A = sp.csr_matrix((np.ones(len(u), np.int64), (u, v)), shape=(n, n))
    hops = np.full((S, n), -1, np.int64)
    hops[np.arange(S), src] = 0
    front = sp.csr_matrix((np.ones(S, np.int64), (np.arange(S), src)), shape=(S, n))
    level = 0
    while front.nnz:
        level += 1
        nxt = (front @ A).tocoo()
        new = hops[nxt.row, nxt.col] < 0
        r, c = nxt.row[new], nxt.col[new]
        hops[r, c] = level
        front = sp.csr_matrix((np.ones(len(r), np.int64), (r, c)), shape=(S, n))
        front.sum_duplicates()
    return hops


def min_labels(n, u, v, directed_only=False):
    """Smallest node id that reaches each node by label propagation: both ways along every arc
    (weak components), or row -> column only (the planted fault)."""
    lab = np.arange(n, dtype=np.int64)
    if not directed_only:
        u, v = np.r_[u, v], np.r_[v, u]
    while len(u):
        new = lab.copy()
        np.minimum.at(new, v, lab[u])
        if np.array_equal(new, lab):
            break
        lab = new
    return lab


# ------------------------------------------------------------------ bins
def detour_bins(route, e, scale, minus_one=True):
    """min(max(floor((route / e - 1) scale), 0), 255) in the precision of the operands."""
    one = route.dtype.type(1.0 if minus_one else 0.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        val = (route / e - one) * route.dtype.type(scale)
    return np.clip(np.floor(np.nan_to_num(val, nan=0.0, posinf=1e30)), 0, BINS - 1).astype(np.int64)


def emulate(c, coords=None, scale=None, src_step=1, fault=None, order_seed=None, chunks=1):
    """snd_graph_paths in the kernel's arithmetic: {"comp" [R], "hops" [B n_src, n] int64, "route"
    [B n_src, n] float32 (None without coords), "hist" [B, 2, 256], "totals" [B, 6], "k32"}.
    ``fault`` plants one of FAULTS."""
    assert fault is None or fault in FAULTS, fault
    B, n = c.B, c.n
    src = sources(n, src_step)
    S = len(src)
    x = None if coords is None else np.asarray(coords, np.float32)
    comp = np.zeros(B * n, np.int64)
    hops = np.zeros((B * S, n), np.int64)
    route = None if x is None else np.zeros((B * S, n), np.float32)
    k32 = None if x is None else np.zeros((B * S, n), np.int64)
    hist = np.zeros((B, 2, BINS), np.int64)
    totals = np.zeros((B, 6), np.int64)
    for g in range(B):
        u, v = graph_arcs(c.rp, c.ci, B, n, g, fault)
        lab = min_labels(n, u, v, fault == "components_directed_only")
        comp[g * n:(g + 1) * n] = lab
        sizes = np.bincount(lab, minlength=n)
        h = bfs_hops(n, u, v, src)
        d = k = None
        if x is not None:
            w = lengths32(x[g * n:(g + 1) * n], u, v)
            d = bellman_ford32(n, u, v, w, src, order_seed, chunks, 1 if fault == "one_sweep_only" else None)
            k = tight_edge_count(n, u, v, w, src, d)
            route[g * S:(g + 1) * S], k32[g * S:(g + 1) * S] = d, k
            if fault == "weighted_path_hops":
                h = k.copy()
        pair = h >= 0
        pair[np.arange(S), src] = fault == "source_counted"
        if fault == "self_loop_followed":          # loops are inert for BFS and relaxation (both are
            loops = np.intersect1d(self_loops(c.rp, c.ci, n, g), src)     # idempotent); what following
            at = np.searchsorted(src, loops)                              # one adds is the closed walk
            h[at, loops] = 1                                              # s -> s of one arc
            pair[at, loops] = True
        hops[g * S:(g + 1) * S] = h
        hb = np.minimum(h[pair], BINS - 1)
        if fault == "unreachable_binned":
            hb = np.r_[hb, np.full(int((h < 0).sum()), BINS - 1, np.int64)]
        hist[g, 0] = np.bincount(hb, minlength=BINS)
        totals[g] = [int((lab == np.arange(n)).sum()), int(sizes.max()), S, int(pair.sum()), int(h[pair].sum()),
                     int(h[pair].max()) if pair.any() else 0]
        if x is not None:
            si, ti = np.nonzero(pair)
            e = lengths32(x[g * n:(g + 1) * n], src[si], ti)
            keep = e > 0
            b = detour_bins(d[si, ti][keep], e[keep], np.float32(scale), fault != "detour_without_minus_one")
            hist[g, 1] = np.bincount(b, minlength=BINS)
    return {"comp": comp, "hops": hops, "route": route, "hist": hist, "totals": totals, "k32": k32}


# ------------------------------------------------------------------ float64 reference
def _path_edges(pred, src):
    """Edge counts along scipy's predecessor chains, by pointer doubling: [S, n], 0 at the
    source, -1 unreachable."""
    S, n = pred.shape
    ok = pred >= 0
    anc = np.where(ok, pred, np.arange(n)[None, :])
    k = ok.astype(np.int64)
    for _ in range(max(1, int(n).bit_length())):
        k = k + np.take_along_axis(k, anc, axis=1)
        anc = np.take_along_axis(anc, anc, axis=1)
    return np.where(ok | (np.arange(n)[None, :] == src[:, None]), k, -1)


_ref_cache = {}


def reference(c, coords=None, scale=None, src_step=1):
    """The float64 reference of case ``c`` with its bounds and envelope (cached):
    comp, hops, totals, hist_lo / hist_amb [B, 2, 256], and with coords route (float64), bound
    (the per-element route bound), pairs1 [B] (pairs with e > 0), ambiguous_share."""
    key = (c.name, None if coords is None else (coords.shape[1], float(scale)), src_step)
    if key in _ref_cache:
        return _ref_cache[key]
    B, n = c.B, c.n
    src = sources(n, src_step)
    S = len(src)
    x = None if coords is None else np.asarray(coords, np.float32)
    emu = emulate(c, x, scale, src_step) if x is not None else None
    A = G.neighbour_matrix(c.rp, c.ci, B, n)
    out = {"comp": np.zeros(B * n, np.int64), "hops": np.zeros((B * S, n), np.int64), "route": None,
           "bound": None, "hist_lo": np.zeros((B, 2, BINS), np.int64), "hist_amb": np.zeros((B, 2, BINS), np.int64),
           "totals": np.zeros((B, 6), np.int64), "pairs1": np.zeros(B, np.int64), "ambiguous_share": 0.0,
           "src": src, "n_src": S}
    if x is not None:
        out["route"] = np.zeros((B * S, n))
        out["bound"] = np.zeros((B * S, n))
    ambiguous = 0
    for g in range(B):
        Ag = A[g * n:(g + 1) * n, g * n:(g + 1) * n].tocsr()
        ncomp, lab = connected_components(Ag, directed=False)
        first = np.full(ncomp, n, np.int64)
        np.minimum.at(first, lab, np.arange(n))
        out["comp"][g * n:(g + 1) * n] = first[lab]
        h = shortest_path(Ag, unweighted=True, directed=True, indices=src)
        h = np.where(np.isfinite(h), h, -1).astype(np.int64).reshape(S, n)
        out["hops"][g * S:(g + 1) * S] = h
        pair = h >= 0
        pair[np.arange(S), src] = False
        out["hist_lo"][g, 0] = np.bincount(np.minimum(h[pair], BINS - 1), minlength=BINS)
        out["totals"][g] = [ncomp, int(np.bincount(lab).max()), S, int(pair.sum()), int(h[pair].sum()),
                            int(h[pair].max()) if pair.any() else 0]
        if x is None:
            continue
        xg = x[g * n:(g + 1) * n]
        coo = Ag.tocoo()
        W = sp.csr_matrix((lengths64(xg, coo.row, coo.col), (coo.row, coo.col)), shape=(n, n))   # zeros stay edges
        r64, pred = dijkstra(W, directed=True, indices=src, return_predecessors=True)
        r64, pred = r64.reshape(S, n), pred.reshape(S, n)
        K = np.maximum(_path_edges(pred, src), emu["k32"][g * S:(g + 1) * S])
        out["route"][g * S:(g + 1) * S] = r64
        with np.errstate(invalid="ignore"):
            out["bound"][g * S:(g + 1) * S] = np.where(np.isfinite(r64), (K + ROUTE_SLACK) * EPS23 * r64, 0.0)
        si, ti = np.nonzero(pair)
        e = lengths64(xg, src[si], ti)
        keep = e > 0
        si, ti, e = si[keep], ti[keep], e[keep]
        out["pairs1"][g] = len(e)
        ratio = r64[si, ti] / e
        v = (ratio - 1.0) * float(np.float32(scale))
        m = float(np.float32(scale)) * ratio * (K[si, ti] + BIN_SLACK) * EPS23
        lo = np.clip(np.floor(v - m), 0, BINS - 1).astype(np.int64)
        hi = np.clip(np.floor(v + m), 0, BINS - 1).astype(np.int64)
        sure = lo == hi
        out["hist_lo"][g, 1] = np.bincount(lo[sure], minlength=BINS)
        for a, b in zip(lo[~sure], hi[~sure]):
            out["hist_amb"][g, 1, a:b + 1] += 1
        ambiguous += int((~sure).sum())
    if x is not None:
        total = int(out["pairs1"].sum())
        out["ambiguous_share"] = ambiguous / total if total else 0.0
        assert ambiguous <= AMBIGUOUS_CAP * total, (c.name, ambiguous, total)
    _ref_cache[key] = out
    return out


def assert_paths(got, ref, n, what=""):
    """comp, hops and totals exactly; route within the bound per element and inf exactly where
    unreachable; hist under the envelope rule.  ``got`` entries may be None (not asked for).  A
    failure names the element, or the graph and bin.  Returns the worst route err / bound."""
    S = ref["n_src"]
    if got.get("comp") is not None:
        g_, w_ = np.asarray(got["comp"], np.int64), ref["comp"]
        bad = np.nonzero(g_ != w_)[0]
        if len(bad):
            i = int(bad[0])
            raise AssertionError(f"{what} comp: element {i} (graph {i // n}, node {i % n}) got {int(g_[i])} want "
                                 f"{int(w_[i])} ({len(bad)} differ)")
    if got.get("hops") is not None:
        g_, w_ = np.asarray(got["hops"], np.int64).reshape(-1, n), ref["hops"]
        bad = np.argwhere(g_ != w_)
        if len(bad):
            r, t = (int(k) for k in bad[0])
            raise AssertionError(f"{what} hops: element ({r}, {t}) (graph {r // S}, source {int(ref['src'][r % S])}, "
                                 f"target {t}) got {int(g_[r, t])} want {int(w_[r, t])} ({len(bad)} differ)")
    worst = 0.0
    if got.get("route") is not None:
        g_ = np.asarray(got["route"], np.float32).reshape(-1, n).astype(np.float64)
        w_ = ref["route"]
        unreach = ~np.isfinite(w_)
        with np.errstate(invalid="ignore"):
            err = np.where(unreach, 0.0, np.abs(g_ - w_))
        bad = np.argwhere((unreach & ~(np.isinf(g_) & (g_ > 0))) | (~unreach & ~(err <= ref["bound"])))
        if len(bad):
            r, t = (int(k) for k in bad[0])
            raise AssertionError(f"{what} route: element ({r}, {t}) (graph {r // S}, source {int(ref['src'][r % S])}, "
                                 f"target {t}) got {g_[r, t]!r} want {w_[r, t]!r} +- {ref['bound'][r, t]:.3e} "
                                 f"({len(bad)} differ)")
        pos = ref["bound"] > 0
        worst = float((err[pos] / ref["bound"][pos]).max()) if pos.any() else 0.0
    g_ = np.asarray(got["hist"], np.int64)
    lo, hi = ref["hist_lo"], ref["hist_lo"] + ref["hist_amb"]
    assert g_.shape == lo.shape, (what, g_.shape, lo.shape)
    bad = np.argwhere((g_ < lo) | (g_ > hi))
    if len(bad):
        b, r, k = (int(t) for t in bad[0])
        raise AssertionError(f"{what} hist: graph {b} {NAMES[r]} bin {k} got {int(g_[b, r, k])} want "
                             f"[{int(lo[b, r, k])}, {int(hi[b, r, k])}] ({len(bad)} bins differ)")
    sums = g_.sum(axis=2)
    want = np.stack([ref["totals"][:, 3], ref["pairs1"]], axis=1)
    bad = np.argwhere(sums != want)
    if len(bad):
        b, r = (int(t) for t in bad[0])
        raise AssertionError(f"{what} hist: graph {b} {NAMES[r]} bin sum got {int(sums[b, r])} want {int(want[b, r])}")
    g_, w_ = np.asarray(got["totals"], np.int64), ref["totals"]
    bad = np.argwhere(g_ != w_)
    if len(bad):
        b, k = (int(t) for t in bad[0])
        raise AssertionError(f"{what} totals: graph {b} element {k} got {int(g_[b, k])} want {int(w_[b, k])}")
    return worst


# ------------------------------------------------------------------ graphs
def rgg(B, n, mean_degree, seed, sd=2):
    """Random geometric graphs in the unit box: (undirected global pairs, fp32 coords [B n, sd]).
    The radius gives the mean degree away from the border."""
    from scipy.spatial import cKDTree
    from math import gamma, pi
    rng = np.random.default_rng(seed)
    x = rng.random((B * n, sd)).astype(np.float32)
    ball = pi ** (sd / 2.0) / gamma(sd / 2.0 + 1.0)
    radius = (mean_degree / (max(n - 1, 1) * ball)) ** (1.0 / sd)
    out = []
    for b in range(B):
        p = cKDTree(x[b * n:(b + 1) * n].astype(np.float64)).query_pairs(radius, output_type="ndarray")
        out.append(p.astype(np.int64).reshape(-1, 2) + b * n)
    return np.concatenate(out), x


def _extras(B, n, pairs, seed):
    """Directed extras: self loops and other blocks' ids (graph_stats_ref._injected), one-way arcs
    inside a block and duplicates of entries already there."""
    rng = np.random.default_rng(seed)
    extra = list(G._injected(B, n, seed))
    have = {(int(a), int(b)) for a, b in pairs} | {(int(b), int(a)) for a, b in pairs}
    for i in rng.choice(B * n, size=max(2, B * n // 6), replace=False):
        j = int(i) // n * n + int(rng.integers(0, n))
        if j != i and (int(i), j) not in have:
            extra.append((int(i), j))                                   # one way only
    extra += [(int(a), int(b)) for a, b in pairs[::5]]                  # duplicates
    return extra


# name -> (B, n, src_step); the smallest shapes at which the kernels can go wrong: one node, one
# edge, several graphs, injected entries, rows longer than 64 and 255 entries, an empty graph,
# hops past bin 255, coincident nodes, more nodes than a wave's stride, both sides of the two n at
# which gp_paths_kernel goes from four waves per workgroup to one (1980 | 1981 with coords,
# 3960 | 3961 without), and the largest n.
CASES = {"b1n1": (1, 1, 1), "b1n2": (1, 2, 1), "b3n33": (3, 33, 1), "b2n70": (2, 70, 1), "b1n257": (1, 257, 1),
         "star200": (1, 200, 1), "deg300": (2, 300, 1), "empty_middle": (3, 33, 1), "path300": (1, 300, 1),
         "coincident": (1, 12, 1), "b2n2049": (2, 2049, 64), "n1980": (1, 1980, 400), "n1981": (1, 1981, 400),
         "n3960": (1, 3960, 800), "n3961": (1, 3961, 800), "ring16384": (1, 16384, 4096)}
SMALL = ("b1n1", "b1n2", "b3n33", "b2n70", "b1n257", "star200", "deg300", "empty_middle", "path300", "coincident")

_case_cache = {}


def build_case(name, sd=2):
    """(Case, fp32 coords [B n, sd], src_step).  Coordinates of the geometric cases are those the
    graph was drawn from (sd = 2); any other sd draws fresh ones for the same graph."""
    key = (name, sd)
    if key in _case_cache:
        return _case_cache[key]
    B, n, step = CASES[name]
    seed = 7000 + n
    x = None
    if name in ("b1n1", "b1n2", "star200", "deg300", "empty_middle"):
        c = G.build_case(name)
        c = G.Case(name, c.B, c.n, c.rp.copy(), c.ci.copy())
    elif name in ("b3n33", "b2n70"):
        pairs, x = rgg(B, n, 5.0, seed)
        c = G.Case(name, B, n, *G.csr_from_pairs(pairs, B, n, shuffle_seed=seed + 1,
                                                 extra=_extras(B, n, pairs, seed + 2)))
    elif name == "path300":
        t = np.arange(n)
        x = np.stack([t / n, 0.5 + 0.3 * np.sin(t / 7.0)], axis=1).astype(np.float32)
        c = G.Case(name, B, n, *G.csr_from_pairs([(i, i + 1) for i in range(n - 1)], B, n))
    elif name == "coincident":
        pairs, x = rgg(B, n, 4.0, seed)
        x[5] = x[2]                                                     # e(2, 5) = 0, joined by an edge
        pairs = np.unique(np.sort(np.concatenate([pairs, [(2, 5), (5, 6), (0, 2)]]), axis=1), axis=0)
        c = G.Case(name, B, n, *G.csr_from_pairs(pairs, B, n, shuffle_seed=seed + 1))
    elif name == "ring16384":
        t = np.arange(n)
        ang = 2.0 * np.pi * t / n
        x = (0.5 + 0.5 * np.stack([np.cos(ang), np.sin(ang)], axis=1)).astype(np.float32)
        pairs = [(i, (i + 1) % n) for i in range(n)] + [(i, (i + 1024) % n) for i in range(0, n, 64)]
        c = G.Case(name, B, n, *G.csr_from_pairs(np.sort(np.array(pairs), axis=1), B, n, shuffle_seed=seed + 1))
    else:                                                               # b1n257, b2n2049, n19xx, n39xx
        pairs, x = rgg(B, n, 8.0, seed)
        c = G.Case(name, B, n, *G.csr_from_pairs(pairs, B, n, shuffle_seed=seed + 1))
    if x is None or sd != 2:
        x = np.random.default_rng(seed + 10 * sd).random((B * n, sd)).astype(np.float32)
    x.setflags(write=False)
    _case_cache[key] = (c, x, step)
    return _case_cache[key]
