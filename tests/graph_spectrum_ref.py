"""Float64 reference of snd_graph_spectrum (include/snd_vae.h), plain NumPy: importable without
a GPU.  It restates the contract and keeps away from the device algorithm where it can:

- the graph is snd_graph_motifs' (``graph_motifs_ref.dense_mutual``: the rule's own words);
- M = L - I is formed densely; exact moments come from ``numpy.linalg.eigvalsh`` as
  sum_i cos(k arccos(lambda_i)), not from a recurrence;
- probe-mode moments come from the plain three-term recurrence, one moment per application of
  M (no doubling), with the Philox signs of ``oracle/ref_rng.philox4x32_10``;
- ``doubled_moments`` is the device's route (doubling identities), held to the two above by
  tests/test_graph_spectrum_cpu.py.

It also holds the closed-form spectra of L of the named graphs and the GPU cases.
"""
from __future__ import annotations

import numpy as np

import graph_motifs_ref as M
import graph_stats_ref as G
from oracle import ref_rng

MAX_N = 16384                           # kGsMaxN
MAX_MOMENTS = 512                       # kGsMaxMoments
WIDTH = 32                              # kGsWidth: probe columns per block
LDS_MAX_N = 64                          # kGsLdsMaxN
PHILOX_TAG = 0x53504543
FORCE_GLOBAL = 1                        # SND_SPECTRUM_FORCE_GLOBAL


# ------------------------------------------------------------------ the operator
def operator(c, g):
    """(M [n, n] float64, info [4] without the probes) of graph g of case c: M = -D^-1/2 A D^-1/2
    on the mutual-edge graph, M_ii = -1 for an isolated node."""
    A, one_way = M.dense_mutual(c.rp, c.ci, c.B, c.n, g)
    A = A.astype(np.float64)
    d = A.sum(axis=1)
    s = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    Mm = -(s[:, None] * A * s[None, :])
    iso = d == 0
    Mm[iso, iso] = -1.0
    return Mm, np.array([int(A.sum()) // 2, int(iso.sum()), one_way], np.int64)


def info(c, n_probes=0):
    out = np.zeros((c.B, 4), np.int64)
    for g in range(c.B):
        out[g, :3] = operator(c, g)[1]
        out[g, 3] = n_probes if n_probes > 0 else c.n
    return out


def moments_of_spectrum(lam_l, K):
    """tr T_k(L - I), k < K, from the eigenvalues of L."""
    theta = np.arccos(np.clip(np.asarray(lam_l, np.float64) - 1.0, -1.0, 1.0))
    return np.cos(np.arange(K)[:, None] * theta[None, :]).sum(axis=1)


def laplacian_spectrum(c, g):
    """Eigenvalues of L of graph g, ascending (eigvalsh of the dense M, shifted)."""
    return np.linalg.eigvalsh(operator(c, g)[0]) + 1.0


def exact_moments(c, K):
    return np.stack([moments_of_spectrum(laplacian_spectrum(c, g), K) for g in range(c.B)])


def probe_signs(n, R, b, seed):
    """[n, R] of +-1: -1 iff bit 0 of the first Philox word of counter (i, r, b, tag) is set."""
    i, r = np.meshgrid(np.arange(n, dtype=np.uint32), np.arange(R, dtype=np.uint32), indexing="ij")
    w0 = ref_rng.philox4x32_10(i.ravel(), r.ravel(), np.full(i.size, b, np.uint32),
                               np.full(i.size, PHILOX_TAG, np.uint32), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return np.where(w0 & np.uint32(1), -1.0, 1.0).reshape(n, R)


def plain_moments(Mm, V, K):
    """sum_r v_r^T T_k(M) v_r for k < K by the plain recurrence."""
    out = np.zeros(K)
    t0, t1 = V, Mm @ V
    out[0] = (V * t0).sum()
    out[1] = (V * t1).sum()
    for k in range(2, K):
        t0, t1 = t1, 2.0 * (Mm @ t1) - t0
        out[k] = (V * t1).sum()
    return out


def probe_moments(c, K, R, seed):
    return np.stack([plain_moments(operator(c, g)[0], probe_signs(c.n, R, g, seed), K) / R for g in range(c.B)])


def doubled_moments(Mm, V, K):
    """The device's route: K // 2 applications of M, mu_{2s+1} = 2 <t_{s+1}, t_s> - mu_1 and
    mu_{2s+2} = 2 <t_{s+1}, t_{s+1}> - mu_0, over the columns of V."""
    out = np.zeros(K)
    out[0] = (V * V).sum()
    prev, cur = None, V
    for s in range(K // 2):
        nxt = Mm @ cur if s == 0 else 2.0 * (Mm @ cur) - prev
        b, a = (nxt * cur).sum(), (nxt * nxt).sum()
        out[2 * s + 1] = b if s == 0 else 2.0 * b - out[1]
        if 2 * s + 2 < K:
            out[2 * s + 2] = 2.0 * a - out[0]
        prev, cur = cur, nxt
    return out


def eigen_histogram(lam_l, bins=200):
    """The normalised histogram of eigenvalues of L over [0, 2] in ``bins`` equal bins."""
    h = np.histogram(np.clip(lam_l, 0.0, 2.0), bins=bins, range=(0.0, 2.0))[0].astype(np.float64)
    return h / h.sum()


# ------------------------------------------------------------------ closed forms
def closed_form(kind, *size):
    """(local undirected pairs, nodes, eigenvalues of L) of a named graph."""
    if kind == "complete":
        n, = size
        return M._complete(n), n, np.array([0.0] + [n / (n - 1.0)] * (n - 1))
    if kind == "cycle":
        n, = size
        return [(i, (i + 1) % n) for i in range(n)], n, 1.0 - np.cos(2.0 * np.pi * np.arange(n) / n)
    if kind == "path":
        n, = size
        return [(i, i + 1) for i in range(n - 1)], n, 1.0 - np.cos(np.pi * np.arange(n) / (n - 1))
    if kind == "star":
        n, = size
        return [(0, i) for i in range(1, n)], n, np.array([0.0] + [1.0] * (n - 2) + [2.0])
    if kind == "bipartite":
        p, q = size
        return [(i, p + j) for i in range(p) for j in range(q)], p + q, np.array([0.0] + [1.0] * (p + q - 2) + [2.0])
    if kind == "empty":
        n, = size
        return [], n, np.zeros(n)
    raise KeyError(kind)


NAMED = {"K40": ("complete", 40), "C30": ("cycle", 30), "P33": ("path", 33), "star50": ("star", 50),
         "K8_12": ("bipartite", 8, 12), "empty25": ("empty", 25)}


def named_case(name, pad=0):
    """A one-graph case of a NAMED graph, ``pad`` isolated nodes appended, with its spectrum of L
    (an isolated node adds an eigenvalue 0)."""
    pairs, n, lam = closed_form(*NAMED[name])
    rp, ci = G.csr_from_pairs(pairs, 1, n + pad, shuffle_seed=5)
    return G.Case(name, 1, n + pad, rp, ci), np.sort(np.concatenate([lam, np.zeros(pad)]))


# ------------------------------------------------------------------ the GPU cases
# name: (exact-mode n_moments).  The smallest shapes at which the kernels can go wrong: one node;
# the reference's scale with every density and the closed forms; the LDS / global boundary from
# both sides; a complete graph at the boundary whose 4032 entries exceed what the LDS path
# stages (it reads them from global memory); unsorted rows with every kind of ignored entry;
# many probe blocks and row tiles; the worst conditioning measured.
CASES = {"n1": 128, "b70_mixed": 128, "n64": 128, "k64": 128, "n65": 128, "r257": 128, "ring1100": 32, "k200": 128}
B70_CLOSED = (("complete", 25), ("cycle", 20), ("path", 17), ("star", 20), ("bipartite", 8, 12), ("empty", 25),
              ("cycle", 25), ("path", 25), ("complete", 7), ("star", 25))

_case_cache = {}


def build_case(name):
    if name in _case_cache:
        return _case_cache[name]
    if name == "n1":
        c = G.Case(name, 1, 1, np.zeros(2, np.int32), np.zeros(0, np.int32))
    elif name == "b70_mixed":
        n, B = 25, 70
        pairs, extra = [], []
        rng = np.random.default_rng(70)
        for b in range(B - len(B70_CLOSED)):
            p = (0.0, 0.04, 0.1, 0.16, 0.3, 0.6)[b % 6]
            up = np.triu(rng.random((n, n)) < p, k=1)
            pairs += [(b * n + int(x), b * n + int(y)) for x, y in zip(*np.nonzero(up))]
            x, y = (int(v) for v in rng.choice(n, size=2, replace=False))
            if not up[min(x, y), max(x, y)]:
                extra.append((b * n + x, b * n + y))                          # a one-way arc
            extra.append((b * n + x, b * n + x))
            extra.append((b * n + y, ((b + 1) % B) * n + x))
        for k, spec in enumerate(B70_CLOSED):
            b = B - len(B70_CLOSED) + k
            pairs += [(b * n + i, b * n + j) for i, j in closed_form(*spec)[0]]
        rp, ci = G.csr_from_pairs(pairs, B, n, shuffle_seed=71, extra=sorted(set(extra)))
        c = G.Case(name, B, n, rp, ci)
    elif name in ("n64", "n65"):
        n = int(name[1:])
        c = G.Case(name, 3, n, *M.random_csr(3, n, 0.1, seed=n))
    elif name == "k64":
        pairs = M._complete(64) + [(64 + int(i), 64 + int(j)) for i, j in G.random_pairs(1, 64, 4.0, 64)]
        c = G.Case(name, 2, 64, *G.csr_from_pairs(pairs, 2, 64, shuffle_seed=64))
    elif name == "r257":
        c = G.Case(name, 2, 257, *M.random_csr(2, 257, 0.012, seed=257))
        i = info(c)
        assert (i[:, 1] > 0).all() and (i[:, 2] > 0).all()                    # isolated nodes, one-way arcs
    elif name == "ring1100":
        n = 1100
        pairs = [(i, (i + 1) % n) for i in range(n)] + [(n + int(i), n + int(j)) for i, j in G.random_pairs(1, n, 3.0, 11)]
        c = G.Case(name, 2, n, *G.csr_from_pairs(pairs, 2, n, shuffle_seed=12))
    elif name == "k200":
        c = G.Case(name, 1, 200, *G.csr_from_pairs(M._complete(200), 1, 200))
    else:
        raise KeyError(name)
    _case_cache[name] = c
    return c


def known_spectra(name):
    """{graph index: eigenvalues of L in closed form} for the graphs of a case that have one."""
    if name == "n1":
        return {0: np.zeros(1)}
    if name == "b70_mixed":
        out = {}
        for k, spec in enumerate(B70_CLOSED):
            _, m, lam = closed_form(*spec)
            out[70 - len(B70_CLOSED) + k] = np.concatenate([lam, np.zeros(25 - m)])
        return out
    if name == "k64":
        return {0: closed_form("complete", 64)[2]}
    if name == "ring1100":
        return {0: closed_form("cycle", 1100)[2]}
    if name == "k200":
        return {0: closed_form("complete", 200)[2]}
    return {}


_ref_cache = {}


def reference(name, K=None, R=0, seed=0):
    """(moments [B, K], info [B, 4]) of a case, computed once per argument set."""
    key = (name, K, R, seed)
    if key not in _ref_cache:
        c = build_case(name)
        K = CASES[name] if K is None else K
        m = exact_moments(c, K) if R == 0 else probe_moments(c, K, R, seed)
        m.setflags(write=False)
        _ref_cache[key] = (m, info(c, R))
    return _ref_cache[key]
