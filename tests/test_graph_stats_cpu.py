"""Graph statistics without a GPU: the integer reference (tests/graph_stats_ref.py) against
networkx, metrics.GraphStats (EMD, MMD, KL divergence, concat, all_gather) against scipy and
hand-computed values, and the planted faults of the kernel's walk.
"""
import os
import socket

import networkx as nx
import numpy as np
import pytest
import scipy.stats

import graph_stats_ref as G
from snd_vae_amd.metrics import GS_BINS, GraphStats, emd


# ------------------------------------------------------------------ reference vs networkx
def _nx_graphs(rp, ci, B, n):
    rows, lc = G.valid_entries(rp, ci, B, n)
    out = []
    for b in range(B):
        g = nx.Graph()
        g.add_nodes_from(range(n))
        sel = rows // n == b
        g.add_edges_from(zip((rows[sel] % n).tolist(), lc[sel].tolist()))
        out.append(g)
    return out


def _cases():
    yield "random", 3, 40, G.csr_from_pairs(G.random_pairs(3, 40, 6.0, 1), 3, 40)
    yield "random_shuffled", 2, 70, G.csr_from_pairs(G.random_pairs(2, 70, 9.0, 2), 2, 70, shuffle_seed=3)
    k = [(i, j) for i in range(12) for j in range(i + 1, 12)]
    yield "complete", 1, 12, G.csr_from_pairs(k, 1, 12)
    yield "star", 1, 30, G.csr_from_pairs([(0, j) for j in range(1, 30)], 1, 30)
    yield "empty", 2, 9, G.csr_from_pairs([], 2, 9)
    p = G.random_pairs(2, 33, 5.0, 4)
    loops = [(i, i) for i in range(0, 66, 3)]
    yield "self_loops", 2, 33, G.csr_from_pairs(p, 2, 33, shuffle_seed=5, extra=loops)
    # entries of the other graph's block in rows of both graphs: a valid CSR of the 66 x 66
    # matrix, but no neighbours
    cross = [(i, (i + 33) % 66) for i in range(0, 66, 2)] + [(5, 40), (40, 5), (32, 33), (33, 32)]
    yield "out_of_block", 2, 33, G.csr_from_pairs(p, 2, 33, shuffle_seed=6, extra=cross)


@pytest.mark.parametrize("name,B,n,csr", list(_cases()), ids=[c[0] for c in _cases()])
def test_reference_equals_networkx(name, B, n, csr):
    rp, ci = csr
    ref = G.ref_stats(rp, ci, B, n)
    for b, g in enumerate(_nx_graphs(rp, ci, B, n)):
        s = slice(b * n, (b + 1) * n)
        deg = np.array([g.degree(v) for v in range(n)])
        tri = np.array([nx.triangles(g, v) for v in range(n)])
        assert np.array_equal(ref["deg"][s], deg), name
        assert np.array_equal(ref["tri2"][s], 2 * tri), name
        dh = np.zeros(GS_BINS, np.int64)
        nxh = nx.degree_histogram(g)
        dh[:len(nxh)] = nxh
        assert np.array_equal(ref["hist"][b, 0], dh), name
        # nx.clustering is 2 T / (deg (deg - 1)) in floats; the bin rule is applied to its exact
        # integer numerator and denominator, and must contain the float value
        c = nx.clustering(g)
        cb = G.cluster_bins(deg, 2 * tri)
        for v in range(n):
            lo, hi = cb[v] / 256.0, (cb[v] + 1) / 256.0 if cb[v] < 255 else 1.0
            assert lo - 1e-12 <= c[v] <= hi + 1e-12, (name, v, c[v], cb[v])
        assert np.array_equal(ref["hist"][b, 1], np.bincount(cb, minlength=GS_BINS)), name
        t = ref["totals"][b]
        assert t[0] == 2 * g.number_of_edges() and t[3] == g.number_of_edges(), name
        assert t[1] == 2 * tri.sum() and t[2] == (deg * (deg - 1)).sum(), name
        gs = GraphStats(ref["hist"][b], t, n)
        assert gs.transitivity == pytest.approx(nx.transitivity(g), abs=1e-12), name
        assert gs.density == pytest.approx(nx.density(g), abs=1e-12), name
        assert gs.mean_degree == pytest.approx(deg.mean(), abs=1e-12), name
        assert gs.n_edges == g.number_of_edges()
        assert np.mean(list(c.values())) - 1.0 / 256 <= gs.mean_clustering <= np.mean(list(c.values())) + 1e-12


def test_reference_special_graphs():
    _, B, n, (rp, ci) = [c for c in _cases() if c[0] == "complete"][0]
    ref = G.ref_stats(rp, ci, B, n)
    assert (ref["tri2"] == 11 * 10).all() and ref["hist"][0, 1, 255] == n
    _, B, n, (rp, ci) = [c for c in _cases() if c[0] == "star"][0]
    ref = G.ref_stats(rp, ci, B, n)
    assert ref["deg"][0] == 29 and (ref["tri2"] == 0).all() and ref["hist"][0, 1, 0] == n
    _, B, n, (rp, ci) = [c for c in _cases() if c[0] == "empty"][0]
    ref = G.ref_stats(rp, ci, B, n)
    assert not ref["totals"].any() and (ref["hist"][:, :2, 0] == n).all()


def test_asymmetric_csr_follows_the_formula():
    """0 -> {1, 2}, 1 -> {2}, 2 -> {}: N(0) & N(1) = {2}, so tri2 = [1, 0, 0] (A A^T o A; A A o A
    would give the same here only by symmetry)."""
    rp, ci = G.csr_from_pairs([], 1, 3, extra=[(0, 1), (0, 2), (1, 2)])
    ref = G.ref_stats(rp, ci, 1, 3)
    assert ref["deg"].tolist() == [2, 1, 0] and ref["tri2"].tolist() == [1, 0, 0]
    assert ref["totals"][0].tolist() == [3, 1, 2, 3]
    G.assert_stats_equal(G.emulate(rp, ci, 1, 3), ref, 3)


def test_edge_length_histogram_and_margin_rule():
    B, n, sd = 2, 70, 2
    rp, ci = G.csr_from_pairs(G.random_pairs(B, n, 8.0, 11), B, n, shuffle_seed=12)
    scale = np.float32(256.0 / np.sqrt(sd))
    x = G.settle_coords(rp, ci, B, n, sd, scale, seed=13)
    assert len(G.ambiguous_edges(rp, ci, B, n, x, scale)) == 0
    ref = G.ref_stats(rp, ci, B, n, x, scale)
    assert ref["hist"][:, 2].sum(axis=1).tolist() == ref["totals"][:, 3].tolist()
    # by hand, graph 1
    g = _nx_graphs(rp, ci, B, n)[1]
    want = np.zeros(GS_BINS, np.int64)
    for u, v in g.edges():
        d = np.linalg.norm(x[n + u].astype(np.float64) - x[n + v].astype(np.float64)) * float(scale)
        want[min(int(np.floor(d)), 255)] += 1
    assert np.array_equal(ref["hist"][1, 2], want)
    # an edge put on a bin edge is found, and the re-draw removes it
    i, j = (int(t) for t in np.argwhere(np.triu(G.neighbour_matrix(rp, ci, B, n).toarray(), 1))[0])
    y = x.copy()
    y[j] = y[i]
    y[j, 0] = y[i, 0] + np.float32(8.0) / scale                        # v = 8 up to rounding
    assert [i, j] in G.ambiguous_edges(rp, ci, B, n, y, scale).tolist()
    # the emulation's float32 lengths fall into the float64 bins
    G.assert_stats_equal(G.emulate(rp, ci, B, n, x, scale), ref, n)


# ------------------------------------------------------------------ planted faults
def _fault_case():
    """n = 70 (not a multiple of 32, the last mask word holds nodes 64..69), two graphs, a hub
    of degree 69 in graph 0 (rows longer than 64 entries), self loops, entries of the other
    block, shuffled rows, coordinates."""
    B, n = 2, 70
    pairs = G.random_pairs(B, n, 7.0, 21).tolist() + [(0, j) for j in range(1, n)]
    pairs = np.unique(np.array([(min(a, b), max(a, b)) for a, b in pairs]), axis=0)
    extra = [(i, i) for i in range(0, 2 * n, 5)] + [(i, (i + n) % (2 * n)) for i in range(1, 2 * n, 4)]
    extra += [(3, n + 10), (n + 3, 10), (n - 1, n), (n, n - 1)]      # another node's id in the other block
    rp, ci = G.csr_from_pairs(pairs, B, n, shuffle_seed=22, extra=extra)
    scale = np.float32(256.0 / np.sqrt(2.0))
    x = G.settle_coords(rp, ci, B, n, 2, scale, seed=23)
    return B, n, rp, ci, x, scale


def test_emulation_equals_reference():
    B, n, rp, ci, x, scale = _fault_case()
    G.assert_stats_equal(G.emulate(rp, ci, B, n, x, scale), G.ref_stats(rp, ci, B, n, x, scale), n)


@pytest.mark.parametrize("fault", [f for f in G.FAULTS if f != "clustering_f32"])
def test_planted_faults_fail_naming_the_place(fault):
    B, n, rp, ci, x, scale = _fault_case()
    ref = G.ref_stats(rp, ci, B, n, x, scale)
    with pytest.raises(AssertionError, match=r"row \d+ \(graph \d+, node \d+\)|graph \d+ edge_length bin \d+"):
        G.assert_stats_equal(G.emulate(rp, ci, B, n, x, scale, fault=fault), ref, n, fault)


def test_planted_float32_clustering_bin_fails():
    """The bin in float32 differs from the integer rule only past deg ~ 4100 (256 tri2 / dd
    within 2^-25 relative below an integer).  deg = 4200, dd = 17 635 800, tri2 = (255 dd - 40)
    / 256 = 17 566 910: the exact quotient is 255 - 40 / dd, bin 254; float32 rounds it to 255.
    Planted in the per-row epilogue (bins_from_rows), which both the emulation and the
    reference share; the walk itself needs no graph of that size."""
    n = 4201
    deg = np.full(n, 2, np.int64)
    tri2 = np.zeros(n, np.int64)
    deg[7], tri2[7] = 4200, 17566910
    assert tri2[7] * 256 == 255 * 4200 * 4199 - 40
    hist, totals, cb = G.bins_from_rows(deg, tri2, 1, n)
    assert cb[7] == 254
    want = {"deg": deg, "tri2": tri2, "hist": hist, "totals": totals, "cbin": cb}
    bad, _, _ = G.bins_from_rows(deg, tri2, 1, n, fault="clustering_f32")
    got = {"deg": deg, "tri2": tri2, "hist": bad, "totals": totals}
    with pytest.raises(AssertionError, match=r"clustering bin 254 .*rows of that bin: \[7\]"):
        G.assert_stats_equal(got, want, n)


def test_case_builders_terminate():
    """Every GPU case's coordinates settle (tests/test_gpu_graph_stats.py takes them from the
    same builders); run here so a non-terminating builder shows without a GPU."""
    for name in G.CASES:
        c = G.build_case(name)
        for sd in (1, 2, 3):
            x, scale = G.case_coords(name, sd)
            assert x.shape == (c.B * c.n, sd) and x.dtype == np.float32
            assert len(G.ambiguous_edges(c.rp, c.ci, c.B, c.n, x, scale)) == 0, (name, sd)
        if name != "b2n2049":           # the emulation admits the case (the large one: GPU only)
            x, scale = G.case_coords(name, 2)
            G.assert_stats_equal(G.emulate(c.rp, c.ci, c.B, c.n, x, scale),
                                 G.ref_stats(c.rp, c.ci, c.B, c.n, x, scale), c.n, name)


# ------------------------------------------------------------------ GraphStats
def _gs_from(rp, ci, B, n, x=None, max_len=None):
    scale = None if x is None else np.float32(256.0 / max_len)
    ref = G.ref_stats(rp, ci, B, n, x, scale)
    return GraphStats(ref["hist"], ref["totals"], n, max_len)


def _gnp_set(B, n, mean_degree, seed, sd=2):
    rp, ci = G.csr_from_pairs(G.random_pairs(B, n, mean_degree, seed), B, n)
    x = np.random.default_rng(seed + 1000).random((B * n, sd)).astype(np.float32)
    return _gs_from(rp, ci, B, n, x, float(np.sqrt(sd)))


def test_emd_equals_wasserstein():
    rng = np.random.default_rng(0)
    for width in (1.0, 1.0 / 256, 0.37):
        p, q = rng.random(GS_BINS), rng.random(GS_BINS)
        p[rng.random(GS_BINS) < 0.5] = 0
        p, q = p / p.sum(), q / q.sum()
        centres = (np.arange(GS_BINS) + 0.5) * width
        want = scipy.stats.wasserstein_distance(centres, centres, p, q)
        assert emd(p, q, width) == pytest.approx(want, abs=1e-12)
    with pytest.raises(ValueError):
        emd(np.ones(3), np.ones(4))


def test_mmd_properties_and_hand_value():
    a, a2 = _gnp_set(6, 60, 4.0, 31), _gnp_set(6, 60, 4.0, 32)
    b = _gnp_set(6, 60, 12.0, 33)
    for kind in ("degree", "clustering", "edge_length"):
        assert a.mmd(a, kind) == pytest.approx(0.0, abs=1e-15)
        assert a.mmd(b, kind) == pytest.approx(b.mmd(a, kind), abs=1e-15)
        assert a.mmd(b, kind) >= 0.0
    for kind in ("degree", "clustering"):
        assert a.mmd(b, kind) > a.mmd(a2, kind) + 0.05, kind
    # two one-graph sets: every node of degree 2 against every node of degree 5 -> EMD 3,
    # MMD^2 = 1 + 1 - 2 exp(-9 / (2 sigma^2))
    h1, h2 = np.zeros((1, 3, GS_BINS), np.int64), np.zeros((1, 3, GS_BINS), np.int64)
    h1[0, 0, 2] = 10
    h2[0, 0, 5] = 10
    h1[0, 1, 0] = h2[0, 1, 0] = 10
    t = np.zeros((1, 4), np.int64)
    s1, s2 = GraphStats(h1, t, 10), GraphStats(h2, t, 10)
    assert s1.mmd(s2, "degree") == pytest.approx(2.0 - 2.0 * np.exp(-4.5), abs=1e-15)
    assert s1.mmd(s2, "degree", sigma=3.0) == pytest.approx(2.0 - 2.0 * np.exp(-0.5), abs=1e-15)
    assert s1.mmd(s2, "clustering") == 0.0
    with pytest.raises(ValueError, match="max_len"):
        s1.mmd(s2, "edge_length")
    # an empty histogram is the zero histogram: its EMD to "all mass in bin 3" is the sum of
    # that cdf over the bins, (256 - 3) widths
    h3 = np.zeros((1, 3, GS_BINS), np.int64)
    h4 = h3.copy()
    h4[0, 2, 3] = 5
    e, f = GraphStats(h3, t, 10, max_len=2.0), GraphStats(h4, t, 10, max_len=2.0)
    d = (GS_BINS - 3) * 2.0 / GS_BINS
    assert e.mmd(f, "edge_length") == pytest.approx(2.0 - 2.0 * np.exp(-d * d / (2 * 0.2 ** 2)), abs=1e-15)


def test_kld_equals_scipy_entropy():
    a, b = _gnp_set(4, 50, 4.0, 41), _gnp_set(4, 50, 8.0, 42)
    for kind in ("degree", "clustering", "edge_length"):
        p, q = a.pooled(kind), b.pooled(kind)
        assert p.sum() == pytest.approx(1.0)
        assert a.kld(b, kind) == pytest.approx(scipy.stats.entropy(p + 1e-12, q + 1e-12), rel=1e-12)
        assert a.kld(a, kind) == pytest.approx(0.0, abs=1e-15)
    assert a.kld(b, "degree") != pytest.approx(b.kld(a, "degree"))


def test_concat_compare_and_errors():
    a, b = _gnp_set(3, 40, 4.0, 51), _gnp_set(2, 40, 6.0, 52)
    c = GraphStats.concat([a, b])
    assert c.n_graphs == 5 and c.n == 40 and c.max_len == a.max_len
    assert np.array_equal(c.hist[:3], a.hist) and np.array_equal(c.totals[3:], b.totals)
    assert c.n_edges == a.n_edges + b.n_edges
    pg = c.per_graph()
    assert pg["density"].shape == (5,) and pg["density"][0] == pytest.approx(a.per_graph()["density"][0])
    assert c == GraphStats.concat([a, b]) and c != a
    out = a.compare(b)
    for kind in ("degree", "clustering", "edge_length"):
        assert np.isfinite(out[f"mmd_{kind}"]) and np.isfinite(out[f"kld_{kind}"]) and out[f"emd_{kind}"] >= 0
    assert out["self"] == a.summary() and out["other"]["n_edges"] == b.n_edges
    assert set(out["self"]) == {"density", "mean_degree", "transitivity", "mean_clustering", "n_edges",
                                "mean_edge_length"}
    centres = (np.arange(GS_BINS) + 0.5) * a.max_len / GS_BINS
    assert a.mean_edge_length == pytest.approx((a.hist[:, 2].sum(axis=0) * centres).sum() / a.n_edges)
    no_len = GraphStats(a.hist, a.totals, 40)
    assert "mmd_edge_length" not in no_len.compare(no_len) and np.isnan(no_len.mean_edge_length)
    with pytest.raises(ValueError, match="differ"):
        GraphStats.concat([a, no_len])
    with pytest.raises(ValueError, match="differ"):
        GraphStats.concat([a, _gnp_set(2, 41, 4.0, 53)])
    with pytest.raises(ValueError):
        GraphStats.concat([])
    with pytest.raises(ValueError, match="hist"):
        GraphStats(np.zeros((2, 2, GS_BINS)), np.zeros((2, 4)), 4)
    with pytest.raises(ValueError, match="hist"):
        GraphStats(np.zeros((2, 3, GS_BINS)), np.zeros((3, 4)), 4)
    with pytest.raises(ValueError, match="max_len"):
        GraphStats(a.hist, a.totals, 40, max_len=0.0)
    with pytest.raises(ValueError, match="kind"):
        a.mmd(b, "orbits")
    with pytest.raises(ValueError, match="sigma"):
        a.mmd(b, "degree", sigma=0.0)
    with pytest.raises(ValueError, match="max_len"):
        a.mmd(GraphStats(b.hist, b.totals, 40, max_len=3.0), "edge_length")


def test_layers_argument_errors_need_no_gpu():
    """layers.graph_stats rejects host tensors and bad shapes before the library is touched."""
    import torch
    from snd_vae_amd import layers
    rp = torch.zeros(9, dtype=torch.int32)
    ci = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="rowptr"):
        layers.graph_stats(rp, ci, 2, 4)
    with pytest.raises(ValueError, match="n_graphs"):
        layers.graph_stats(rp, ci, 0, 4)


# ------------------------------------------------------------------ all_gather (gloo)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_stats(rank):
    return _gnp_set(2, 30, 3.0 + 4.0 * rank, 60 + rank)


def _gather_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from snd_vae_amd.parallel import init_from_env
    info = init_from_env("gloo")
    g = _rank_stats(rank).all_gather(info.group)
    q.put((rank, g.hist.copy(), g.totals.copy(), g.n, g.max_len))
    dist.barrier()
    dist.destroy_process_group()


def test_all_gather_world_2():
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = GraphStats.concat([_rank_stats(0), _rank_stats(1)])
    for rank, h, t, n, ml in res:
        assert np.array_equal(h, want.hist) and np.array_equal(t, want.totals), rank
        assert n == want.n and ml == want.max_len
