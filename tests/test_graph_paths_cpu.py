"""snd_graph_paths without a GPU (ABI 26): the float32 emulation of the kernel's fixed point
against the float64 reference (tests/graph_paths_ref.py) and its independence of the relaxation
order, ``metrics.PathStats`` on planted graphs and against networkx, the two-sample statistics,
every SND_ERR_ARG rule through ctypes (they return before the device is touched), the header,
the exports and the ABI number, and the planted faults of the emulation."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import graph_paths_ref as P
import graph_stats_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = P.DETOUR_SCALE


def stats_of(c, x=None, scale=None, src_step=1):
    from snd_vae_amd.metrics import PathStats
    e = P.emulate(c, x, scale, src_step)
    return PathStats(e["hist"], e["totals"], c.n, None if x is None else float(scale), src_step)


# ---------------------------------------------------------------- emulation vs reference
@pytest.mark.parametrize("name", P.SMALL + ("b2n2049", "n1981", "ring16384"))
def test_emulation_within_the_bound_of_the_reference(name):
    c, x, step = P.build_case(name)
    ref = P.reference(c, x, SCALE, step)                     # asserts the 1 % condition
    emu = P.emulate(c, x, SCALE, step)
    worst = P.assert_paths(emu, ref, c.n, name)
    print(f"GPATHS-CPU {name} ambiguous_share {ref['ambiguous_share']:.2e} worst_err_over_bound {worst:.3f}")
    assert ref["ambiguous_share"] <= P.AMBIGUOUS_CAP
    P.assert_paths(P.emulate(c, None, None, step), P.reference(c, None, None, step), c.n, name + " no coords")


@pytest.mark.parametrize("name,sd", [("b2n70", 1), ("b2n70", 3), ("b3n33", 3)])
def test_emulation_other_dimensions(name, sd):
    c, x, step = P.build_case(name, sd)
    assert x.shape[1] == sd
    P.assert_paths(P.emulate(c, x, SCALE, step), P.reference(c, x, SCALE, step), c.n, f"{name} sd={sd}")


@pytest.mark.parametrize("name", ["b2n70", "coincident", "deg300"])
def test_fixed_point_is_bitwise_independent_of_the_relaxation_order(name):
    c, x, step = P.build_case(name)
    base = P.emulate(c, x, SCALE, step)
    for seed, chunks in ((1, 1), (2, 7), (3, 64)):
        other = P.emulate(c, x, SCALE, step, order_seed=seed, chunks=chunks)
        assert np.array_equal(base["route"].view(np.uint32), other["route"].view(np.uint32)), (seed, chunks)
        assert np.array_equal(base["hist"], other["hist"])
    src = P.sources(c.n, step)
    for g in range(c.B):
        u, v = P.graph_arcs(c.rp, c.ci, c.B, c.n, g)
        w = P.lengths32(x[g * c.n:(g + 1) * c.n], u, v)
        for s in (0, c.n // 2, c.n - 1):
            d, edges = P.dijkstra32(c.n, u, v, w, s)
            row = g * len(src) + s
            assert np.array_equal(d.view(np.uint32), base["route"][row].view(np.uint32)), (g, s)
            assert np.all(edges >= base["k32"][row]) and np.array_equal(edges < 0, base["k32"][row] < 0)


# ---------------------------------------------------------------- PathStats on planted graphs
def test_path_graph():
    n = 40
    c = G.Case("p", 1, n, *G.csr_from_pairs([(i, i + 1) for i in range(n - 1)], 1, n))
    s = stats_of(c)
    assert s.diameter == n - 1 and abs(s.mean_hops - (n + 1) / 3.0) <= 1e-12
    pg = s.per_graph()
    assert pg["n_components"][0] == 1 and pg["connected"][0] == 1.0 and pg["lcc_fraction"][0] == 1.0
    assert math.isnan(s.mean_detour)
    # on a straight line every route is the straight line: detour bin 0 everywhere
    x = np.stack([np.arange(n) / 64.0, np.zeros(n)], axis=1).astype(np.float32)
    s = stats_of(c, x, SCALE)
    assert s.hist[0, 1, 0] == n * (n - 1) and s.hist[0, 1, 1:].sum() == 0


def test_complete_graph():
    n = 17
    c = G.Case("k", 1, n, *G.csr_from_pairs([(i, j) for i in range(n) for j in range(i + 1, n)], 1, n))
    x = np.random.default_rng(0).random((n, 3)).astype(np.float32)
    s = stats_of(c, x, SCALE)
    assert s.global_efficiency == 1.0 and s.diameter == 1 and s.mean_hops == 1.0
    assert s.hist[0, 1, 0] == n * (n - 1) and s.hist[0, 1, 1:].sum() == 0
    assert abs(s.mean_detour - 0.5 / float(SCALE)) <= 1e-15        # the centre of bin 0


def test_ring_on_a_circle():
    n = 64
    ang = 2 * np.pi * np.arange(n) / n
    x = np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)
    c = G.Case("r", 1, n, *G.csr_from_pairs([(i, (i + 1) % n) for i in range(n)], 1, n))
    s = stats_of(c, x, SCALE)
    assert s.diameter == n // 2 and abs(s.mean_hops - (n * n / 4.0) / (n - 1)) <= 1e-12
    # k steps round the ring: route 2 k sin(pi / n), chord 2 sin(k pi / n)
    k = np.minimum(np.arange(1, n), n - np.arange(1, n))
    want = np.bincount(np.floor((k * np.sin(np.pi / n) / np.sin(k * np.pi / n) - 1.0) * float(SCALE)).astype(int),
                       minlength=256) * n
    assert np.array_equal(s.hist[0, 1], want)                       # no pair within 1e-3 of a bin edge
    frac = (k * np.sin(np.pi / n) / np.sin(k * np.pi / n) - 1.0) * float(SCALE) % 1.0
    assert frac[k > 1].min() > 1e-3 and frac.max() < 1 - 1e-3


def test_two_components_and_an_empty_graph():
    n = 10
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (5, 6), (6, 7)] + [(n + 8, n + 9)]
    c = G.Case("t", 3, n, *G.csr_from_pairs(pairs, 3, n))
    s = stats_of(c)
    pg = s.per_graph()
    assert pg["n_components"].tolist() == [4.0, 9.0, 10.0]
    assert pg["lcc_fraction"].tolist() == [0.5, 0.2, 0.1] and pg["connected"].tolist() == [0.0, 0.0, 0.0]
    assert pg["diameter"].tolist() == [4.0, 1.0, 0.0]
    assert s.totals[:, 3].tolist() == [5 * 4 + 3 * 2, 2, 0] and math.isnan(pg["mean_hops"][2])
    assert pg["global_efficiency"][2] == 0.0 and abs(pg["global_efficiency"][1] - 2.0 / 90.0) <= 1e-15
    e = P.emulate(c)
    assert e["comp"][:n].tolist() == [0, 0, 0, 0, 0, 5, 5, 5, 8, 9]
    assert s.summary()["connected"] == 0.0 and s.summary()["diameter"] == 4.0
    one = G.Case("o", 1, 1, *G.csr_from_pairs([], 1, 1))
    s1 = stats_of(one)
    assert s1.totals.tolist() == [[1, 1, 1, 0, 0, 0]] and math.isnan(s1.global_efficiency) and s1.connected == 1.0


@pytest.mark.parametrize("name", ["b1n257", "b2n70", "star200"])
def test_networkx_identities(name):
    import networkx as nx
    c, x, step = P.build_case(name)
    A = G.neighbour_matrix(c.rp, c.ci, c.B, c.n)
    A = ((A + A.T) > 0).astype(np.int64).tocsr()                   # the undirected graph of the CSR
    coo = A.tocoo()
    sym = G.Case(name + "_sym", c.B, c.n, *G.csr_from_pairs(np.stack([coo.row, coo.col], 1)[coo.row < coo.col],
                                                            c.B, c.n))
    pg = stats_of(sym).per_graph()
    for g in range(c.B):
        Gx = nx.from_scipy_sparse_array(A[g * c.n:(g + 1) * c.n, g * c.n:(g + 1) * c.n])
        assert abs(pg["global_efficiency"][g] - nx.global_efficiency(Gx)) <= 1e-12
        assert pg["n_components"][g] == nx.number_connected_components(Gx)
        big = Gx.subgraph(max(nx.connected_components(Gx), key=len))
        assert pg["lcc_fraction"][g] == big.number_of_nodes() / c.n
        if nx.is_connected(Gx):
            assert abs(pg["mean_hops"][g] - nx.average_shortest_path_length(Gx)) <= 1e-12
            assert pg["diameter"][g] == nx.diameter(Gx)
        else:
            assert pg["diameter"][g] == max(nx.diameter(Gx.subgraph(k)) for k in nx.connected_components(Gx))


def test_source_sampling_counts_the_sampled_sources_only():
    c, x, _ = P.build_case("b1n257")
    full, part = P.emulate(c, x, SCALE, 1), P.emulate(c, x, SCALE, 16)
    src = P.sources(c.n, 16)
    assert len(src) == 17 and part["totals"][0, 2] == 17 and full["totals"][0, 2] == 257
    assert np.array_equal(part["hops"], full["hops"][src])
    assert np.array_equal(part["route"].view(np.uint32), full["route"][src].view(np.uint32))
    assert np.array_equal(part["totals"][0, :2], full["totals"][0, :2])


# ---------------------------------------------------------------- two-sample statistics
def test_mmd_kld_concat_and_errors():
    from snd_vae_amd.metrics import KINDS, PATH_KINDS, GraphStats, PathStats, emd
    assert KINDS == ("degree", "clustering", "edge_length") and PATH_KINDS == ("hops", "detour")
    ca, xa, _ = P.build_case("b3n33")
    cb, xb, _ = P.build_case("empty_middle")
    a, b = stats_of(ca, xa, SCALE), stats_of(cb, xb, SCALE)
    assert a.n_graphs == 3 and a == stats_of(ca, xa, SCALE) and a != b
    for kind in PATH_KINDS:
        assert abs(a.mmd(a, kind)) <= 1e-12 and a.mmd(b, kind) > 0 and a.kld(a, kind) == 0.0
        assert abs(a.mmd(b, kind) - b.mmd(a, kind)) <= 1e-12 and a.kld(b, kind) > 0
        assert a.mmd(b, kind, sigma=10.0) < a.mmd(b, kind, sigma=1.0) or kind == "detour"
    # a hand value: two one-graph sets, all pairs at 1 hop against all at 3 hops: EMD 2
    h1, h3 = np.zeros((1, 2, 256), np.int64), np.zeros((1, 2, 256), np.int64)
    h1[0, 0, 1], h3[0, 0, 3] = 6, 6
    t = np.array([[1, 3, 3, 6, 6, 1]])
    p1, p3 = PathStats(h1, t, 3), PathStats(h3, t, 3)
    assert abs(p1.mmd(p3, "hops") - (2.0 - 2.0 * math.exp(-4.0 / 2.0))) <= 1e-12
    assert abs(p1.mmd(p3, "hops", sigma=2.0) - (2.0 - 2.0 * math.exp(-4.0 / 8.0))) <= 1e-12
    assert emd(p1.pooled("hops"), p3.pooled("hops")) == 2.0
    cat = PathStats.concat([a, b])
    assert cat.n_graphs == 6 and np.array_equal(cat.hist[3:], b.hist) and np.array_equal(cat.totals[:3], a.totals)
    cmp = a.compare(b)
    assert set(cmp) == {"mmd_hops", "kld_hops", "emd_hops", "mmd_detour", "kld_detour", "emd_detour", "self", "other"}
    assert cmp["self"] == a.summary() and cmp["mmd_hops"] == a.mmd(b, "hops")
    nocoords = stats_of(ca)
    assert set(nocoords.compare(a)) == {"mmd_hops", "kld_hops", "emd_hops", "self", "other"}
    with pytest.raises(ValueError, match="kind"):
        a.mmd(b, "degree")
    with pytest.raises(ValueError, match="detour"):
        nocoords.mmd(nocoords, "detour")
    with pytest.raises(ValueError, match="detour_scale"):
        a.mmd(PathStats(b.hist, b.totals, b.n, 32.0), "detour")
    with pytest.raises(ValueError, match="differ"):
        PathStats.concat([a, nocoords])
    with pytest.raises(ValueError, match="differ"):
        PathStats.concat([a, PathStats(a.hist, a.totals, a.n, float(SCALE), 2)])
    with pytest.raises(ValueError):
        PathStats(np.zeros((2, 3, 256)), np.zeros((2, 6)), 5)
    with pytest.raises(ValueError):
        PathStats(a.hist, a.totals, a.n, detour_scale=0.0)
    with pytest.raises(ValueError):
        a.compare(GraphStats(np.zeros((1, 3, 256)), np.zeros((1, 4)), 33))
    a.invalidate()
    assert a.tensors is None and a.n_graphs == 3


# ---------------------------------------------------------------- the C ABI without a device
def test_header_library_and_integration_agree_on_abi_26(lib_built):
    from snd_vae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snd_vae.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    so = ctypes.CDLL(lib_built)
    for name in ("snd_graph_paths", "snd_graph_paths_workspace"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(so, name) and name in doc, name
    abi = int(re.search(r"#define\s+SND_ABI_VERSION\s+(\d+)", hdr).group(1))
    stub = int(re.search(r"SND_ABI_VERSION\s*=\s*(\d+)", doc).group(1))
    assert abi == _lib.ABI_VERSION == so.snd_abi_version() == stub and abi >= 26


def test_no_spill_or_scratch_in_the_new_kernels(lib_built):
    from snd_vae_amd.build import build_info, kernel_resources
    res = {k: v for k, v in kernel_resources().items()
           if any(s in k for s in ("gp_edge_len_kernel", "gp_components_kernel", "gp_paths_kernel"))}
    assert len(res) == 4, sorted(res)                        # gp_paths_kernel with and without routes
    for k, v in res.items():
        assert v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v.get("scratch", 0) == 0, (k, v)
    assert not any("gp_" in k for k in build_info().get("spills", {}))


class HostArgs:
    """A well-formed argument list over host memory.  No rule below reaches a launch, so nothing
    dereferences these pointers."""

    def __init__(self, _lib, B=2, n=10, cap=40, step=3):
        self.L, self._lib = _lib.lib(), _lib
        n_src = -(-n // step)
        self.d = dict(nnz_cap=cap, n_graphs=B, n=n, ldc=2, sd=2, detour_scale=64.0, src_step=step)
        self.need = self.L.snd_graph_paths_workspace(B, n, cap, 1)
        self.keep = {"rowptr": np.zeros(B * n + 1, np.int32), "colidx": np.zeros(cap, np.int32),
                     "coords": np.zeros(B * n * 2, np.float32), "comp": np.zeros(B * n, np.int32),
                     "hops": np.zeros(B * n_src * n, np.int32), "route": np.zeros(B * n_src * n, np.float32),
                     "hist": np.zeros(B * 2 * 256, np.int64), "totals": np.zeros(B * 6, np.int64),
                     "ws": np.zeros(self.need, np.uint8)}

    def call(self, **kw):
        a = dict(self.d, ws_bytes=self.need, **{k: v.ctypes.data for k, v in self.keep.items()})
        a.update(kw)
        rc = self.L.snd_graph_paths(a["rowptr"], a["colidx"], a["nnz_cap"], a["n_graphs"], a["n"], a["coords"],
                                    a["ldc"], a["sd"], a["detour_scale"], a["src_step"], a["comp"], a["hops"],
                                    a["route"], a["hist"], a["totals"], a["ws"], a["ws_bytes"], None)
        return rc, self._lib.last_error()


def test_the_op_rejects_bad_arguments_before_any_launch(lib_built):
    from snd_vae_amd import _lib
    h = HostArgs(_lib)
    assert h.need >= 40 * 4
    nan, inf = float("nan"), float("inf")
    bad = [dict(n_graphs=0), dict(n=0), dict(n=16385), dict(src_step=0), dict(src_step=-2), dict(coords=None),
           dict(sd=0), dict(sd=4), dict(ldc=1), dict(detour_scale=nan), dict(detour_scale=0.0),
           dict(detour_scale=-1.0), dict(detour_scale=inf), dict(rowptr=None), dict(hist=None), dict(totals=None),
           dict(ws_bytes=h.need - 1), dict(ws=None), dict(nnz_cap=-1), dict(colidx=None)]
    for kw in bad:
        rc, msg = h.call(**kw)
        assert rc == -1, (kw, rc)
        assert msg.startswith("snd_graph_paths:"), (kw, msg)
    assert "route_out needs coords" in h.call(coords=None)[1]
    assert "workspace" in h.call(ws_bytes=h.need - 1)[1] and "src_step" in h.call(src_step=0)[1]
    assert "detour_scale" in h.call(detour_scale=nan)[1] and "null operand" in h.call(hist=None)[1]
    assert not any(v.any() for v in h.keep.values())                         # nothing was written
    W = h.L.snd_graph_paths_workspace
    assert W(2, 10, 40, 0) == 0 and W(0, 10, 40, 1) == 0 and W(2, 16385, 40, 1) == 0 and W(2, 10, -1, 1) == 0
    assert W(2, 10, 0, 1) > 0 and W(1, 16384, 1 << 20, 1) >= 4 << 20
    assert W(2, 10, 4000, 1) - W(2, 10, 2000, 1) == 2000 * 4


def test_layers_graph_paths_validates_before_the_library():
    import torch
    from snd_vae_amd import layers
    rp, ci = torch.zeros(11, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="device tensor"):
        layers.graph_paths(rp, ci, 1, 10)                                     # host tensors: there is no CPU path
    with pytest.raises(ValueError, match="src_step"):
        layers.graph_paths(rp, ci, 1, 10, src_step=0)
    with pytest.raises(ValueError, match="n_graphs"):
        layers.graph_paths(rp, ci, 0, 10)


# ---------------------------------------------------------------- planted faults
FAULT_CASE = {"bfs_stops_at_64": "star200", "self_loop_followed": "b2n70", "next_block_followed": "b3n33",
              "source_counted": "b2n70", "unreachable_binned": "empty_middle", "one_sweep_only": "b2n70",
              "weighted_path_hops": "b2n70", "detour_without_minus_one": "b2n70",
              "components_directed_only": "b3n33"}


def test_every_fault_has_a_case():
    assert set(FAULT_CASE) == set(P.FAULTS)


@pytest.mark.parametrize("fault", P.FAULTS)
def test_planted_faults_fail_naming_the_place(fault):
    c, x, step = P.build_case(FAULT_CASE[fault])
    ref = P.reference(c, x, SCALE, step)
    P.assert_paths(P.emulate(c, x, SCALE, step), ref, c.n, "clean")
    with pytest.raises(AssertionError, match=r"(graph \d+ (hops|detour) bin \d+|element \(?\d+)"):
        P.assert_paths(P.emulate(c, x, SCALE, step, fault=fault), ref, c.n, fault)


def test_cases_hold_what_they_are_there_for():
    for name in ("b3n33", "b2n70"):
        c, _, _ = P.build_case(name)
        rows = np.repeat(np.arange(c.B * c.n), np.diff(c.rp))
        ci = c.ci[:c.rp[-1]]
        assert (ci == rows).any() and (ci // c.n != rows // c.n).any(), name         # loops, other blocks
        key = rows.astype(np.int64) * c.B * c.n + ci
        assert len(np.unique(key)) < len(key), name                                   # duplicates
        A = G.neighbour_matrix(c.rp, c.ci, c.B, c.n)
        assert (A != A.T).nnz > 0, name                                               # one-way arcs
    c, x, _ = P.build_case("coincident")
    assert np.array_equal(x[2], x[5]) and P.reference(c, x, SCALE)["pairs1"][0] < P.reference(c, x, SCALE)["totals"][0, 3]
    c, x, _ = P.build_case("path300")
    assert P.reference(c, x, SCALE)["hist_lo"][0, 0, 255] == 2 * sum(range(1, 300 - 254))
    assert np.diff(P.build_case("star200")[0].rp).max() > 64 and np.diff(P.build_case("deg300")[0].rp).max() > 255
    assert not P.reference(P.build_case("empty_middle")[0])["totals"][1, 3]
    # the two n at which gp_paths_kernel leaves four waves per workgroup (snd_gpaths.hpp)
    assert 2176 + 4 * 1980 * 8 <= 65536 < 2176 + 4 * 1981 * 8 and 2176 + 4 * 3960 * 4 <= 65536 < 2176 + 4 * 3961 * 4
