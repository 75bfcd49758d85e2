"""snd_graph_motifs without a GPU (ABI 27): the counting route of the header restated on
scipy.sparse (tests/graph_motifs_ref.py) against brute-force enumeration of every 3- and 4-subset
and against networkx where networkx is exact, the orbit sums against a brute-force per-node orbit
table, ``metrics.MotifStats``, the planted faults of the restatement, every SND_ERR_ARG rule
through ctypes (they return before the device is touched), the header, the exports and the ABI
number."""
import ctypes
import os
import re
from math import comb

import numpy as np
import pytest

import graph_motifs_ref as M
import graph_stats_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSITIES = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 1.0)


def small_graphs():
    """24 + 2 batches of two graphs, n = 5 .. 12, every density, with self loops, out-of-block
    entries and one-way arcs planted, rows shuffled."""
    out = []
    for k, p in enumerate(DENSITIES + DENSITIES):
        n = 5 + (k * 5) % 8
        out.append((2, n, *M.random_csr(2, n, p, 40 + k)))
    out.append((2, 4, *M.random_csr(2, 4, 0.8, 90)))
    out.append((1, 12, *G.csr_from_pairs(M._complete(12), 1, 12)))
    return out


SMALL = small_graphs()
BRUTE = [M.brute_census(rp, ci, B, n) for B, n, rp, ci in SMALL]     # computed once, never written


# ---------------------------------------------------------------- the route
def test_the_counting_route_equals_brute_force_at_every_density():
    seen = np.zeros(10, np.int64)
    for (B, n, rp, ci), want in zip(SMALL, BRUTE):
        got = M.route_census(rp, ci, B, n)
        M.assert_census(got, M.work(rp, ci, B, n), want, M.work(rp, ci, B, n), f"n={n}")
        seen += want.sum(axis=0)
    assert (seen > 0).all(), seen                              # every kind and the one-way arcs occurred
    assert BRUTE[-1][0].tolist() == [66, 0, comb(12, 3), 0, 0, 0, 0, 0, comb(12, 4), 0]


def test_the_route_equals_networkx_where_networkx_is_exact():
    nx = pytest.importorskip("networkx")
    for name in ("r33", "r65", "one_way", "k40", "lattice12", "deg300"):
        c = M.build_case(name)
        cen, _ = M.reference(c)
        A = M.arc_matrix(c.rp, c.ci, c.B, c.n)
        Mu = A.multiply(A.T).tocsr()
        for g in range(c.B):
            s = slice(g * c.n, (g + 1) * c.n)
            H = nx.from_scipy_sparse_array(Mu[s][:, s])
            assert H.number_of_edges() == cen[g, 0], (name, g)
            assert sum(nx.triangles(H).values()) // 3 == cen[g, 2], (name, g)
            if name != "deg300":
                k4 = 0
                for q in nx.enumerate_all_cliques(H):          # by size, ascending: stop after 4
                    if len(q) > 4:
                        break
                    k4 += len(q) == 4
                assert k4 == cen[g, 8], (name, g)
            d = np.array([v for _, v in H.degree()], np.int64)
            assert int((d * (d - 1) // 2).sum()) == cen[g, 1] + 3 * cen[g, 2], (name, g)     # wedges


def test_closed_forms_of_the_named_cases():
    for name in M.CASES:
        known = M.known_counts(name)
        if not known:
            continue
        cen, _ = M.reference(M.build_case(name))
        for g, kv in known.items():
            for k, v in kv.items():
                assert cen[g, M.NAMES.index(k)] == v, (name, g, k, int(cen[g, M.NAMES.index(k)]), v)


def test_orbit_sums_equal_a_per_node_orbit_table():
    from snd_vae_amd.metrics import MotifStats
    for (B, n, rp, ci), want in zip(SMALL[:12], BRUTE[:12]):
        for g in range(B):
            m, _ = M.dense_mutual(rp, ci, B, n, g)
            cen, orb = M.brute_orbits(m)
            assert np.array_equal(cen, want[g, :9])
            assert np.array_equal(orb.sum(axis=0), M.orbit_sums(want[g])), (n, g)
        ms = MotifStats(want, n)
        ref = np.stack([M.brute_orbits(M.dense_mutual(rp, ci, B, n, g)[0])[1].sum(axis=0) for g in range(B)]) / n
        assert np.allclose(ms.orbits(), ref, rtol=0, atol=1e-12)


def test_work_bounds_the_column_ids_the_passes_read():
    """The header's claim behind the formula, on the mutual-edge degrees d <= l: the three
    counting kernels read at most 9 l_i + 4 a_i + c_i column ids per row in all."""
    for name in ("r33", "k40", "deg300", "one_way", "b70_mixed"):
        c = M.build_case(name)
        A = M.arc_matrix(c.rp, c.ci, c.B, c.n)
        Mu = A.multiply(A.T).tocsr().astype(np.int64)
        d = np.asarray(Mu.sum(axis=1)).ravel()
        ln = np.diff(np.asarray(c.rp, np.int64))
        first = np.asarray(A.sum(axis=1)).ravel()
        mutual = 2 * ln + A @ ln                               # row i twice; row j per first occurrence
        wedge = 4 * d + 2 * (Mu @ d)
        U = np.triu(Mu.toarray(), k=1)
        # clique: rows v > u of every row u with its mask; per triangle u < v < w one row w
        tri_rows = np.zeros(len(d), np.int64)
        for u, v in zip(*np.nonzero(U)):
            w = np.nonzero(U[v] & Mu[u].toarray().ravel())[0]
            tri_rows[u] += d[w].sum()
        clique = 3 * d + U @ d + tri_rows
        used = (mutual + wedge + clique).reshape(c.B, c.n).sum(axis=1)
        assert (used <= M.work(c.rp, c.ci, c.B, c.n)).all(), (name, used, M.work(c.rp, c.ci, c.B, c.n))
        assert (first <= ln).all()


@pytest.mark.parametrize("fault", M.FAULTS)
def test_planted_faults_fail(fault):
    wrong = 0
    for (B, n, rp, ci), want in zip(SMALL, BRUTE):
        got = M.route_census(rp, ci, B, n, fault)
        try:
            M.assert_census(got, M.work(rp, ci, B, n), want, M.work(rp, ci, B, n))
        except AssertionError:
            wrong += 1
    assert wrong >= len(SMALL) // 3, (fault, wrong)


def test_work_cap_rule_of_the_reference():
    c = M.build_case("k200_middle")
    cap = M.case_work_cap("k200_middle")
    cen, wk = M.reference(c, cap)
    assert (cen[1] == -1).all() and (cen[[0, 2]] >= 0).all() and wk[1] > cap > max(wk[0], wk[2])
    cen0, wk0 = M.reference(M.build_case("cap0"), 0)
    assert wk0[1] == 0 and cen0[1].tolist() == [0] * 10 and (cen0[[0, 2]] == -1).all()


# ---------------------------------------------------------------- metrics.MotifStats
def test_motif_stats_descriptors():
    from snd_vae_amd.metrics import GRAPHLETS4, MotifStats
    cen = np.array([[6, 0, 4, 0, 0, 0, 0, 0, 1, 2],           # K4 with two one-way arcs
                    [-1] * 10,                                 # skipped
                    [4, 4, 0, 0, 0, 1, 0, 0, 0, 0],           # C4
                    [0] * 10], np.int64)
    ms = MotifStats(cen, 4)
    assert (ms.n_graphs, ms.n_skipped, ms.one_way) == (4, 1, 2)
    o = ms.orbits()
    assert o.shape == (3, 15)
    assert o[0].tolist() == [3.0, 0, 0, 3.0] + [0] * 10 + [1.0]
    assert o[1].tolist() == [2.0, 2.0, 1.0, 0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 0, 0]
    f = ms.frequencies()
    assert f[0].tolist() == [0, 0, 0, 0, 0, 1.0] and f[1].tolist() == [0, 0, 1.0, 0, 0, 0] and np.isnan(f[2]).all()
    s = ms.summary()
    assert s["n_skipped"] == 1 and s["mean_E"] == 10 / 3 and s["frequencies"]["K4"] == 0.5
    assert list(s["frequencies"]) == list(GRAPHLETS4)
    assert ms.per_graph()["K4"].tolist() == [1, 0, 0] and ms.per_graph()["one_way"].tolist() == [2, 0, 0]
    both = MotifStats.concat([ms, MotifStats(cen[:1], 4)])
    assert both.n_graphs == 5 and both == MotifStats(np.concatenate([cen, cen[:1]]), 4)
    with pytest.raises(ValueError):
        MotifStats.concat([ms, MotifStats(cen, 5)])
    with pytest.raises(ValueError):
        MotifStats(cen[:, :9], 4)


def test_motif_stats_mmd_equals_a_numpy_restatement():
    from snd_vae_amd.metrics import MotifStats
    a = MotifStats(np.concatenate(BRUTE[:8]), 9)
    b = MotifStats(np.concatenate(BRUTE[8:20] + [np.full((1, 10), -1)]), 9)

    def restated(x, y, sigma):
        k = lambda p, q: np.mean([[np.exp(-np.sum((u - v) ** 2) / (2 * sigma ** 2)) for v in q] for u in p])
        return k(x, x) + k(y, y) - 2 * k(x, y)

    for sigma in (30.0, 2.0):
        want = restated(a.orbits(), b.orbits(), sigma)
        assert want > 0 and abs(a.mmd(b, sigma) - want) <= 1e-12
    assert a.mmd(b) == a.mmd(b, 30.0) and abs(a.mmd(a)) <= 1e-15
    cmp = a.compare(b)
    assert set(cmp) == {"mmd_orbits", "self", "other"} and cmp["mmd_orbits"] == a.mmd(b)
    assert cmp["self"] == a.mean_frequencies() and cmp["other"] == b.mean_frequencies()
    assert np.isnan(a.mmd(MotifStats(np.full((2, 10), -1), 9)))
    assert "GraphRNN" in MotifStats.mmd.__doc__ and "restatement" in MotifStats.mmd.__doc__
    with pytest.raises(ValueError):
        a.mmd(b, 0.0)


# ---------------------------------------------------------------- the C ABI without a device
def test_header_library_and_integration_agree_on_abi_27(lib_built):
    from snd_vae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snd_vae.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    so = ctypes.CDLL(lib_built)
    for name in ("snd_graph_motifs", "snd_graph_motifs_workspace"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(so, name) and name in doc, name
    abi = int(re.search(r"#define\s+SND_ABI_VERSION\s+(\d+)", hdr).group(1))
    stub = int(re.search(r"SND_ABI_VERSION\s*=\s*(\d+)", doc).group(1))
    assert abi == _lib.ABI_VERSION == so.snd_abi_version() == stub and abi >= 27


def test_no_spill_or_scratch_in_the_new_kernels(lib_built):
    from snd_vae_amd.build import build_info, kernel_resources
    names = ("gm_work_kernel", "gm_mutual_kernel", "gm_wedge_kernel", "gm_clique_kernel", "gm_final_kernel")
    res = {k: v for k, v in kernel_resources().items() if any(s in k for s in names)}
    assert len(res) == 5, sorted(res)
    for k, v in res.items():
        assert v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v.get("scratch", 0) == 0, (k, v)
    assert not any("gm_" in k for k in build_info().get("spills", {}))


def test_lds_layout_threshold_of_the_header():
    """Four waves per workgroup while four sets of (two masks + n 16-bit ids) fit in 64 KiB."""
    per_wave = lambda n: (2 * ((n + 31) // 32) + (n + 1) // 2) * 4
    assert 4 * per_wave(M.LDS_THRESHOLD) <= 65536 < 4 * per_wave(M.LDS_THRESHOLD + 1)
    assert 4 * per_wave(M.MAX_N) <= 160 * 1024                 # four one-wave workgroups per CU


class HostArgs:
    """A well-formed argument list over host memory.  No rule below reaches a launch, so nothing
    dereferences these pointers."""

    def __init__(self, _lib, B=2, n=10, cap=40):
        self.L = _lib.lib()
        self._lib = _lib
        self.need = self.L.snd_graph_motifs_workspace(B, n, cap)
        self.bufs = {"rowptr": np.zeros(B * n + 1, np.int32), "colidx": np.zeros(cap, np.int32),
                     "census": np.full(B * 10, 7, np.int64), "work": np.full(B, 7, np.int64),
                     "ws": np.full(self.need // 8 + 1, 7, np.int64)}
        self.args = dict(rowptr=self.bufs["rowptr"].ctypes.data, colidx=self.bufs["colidx"].ctypes.data,
                         nnz_cap=cap, n_graphs=B, n=n, work_cap=1000, census=self.bufs["census"].ctypes.data,
                         work=self.bufs["work"].ctypes.data, ws=self.bufs["ws"].ctypes.data, ws_bytes=self.need)

    def call(self, **kw):
        a = dict(self.args)
        a.update(kw)
        rc = self.L.snd_graph_motifs(*a.values(), None)
        msg = self._lib.last_error() if rc else ""
        for k in ("census", "work", "ws"):
            assert (self.bufs[k] == 7).all(), (kw, k)
        return rc, msg


def test_the_op_rejects_bad_arguments_before_any_launch(lib_built):
    from snd_vae_amd import _lib
    h = HostArgs(_lib)
    assert h.need >= 2 * 80 + 20 * 4 + 40 * 4 and h.need % 16 == 0
    bad = [dict(n_graphs=0), dict(n_graphs=-1), dict(n=0), dict(n=M.MAX_N + 1), dict(n=M.MAX_N, n_graphs=1 << 17),
           dict(nnz_cap=-1), dict(work_cap=-1), dict(rowptr=None), dict(census=None), dict(work=None),
           dict(colidx=None), dict(ws_bytes=h.need - 1), dict(ws=None), dict(ws=h.args["ws"] + 4)]
    for kw in bad:
        rc, msg = h.call(**kw)
        assert rc == -1, (kw, rc)
        assert msg.startswith("snd_graph_motifs:"), (kw, msg)
    assert "workspace" in h.call(ws_bytes=h.need - 1)[1] and "work_cap" in h.call(work_cap=-1)[1]
    assert "colidx" in h.call(colidx=None)[1] and "n=" in h.call(n=0)[1]
    L = h.L
    assert L.snd_graph_motifs_workspace(0, 10, 40) == 0 and L.snd_graph_motifs_workspace(2, M.MAX_N + 1, 40) == 0
    assert L.snd_graph_motifs_workspace(2, 10, -1) == 0 and L.snd_graph_motifs_workspace(1 << 17, M.MAX_N, 0) == 0
    assert L.snd_graph_motifs_workspace(2, 10, 0) == 160 + 80 + 16


def test_layers_checks_without_a_device():
    import torch
    from snd_vae_amd import layers
    rp, ci = torch.zeros(21, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    assert layers.MOTIFS_MAX_N == M.MAX_N and layers.MOTIFS_WORK_CAP > 0
    for kw, match in ((dict(n_graphs=0), "n_graphs"), (dict(n=M.MAX_N + 1), "16384"), (dict(work_cap=-1), "work_cap"),
                      (dict(), "device tensor")):
        a = dict(rowptr=rp, colidx=ci, n_graphs=2, n=10)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            layers.graph_motifs(**a)
