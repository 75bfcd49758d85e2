"""The disentanglement evaluation without a GPU (``snd_latent_mi``, ABI 25): the float64
restatement of the op (tests/latent_mi_ref.py) against sklearn and scipy on its own bin labels,
the bin rule on its edges, ``metrics.LatentMI`` on planted matrices, every SND_ERR_ARG rule
through ctypes (they return before the device is touched), the header, the exports and the ABI
number, ``input_data.write_factor_dataset`` and the factor validation of
``DisentTrainer.evaluate_disentanglement``."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import latent_mi_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("rows,L,K,nbz,nbf", [(1000, 6, 3, 20, 20), (257, 4, 2, 7, 5), (64, 3, 1, 32, 2),
                                              (1, 2, 2, 20, 20)])
def test_restatement_equals_sklearn_and_scipy(rows, L, K, nbz, nbf):
    import scipy.stats
    from sklearn.metrics import mutual_info_score
    z, f = MR.random_case(rows, L, K, seed=rows)
    r = MR.latent_mi_ref(z, f, nbz, nbf)
    assert r["joint"].shape == (L, K, nbz, nbf) and np.all(r["joint"].sum((2, 3)) == rows)
    for l in range(L):
        for k in range(K):
            want = mutual_info_score(r["zb"][:, l], r["fb"][:, k])
            assert abs(r["mi"][l, k] - want) <= 1e-12, (l, k, r["mi"][l, k], want)
            assert abs(MR.mi_of(r["joint"][l, k], rows) - r["mi"][l, k]) <= 1e-15
        assert abs(r["hz"][l] - scipy.stats.entropy(np.bincount(r["zb"][:, l], minlength=nbz))) <= 1e-12
    for k in range(K):
        assert abs(r["hf"][k] - scipy.stats.entropy(np.bincount(r["fb"][:, k], minlength=nbf))) <= 1e-12
    assert np.all(r["mi"] >= -1e-15) and np.all(r["mi"] <= np.minimum.outer(r["hz"], r["hf"]) + 1e-12)


@pytest.mark.parametrize("nb", [1, 2, 5, 20, 32])
def test_values_on_interior_edges_go_to_their_bin_and_the_maximum_to_the_last(nb):
    v = np.arange(nb + 1, dtype=np.float32)                  # lo = 0, hi = nb: the edges are the integers
    b = MR.bin_column(v, v.min(), v.max(), nb)
    assert np.array_equal(b[:-1], np.arange(nb)) and b[-1] == nb - 1
    below = np.nextafter(v[1:], np.float32(0))               # just under an edge: the bin before it
    assert np.array_equal(MR.bin_column(below, 0.0, float(nb), nb), np.arange(nb))


def test_a_constant_column_has_bin_zero_no_entropy_and_no_information():
    z, f = MR.random_case(100, 3, 2, seed=1)
    z[:, 1] = 3.25
    f[:, 0] = -7.0
    r = MR.latent_mi_ref(z, f, 20, 5)
    assert np.all(r["zb"][:, 1] == 0) and np.all(r["fb"][:, 0] == 0)
    assert r["hz"][1] == 0.0 and r["hf"][0] == 0.0
    assert np.all(r["mi"][1] == 0.0) and np.all(r["mi"][:, 0] == 0.0)
    assert np.array_equal(r["range"][1], [3.25, 3.25]) and np.array_equal(r["range"][3], [-7.0, -7.0])


@pytest.mark.parametrize("k", [2, 3, 5, 7, 20, 32])
def test_k_equally_spaced_factor_values_fill_k_bins(k):
    for lo, step in ((0.0, 1.0), (-3.0, 0.5), (10.0, 0.1), (1.0, 1e-3)):
        v = (lo + step * np.arange(k)).astype(np.float32)
        b = MR.bin_column(v, v.min(), v.max(), k)
        assert np.array_equal(b, np.arange(k)), (k, lo, step, b)


# ---------------------------------------------------------------- metrics.LatentMI
GROUPS3 = {"s": slice(0, 1), "g": slice(1, 2), "sg": slice(2, 3)}


def test_planted_copies_score_as_disentangled():
    from snd_vae_amd.metrics import LatentMI
    rng = np.random.default_rng(0)
    rows, levels = 5000, 5
    f = rng.integers(0, levels, size=(rows, 2)).astype(np.float32)
    z = np.stack([f[:, 0], f[:, 1], rng.standard_normal(rows).astype(np.float32)], axis=1)
    r = MR.latent_mi_ref(z, f, levels, levels)
    m = LatentMI(r["mi"], r["hz"], r["hf"], GROUPS3)
    R = m.normalised()
    assert abs(R[0, 0] - 1.0) <= 1e-12 and abs(R[1, 1] - 1.0) <= 1e-12
    off = [max(R[1, 0], R[2, 0]), max(R[0, 1], R[2, 1])]
    assert max(off) < 0.01
    assert abs(m.mig() - (1.0 - np.mean(off))) <= 1e-12
    assert 0.0 <= m.avg_mi() < 1e-4
    assert abs(m.avg_mi() - (R[1, 0] ** 2 + R[2, 0] ** 2 + R[0, 1] ** 2 + R[2, 1] ** 2
                             + (R[0, 0] - 1) ** 2 + (R[1, 1] - 1) ** 2) / 2) <= 1e-15
    share = m.group_share()
    assert share.shape == (2, 3) and share[0, 0] > 0.99 and share[1, 1] > 0.99
    assert np.allclose(share.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert m.best_latent() == [("s", 0), ("g", 0)]
    # the two copies are modular; the noise latent's two estimation-bias values are of one size,
    # so it scores anything in [0, 1]: the mean is the formula's, and at least 2/3 of a clean 1
    m2 = r["mi"] ** 2
    per = [1.0 - m2[l].min() / m2[l].max() for l in range(3)]
    assert per[0] > 0.999 and per[1] > 0.999 and 0.0 <= per[2] <= 1.0
    assert abs(m.modularity() - np.mean(per)) <= 1e-15
    s = m.summary()
    assert set(s) == {"mig", "avg_mi", "modularity", "group_share", "best_latent", "groups"}
    assert s["groups"] == ["s", "g", "sg"] and s["mig"] == m.mig()


def test_one_latent_copying_two_factors_costs_modularity_by_the_formula():
    from snd_vae_amd.metrics import LatentMI
    hz, hf = np.ones(2), np.ones(2)
    clean = LatentMI([[1.0, 0.0], [0.0, 0.5]], hz, hf)
    assert clean.modularity() == 1.0
    both = LatentMI([[1.0, 1.0], [0.0, 0.5]], hz, hf)       # latent 0: 1 - 1 / (1 (2 - 1)) = 0; latent 1: 1
    assert both.modularity() == 0.5
    part = LatentMI([[1.0, 0.5, 0.5], [0.0, 0.0, 0.0]], np.ones(2), np.ones(3))
    assert abs(part.modularity() - (1.0 - (0.25 + 0.25) / (1.0 * 2))) <= 1e-15    # the dead latent is left out
    assert both.mig() == np.mean([1.0 - 0.0, 1.0 - 0.5])
    # ties go to the lowest index: T = [[1, 1], [0, 0]]
    tie = LatentMI([[0.5, 0.5], [0.5, 0.5]], hz, hf)
    assert tie.avg_mi() == (0.25 * 4) / 2 and tie.mig() == 0.0 and tie.best_latent() == [("z", 0), ("z", 0)]


def test_edge_cases_one_factor_one_latent_and_a_dead_factor():
    from snd_vae_amd.metrics import LatentMI
    one_factor = LatentMI([[0.2], [0.6], [0.1]], np.ones(3), [0.8])
    assert one_factor.modularity() == 1.0
    assert abs(one_factor.mig() - (0.6 - 0.2) / 0.8) <= 1e-15
    assert one_factor.best_latent() == [("z", 1)]
    one_latent = LatentMI([[0.3, 0.6]], [1.0], [0.6, 1.2])
    assert abs(one_latent.mig() - 0.5) <= 1e-15                # the second largest is 0
    assert abs(one_latent.avg_mi() - 0.25) <= 1e-15            # ((0.5 - 1)^2 + (0.5 - 1)^2) / 2
    dead = LatentMI([[0.4, 0.0], [0.1, 0.0]], np.ones(2), [0.8, 0.0])
    R = dead.normalised()
    assert np.array_equal(R[:, 1], [0.0, 0.0]) and np.all(np.isfinite(R))
    assert abs(dead.mig() - (0.5 - 0.125)) <= 1e-15            # over the live factor only
    assert np.array_equal(dead.group_share()[1], [0.0])
    none = LatentMI(np.zeros((2, 2)), np.zeros(2), np.zeros(2))
    assert math.isnan(none.mig()) and math.isnan(none.modularity())
    assert np.array_equal(none.group_share(), np.zeros((2, 1)))


def test_latent_mi_rejects_bad_shapes_and_groups():
    from snd_vae_amd.metrics import LatentMI
    with pytest.raises(ValueError):
        LatentMI(np.zeros((2, 2)), np.zeros(3), np.zeros(2))
    with pytest.raises(ValueError):
        LatentMI(np.zeros((2, 2)), np.zeros(2), np.zeros(2), {"s": slice(0, 1)})               # latent 1 uncovered
    with pytest.raises(ValueError):
        LatentMI(np.zeros((2, 2)), np.zeros(2), np.zeros(2), {"s": slice(0, 2), "g": slice(1, 2)})
    a = LatentMI(np.eye(2), np.ones(2), np.ones(2))
    assert a == LatentMI(np.eye(2), np.ones(2), np.ones(2)) and a != LatentMI(np.eye(2), np.ones(2), 2 * np.ones(2))
    assert a.tensors is None and a.n_latents == 2 and a.n_factors == 2
    a.invalidate()                                              # host arrays stay
    assert a.mig() == 1.0


# ---------------------------------------------------------------- the C ABI without a device
def test_header_and_library_declare_the_op(lib_built):
    from snd_vae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snd_vae.h")).read()
    so = ctypes.CDLL(lib_built)
    for name in ("snd_latent_mi", "snd_latent_mi_workspace"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert hasattr(so, name), name
    abi = int(re.search(r"#define\s+SND_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert abi == _lib.ABI_VERSION == so.snd_abi_version() and abi >= 25      # 25 introduced the entry points
    assert "floor(i k / (k - 1)) = i" in hdr                                  # the k-levels-in-k-bins statement


def test_no_spill_or_scratch_in_the_new_kernels(lib_built):
    from snd_vae_amd.build import kernel_resources
    res = {k: v for k, v in kernel_resources().items()
           if any(s in k for s in ("mi_range_kernel", "mi_range_final_kernel", "mi_count_kernel", "mi_reduce_kernel"))}
    assert len(res) == 4, sorted(res)
    for k, v in res.items():
        assert v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v.get("scratch", 0) == 0, (k, v)


class HostArgs:
    """A well-formed argument list over host memory.  No rule below reaches a launch, so
    nothing dereferences these pointers."""

    def __init__(self, _lib, rows=10, L=4, K=3, nbz=20, nbf=5):
        self.L, self._lib = _lib.lib(), _lib
        self.d = dict(rows=rows, n_lat=L, n_fac=K, nbz=nbz, nbf=nbf, ldz=L, ldf=K)
        self.need = self.L.snd_latent_mi_workspace(rows, L, K, nbz, nbf)
        self.keep = {"z": np.zeros(rows * L, np.float32), "f": np.zeros(rows * K, np.float32),
                     "mi": np.zeros(L * K), "hz": np.zeros(L), "hf": np.zeros(K),
                     "range": np.zeros(2 * (L + K), np.float32), "joint": np.zeros(L * K * nbz * nbf, np.int32),
                     "ws": np.zeros(max(self.need, 1), np.uint8)}

    def call(self, **kw):
        a = dict(self.d, ws_bytes=self.need, **{k: v.ctypes.data for k, v in self.keep.items()})
        a.update(kw)
        rc = self.L.snd_latent_mi(a["z"], a["ldz"], a["f"], a["ldf"], a["rows"], a["n_lat"], a["n_fac"], a["nbz"],
                                  a["nbf"], a["mi"], a["hz"], a["hf"], a["range"], a["joint"], a["ws"], a["ws_bytes"],
                                  None)
        return rc, self._lib.last_error()


def test_the_op_rejects_bad_arguments_before_any_launch(lib_built):
    from snd_vae_amd import _lib
    h = HostArgs(_lib)
    assert h.need > 0
    bad = ([{k: None} for k in ("z", "f", "mi", "hz", "hf", "ws")]
           + [dict(rows=0), dict(rows=-1), dict(n_lat=0), dict(n_lat=65537, ldz=65537, ws_bytes=1 << 40),
              dict(n_fac=0), dict(n_fac=65, ldf=65, ws_bytes=1 << 40), dict(nbz=0), dict(nbz=33, ws_bytes=1 << 40),
              dict(nbf=0), dict(nbf=33, ws_bytes=1 << 40), dict(nbz=-1), dict(ldz=3), dict(ldf=2),
              dict(ws_bytes=h.need - 1), dict(ws_bytes=0)])
    for kw in bad:
        rc, msg = h.call(**kw)
        assert rc == -1, (kw, rc)
        assert msg.startswith("snd_latent_mi:"), (kw, msg)
    for k in ("z", "f", "mi", "hz", "hf"):
        assert "null operand" in h.call(**{k: None})[1], k
    assert "workspace" in h.call(ws_bytes=h.need - 1)[1] and "workspace" in h.call(ws=None)[1]
    assert "ldz" in h.call(ldz=3)[1] and "ldf" in h.call(ldf=2)[1]
    assert "rows" in h.call(rows=0)[1] and "n_lat" in h.call(n_lat=0)[1] and "n_fac" in h.call(n_fac=65, ldf=65)[1]
    assert "bins" in h.call(nbz=33)[1] and "bins" in h.call(nbf=0)[1]
    assert not any(v.any() for v in h.keep.values())                         # nothing was written
    # a bad shape has no workspace size; the limits themselves are fine shapes
    W = h.L.snd_latent_mi_workspace
    assert W(0, 4, 3, 20, 5) == 0 and W(10, 0, 3, 20, 5) == 0 and W(10, 65537, 3, 20, 5) == 0
    assert W(10, 4, 0, 20, 5) == 0 and W(10, 4, 65, 20, 5) == 0
    assert W(10, 4, 3, 0, 5) == 0 and W(10, 4, 3, 33, 5) == 0 and W(10, 4, 3, 20, 0) == 0 and W(10, 4, 3, 20, 33) == 0
    assert W(1, 1, 1, 1, 1) > 0 and W(10, 65536, 64, 32, 32) >= 65536 * 64 * 32 * 32 * 4
    # the workspace grows with the counts it holds
    assert W(10, 4, 3, 20, 5) - W(10, 4, 3, 10, 5) == 4 * 3 * 10 * 5 * 4


def test_layers_latent_mi_validates_before_the_library():
    import torch
    from snd_vae_amd import layers
    z, f = torch.zeros(4, 3), torch.zeros(4, 2)
    with pytest.raises(ValueError, match="device tensor"):
        layers.latent_mi(z, f)                                                # host tensors: there is no CPU path


# ---------------------------------------------------------------- write_factor_dataset
S, N = 3, 25


def data_cfg():
    from snd_vae_amd.config import sgjoint
    return sgjoint(N, 20, mean_degree=4.0, sampling_num=S)


def test_factor_dataset_round_trips_and_takes_every_level(tmp_path):
    from snd_vae_amd.input_data import FACTOR_NAMES, factor_graph, load_data_syn, write_factor_dataset
    cfg, G, levels = data_cfg(), 40, 5
    write_factor_dataset(str(tmp_path), cfg, G, seed=2, levels=levels)
    ds = load_data_syn("train", str(tmp_path), sampling_num=S, rng=np.random.RandomState(1), shuffle=False)
    assert FACTOR_NAMES == ("spatial", "graph", "joint")
    assert ds.n_graphs == G and ds.factor.shape == (G, 3) and ds.rel.shape == (G, N, N)
    for k in range(3):
        assert np.array_equal(np.unique(ds.factor[:, k]), np.arange(levels)), k
    for g in (0, 7, G - 1):
        adj, coords, x = factor_graph(cfg, ds.factor[g], 2 + 1 + g)
        assert np.array_equal(ds.dense_adj(g), adj.astype(np.float32))
        assert np.allclose(ds.spatial[g], coords, rtol=0, atol=1e-12)
        assert np.allclose(ds.node[g], x, rtol=0, atol=1e-12)
        d = np.sqrt(((coords[:, None] - coords[None]) ** 2).sum(-1))
        assert np.allclose(ds.rel[g], d, rtol=0, atol=1e-12)
    # the shuffled load keeps every graph with its factors
    sh = load_data_syn("train", str(tmp_path), sampling_num=S, rng=np.random.RandomState(1))
    assert sh.factor.shape == (G, 3) and not np.array_equal(sh.factor, ds.factor)
    for g in (0, 5):
        src = next(i for i in range(G) if np.array_equal(ds.spatial[i], sh.spatial[g]))
        assert np.array_equal(sh.factor[g], ds.factor[src])
    # the same seed writes the same dataset
    other = tmp_path / "again"
    write_factor_dataset(str(other), cfg, G, seed=2, levels=levels, with_rel=False)
    assert np.array_equal(np.load(other / "train" / "2D_prop.npy"), ds.factor)
    assert not (other / "train" / "2D_rel.npy").exists()


def test_each_factor_changes_only_what_it_claims():
    from snd_vae_amd.input_data import factor_graph
    cfg, levels = data_cfg(), 5
    for seed in (11, 12, 13):
        base = factor_graph(cfg, (2, 2, 2), seed)
        for lv in range(levels):
            # spatial: geometry only, a scaling about the centre
            adj, coords, x = factor_graph(cfg, (lv, 2, 2), seed)
            assert np.array_equal(adj, base[0]) and np.array_equal(x, base[2])
            assert np.allclose((coords - 0.5) * (0.5 + 0.1 * 2), (base[1] - 0.5) * (0.5 + 0.1 * lv), rtol=0, atol=1e-15)
            assert (lv == 2) == np.array_equal(coords, base[1])
            # graph: topology only, lv edges on top of the level-0 graph
            adj, coords, x = factor_graph(cfg, (2, lv, 2), seed)
            none = factor_graph(cfg, (2, 0, 2), seed)[0]
            assert np.array_equal(coords, base[1]) and np.array_equal(x, base[2])
            assert np.array_equal(adj, adj.T) and not adj.diagonal().any()
            assert np.all(adj[none]) and (adj.sum() - none.sum()) // 2 == lv
            # joint: the radius; the coordinates stay, the edges grow with the level
            adj, coords, x = factor_graph(cfg, (2, 0, lv), seed)
            assert np.array_equal(coords, base[1]) and np.array_equal(x, base[2])
            if lv:
                smaller = factor_graph(cfg, (2, 0, lv - 1), seed)[0]
                assert np.all(adj[smaller]) and adj.sum() > smaller.sum()
            d = np.sqrt(((coords[:, None] - coords[None]) ** 2).sum(-1))
            assert adj[~np.eye(N, dtype=bool)].sum() > 0
            # joined iff close: the topology is a function of the geometry
            assert d[adj].max() < d[~adj & ~np.eye(N, dtype=bool)].min()


# ---------------------------------------------------------------- evaluate_disentanglement's validation
def test_the_factor_validation_raises_on_missing_flat_and_misaligned_factors(tmp_path):
    from snd_vae_amd.disent_trainer import dataset_factors
    from snd_vae_amd.input_data import load_data_syn, write_factor_dataset
    import dataclasses
    cfg = data_cfg()
    write_factor_dataset(str(tmp_path), cfg, 12, seed=1)
    write_factor_dataset(str(tmp_path), cfg, 5, seed=2, split="test")
    ds = load_data_syn("train", str(tmp_path), sampling_num=0, rng=np.random.RandomState(1))
    f = dataset_factors(ds)
    assert f.dtype == np.float32 and f.shape == (12, 3) and f.flags.c_contiguous and np.array_equal(f, ds.factor)
    assert np.array_equal(dataset_factors(ds, 10), ds.factor[:10].astype(np.float32))   # the leftover graphs are cut
    with pytest.raises(ValueError, match="no generative factors"):
        dataset_factors(dataclasses.replace(ds, factor=None))
    with pytest.raises(ValueError, match=r"\[n_graphs, K\]"):
        dataset_factors(dataclasses.replace(ds, factor=ds.factor[:, 0]))
    with pytest.raises(ValueError, match="no alignment is guessed"):
        dataset_factors(dataclasses.replace(ds, factor=ds.factor[:11]))
    # the test split reads the training split's factors (input_data.py:101): 12 rows for 5 graphs
    test = load_data_syn("test", str(tmp_path), sampling_num=0, rng=np.random.RandomState(1), shuffle=False)
    assert test.n_graphs == 5 and test.factor.shape[0] == 12
    with pytest.raises(ValueError, match="12 rows for 5 graphs"):
        dataset_factors(test)
