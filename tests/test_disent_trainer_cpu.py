"""Host side of the disentangled trainer (ABI 23): the header and the binding of
snd_disent_losses / snd_margin_eval, the NumPy restatement of the margin histogram
(tests/margin_eval_ref.py) against sklearn through metrics.EdgeCounts and on the values the
bin rule turns on, the per-step normals as a function of (seed, t), and
write_synthetic_dataset(with_rel=True).
"""
import os
import re

import numpy as np
import torch

import margin_eval_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("snd_disent_losses", "snd_margin_eval", "snd_margin_eval_workspace")


def test_header_declares_and_lib_binds_the_ops():
    from snd_vae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snd_vae.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, code), name
        assert name in _lib._SIGS and name in _lib.EXPORTS
    assert len(_lib._SIGS["snd_disent_losses"][1]) == 13
    assert len(_lib._SIGS["snd_margin_eval"][1]) == 10
    assert int(re.search(r"#define\s+SND_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 23
    assert _lib.ABI_VERSION >= 23


def test_library_exports_the_ops(lib_built):
    import ctypes
    so = ctypes.CDLL(lib_built)
    for name in NEW:
        assert hasattr(so, name), name


def test_histogram_gives_sklearn_auc_and_ap():
    """Every distinct margin alone in its bin ((k + 1/2) / 64), so the histogram loses
    nothing: EdgeCounts' ROC-AUC and AP are sklearn's on the raw margins."""
    from sklearn.metrics import average_precision_score, roc_auc_score
    from snd_vae_amd.metrics import EdgeCounts
    rng = np.random.default_rng(7)
    N = 25
    off = ~np.eye(N, dtype=bool)
    k = rng.permutation(np.arange(-1024, 1024))[:N * N - N]
    margin = np.full((1, N, N), -1.0, np.float32)
    margin[0][off] = ((k + 0.5) / 64.0).astype(np.float32)
    adj = (rng.random((1, N, N)) < 0.3).astype(np.float32)
    hist, counts = M.margin_eval_ref(margin, adj)
    assert hist.max() == 1 and hist.sum() == N * N - N
    ec = EdgeCounts(hist, counts)
    y, s = adj[0][off] != 0, margin[0][off].astype(np.float64)
    assert abs(ec.roc_auc - roc_auc_score(y, s)) < 1e-12
    assert abs(ec.average_precision - average_precision_score(y, s)) < 1e-12
    pred = s > 0
    assert (ec.tp, ec.fp, ec.fn) == (int((y & pred).sum()), int((~y & pred).sum()), int((y & ~pred).sum()))
    assert ec.tp + ec.fp + ec.fn + ec.tn == N * N


def test_bin_edges_land_where_the_rule_says():
    vals = np.array([v for v, _ in M.EDGE_VALUES], np.float32)
    want = np.array([b for _, b in M.EDGE_VALUES])
    assert np.array_equal(M.margin_bins(vals), want)
    margin, adj, expect = M.edge_case()
    hist, counts = M.margin_eval_ref(margin, adj)
    N = margin.shape[1]
    off = ~np.eye(N, dtype=bool)
    for label in (0, 1):
        sel = off & ((adj[0] != 0) == bool(label))
        assert np.array_equal(hist[0, label], np.bincount(expect[0][sel], minlength=M.BINS))
    assert hist.sum() == N * N - N and counts.sum() == N * N
    # +-0.0 and every value at or below zero are not predicted edges
    pos = (margin[0] > 0) & off
    assert counts[0, 0] + counts[0, 1] == pos.sum()


def test_diagonal_is_skipped_by_index():
    m, adj = M.random_case(2, 5, seed=3)
    h0, c0 = M.margin_eval_ref(m, adj)
    m2, adj2 = m.copy(), adj.copy()
    m2[:, np.arange(5), np.arange(5)] = 1e30
    adj2[:, np.arange(5), np.arange(5)] = 1.0
    h1, c1 = M.margin_eval_ref(m2, adj2)
    assert np.array_equal(h0, h1) and np.array_equal(c0, c1)
    h, c = M.margin_eval_ref(np.full((1, 1, 1), 3.0, np.float32), np.ones((1, 1, 1), np.float32))
    assert h.sum() == 0 and c.tolist() == [[0, 0, 0, 1]]


def test_step_eps_are_a_function_of_seed_and_step():
    from snd_vae_amd.disent_model import DisentangledConfig
    from snd_vae_amd.disent_trainer import draw_step_eps, eps_shapes
    cfg = DisentangledConfig(sampling_num=3)
    shapes = eps_shapes(cfg, 2)
    assert shapes == {"s": (2, 100), "g": (2, 100), "sg": (6, 100)}
    new = lambda: {k: torch.full(s, 7.0) for k, s in shapes.items()}
    a = draw_step_eps(1234, 5, new())
    draw_step_eps(1234, 6, new())                                       # a draw in between changes nothing
    b = draw_step_eps(1234, 5, new())
    assert all(torch.equal(a[k], b[k]) for k in a)
    for seed, t in ((1234, 6), (1235, 5), (5, 1234)):
        c = draw_step_eps(seed, t, new())
        assert all(not torch.equal(a[k], c[k]) for k in a), (seed, t)
    assert not torch.equal(a["s"], a["g"])
    big = torch.cat([v.reshape(-1) for v in a.values()])
    assert abs(float(big.mean())) < 0.15 and abs(float(big.std()) - 1.0) < 0.15


def test_write_synthetic_dataset_with_rel_round_trips(tmp_path):
    from snd_vae_amd.config import sgjoint
    from snd_vae_amd.input_data import load_data_syn, write_synthetic_dataset
    cfg = sgjoint(12, 16, mean_degree=4.0, sampling_num=2)
    root = str(tmp_path)
    d = write_synthetic_dataset(root, cfg, 3, seed=4)
    assert not os.path.exists(os.path.join(d, "2D_rel.npy"))            # the default is unchanged
    d = write_synthetic_dataset(root, cfg, 3, seed=4, with_rel=True)
    ds = load_data_syn("train", root, sampling_num=2, rng=np.random.RandomState(1), shuffle=False, load_rel=True)
    assert ds.rel is not None and ds.rel.shape == (3, 12, 12)
    sp = ds.spatial
    want = np.sqrt(((sp[:, :, None] - sp[:, None]) ** 2).sum(-1))
    assert np.allclose(ds.rel, want, rtol=1e-6, atol=1e-7)
    assert np.allclose(ds.rel, np.swapaxes(ds.rel, 1, 2)) and np.all(ds.rel[:, np.arange(12), np.arange(12)] == 0)
