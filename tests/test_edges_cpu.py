"""The host side of the generated-graph CSR (snd_zzt_edges) that needs no GPU:
data.generated_batch, and the argument errors of layers.zzt_edges and generate() that are
raised before the library is touched."""
import numpy as np
import pytest
import torch

from snd_vae_amd.config import tscale


def hand_example():
    """Two graphs of three nodes: 0-1, 1-2 in the first, 0-2 in the second."""
    rowptr = np.array([0, 1, 3, 4, 5, 5, 6], np.int32)
    colidx = np.array([1, 0, 2, 1, 5, 3], np.int32)
    x = np.arange(6, dtype=np.float32).reshape(6, 1) / 8
    s = np.arange(12, dtype=np.float32).reshape(6, 2) / 16
    return rowptr, colidx, x, s


def small_cfg(encoder_coords):
    import dataclasses
    cfg = tscale(3, 16, mean_degree=1.0)
    assert cfg.num_feature == 1 and cfg.spatial_dim == 2
    cfg = dataclasses.replace(cfg, encoder_coords=encoder_coords)
    assert cfg.f_in == (3 if encoder_coords else 1)
    return cfg


@pytest.mark.parametrize("coords", [True, False])
def test_generated_batch_hand_example(coords):
    from snd_vae_amd.data import GraphBatch, generated_batch, synthetic_batch
    cfg = small_cfg(coords)
    rowptr, colidx, x, s = hand_example()
    gb = generated_batch(cfg, rowptr, colidx, x, s, 2)
    assert isinstance(gb, GraphBatch) and gb.n_graphs == 2 and gb.n_nodes == 3 and gb.nnz == 6
    assert gb.rowptr.dtype == np.int32 and gb.colidx.dtype == np.int32
    assert np.array_equal(gb.rowptr, rowptr) and np.array_equal(gb.colidx, colidx)
    assert np.array_equal(gb.dense_adj(0), [[0, 1, 0], [1, 0, 1], [0, 1, 0]])
    assert np.array_equal(gb.dense_adj(1), [[0, 0, 1], [0, 0, 0], [1, 0, 0]])
    assert np.array_equal(gb.graph_nnz(), [4, 2])
    assert np.array_equal(gb.feature_truth, x) and np.array_equal(gb.spatial_truth, s)
    want = np.concatenate([x, s], 1) if coords else x
    assert gb.features.dtype == np.float32 and np.array_equal(gb.features, want)
    # the same composition and shapes as a synthetic batch of this configuration
    syn = synthetic_batch(cfg, 2, seed=1)
    assert gb.features.shape == syn.features.shape
    assert np.array_equal(syn.features, np.concatenate([syn.feature_truth, syn.spatial_truth], 1)
                          if coords else syn.feature_truth)
    # a colidx buffer longer than the total (a fixed capacity) is cut at rowptr[-1]
    longer = generated_batch(cfg, rowptr, np.concatenate([colidx, [99, 99]]), x, s, 2)
    assert np.array_equal(longer.colidx, colidx)
    # an empty graph
    empty = generated_batch(cfg, np.zeros(7, np.int32), np.zeros(0, np.int32), x, s, 2)
    assert empty.nnz == 0 and not empty.dense_adj(0).any()


def test_generated_batch_rejects_malformed_csr():
    from snd_vae_amd.data import generated_batch
    cfg = small_cfg(True)
    rowptr, colidx, x, s = hand_example()
    bad = [(rowptr[:-1], colidx), (rowptr, colidx[:-1]),
           (rowptr, np.array([1, 0, 2, 1, 2, 3], np.int32)),          # row 3 reaches into graph 0
           (rowptr, np.array([0, 0, 2, 1, 5, 3], np.int32)),          # a diagonal entry
           (rowptr, np.array([1, 2, 0, 1, 5, 3], np.int32))]          # row 1 descends
    for rp, ci in bad:
        with pytest.raises(ValueError):
            generated_batch(cfg, rp, ci, x, s, 2)
    with pytest.raises(ValueError):
        generated_batch(cfg, rowptr, colidx, x[:, :0], s, 2)


def test_zzt_edges_argument_errors_before_the_library(monkeypatch):
    from snd_vae_amd import _lib, layers

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    z = torch.zeros(6, 4)
    for args, kw in (((z.double(), 2, 3), {}), ((z.t(), 2, 2), {}), ((z[0], 1, 4), {}),
                     ((z, 2, 4), {}), ((z, 0, 3), {}),
                     ((z, 2, 3), {"threshold": float("nan")}),
                     ((z, 2, 3), {"capacity": -1}), ((z, 2, 3), {"capacity": 2.5}),
                     ((z, 2, 3), {})):                                # a host tensor: no CPU path
        with pytest.raises(ValueError, match="zzt_edges"):
            layers.zzt_edges(*args, **kw)


def test_generate_rejects_a_threshold_with_the_dense_format():
    from snd_vae_amd.model import SGCNModelVAE
    model = object.__new__(SGCNModelVAE)                # the check precedes any use of the plan
    for kw in ({"threshold": 0.5}, {"inclusive": True}, {"threshold": float("-inf")},
               {"adj_format": "dense", "threshold": -1.0}):
        with pytest.raises(ValueError, match="csr"):
            model.generate(None, mode="prior", **kw)
    with pytest.raises(ValueError, match="adj_format"):
        model.generate(None, mode="prior", adj_format="coo")
