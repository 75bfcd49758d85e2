"""Graph statistics at the model and trainer level, on a small node-latent model (N = 70,
B = 2): generate(adj_format="csr", stats=True), SGCNModelVAE.graph_stats and
Trainer.evaluate_generation against tests/graph_stats_ref.py on the read-back tensors.
"""
import math

import numpy as np
import pytest
import torch

import graph_stats_ref as G

pytestmark = pytest.mark.gpu

N, B = 70, 2
MAX_LEN = math.sqrt(2.0)


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def _cfg():
    from snd_vae_amd.config import tscale
    return tscale(N, 16, mean_degree=6.0)


def _ref_equal(gs, rp, ci, coords, what):
    """gs (a GraphStats over device tensors) equals the reference on the host copies; the edge
    lengths under the margin rule, which the operands are first shown to satisfy."""
    scale = np.float32(256.0 / MAX_LEN)
    assert len(G.ambiguous_edges(rp, ci, B, N, coords, scale)) == 0, what
    ref = G.ref_stats(rp, ci, B, N, coords, scale)
    assert gs.tensors is not None and gs.n == N and gs.max_len == MAX_LEN
    G.assert_stats_equal({"hist": gs.hist, "totals": gs.totals}, ref, N, what)
    return ref


def test_generate_stats_and_batch_stats():
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    cfg = _cfg()
    batch = synthetic_batch(cfg, B, seed=31)
    model = SGCNModelVAE(cfg, B, dtype="f32", seed=4)
    db = DeviceBatch(batch)

    plain = model.generate(db, mode="mean", adj_format="csr")
    assert "generated_stats" not in plain
    out = model.generate(db, mode="mean", adj_format="csr", stats=True)
    assert set(out) == set(plain) | {"generated_stats"}
    for k in ("generated_rowptr", "generated_colidx", "generated_spatial"):
        assert torch.equal(out[k], plain[k]), k
    rp, ci = out["generated_rowptr"].cpu().numpy(), out["generated_colidx"].cpu().numpy()
    ref = _ref_equal(out["generated_stats"], rp, ci, out["generated_spatial"].cpu().numpy(), "generated")
    assert 0 < out["generated_nnz"] == ref["totals"][:, 0].sum()         # symmetric, no self loops
    assert out["generated_stats"].n_edges * 2 == out["generated_nnz"]

    with pytest.raises(ValueError, match="stats"):
        model.generate(db, mode="mean", stats=True)

    gs = model.graph_stats(db)
    ref = _ref_equal(gs, batch.rowptr, batch.colidx, np.asarray(batch.spatial_truth, np.float32), "batch")
    assert ref["totals"][:, 0].sum() == batch.nnz and gs.summary()["mean_degree"] == batch.nnz / (B * N)


def test_trainer_evaluate_generation(tmp_path):
    from snd_vae_amd.input_data import load_data_syn, write_synthetic_dataset
    from snd_vae_amd.metrics import GraphStats
    from snd_vae_amd.trainer import Trainer
    cfg = _cfg()
    write_synthetic_dataset(str(tmp_path), cfg, 4, seed=11)
    np.random.seed(1)
    ds = load_data_syn("train", str(tmp_path), sampling_num=2)
    t = Trainer(cfg, ds, batch_size=B, dtype="f32")
    assert t.batch_num == 2
    t.train_epoch()                                 # captured graphs and Adam state exist
    o = t.opt
    state = [x.clone() for x in (t.model.params, o.m, o.v, o.step_counter)]

    res = t.evaluate_generation()                   # prior, at evaluate()'s best-F1 threshold
    assert res["threshold"] == t.evaluate("prior")["best_f1_threshold"]
    for kind in ("degree", "clustering", "edge_length"):
        assert math.isfinite(res[f"mmd_{kind}"]) and res[f"mmd_{kind}"] >= -1e-12, (kind, res[f"mmd_{kind}"])
    data, gen = res["dataset"], res["generated"]
    assert isinstance(data, GraphStats) and data.n_graphs == gen.n_graphs == 4
    assert data == GraphStats.concat([t.model.graph_stats(b) for b in t.batches])
    assert data.n_edges * 2 == sum(b.nnz for b in t.batches)
    assert res["self"] == data.summary() and res["other"] == gen.summary()

    # the reconstruction at L > 0 holds exactly the pairs evaluate() counts as predicted
    rec = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False)
    ev = t.evaluate("mean")
    assert int(rec["generated"].totals[:, 0].sum()) == ev["tp"] + ev["fp"] > 0

    for x, y in zip(state, (t.model.params, o.m, o.v, o.step_counter)):
        assert torch.equal(x, y)
    with pytest.raises(ValueError, match="mode"):
        t.evaluate_generation(mode="sample")
    t.train_epoch()                                 # the captured graphs still replay
    assert o.global_step == 4
