"""DisentTrainer (snd_vae_amd/disent_trainer.py) and the sync-free step of the disentangled
model, at the shape of tests/test_gpu_disent_model.py: reference widths, N = 25, S = 3,
B = 2, a dataset of 6 graphs written to a temporary directory (3 batches).

* step_device() against step(): the same launches, so parameters, gradients and Adam state
  are bitwise equal; the loss terms differ only in the order the sse partials are summed
  (1e-12 relative), the count of correct entries is exact.
* a replayed run against an eager one, a resumed run against an uninterrupted one and the
  capacity schedule against an eager loop: bitwise.
* the first step against the float64 oracle on the bars of tests/test_gpu_disent_model.py.
* evaluate() / evaluate_generation() against the NumPy restatements
  (tests/margin_eval_ref.py, tests/graph_stats_ref.py).
"""
import math
import os

import numpy as np
import pytest
import torch

import graph_stats_ref as G
import margin_eval_ref as M
from test_gpu_disent_model import compare, dense_trees

pytestmark = pytest.mark.gpu

N, S, B, GRAPHS = 25, 3, 2, 6
STATE = ("params", "m", "v", "step_counter")


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def data_cfg():
    from snd_vae_amd.config import sgjoint
    return sgjoint(N, 20, mean_degree=4.0, sampling_num=S)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from snd_vae_amd.input_data import load_data_syn, write_synthetic_dataset
    root = str(tmp_path_factory.mktemp("disent_ds"))
    write_synthetic_dataset(root, data_cfg(), GRAPHS, seed=3, with_rel=True)
    return load_data_syn("train", root, sampling_num=S, rng=np.random.RandomState(1))


def model_cfg(**kw):
    from snd_vae_amd.disent_model import DisentangledConfig
    return DisentangledConfig(n_nodes=N, sampling_num=S, **kw)


def blocks(cfg, seed=0):
    from snd_vae_amd.disent_model import init_blocks
    return {k: v.astype(np.float32).astype(np.float64) for k, v in init_blocks(cfg, seed).items()}


def trainer(dataset, cfg=None, **kw):
    from snd_vae_amd.disent_trainer import DisentTrainer
    cfg = cfg or model_cfg()
    kw.setdefault("use_graphs", True)
    return DisentTrainer(cfg, dataset, B, blocks=blocks(cfg), **kw)


def state(model):
    return {k: getattr(model, k).clone() for k in STATE}


def same_state(a, b, what):
    for k in STATE:
        assert torch.equal(a[k], b[k]), (what, k)


def same_history(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            if k != "epoch_time":
                assert np.array_equal(x[k], y[k]), k


# --------------------------------------------------------------- step_device == step
@pytest.mark.parametrize("model_type,kw", [("disentangled", {}), ("beta-TCVAE", {}), ("NED-VAE-IP", {}),
                                           ("disentangled_C", {"capacity": 0.5, "gamma": 2.0}), ("base", {})])
def test_step_device_equals_step(dataset, model_type, kw):
    from snd_vae_amd.disent_model import LOSS_NAMES, DisentangledSGCNModelVAE
    from snd_vae_amd.disent_trainer import draw_step_eps, eps_shapes
    cfg = model_cfg(model_type=model_type, **kw)
    tr = trainer(dataset, cfg, use_graphs=False)                        # for its batches
    batch = tr.batches[1]
    eps = draw_step_eps(9, 0, {k: torch.empty(*s, device="cuda") for k, s in eps_shapes(cfg, B).items()})
    p = blocks(cfg, 1)
    a, b = DisentangledSGCNModelVAE(cfg, B, blocks=p), DisentangledSGCNModelVAE(cfg, B, blocks=p)
    got = a.step(batch, eps)
    assert b.step_device(batch, eps) is None
    same_state(state(a), state(b), model_type)
    assert torch.equal(a.grads, b.grads) and int(b.step_counter) == 1
    losses = dict(zip(LOSS_NAMES, b.losses.cpu().tolist()))
    assert set(got) == set(LOSS_NAMES) - ({"kl_g", "kl_s"} if model_type == "base" else set())
    for k, v in got.items():
        if k == "correct":
            assert losses[k] == v
        else:
            assert abs(losses[k] - v) <= 1e-12 * abs(v), (k, losses[k], v)
    if model_type == "base":
        assert losses["kl_g"] == 0.0 and losses["kl_s"] == 0.0


# --------------------------------------------------- replay == eager, resume == uninterrupted
@pytest.fixture(scope="module")
def runs(dataset, tmp_path_factory):
    """A replayed trainer after 2 epochs (saved there) and after 3."""
    from types import SimpleNamespace as NS
    r = NS(path=os.path.join(str(tmp_path_factory.mktemp("disent_ck")), "two.safetensors"))
    t = trainer(dataset)
    t.train(2)
    torch.cuda.synchronize()
    r.two, r.hist_two = state(t.model), list(t.history)
    r.global_step_two = t.global_step
    t.save(r.path)
    t.train(1)
    r.three, r.hist_three = state(t.model), list(t.history)
    return r


def test_replay_equals_eager(dataset, runs):
    e = trainer(dataset, use_graphs=False)
    e.train(2)
    same_state(runs.two, state(e.model), "replay vs eager")
    same_history(runs.hist_two, e.history)
    assert runs.global_step_two == e.global_step == 6 and int(runs.two["step_counter"]) == 6
    h = e.history[-1]
    assert set(h) == {"loss", "spatial_loss", "adj_loss", "adj_acc", "node_loss", "graph_kl", "spatial_kl", "sg_kl",
                      "epoch_time", "capacity"}
    assert all(h[k].shape == (3,) and np.isfinite(h[k]).all() for k in h if k not in ("epoch_time", "capacity"))
    assert np.all((h["adj_acc"] > 0.5) & (h["adj_acc"] <= 1.0))


def test_resume_equals_uninterrupted(dataset, runs):
    from snd_vae_amd import checkpoint as ckpt
    from snd_vae_amd.config import PRESETS
    from snd_vae_amd.model import SGCNModelVAE
    t = trainer(dataset)
    assert t.restore(runs.path) == 6 and t.epoch == 2 and t.global_step == 6
    same_state(runs.two, state(t.model), "restored")
    t.train(1)
    same_state(runs.three, state(t.model), "resumed")
    same_history(runs.hist_three[2:], t.history)
    assert ckpt.read_disent_config(runs.path) == model_cfg()
    other = trainer(dataset, model_cfg(beta=2.0))
    with pytest.raises(ValueError, match="config"):
        other.restore(runs.path)
    with pytest.raises(ValueError, match="layout"):
        trainer(dataset, model_cfg(g_hidden=64)).restore(runs.path)
    node_latent = SGCNModelVAE(PRESETS["SG25"].replace(sampling_num=S), B, dtype="f32")
    with pytest.raises(ValueError, match="disentangled"):
        ckpt.restore(runs.path, node_latent)
    with pytest.raises(ValueError, match="disentangled"):
        ckpt.read_config(runs.path)
    back = os.path.join(os.path.dirname(runs.path), "node_latent.safetensors")
    ckpt.save(back, node_latent)
    with pytest.raises(ValueError, match="node-latent"):
        ckpt.restore(back, t.model, t.model)
    with pytest.raises(ValueError):
        ckpt.read_disent_config(back)


def test_train_saves_checkpoints(dataset, tmp_path):
    t = trainer(dataset, use_graphs=False)
    t.train(3, checkpoint_dir=str(tmp_path), save_every=2)
    assert sorted(os.listdir(str(tmp_path))) == ["model_dgt_global_0.safetensors", "model_dgt_global_2.safetensors"]
    r = trainer(dataset, use_graphs=False)
    assert r.restore(os.path.join(str(tmp_path), "model_dgt_global_2.safetensors")) == 9 and r.epoch == 3
    same_state(state(t.model), state(r.model), "checkpoint of the last epoch")


# -------------------------------------------------------------- first step against the oracle
def test_first_step_against_the_float64_oracle(dataset):
    from oracle import ref_disent_model as RM
    from snd_vae_amd.disent_model import LOSS_NAMES
    from snd_vae_amd.disent_trainer import draw_step_eps
    from snd_vae_amd.input_data import dataset_sg_batch
    t = trainer(dataset)
    cfg = t.cfg
    hb = dataset_sg_batch(dataset, data_cfg(), range(B))
    ins = {"x": hb.feature_truth.reshape(B, N, -1), "spatial": hb.spatial_truth.reshape(B, N, 2),
           "adj": np.stack([hb.dense_adj(g) for g in range(B)]), "x_sg": hb.features.reshape(B * S, N, -1),
           "trees": dense_trees(hb), "rel": hb.rel}
    t.step(0)
    got = dict(zip(LOSS_NAMES, t.model.losses.cpu().tolist()))
    eps = {k: v.double().cpu().numpy() for k, v in draw_step_eps(t.seed, 0, t.eps).items()}
    p = blocks(cfg)
    ref, rg = RM.disent_forward_backward(p, ins, eps, cfg)
    compare(got, ref, t.model.grad_blocks(), rg, "trainer step 0", p, ins, eps, cfg)


# ------------------------------------------------------------------------ capacity schedule
def test_capacity_schedule(dataset):
    from snd_vae_amd.disent_model import DisentangledSGCNModelVAE
    from snd_vae_amd.disent_trainer import draw_step_eps
    cfg = model_cfg(model_type="disentangled_C", gamma=2.0)
    t = trainer(dataset, cfg, c_max=1.0, c_step=1, c_stop_iter=2)
    t.train(3)
    assert [float(h["capacity"][0]) for h in t.history] == [0.0, 0.5, 1.0]
    m = DisentangledSGCNModelVAE(cfg, B, blocks=blocks(cfg))
    step = 0
    for c in (0.0, 0.5, 1.0):
        for b in t.batches:
            m.step_device(b, draw_step_eps(t.seed, step, t.eps), capacity=c)
            step += 1
    same_state(state(t.model), state(m), "capacity schedule")
    fixed = trainer(dataset, cfg)                                       # no schedule: cfg.capacity throughout
    fixed.train(2)
    assert not torch.equal(fixed.model.params, t.model.params)
    assert [float(h["capacity"][0]) for h in fixed.history] == [0.0, 0.0]


# ------------------------------------------------------------------------------- evaluation
@pytest.fixture(scope="module")
def trained(dataset):
    """A trainer after one epoch whose d_e_lin2 bias puts the decision threshold into the
    widest gap of the central fifth of the reconstruction's margins: both classes are
    predicted, and no margin is close enough to zero for two decoders to disagree on it."""
    t = trainer(dataset)
    t.train(1)
    off = ~np.eye(N, dtype=bool)
    m = np.sort(np.concatenate([t.model.generate(b, z="mean", want_margin=True)["margin"].cpu().numpy()[:, off].ravel()
                                for b in t.batches]).astype(np.float64))
    lo, hi = int(0.4 * len(m)), int(0.6 * len(m))
    k = lo + int(np.argmax(np.diff(m[lo:hi])))
    assert m[k + 1] - m[k] > 1e-4 * max(abs(m[0]), abs(m[-1]))
    t.model.w("d_e_lin2/bias")[1] -= float(0.5 * (m[k] + m[k + 1]))
    return t


def test_evaluate(trained):
    from snd_vae_amd.metrics import EdgeCounts
    t = trained
    before = state(t.model)
    ev = t.evaluate()
    same_state(before, state(t.model), "evaluate")
    ref = EdgeCounts.zeros(B)
    ones = correct = 0
    node = spatial = 0.0
    for b in t.batches:
        gen = t.model.generate(b, z="mean", want_margin=True)
        ref = ref + EdgeCounts(*M.margin_eval_ref(gen["margin"].cpu().numpy(), b.adj_dense.cpu().numpy()))
        ones += int(gen["generated_adj"].sum())
        assert t.model.evaluate(b) == EdgeCounts(*M.margin_eval_ref(gen["margin"].cpu().numpy(),
                                                                    b.adj_dense.cpu().numpy()))
        node += float(((gen["generated_node_feat"].double().reshape(-1) - b.x.double().reshape(-1)) ** 2).sum())
        spatial += float(((gen["generated_spatial"].double().reshape(-1) - b.spatial.double().reshape(-1)) ** 2).sum())
        # structure_decoder's count for the same latents: a step with eps = 0 decodes the means
        saved = [x.clone() for x in (t.model.params, t.model.m, t.model.v, t.model.step_counter, t.model.grads)]
        correct += t.model.step(b, {k: torch.zeros_like(v) for k, v in t.eps.items()})["correct"]
        for dst, src in zip((t.model.params, t.model.m, t.model.v, t.model.step_counter, t.model.grads), saved):
            dst.copy_(src)
    tot = ev["edge_counts"]
    assert tot == ref.total()
    assert tot.tp + tot.fp == ones and 0.25 < ones / (GRAPHS * (N * N - N)) < 0.75
    assert tot.tp + tot.tn == correct and ev["accuracy"] == correct / (GRAPHS * N * N)
    assert ev["node_mse"] == pytest.approx(node / (GRAPHS * N), rel=1e-12)
    assert ev["spatial_mse"] == pytest.approx(spatial / (GRAPHS * N * 2), rel=1e-12)
    assert 0.0 <= ev["roc_auc"] <= 1.0
    buf = EdgeCounts.zeros(B, device="cuda")
    for b in t.batches:
        assert t.model.evaluate(b, out=buf) is buf
    assert buf.total() == tot
    with pytest.raises(ValueError, match="mode"):
        t.evaluate("prior")


def test_evaluate_generation(trained):
    from snd_vae_amd.metrics import GraphStats
    t = trained
    before = state(t.model)
    rec = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False)
    same_state(before, state(t.model), "evaluate_generation")
    scale = np.float32(256.0 / math.sqrt(2.0))
    data = []
    for i, b in enumerate(t.batches):
        adj = t.model.generate(b, z="mean")["generated_adj"].cpu().numpy()
        g, r, c = np.nonzero(adj)
        rp, ci = (x.cpu().numpy().astype(np.int64) for x in rec["generated_csr"][i])
        rows = np.repeat(np.arange(B * N), np.diff(rp))
        assert len(g) > 0 and np.array_equal(rows, g * N + r) and np.array_equal(ci, g * N + c)
        rp, ci, xy = b.rowptr.cpu().numpy(), b.colidx.cpu().numpy(), b.spatial.cpu().numpy()
        assert len(G.ambiguous_edges(rp, ci, B, N, xy, scale)) == 0
        data.append(G.ref_stats(rp, ci, B, N, xy, scale))
    want = GraphStats(np.concatenate([d["hist"] for d in data]), np.concatenate([d["totals"] for d in data]), N,
                      math.sqrt(2.0))
    assert rec["dataset"] == want and rec["dataset"].n_graphs == rec["generated"].n_graphs == GRAPHS
    ev = t.evaluate()
    assert int(rec["generated"].totals[:, 0].sum()) == ev["tp"] + ev["fp"] and rec["threshold"] == 0.0
    prior = t.evaluate_generation()                                     # prior samples at evaluate()'s best-F1 threshold
    assert prior["threshold"] == ev["best_f1_threshold"]
    for kind in ("degree", "clustering", "edge_length"):
        assert math.isfinite(prior[f"mmd_{kind}"])
    with pytest.raises(ValueError, match="mode"):
        t.evaluate_generation(mode="sample")
    t.train(1)                                                          # the captured graphs still replay
    assert t.global_step == 6
