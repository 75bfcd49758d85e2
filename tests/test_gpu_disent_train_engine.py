"""The disentangled model and ``DisentTrainer`` with ``e2e_engine="factorised"`` (the training
structure decoder behind ``snd_e2e_train``), at the shapes of tests/test_gpu_disent_trainer.py:
reference widths, N = 25, S = 3, B = 2, a dataset of 6 graphs (3 batches).

* the first ``step_device`` against the float64 oracle on DESIGN.md §3's bars (``compare`` of
  tests/test_gpu_disent_model.py) for disentangled, beta-TCVAE and base, and the same step
  under the direct engine; three Adam steps of
  disentangled on the bars tests/test_gpu_disent_model.py applies;
* step_device == step, replay == eager, resume == uninterrupted: bitwise;
* a checkpoint saved under one engine restores under the other (the engine is not part of
  the config);
* with the default engine a step is bitwise what a model built without the argument does;
* ``disent.structure_decoder(..., grads_out=...)`` writes what it returns without it, under
  either engine.
"""
import os

import numpy as np
import pytest
import torch

from oracle import ref_disent_model as RM
from oracle import ref_numpy as R
from test_gpu_disent_model import compare, dense_trees
from test_gpu_disent_trainer import B, GRAPHS, N, S, blocks, data_cfg, model_cfg, same_history, same_state, state, trainer

pytestmark = pytest.mark.gpu
ENGINE = "factorised"


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from snd_vae_amd.input_data import load_data_syn, write_synthetic_dataset
    root = str(tmp_path_factory.mktemp("disent_engine_ds"))
    write_synthetic_dataset(root, data_cfg(), GRAPHS, seed=3, with_rel=True)
    return load_data_syn("train", root, sampling_num=S, rng=np.random.RandomState(1))


def oracle_inputs(dataset):
    from snd_vae_amd.input_data import dataset_sg_batch
    hb = dataset_sg_batch(dataset, data_cfg(), range(B))
    return {"x": hb.feature_truth.reshape(B, N, -1), "spatial": hb.spatial_truth.reshape(B, N, 2),
            "adj": np.stack([hb.dense_adj(g) for g in range(B)]), "x_sg": hb.features.reshape(B * S, N, -1),
            "trees": dense_trees(hb), "rel": hb.rel}


@pytest.mark.parametrize("engine", ["factorised", "direct"])
@pytest.mark.parametrize("model_type", ["disentangled", "beta-TCVAE", "base"])
def test_first_step_device_against_the_float64_oracle(dataset, model_type, engine):
    """The trainer's own first step (seed 1234, init_blocks seed 0, batch 0: the operands of
    tests/test_gpu_disent_trainer.py::test_first_step_against_the_float64_oracle).

    Under both engines: beta-TCVAE at B = 2 is the hard case for either, because the two
    softmaxes of the total-correlation gradient nearly cancel there
    (tests/test_gpu_latent_reg_small_batch.py).  With fp32 sums in snd_latent_reg's TC block the
    step is 2.178e-4 (factorised) / 2.179e-4 (direct) of max-abs off on encoder_g/gamma against a
    bar of 2e-4; with the block in double, 2.6e-6 under both."""
    from snd_vae_amd.disent_model import LOSS_NAMES
    from snd_vae_amd.disent_trainer import draw_step_eps
    cfg = model_cfg(model_type=model_type)
    t = trainer(dataset, cfg, use_graphs=False, e2e_engine=engine)
    assert t.model.e2e_engine == engine
    t.step(0)
    got = dict(zip(LOSS_NAMES, t.model.losses.cpu().tolist()))
    if model_type == "base":
        got = {k: v for k, v in got.items() if k not in ("kl_g", "kl_s")}
    eps = {k: v.double().cpu().numpy() for k, v in draw_step_eps(t.seed, 0, t.eps).items()}
    p = blocks(cfg)
    ref, rg = RM.disent_forward_backward(p, oracle_inputs(dataset), eps, cfg)
    compare(got, ref, t.model.grad_blocks(), rg, (engine, model_type), p, oracle_inputs(dataset), eps, cfg)


def test_three_adam_steps_against_the_float64_oracle(dataset):
    from snd_vae_amd.disent_trainer import draw_step_eps
    cfg = model_cfg()
    t = trainer(dataset, cfg, use_graphs=False, e2e_engine=ENGINE)
    ins = oracle_inputs(dataset)
    p = blocks(cfg)
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    for step in range(1, 4):
        eps = draw_step_eps(t.seed, step - 1, t.eps)
        got = t.model.step(t.batches[0], eps)
        e64 = {k: e.double().cpu().numpy() for k, e in eps.items()}
        ref, rg = RM.disent_forward_backward(p, ins, e64, cfg)
        compare(got, ref, t.model.grad_blocks(), rg, (ENGINE, step), p, ins, e64, cfg)
        R.adam_tf1(p, rg, m, v, step, cfg.learning_rate, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps)
        now = t.model.blocks()
        for k in p:     # Adam normalises each update to ~lr: compare against the step size
            assert np.abs(now[k] - p[k]).max() < 0.05 * step * cfg.learning_rate, (step, k)


def test_step_device_equals_step(dataset):
    from snd_vae_amd.disent_model import LOSS_NAMES, DisentangledSGCNModelVAE
    from snd_vae_amd.disent_trainer import draw_step_eps, eps_shapes
    cfg = model_cfg()
    batch = trainer(dataset, cfg, use_graphs=False).batches[1]
    eps = draw_step_eps(9, 0, {k: torch.empty(*s, device="cuda") for k, s in eps_shapes(cfg, B).items()})
    p = blocks(cfg, 1)
    a = DisentangledSGCNModelVAE(cfg, B, blocks=p, e2e_engine=ENGINE)
    b = DisentangledSGCNModelVAE(cfg, B, blocks=p, e2e_engine=ENGINE)
    got = a.step(batch, eps)
    assert b.step_device(batch, eps) is None
    same_state(state(a), state(b), ENGINE)
    assert torch.equal(a.grads, b.grads) and int(b.step_counter) == 1
    losses = dict(zip(LOSS_NAMES, b.losses.cpu().tolist()))
    for k, v in got.items():
        if k == "correct":
            assert losses[k] == v
        else:
            assert abs(losses[k] - v) <= 1e-12 * abs(v), (k, losses[k], v)


def test_the_default_engine_is_the_direct_one_bit_for_bit(dataset):
    from snd_vae_amd.disent_model import DisentangledSGCNModelVAE
    from snd_vae_amd.disent_trainer import draw_step_eps, eps_shapes
    cfg = model_cfg()
    batch = trainer(dataset, cfg, use_graphs=False).batches[0]
    eps = draw_step_eps(4, 0, {k: torch.empty(*s, device="cuda") for k, s in eps_shapes(cfg, B).items()})
    p = blocks(cfg, 2)
    a, b = DisentangledSGCNModelVAE(cfg, B, blocks=p), DisentangledSGCNModelVAE(cfg, B, blocks=p, e2e_engine="direct")
    assert a.e2e_engine == "direct"
    a.step_device(batch, eps)
    b.step_device(batch, eps)
    same_state(state(a), state(b), "default engine")
    assert torch.equal(a.grads, b.grads) and torch.equal(a.losses, b.losses)
    f = DisentangledSGCNModelVAE(cfg, B, blocks=p, e2e_engine=ENGINE)
    f.step_device(batch, eps)
    assert not torch.equal(f.grads, a.grads)                            # another summation order
    with pytest.raises(ValueError, match="e2e_engine"):
        DisentangledSGCNModelVAE(cfg, B, blocks=p, e2e_engine="fused")


@pytest.fixture(scope="module")
def runs(dataset, tmp_path_factory):
    """A replayed factorised trainer after 2 epochs (saved there) and after 3."""
    from types import SimpleNamespace as NS
    r = NS(path=os.path.join(str(tmp_path_factory.mktemp("disent_engine_ck")), "two.safetensors"))
    t = trainer(dataset, e2e_engine=ENGINE)
    t.train(2)
    torch.cuda.synchronize()
    r.two, r.hist_two = state(t.model), list(t.history)
    t.save(r.path)
    t.train(1)
    r.three, r.hist_three = state(t.model), list(t.history)
    return r


def test_replay_equals_eager(dataset, runs):
    e = trainer(dataset, use_graphs=False, e2e_engine=ENGINE)
    e.train(2)
    same_state(runs.two, state(e.model), "replay vs eager")
    same_history(runs.hist_two, e.history)
    assert e.global_step == 6 and int(runs.two["step_counter"]) == 6


def test_resume_equals_uninterrupted(dataset, runs):
    t = trainer(dataset, e2e_engine=ENGINE)
    assert t.restore(runs.path) == 6 and t.epoch == 2
    same_state(runs.two, state(t.model), "restored")
    t.train(1)
    same_state(runs.three, state(t.model), "resumed")
    same_history(runs.hist_three[2:], t.history)


def test_a_checkpoint_restores_under_the_other_engine(dataset, runs, tmp_path):
    d = trainer(dataset, use_graphs=False)                              # direct
    assert d.restore(runs.path) == 6 and d.epoch == 2
    same_state(runs.two, state(d.model), "factorised -> direct")
    d.train(1)
    path = os.path.join(str(tmp_path), "direct.safetensors")
    d.save(path)
    f = trainer(dataset, use_graphs=False, e2e_engine=ENGINE)
    assert f.restore(path) == 9 and f.epoch == 3
    same_state(state(d.model), state(f.model), "direct -> factorised")
    f.train(1)
    assert np.isfinite(f.history[-1]["loss"]).all()


@pytest.mark.parametrize("engine", ["direct", "factorised"])
def test_structure_decoder_writes_into_grads_out(engine):
    """``grads_out`` receives what the call returns without it, bit for bit, under either engine."""
    import e2e_train_ref as TR
    from snd_vae_amd import disent
    c = TR.operands(2, 7, 3, (5, 4), seed=0)
    cu = lambda a: torch.from_numpy(a).cuda()
    z, adj = cu(c.z), cu(c.adj)
    layers, head = [{k: cu(v) for k, v in l.items()} for l in c.layers], {k: cu(v) for k, v in c.head.items()}
    ce, correct, dz, lg, hg = disent.structure_decoder(z, adj, layers, head, engine=engine)
    dst = ([{k: torch.full_like(v, float("nan")) for k, v in l.items()} for l in layers],
           {k: torch.full_like(v, float("nan")) for k, v in head.items()})
    ce2, correct2, dz2, lg2, hg2 = disent.structure_decoder(z, adj, layers, head, engine=engine, grads_out=dst)
    assert (ce2, correct2) == (ce, correct) and torch.equal(dz2, dz)
    assert lg2 is dst[0] and hg2 is dst[1]
    for a, b in zip(lg + [hg], dst[0] + [dst[1]]):
        for k in ("gamma", "beta", "w", "b"):
            assert torch.equal(a[k].view(-1), b[k].view(-1)), (engine, k)
    rce, rcorrect = TR.train_ref(c.z, c.adj, c.layers, c.head)[:2]
    assert ce == pytest.approx(rce, rel=1e-5) and correct == rcorrect
