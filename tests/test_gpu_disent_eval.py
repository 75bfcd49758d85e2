"""``DisentangledSGCNModelVAE.latent_means`` and ``DisentTrainer.evaluate_disentanglement``
on a ``write_factor_dataset`` set: 40 graphs at N = 25 and the reference's (synthetic2)
widths, S = 3 spanning-tree copies, batch size 10, after two training steps.

The evaluation must equal ``metrics.LatentMI`` built from the NumPy restatement
(tests/latent_mi_ref.py) applied to the read-back means and ``dataset.factor``: the joint
counts exactly, mi / hz / hf to 1e-11 (the bound of tests/test_gpu_latent_mi.py).  Nothing is
asserted about how well a two-step model disentangles.
"""
import dataclasses

import numpy as np
import pytest
import torch

import latent_mi_ref as MR

pytestmark = pytest.mark.gpu

N, S, B, GRAPHS, EXTRA = 25, 3, 10, 40, 5
STATE = ("params", "m", "v", "step_counter")
TOL = 1e-11


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


@pytest.fixture(scope="module")
def dataset45(tmp_path_factory):
    from snd_vae_amd.config import sgjoint
    from snd_vae_amd.input_data import load_data_syn, write_factor_dataset
    root = str(tmp_path_factory.mktemp("factor_ds"))
    write_factor_dataset(root, sgjoint(N, 20, mean_degree=4.0, sampling_num=S), GRAPHS + EXTRA, seed=2)
    return load_data_syn("train", root, sampling_num=S, rng=np.random.RandomState(1))


def first_graphs(ds, n):
    return dataclasses.replace(ds, node=ds.node[:n], spatial=ds.spatial[:n], adj_truth=ds.adj_truth[:n],
                               trees=ds.trees[:n], rel=ds.rel[:n], factor=ds.factor[:n])


def make_trainer(ds):
    from snd_vae_amd.disent_model import DisentangledConfig, init_blocks
    from snd_vae_amd.disent_trainer import DisentTrainer
    cfg = DisentangledConfig(n_nodes=N, sampling_num=S)
    blocks = {k: v.astype(np.float32).astype(np.float64) for k, v in init_blocks(cfg, 0).items()}
    t = DisentTrainer(cfg, ds, B, blocks=blocks)
    t.step(0)
    t.step(1)
    return t


@pytest.fixture(scope="module")
def trained(dataset45):
    return make_trainer(first_graphs(dataset45, GRAPHS))


def state(model):
    return {k: getattr(model, k).clone() for k in STATE}


def test_latent_means_is_the_concatenation_of_the_encoder_means(trained):
    from snd_vae_amd.disent_model import mean_over_copies
    t = trained
    cfg = t.cfg
    width = cfg.s_latent + cfg.g_latent + cfg.sg_latent
    cols = t.model.latent_groups_columns()
    assert list(cols) == ["s", "g", "sg"] and cols["sg"].stop == width
    b = t.batches[1]
    enc = t.model.encode(b)
    want = torch.cat([enc["s"]["mu"], enc["g"]["mu"], mean_over_copies(enc["sg"]["mu"], S)], dim=1)
    got = t.model.latent_means(b)
    assert tuple(got.shape) == (B, width) and got.dtype == torch.float32
    assert torch.equal(got, want)
    # into a row block of a caller-owned matrix, and into a column block of a wider one
    big = torch.full((3 * B, width), float("nan"), device="cuda")
    ret = t.model.latent_means(b, out=big[B:2 * B])
    assert ret.data_ptr() == big[B:2 * B].data_ptr() and torch.equal(big[B:2 * B], want)
    assert torch.isnan(big[:B]).all() and torch.isnan(big[2 * B:]).all()
    wide = torch.full((B, width + 8), float("nan"), device="cuda")
    t.model.latent_means(b, out=wide[:, 4:4 + width])
    assert torch.equal(wide[:, 4:4 + width], want) and torch.isnan(wide[:, :4]).all() and torch.isnan(wide[:, -4:]).all()
    for bad in (torch.empty(B, width - 1, device="cuda"), torch.empty(B + 1, width, device="cuda"),
                torch.empty(B, width, device="cuda", dtype=torch.float64), torch.empty(B, width)):
        with pytest.raises(ValueError, match="latent_means"):
            t.model.latent_means(b, out=bad)


def reference(t, factor, n_bins, factor_bins):
    z = torch.cat([t.model.latent_means(b) for b in t.batches]).cpu().numpy()
    f = np.asarray(factor, np.float32)
    assert z.shape[0] == f.shape[0]
    return z, f, MR.latent_mi_ref(z, f, n_bins, factor_bins)


def assert_equals_the_restatement(t, ev, factor, n_bins, factor_bins):
    from snd_vae_amd import layers
    from snd_vae_amd.metrics import LatentMI
    z, f, ref = reference(t, factor, n_bins, factor_bins)
    got = ev["latent_mi"]
    want = LatentMI(ref["mi"], ref["hz"], ref["hf"], t.model.latent_groups_columns())
    assert isinstance(got, LatentMI) and got.groups == want.groups and list(got.groups) == ["s", "g", "sg"]
    assert got.mi.shape == (z.shape[1], 3)
    for k in ("mi", "hz", "hf"):
        err = float(np.max(np.abs(getattr(got, k) - getattr(want, k))))
        print(f"{k}: max abs err {err:.3e}")
        assert err <= TOL, (k, err)
    # the counts behind it, exactly
    joint = layers.latent_mi(torch.from_numpy(z).cuda(), torch.from_numpy(f).cuda(), n_bins, factor_bins,
                             want_joint=True)[3]
    assert np.array_equal(joint.cpu().numpy(), ref["joint"])
    for k in ("mig", "avg_mi", "modularity"):
        assert ev[k] == getattr(got, k)() and np.isfinite(ev[k])
        assert abs(ev[k] - getattr(want, k)()) <= 1e-6, k
    assert np.array_equal(ev["group_share"], got.group_share()) and ev["group_share"].shape == (3, 3)
    assert len(ev["best_latent"]) == 3 and ev["groups"] == ["s", "g", "sg"]


def test_evaluate_disentanglement_equals_the_restatement_and_writes_no_state(trained):
    t = trained
    before = state(t.model)
    ev = t.evaluate_disentanglement()
    after = state(t.model)
    for k in STATE:
        assert torch.equal(before[k], after[k]), k
    assert t.global_step == 2 and int(t.model.step_counter.item()) == 2
    assert_equals_the_restatement(t, ev, t.dataset.factor, 20, 20)
    ev5 = t.evaluate_disentanglement(n_bins=12, factor_bins=5)            # 5 levels in 5 bins
    assert_equals_the_restatement(t, ev5, t.dataset.factor, 12, 5)
    hf = ev5["latent_mi"].hf
    for k in range(3):
        p = np.bincount(t.dataset.factor[:, k].astype(np.int64), minlength=5) / GRAPHS
        assert abs(hf[k] + np.sum(p[p > 0] * np.log(p[p > 0]))) <= TOL
    again = t.evaluate_disentanglement()
    assert again["latent_mi"] == ev["latent_mi"]                          # bitwise repeatable
    t.step(2)                                                             # training goes on
    assert t.global_step == 3


def test_the_leftover_graphs_are_excluded(dataset45):
    t = make_trainer(dataset45)
    assert t.batch_num == 4 and t.dataset.n_graphs == GRAPHS + EXTRA
    ev = t.evaluate_disentanglement()
    assert_equals_the_restatement(t, ev, dataset45.factor[:GRAPHS], 20, 20)


def test_bad_factors_raise(dataset45, trained):
    t = trained
    good = t.dataset
    try:
        for bad, match in ((None, "no generative factors"), (good.factor[:, 0], r"\[n_graphs, K\]"),
                           (dataset45.factor, "no alignment is guessed")):
            t.dataset = dataclasses.replace(good, factor=bad)
            with pytest.raises(ValueError, match=match):
                t.evaluate_disentanglement()
    finally:
        t.dataset = good
