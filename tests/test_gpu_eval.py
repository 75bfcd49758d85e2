"""snd_zzt_eval (fused zz^T evaluation: edge-score histograms and confusion counts) on the GPU.

* Exact: z on small dyadic grids, so every product and partial sum is exact in fp32 and the
  float64 NumPy histogram must be matched bit for bit, whatever the summation order.
* Real-valued z: the histogram may differ from the float64 one only on pairs whose logit lies
  within the fmaf-chain bound of a bin edge; the exact AUC lies within the binned AUC's
  resolution.
* accumulate, the model-level identities against generate() / adj_accuracy, Trainer.evaluate,
  and the arguments rejected before launch.
"""
import functools

import numpy as np
import pytest
import torch

import abi_ops as A

pytestmark = pytest.mark.gpu

BINS = 2048


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


# ------------------------------------------------------------------ operands and reference
def random_adjacency(rng, B, n, p=0.06):
    """Symmetric 0/1 adjacencies without self loops: rows 3 and 7 empty, graph 1 of a batch
    of three or more without any edge, row 5 of graph 0 of degree 70 where n allows."""
    out = []
    for b in range(B):
        a = np.triu(rng.random((n, n)) < p, 1)
        a = a | a.T
        for r in (3, 7):
            if r < n:
                a[r, :] = a[:, r] = False
        if b == 0 and n > 80:
            a[5, :] = a[:, 5] = False
            nb = 8 + rng.permutation(n - 8)[:70]
            a[5, nb] = a[nb, 5] = True
        if b == 1 and B >= 3:
            a[:] = False
        out.append(a)
    return out


def csr_of(adjs, rng):
    """Block-diagonal CSR with global column ids, the entries of every row shuffled."""
    n = adjs[0].shape[0]
    rp, ci = [0], []
    for b, a in enumerate(adjs):
        for r in range(n):
            c = np.nonzero(a[r])[0]
            ci.append(rng.permutation(c) + b * n)
            rp.append(rp[-1] + len(c))
    ci = np.concatenate(ci) if rp[-1] else np.zeros(0, np.int64)
    return np.asarray(rp, np.int32), ci.astype(np.int32)


def reference(z, adjs):
    """hist [B, 2, 2048], counts [B, 4] and the float64 logits of fp32 z [B, n, d]."""
    B, n, _ = z.shape
    hist = np.zeros((B, 2, BINS), np.int64)
    counts = np.zeros((B, 4), np.int64)
    off = ~np.eye(n, dtype=bool)
    logits = []
    for b in range(B):
        zb = z[b].astype(np.float64)
        L = zb @ zb.T
        a = adjs[b]
        bins = np.clip(np.floor(L * 64.0) + 1024.0, 0, BINS - 1).astype(np.int64)
        hist[b] = np.bincount((a.astype(np.int64) * BINS + bins)[off], minlength=2 * BINS).reshape(2, BINS)
        pred = L > 0
        counts[b] = ((pred & a & off).sum(), (pred & ~a & off).sum(), (~pred & a & off).sum(),
                     (~pred & ~a & off).sum() + n)
        logits.append(L)
    return hist, counts, logits


EXACT_SHAPES = [(3, 200, 16), (2, 129, 64), (1, 25, 20), (2, 384, 128)]


@functools.lru_cache(maxsize=None)
def exact_case(B, n, d):
    rng = np.random.default_rng(1000 * B + n + d)
    m = 16 if d <= 20 else (8 if d <= 64 else 4)       # multiples of 1/8; narrower for wide d
    z = rng.integers(-m, m + 1, size=(B, n, d)).astype(np.float32) / 8.0
    z[:, [0, 1, 11]] *= 4.0                             # a few rows reach past +-16
    adjs = random_adjacency(rng, B, n)
    rp, ci = csr_of(adjs, rng)
    hist, counts, _ = reference(z, adjs)
    for v in (z, rp, ci, hist, counts):
        v.setflags(write=False)
    return z, adjs, rp, ci, hist, counts


def dev_csr(rp, ci):
    rowptr = torch.from_numpy(rp.copy()).cuda()                 # the cached cases are read-only
    colidx = torch.from_numpy(ci.copy()).cuda() if ci.size else torch.zeros(1, dtype=torch.int32, device="cuda")
    return rowptr, colidx


def run_op(z, rp, ci, **kw):
    from snd_vae_amd import layers
    B, n, d = z.shape
    rowptr, colidx = dev_csr(rp, ci)
    hist, counts = layers.zzt_eval(torch.from_numpy(z.reshape(B * n, d).copy()).cuda(), rowptr, colidx, B, n, **kw)
    torch.cuda.synchronize()
    return hist.cpu().numpy(), counts.cpu().numpy()


# ------------------------------------------------------------------ exact
def test_exact_cases_reach_both_end_bins():
    hs = [exact_case(*s)[4] for s in EXACT_SHAPES]
    assert any(h[:, :, 0].sum() > 0 for h in hs) and any(h[:, :, BINS - 1].sum() > 0 for h in hs)
    assert any(h[:, 1, 0].sum() + h[:, 1, BINS - 1].sum() > 0 for h in hs)     # labelled pairs too
    z, adjs = exact_case(3, 200, 16)[:2]
    assert not adjs[1].any() and adjs[0][5].sum() > 63 and not adjs[0][3].any()
    zb = z[0].astype(np.float64)
    assert ((zb @ zb.T)[~np.eye(200, dtype=bool)] == 0).any()       # L == 0: bin 1024, not predicted


@pytest.mark.parametrize("B,n,d", EXACT_SHAPES)
def test_exact_histogram_and_counts(B, n, d):
    z, adjs, rp, ci, hist, counts = exact_case(B, n, d)
    got_h, got_c = run_op(z, rp, ci)
    for b in range(B):
        nnz = int(adjs[b].sum())
        assert got_h[b, 1].sum() == nnz and got_h[b, 0].sum() == n * n - n - nnz
        assert got_c[b].sum() == n * n
    assert np.array_equal(got_c, counts), (got_c, counts)
    assert np.array_equal(got_h, hist), int(np.abs(got_h - hist).sum())


@pytest.mark.parametrize("ld,offset", [(72, 0), (67, 1)], ids=["ld72_aligned", "ld67_unaligned"])
def test_exact_strided_guarded(ld, offset):
    """ldz > d through the raw entry point, with guard bands around z, hist and counts (the
    int64 outputs ride in the helpers' 8-byte "f64" buffers)."""
    from snd_vae_amd import _lib
    B, n, d = 2, 129, 64
    z, adjs, rp, ci, hist, counts = exact_case(B, n, d)
    bufs = {"z": A.guarded(B * n, d, ld, "f32", offset, z.reshape(B * n, d), "z"),
            "hist": A.guarded(B, 2 * BINS, None, "f64", 0, None, "hist"),
            "counts": A.guarded(B, 4, None, "f64", 0, None, "counts")}
    dev = {k: torch.from_numpy(g.arr).cuda() for k, g in bufs.items()}
    ptr = {k: dev[k].data_ptr() + g.off * g.arr.itemsize for k, g in bufs.items()}
    rowptr, colidx = dev_csr(rp, ci)
    L = _lib.lib()
    assert L.snd_zzt_eval_workspace(B, n, d) == 0
    _lib.check(L.snd_zzt_eval(ptr["z"], ld, B, n, d, _lib.ptr(rowptr), _lib.ptr(colidx), ptr["hist"],
                              ptr["counts"], 0, None, 0, _lib.stream_ptr()), "snd_zzt_eval")
    torch.cuda.synchronize()
    after = {k: t.cpu().numpy() for k, t in dev.items()}
    for k, g in bufs.items():
        g.check_untouched(after[k])
    assert np.array_equal(after["z"].view(np.uint32), bufs["z"].arr.view(np.uint32))
    got_h = np.ascontiguousarray(bufs["hist"].block(after["hist"])).view(np.int64).reshape(B, 2, BINS)
    got_c = np.ascontiguousarray(bufs["counts"].block(after["counts"])).view(np.int64).reshape(B, 4)
    assert np.array_equal(got_h, hist) and np.array_equal(got_c, counts)


# ------------------------------------------------------------------ real-valued
def test_real_valued_within_fmaf_bound():
    """z = 0.5 randn (B, N, d) = (2, 200, 64) against float64 logits of the same fp32 z.

    An fp32 fmaf chain of d terms is within delta_ij = gamma_d sum_k |z_ik z_jk| of the exact
    logit (gamma_d = d u / (1 - d u), u = 2^-24), so only the M pairs within delta of a bin
    edge may land in a neighbouring bin, each moving two histogram cells by one:
    sum |hist_gpu - hist_ref| <= 2 M, and M <= 2 % of the pairs so the bound means something.
    The AUC of the exact scores differs from the binned AUC by at most half of the pairs that
    the binning (and a one-bin move) cannot order: 1/2 sum_b pos_b neg'_b / (P N), neg'_b the
    negatives of bins b - 1 .. b + 1."""
    from sklearn.metrics import roc_auc_score
    from snd_vae_amd.metrics import EdgeCounts
    B, n, d = 2, 200, 64
    rng = np.random.default_rng(77)
    z = (0.5 * rng.standard_normal((B, n, d))).astype(np.float32)
    adjs = random_adjacency(rng, B, n)
    rp, ci = csr_of(adjs, rng)
    hist, counts, logits = reference(z, adjs)
    got_h, got_c = run_op(z, rp, ci)
    u = 2.0 ** -24
    gamma = d * u / (1.0 - d * u)
    off = ~np.eye(n, dtype=bool)
    M = 0
    for b in range(B):
        az = np.abs(z[b].astype(np.float64))
        delta = gamma * (az @ az.T)
        s = logits[b] * 64.0
        edge = np.clip(np.rint(s), -1023, 1023)                 # the nearest edge between two bins
        M += int(((np.abs(s - edge) / 64.0 <= delta) & off).sum())
    pairs = B * (n * n - n)
    diff = int(np.abs(got_h - hist).sum())
    print(f"EVAL_REAL pairs {pairs} M {M} ({M / pairs:.4%}) sum|dhist| {diff} "
          f"count diffs {np.abs(got_c - counts).sum(axis=0).tolist()}")
    assert M <= 0.02 * pairs, (M, pairs)
    assert diff <= 2 * M, (diff, M)
    assert got_h.sum() == pairs and np.array_equal(got_h.sum(axis=2), hist.sum(axis=2))
    assert np.abs(got_c - counts).sum() <= 2 * M and np.array_equal(got_c.sum(axis=1), counts.sum(axis=1))

    ec = EdgeCounts(got_h, got_c)
    y = np.concatenate([adjs[b][off] for b in range(B)])
    s = np.concatenate([logits[b][off] for b in range(B)])
    exact = roc_auc_score(y, s)
    tot = got_h.sum(axis=0)
    neg, pos = tot[0].astype(np.float64), tot[1].astype(np.float64)
    wide = neg.copy()
    wide[1:] += neg[:-1]
    wide[:-1] += neg[1:]
    bound = 0.5 * float((pos * wide).sum()) / (pos.sum() * neg.sum())
    print(f"EVAL_REAL auc exact {exact:.9f} binned {ec.roc_auc:.9f} bound {bound:.3e}")
    assert abs(exact - ec.roc_auc) <= bound, (exact, ec.roc_auc, bound)


# ------------------------------------------------------------------ accumulate
def test_accumulate_and_clear():
    from snd_vae_amd import layers
    B, n, d = 2, 129, 64
    z, adjs, rp, ci, hist, counts = exact_case(B, n, d)
    rowptr, colidx = dev_csr(rp, ci)
    zt = torch.from_numpy(z.reshape(B * n, d).copy()).cuda()
    h = torch.zeros(B, 2, BINS, dtype=torch.int64, device="cuda")
    c = torch.zeros(B, 4, dtype=torch.int64, device="cuda")
    for _ in range(2):
        layers.zzt_eval(zt, rowptr, colidx, B, n, h, c, accumulate=True)
    assert np.array_equal(h.cpu().numpy(), 2 * hist) and np.array_equal(c.cpu().numpy(), 2 * counts)
    h.fill_(-12345)
    c.fill_(7)
    rh, rc = layers.zzt_eval(zt, rowptr, colidx, B, n, h, c, accumulate=False)
    assert rh is h and rc is c
    assert np.array_equal(h.cpu().numpy(), hist) and np.array_equal(c.cpu().numpy(), counts)


# ------------------------------------------------------------------ model level
@pytest.mark.parametrize("preset,dtype", [("C1s", "f32"), ("C1s", "bf16"), ("C1", "f32"), ("C1", "bf16"),
                                          ("SG25", "f32")])
def test_model_evaluate_agrees_with_generate(preset, dtype):
    """Node latent (C1s), graph latent (C1) and the spatial-graph encoder (SG25):
    evaluate() and generate() threshold the same fp32 fmaf chains: per graph TP + FP is the
    number of generated ones, TP the generated ones on CSR positions, and the accuracy is
    adj_accuracy to the last bit."""
    from snd_vae_amd.config import PRESETS
    from snd_vae_amd.data import sgjoint_batch, synthetic_batch
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE, adj_accuracy
    cfg = PRESETS[preset]
    assert cfg.n_nodes == (25 if preset == "SG25" else 200)
    batch = sgjoint_batch(cfg, 2, seed=31) if preset == "SG25" else synthetic_batch(cfg, 2, seed=31)
    model = SGCNModelVAE(cfg, 2, dtype=dtype, seed=4)
    db = DeviceBatch(batch)
    ec = model.evaluate(db, mode="mean")
    gen = model.generate(db, mode="mean")["generated_adj"]
    g = gen.cpu().numpy().astype(np.int64)
    n = cfg.n_nodes
    for b in range(2):
        a = batch.dense_adj(b) != 0
        assert ec.counts[b, 0] + ec.counts[b, 1] == g[b].sum()
        assert ec.counts[b, 0] == g[b][a].sum()
        assert ec.counts[b].sum() == n * n
        assert ec.hist[b, 1].sum() == a.sum() and ec.hist[b, 0].sum() == n * n - n - a.sum()
    assert ec.accuracy == adj_accuracy(gen, db)
    assert 0 < g.sum() < g.size                     # both classes predicted: the identities bite
    # accumulating into a device buffer, no read-back until a metric is used
    from snd_vae_amd.metrics import EdgeCounts
    buf = EdgeCounts.zeros(2, device="cuda")
    assert model.evaluate(db, mode="mean", out=buf) is buf
    model.evaluate(db, mode="mean", out=buf)
    assert buf == ec + ec


def test_trainer_evaluate_sums_batches_and_leaves_state(tmp_path):
    from snd_vae_amd.config import tscale
    from snd_vae_amd.input_data import load_data_syn, write_synthetic_dataset
    from snd_vae_amd.trainer import Trainer
    cfg = tscale(96, 16, mean_degree=6.0)
    write_synthetic_dataset(str(tmp_path), cfg, 4, seed=11)
    np.random.seed(1)
    ds = load_data_syn("train", str(tmp_path), sampling_num=2)
    t = Trainer(cfg, ds, batch_size=2, dtype="f32")
    assert t.batch_num == 2
    t.train_epoch()                                 # captured graphs and Adam state exist
    o = t.opt
    state = [x.clone() for x in (t.model.params, o.m, o.v, o.step_counter)]
    res = t.evaluate()
    want = t.model.evaluate(t.batches[0]).total() + t.model.evaluate(t.batches[1]).total()
    assert res["edge_counts"] == want
    assert res["tp"] + res["fp"] + res["fn"] + res["tn"] == 4 * 96 * 96
    assert res["accuracy"] == want.accuracy and res["roc_auc"] == want.roc_auc
    for x, y in zip(state, (t.model.params, o.m, o.v, o.step_counter)):
        assert torch.equal(x, y)
    t.train_epoch()                                 # the captured graphs still replay
    assert o.global_step == 4


# ------------------------------------------------------------------ argument errors
def test_rejected_arguments():
    from snd_vae_amd import _lib, layers
    n = 8
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    colidx = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.SNDError, match="d=129"):
        layers.zzt_eval(torch.zeros(n, 129, device="cuda"), rowptr, colidx, 1, n)
    L = _lib.lib()
    z = torch.zeros(n, 16, device="cuda")
    h = torch.full((1, 2, BINS), 5, dtype=torch.int64, device="cuda")
    c = torch.full((1, 4), 5, dtype=torch.int64, device="cuda")
    P = _lib.ptr
    with pytest.raises(_lib.SNDError, match="ldz"):
        _lib.check(L.snd_zzt_eval(P(z), 15, 1, n, 16, P(rowptr), P(colidx), P(h), P(c), 0, None, 0,
                                  _lib.stream_ptr()), "snd_zzt_eval")
    for bad in ((0, P(rowptr), P(colidx), P(h), P(c)), (P(z), P(rowptr), P(colidx), 0, P(c))):
        rc = L.snd_zzt_eval(bad[0], 16, 1, n, 16, bad[1], bad[2], bad[3], bad[4], 0, None, 0, _lib.stream_ptr())
        assert rc == -1 and "null" in _lib.last_error()
    torch.cuda.synchronize()
    assert int(h.min()) == 5 and int(c.min()) == 5          # nothing was launched or cleared
    with pytest.raises(ValueError):
        layers.zzt_eval(z, rowptr, colidx, 2, n)
    with pytest.raises(ValueError):
        layers.zzt_eval(z, rowptr, colidx, 1, n, accumulate=True)
