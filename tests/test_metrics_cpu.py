"""snd_vae_amd.metrics on the CPU: the edge-score counters' derived values.

* roc_auc / average_precision equal sklearn's roc_auc_score / average_precision_score
  on the expanded (label, bin index) samples to 1e-12 (the AUC of the binned score:
  ties inside a bin count 1/2; AP is the step sum over the bin thresholds).
* precision / recall / f1 / best_f1 against brute force over the same samples.
* The degenerate cases return nan and never raise.
* `+`, per_graph() and total(); a gloo world-2 all_reduce of two different
  EdgeCounts equals their sum.
"""
import math
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from snd_vae_amd.metrics import BINS, EdgeCounts, bin_edge


def random_hist(seed, n_graphs=1, fill=0.05, top=40, ends=True):
    """Sparse random histograms: most bins empty, both end bins populated when asked."""
    rng = np.random.default_rng(seed)
    h = rng.integers(0, top, size=(n_graphs, 2, BINS)) * (rng.random((n_graphs, 2, BINS)) < fill)
    h[:, 0] *= 3                                   # more negatives than positives
    if ends:
        h[:, :, 0] = rng.integers(1, 9, size=(n_graphs, 2))
        h[:, :, BINS - 1] = rng.integers(1, 9, size=(n_graphs, 2))
    else:
        h[:, :, 0] = 0
        h[:, :, BINS - 1] = 0
    return h.astype(np.int64)


def counts_at_zero(h, zeros1=0, zeros0=0, diag=0):
    """{TP, FP, FN, TN} the kernel would report for hist h when zeros1 / zeros0 pairs of
    bin 1024 have L == 0 exactly (not predicted) and diag diagonal pairs are TN."""
    c = np.zeros((h.shape[0], 4), np.int64)
    c[:, 0] = h[:, 1, 1024:].sum(axis=1) - zeros1
    c[:, 1] = h[:, 0, 1024:].sum(axis=1) - zeros0
    c[:, 2] = h[:, 1].sum(axis=1) - c[:, 0]
    c[:, 3] = h[:, 0].sum(axis=1) - c[:, 1] + diag
    return c


def expand(h):
    """(labels, scores): one sample per counted pair, the bin index as its score."""
    tot = h.sum(axis=0)
    bins = np.arange(BINS)
    y = np.concatenate([np.zeros(int(tot[0].sum()), np.int64), np.ones(int(tot[1].sum()), np.int64)])
    s = np.concatenate([np.repeat(bins, tot[0]), np.repeat(bins, tot[1])])
    return y, s


@pytest.mark.parametrize("seed,n_graphs,ends", [(0, 1, True), (1, 3, True), (2, 2, False), (3, 1, True)])
def test_auc_and_ap_equal_sklearn(seed, n_graphs, ends):
    from sklearn.metrics import average_precision_score, roc_auc_score
    h = random_hist(seed, n_graphs, ends=ends)
    assert (h.sum(axis=0) == 0).any()              # empty bins are part of the case
    if ends:
        assert h[:, :, 0].all() and h[:, :, BINS - 1].all()
    ec = EdgeCounts(h, counts_at_zero(h))
    y, s = expand(h)
    assert abs(ec.roc_auc - roc_auc_score(y, s)) <= 1e-12
    assert abs(ec.average_precision - average_precision_score(y, s)) <= 1e-12
    for g, e in zip(range(n_graphs), ec.per_graph()):
        yg, sg = expand(h[g:g + 1])
        assert abs(e.roc_auc - roc_auc_score(yg, sg)) <= 1e-12
        assert abs(e.average_precision - average_precision_score(yg, sg)) <= 1e-12


def test_perfect_and_inverted_ranking():
    h = np.zeros((1, 2, BINS), np.int64)
    h[0, 0, 100], h[0, 1, 1500] = 7, 3
    ec = EdgeCounts(h, counts_at_zero(h))
    assert ec.roc_auc == 1.0 and ec.average_precision == 1.0
    h2 = h[:, ::-1].copy()
    ec2 = EdgeCounts(h2, counts_at_zero(h2))
    assert ec2.roc_auc == 0.0 and ec2.average_precision == pytest.approx(0.7)
    h3 = np.zeros((1, 2, BINS), np.int64)
    h3[0, :, 1024] = (5, 5)                         # everything tied in one bin
    assert EdgeCounts(h3, counts_at_zero(h3)).roc_auc == 0.5


def test_threshold_metrics_against_brute_force():
    h = random_hist(5, 2)
    c = counts_at_zero(h, zeros1=1, zeros0=2, diag=25)
    ec = EdgeCounts(h, c)
    tp, fp, fn, tn = (int(v) for v in c.sum(axis=0))
    assert (ec.tp, ec.fp, ec.fn, ec.tn) == (tp, fp, fn, tn)
    assert ec.precision == tp / (tp + fp) and ec.recall == tp / (tp + fn)
    assert ec.f1 == 2 * tp / (2 * tp + fp + fn)
    assert ec.accuracy == (tp + tn) / (tp + fp + fn + tn)
    # best_f1: every bin edge as the threshold "edge iff bin >= b", b = 0 is -inf
    y, s = expand(h)
    best, at = -1.0, None
    for b in range(BINS):
        pred = s >= b
        t, f, m = int((pred & (y == 1)).sum()), int((pred & (y == 0)).sum()), int((~pred & (y == 1)).sum())
        f1 = 2 * t / (2 * t + f + m)
        if f1 >= best:                              # of equal F1 the highest threshold
            best, at = f1, b
    thr, f1 = ec.best_f1()
    assert f1 == pytest.approx(best, rel=1e-15) and thr == bin_edge(at)
    assert bin_edge(1024) == 0.0 and bin_edge(1025) == 1 / 64 and bin_edge(0) == -math.inf
    s = ec.summary()
    assert s["best_f1"] == f1 and s["roc_auc"] == ec.roc_auc and s["tn"] == tn


def test_best_f1_can_be_minus_infinity():
    h = np.zeros((1, 2, BINS), np.int64)
    h[0, 1, 0], h[0, 1, 900], h[0, 0, 0] = 4, 4, 1  # positives in the underflow bin
    thr, f1 = EdgeCounts(h, counts_at_zero(h)).best_f1()
    assert thr == -math.inf and f1 == pytest.approx(16 / 17)


def test_degenerate_cases_are_nan():
    z = EdgeCounts.zeros(2)
    for v in (z.accuracy, z.precision, z.recall, z.f1, z.roc_auc, z.average_precision, *z.best_f1()):
        assert math.isnan(v)
    h = np.zeros((1, 2, BINS), np.int64)
    h[0, 0, 1000] = 9                               # no positive
    e = EdgeCounts(h, counts_at_zero(h, diag=3))
    assert math.isnan(e.roc_auc) and math.isnan(e.average_precision) and math.isnan(e.recall)
    assert math.isnan(e.precision) and math.isnan(e.f1) and all(math.isnan(v) for v in e.best_f1())
    assert e.accuracy == 1.0
    h = np.zeros((1, 2, BINS), np.int64)
    h[0, 1, 1100] = 4                               # no negative
    e = EdgeCounts(h, counts_at_zero(h))
    assert math.isnan(e.roc_auc) and e.average_precision == 1.0 and e.recall == 1.0
    assert all(isinstance(v, (int, float)) for v in e.summary().values())


def test_add_per_graph_total():
    ha, hb = random_hist(7, 2), random_hist(8, 2)
    a, b = EdgeCounts(ha, counts_at_zero(ha, diag=10)), EdgeCounts(hb, counts_at_zero(hb, diag=10))
    s = a + b
    assert np.array_equal(s.hist, ha + hb) and np.array_equal(s.counts, a.counts + b.counts)
    assert s == EdgeCounts(ha + hb, a.counts + b.counts) and not (s == a)
    t = s.total()
    assert t.n_graphs == 1 and np.array_equal(t.hist[0], (ha + hb).sum(axis=0))
    assert np.array_equal(t.counts[0], (a.counts + b.counts).sum(axis=0))
    assert t.roc_auc == s.roc_auc and t.f1 == s.f1          # the properties describe the total
    pg = s.per_graph()
    assert len(pg) == 2 and np.array_equal(pg[1].hist[0], (ha + hb)[1])
    assert pg[0].total() + pg[1].total() == t
    with pytest.raises(ValueError):
        s + t
    with pytest.raises(ValueError):
        EdgeCounts(np.zeros((1, 2, 7)), np.zeros((1, 4)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_counts(rank):
    h = random_hist(20 + rank, 2)
    return EdgeCounts(h, counts_at_zero(h, zeros1=rank, diag=5 + rank))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from snd_vae_amd.parallel import init_from_env
    info = init_from_env("gloo", force=True)
    mine = _rank_counts(rank)
    red = mine.all_reduce(info.group)
    assert mine == _rank_counts(rank)               # the rank's own counters are left alone
    q.put((rank, red.hist.copy(), red.counts.copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_gloo_world2_equals_sum():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    got = [q.get(timeout=180) for _ in range(world)]
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    want = _rank_counts(0) + _rank_counts(1)
    assert not (_rank_counts(0) == _rank_counts(1))
    for _, h, c in got:
        assert h.dtype == np.int64 and np.array_equal(h, want.hist) and np.array_equal(c, want.counts)
