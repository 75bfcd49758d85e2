"""NumPy restatement of ``snd_margin_eval`` (include/snd_vae.h, ABI 23) and of
``snd_disent_losses``, the operands the tests of both share, and guarded device buffers.

The bin rule is ``snd_zzt_eval``'s, evaluated as the kernel evaluates it: 64 m and the
+ 1024 in float32 (64 m is exact; the sum only rounds where the clamp decides anyway), the
clamp in float, then the conversion to an integer.
"""
from __future__ import annotations

import numpy as np

BINS = 2048


def margin_bins(margin):
    """clamp(floor(64 m) + 1024, 0, 2047) per entry, float32 arithmetic (no NaN)."""
    m = np.asarray(margin, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.floor(m * np.float32(64.0)) + np.float32(1024.0)
    return np.clip(t, np.float32(0.0), np.float32(BINS - 1)).astype(np.int64)


def margin_eval_ref(margin, adj):
    """(hist int64 [B, 2, 2048], counts int64 [B, 4] = {TP, FP, FN, TN}) of margin, adj
    [B, N, N]: the label is adj != 0, the diagonal is skipped by index and counted as TN, the
    decision rule is m > 0."""
    m = np.asarray(margin, np.float32)
    lab = np.asarray(adj) != 0
    B, N, _ = m.shape
    off = ~np.eye(N, dtype=bool)
    bins = margin_bins(m)
    pred = m > 0
    hist = np.zeros((B, 2, BINS), np.int64)
    counts = np.zeros((B, 4), np.int64)
    for b in range(B):
        for label in (0, 1):
            sel = off & (lab[b] == bool(label))
            np.add.at(hist[b, label], bins[b][sel], 1)
        tp = int((off & lab[b] & pred[b]).sum())
        fp = int((off & ~lab[b] & pred[b]).sum())
        fn = int((off & lab[b] & ~pred[b]).sum())
        counts[b] = (tp, fp, fn, N * N - tp - fp - fn)
    return hist, counts


# The values on which the bin rule turns, with the bin each must land in.
EDGE_VALUES = (
    [(k / 64.0, k + 1024) for k in (-1024, -1023, -513, -1, 1, 2, 511, 1022, 1023)]
    + [(0.0, 1024), (-0.0, 1024), (16.0, 2047), (-16.0, 0), (15.984375, 2047), (-16.015625, 0),
       (1e30, 2047), (-1e30, 0), (np.inf, 2047), (-np.inf, 0),
       (-1e-30, 1023), (1e-30, 1024), (np.nextafter(np.float32(1 / 64), np.float32(0)), 1024)]
)


def edge_case(N=7, seed=0):
    """(margin, adj [1, N, N], expected bin per off-diagonal entry or -1): EDGE_VALUES placed
    off the diagonal in seeded positions, seeded labels, and a diagonal that holds EDGE_VALUES
    too (it must be ignored)."""
    rng = np.random.default_rng(seed)
    vals = np.array([v for v, _ in EDGE_VALUES], np.float32)
    want = np.array([b for _, b in EDGE_VALUES], np.int64)
    assert N * N - N >= len(vals)
    margin = np.zeros((1, N, N), np.float32)
    expect = np.full((1, N, N), -1, np.int64)
    offs = np.flatnonzero(~np.eye(N, dtype=bool).reshape(-1))
    pick = rng.permutation(offs)
    fill = rng.integers(0, len(vals), len(offs))
    fill[:len(vals)] = np.arange(len(vals))          # every value at least once
    margin.reshape(-1)[pick] = vals[fill]
    expect.reshape(-1)[pick] = want[fill]
    margin[0, np.arange(N), np.arange(N)] = vals[rng.integers(0, len(vals), N)]
    adj = (rng.random((1, N, N)) < 0.4).astype(np.float32)
    return margin, adj, expect


def random_case(B, N, seed, diag=None):
    """Seeded margins over [-20, 20] (both overflow bins reached), a share of exact zeros and
    bin edges, labels at density 0.3; ``diag`` fills the diagonal."""
    rng = np.random.default_rng([seed, B, N])
    m = rng.uniform(-20.0, 20.0, (B, N, N)).astype(np.float32)
    edge = rng.random((B, N, N)) < 0.2
    m[edge] = (rng.integers(-1100, 1100, int(edge.sum())) / 64.0).astype(np.float32)
    m[rng.random((B, N, N)) < 0.05] = 0.0
    adj = (rng.random((B, N, N)) < 0.3).astype(np.float32)
    adj[rng.random((B, N, N)) < 0.05] = 2.5           # the label is adj != 0, not adj == 1
    if diag is not None:
        m[:, np.arange(N), np.arange(N)] = diag
    return m, adj


def disent_losses_ref(sse_node, node_count, sse_spatial, spatial_count, ce_out, pair_count, reg_s, reg_g, reg_sg):
    """losses[8] of snd_disent_losses in float64, sums in index order."""
    def seq(v):
        s = np.float64(0.0)
        for x in np.asarray(v, np.float64):
            s = s + x
        return s
    node, spatial = seq(sse_node) / np.float64(node_count), seq(sse_spatial) / np.float64(spatial_count)
    adj = np.float64(ce_out[0]) / np.float64(pair_count)
    reg = np.float64(0.0)
    for r in (reg_s, reg_g, reg_sg):
        if r is not None:
            reg = reg + np.float64(r[1])
    return np.array([adj + node + spatial + reg, spatial, adj, node,
                     0.0 if reg_g is None else reg_g[0], 0.0 if reg_s is None else reg_s[0], reg_sg[0],
                     ce_out[1]], np.float64)


class Guarded:
    """A device operand between two guard bands: ``t`` is the operand (a view, ``offset``
    elements past the band so its pointer can be off 16-byte alignment), ``intact()`` says
    whether the bands still hold their pattern."""
    GUARD = 64

    def __init__(self, data, device="cuda", offset=0):
        import torch
        data = np.ascontiguousarray(data)
        self.n, self.lo = data.size, self.GUARD + offset
        if data.dtype.kind == "f":
            pattern = np.full(self.lo + self.n + self.GUARD, 12345.678, data.dtype)
        else:
            pattern = np.full(self.lo + self.n + self.GUARD, 0x5A5A5A5A, data.dtype)
        self.pattern = pattern.copy()
        pattern[self.lo:self.lo + self.n] = data.reshape(-1)
        self.buf = torch.from_numpy(pattern).to(device)
        self.t = self.buf[self.lo:self.lo + self.n].view(*data.shape)

    def intact(self):
        got = self.buf.cpu().numpy()
        return (np.array_equal(got[:self.lo], self.pattern[:self.lo])
                and np.array_equal(got[self.lo + self.n:], self.pattern[self.lo + self.n:]))
