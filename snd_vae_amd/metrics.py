"""Link-prediction metrics from the edge-score counters of ``snd_zzt_eval``.

The reference imports ``roc_auc_score`` / ``average_precision_score``
(`main.py:13-14`) for its post-training evaluation (`main.py:423,467`); at the
scales this code runs, the N^2 scores those functions take are never stored.
The evaluation kernel leaves, per graph, an int64 histogram of the logits by
label (``hist [B, 2, 2048]``: bins of width 1/64 over [-16, 16), bins 0 and
2047 the under- and overflow) and the confusion counts ``counts [B, 4] = {TP,
FP, FN, TN}`` at the reference's decision rule L > 0 (`model.py:208`, the
diagonal counted as TN).  Everything here is a function of those integers, in
float64; the counters are additive, so metrics of a dataset or of a
data-parallel run are those of the summed counters, exactly.

``GraphStats`` (below) is the generative side of the same evaluation: degree,
clustering and edge-length histograms per graph from ``snd_graph_stats``, and the
two-sample statistics (MMD with an EMD kernel, KL divergence) between a set of
generated graphs and the data.

``PathStats`` is its companion for the graph as a network: components, hop distances
and the detour of the network route over the straight line, from ``snd_graph_paths``.
``MotifStats`` is the 4-node side: the graphlet census of ``snd_graph_motifs``, its orbit
vectors and their Gaussian-kernel MMD.  ``SpectrumStats`` is the global side: the spectral
density of the normalised Laplacian from the Chebyshev moments of ``snd_graph_spectrum``.

``LatentMI`` (at the end) is the disentanglement side (`main.py:424`): MIG, avgMI,
modularity and the per-group share of each factor's information, from the
latent-factor mutual-information matrix of ``snd_latent_mi``.

Pure NumPy: imports without a GPU.  torch is imported only when a device tensor
or a process group is handed in.
"""
from __future__ import annotations

import math
from typing import List, Tuple

import numpy as np

BINS = 2048
BIN_SCALE = 64.0          # bins per unit of logit
BIN_ZERO = 1024           # the bin of L in [0, 1/64)
NAN = float("nan")


def bin_edge(b: int) -> float:
    """Lower edge of bin b as a logit (bin 0, the underflow bin, has none: -inf)."""
    return -math.inf if b <= 0 else (b - BIN_ZERO) / BIN_SCALE


def _is_tensor(x) -> bool:
    return hasattr(x, "device") and hasattr(x, "data_ptr")


class EdgeCounts:
    """hist [B, 2, 2048] and counts [B, 4] of one or more evaluated batches.

    Built from NumPy arrays (or anything ``np.asarray`` takes) or from two int64
    torch tensors; device tensors are read back once, on first use.  The metric
    properties describe all B graphs together (``total()``); ``per_graph()``
    gives one EdgeCounts per graph.
    """

    def __init__(self, hist, counts):
        self._dev = None
        self._np = None
        if _is_tensor(hist):
            if tuple(hist.shape[1:]) != (2, BINS) or tuple(counts.shape) != (hist.shape[0], 4):
                raise ValueError("EdgeCounts: expected hist [B, 2, 2048] and counts [B, 4]")
            self._dev = (hist, counts)
        else:
            h = np.asarray(hist, dtype=np.int64)
            c = np.asarray(counts, dtype=np.int64)
            if h.ndim == 2:
                h, c = h[None], c.reshape(1, -1)
            if h.shape[1:] != (2, BINS) or c.shape != (h.shape[0], 4):
                raise ValueError("EdgeCounts: expected hist [B, 2, 2048] and counts [B, 4]")
            self._np = (h, c)

    # ---- storage
    @classmethod
    def zeros(cls, n_graphs: int, device=None) -> "EdgeCounts":
        """Cleared counters: NumPy (device None) or int64 torch tensors on ``device``
        (the accumulation buffer of ``SGCNModelVAE.evaluate(..., out=...)``)."""
        if device is None:
            return cls(np.zeros((n_graphs, 2, BINS), np.int64), np.zeros((n_graphs, 4), np.int64))
        import torch
        return cls(torch.zeros(n_graphs, 2, BINS, dtype=torch.int64, device=device),
                   torch.zeros(n_graphs, 4, dtype=torch.int64, device=device))

    @property
    def tensors(self):
        """The (hist, counts) torch tensors this object was built on, or None."""
        return self._dev

    def invalidate(self) -> None:
        """Forget the host copy: the device tensors were written since it was read."""
        if self._dev is not None:
            self._np = None

    def _arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        if self._np is None:
            import torch
            h, c = self._dev
            both = torch.cat([h.reshape(-1), c.reshape(-1)]).cpu().numpy()     # one read-back
            n = h.numel()
            self._np = (both[:n].reshape(tuple(h.shape)), both[n:].reshape(tuple(c.shape)))
        return self._np

    @property
    def hist(self) -> np.ndarray:
        return self._arrays()[0]

    @property
    def counts(self) -> np.ndarray:
        return self._arrays()[1]

    @property
    def n_graphs(self) -> int:
        return int((self._dev[0] if self._np is None else self._np[0]).shape[0])

    # ---- algebra
    def __add__(self, other: "EdgeCounts") -> "EdgeCounts":
        if not isinstance(other, EdgeCounts):
            return NotImplemented
        if self.hist.shape != other.hist.shape:
            raise ValueError("EdgeCounts +: different numbers of graphs (add total()s instead)")
        return EdgeCounts(self.hist + other.hist, self.counts + other.counts)

    def __eq__(self, other) -> bool:
        return (isinstance(other, EdgeCounts) and np.array_equal(self.hist, other.hist)
                and np.array_equal(self.counts, other.counts))

    __hash__ = None

    def per_graph(self) -> List["EdgeCounts"]:
        return [EdgeCounts(self.hist[b:b + 1].copy(), self.counts[b:b + 1].copy())
                for b in range(self.hist.shape[0])]

    def total(self) -> "EdgeCounts":
        return EdgeCounts(self.hist.sum(axis=0, keepdims=True), self.counts.sum(axis=0, keepdims=True))

    def all_reduce(self, process_group=None) -> "EdgeCounts":
        """The sum of every rank's counters (data parallel), as a new EdgeCounts.
        Integer sums: the same on every rank, whatever the reduction order."""
        import torch
        import torch.distributed as dist
        dev = self._dev[0].device if self._dev is not None else torch.device("cpu")
        if dev.type == "cpu" and dist.get_backend(process_group) == "nccl":
            dev = torch.device("cuda", torch.cuda.current_device())
        if self._dev is not None and self._dev[0].device == dev:
            h, c = self._dev[0].clone(), self._dev[1].clone()
        else:
            h = torch.from_numpy(self.hist.copy()).to(dev)
            c = torch.from_numpy(self.counts.copy()).to(dev)
        flat = torch.cat([h.reshape(-1), c.reshape(-1)])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=process_group)
        n = h.numel()
        return EdgeCounts(flat[:n].reshape(h.shape), flat[n:].reshape(c.shape))

    # ---- totals
    def _tot(self):
        return self.hist.sum(axis=0), self.counts.sum(axis=0)

    @property
    def tp(self) -> int:
        return int(self.counts[:, 0].sum())

    @property
    def fp(self) -> int:
        return int(self.counts[:, 1].sum())

    @property
    def fn(self) -> int:
        return int(self.counts[:, 2].sum())

    @property
    def tn(self) -> int:
        return int(self.counts[:, 3].sum())

    # ---- at the decision rule L > 0 (diagonal pairs are TN)
    @property
    def accuracy(self) -> float:
        """`main.py:334`: (TP + TN) / (B N^2)."""
        t = self.tp + self.fp + self.fn + self.tn
        return (self.tp + self.tn) / t if t else NAN

    @property
    def precision(self) -> float:
        d = self.tp + self.fp
        return self.tp / d if d else NAN

    @property
    def recall(self) -> float:
        d = self.tp + self.fn
        return self.tp / d if d else NAN

    @property
    def f1(self) -> float:
        d = 2 * self.tp + self.fp + self.fn
        return 2 * self.tp / d if d else NAN

    # ---- ranking metrics of the binned score (off-diagonal pairs)
    @property
    def roc_auc(self) -> float:
        """P(score of a positive > score of a negative) + 1/2 P(equal) on the bin index:
        pairs inside one bin count 1/2.  nan without a positive or without a negative."""
        h, _ = self._tot()
        neg, pos = h[0], h[1]
        P, N = int(pos.sum()), int(neg.sum())
        if P == 0 or N == 0:
            return NAN
        below = np.cumsum(neg) - neg                      # negatives in lower bins (int64, exact)
        s = np.sum(pos.astype(np.float64) * (below.astype(np.float64) + 0.5 * neg.astype(np.float64)))
        return float(s / (float(P) * float(N)))

    @property
    def average_precision(self) -> float:
        """sum_b (R_b - R_{b+1}) P_b over the bin thresholds, highest bin first (the
        step-sum definition, no interpolation).  nan without a positive."""
        h, _ = self._tot()
        neg, pos = h[0][::-1], h[1][::-1]
        P = int(pos.sum())
        if P == 0:
            return NAN
        tp = np.cumsum(pos).astype(np.float64)
        pp = tp + np.cumsum(neg).astype(np.float64)
        prec = np.divide(tp, pp, out=np.zeros_like(tp), where=pp > 0)
        return float(np.sum(pos.astype(np.float64) / float(P) * prec))

    def best_f1(self) -> Tuple[float, float]:
        """(threshold, F1) of the F1-optimal rule "edge iff L >= threshold" over the bin
        edges (-inf: every pair an edge); of equal F1 the highest threshold.  (nan, nan)
        without a positive."""
        h, _ = self._tot()
        neg, pos = h[0][::-1], h[1][::-1]
        P = int(pos.sum())
        if P == 0:
            return NAN, NAN
        tp = np.cumsum(pos).astype(np.float64)          # predicted = bins >= b, b descending
        fp = np.cumsum(neg).astype(np.float64)
        f1 = 2.0 * tp / (tp + fp + float(P))            # 2TP / (2TP + FP + FN), FN = P - TP
        k = int(np.argmax(f1))                          # first maximum = highest bin
        return bin_edge(BINS - 1 - k), float(f1[k])

    def summary(self) -> dict:
        thr, bf = self.best_f1()
        return {"accuracy": self.accuracy, "precision": self.precision, "recall": self.recall,
                "f1": self.f1, "roc_auc": self.roc_auc, "average_precision": self.average_precision,
                "best_f1": bf, "best_f1_threshold": thr,
                "tp": self.tp, "fp": self.fp, "fn": self.fn, "tn": self.tn}

    def __repr__(self) -> str:
        return f"EdgeCounts(n_graphs={self.n_graphs}, tp={self.tp}, fp={self.fp}, fn={self.fn}, tn={self.tn})"


# ---------------------------------------------------------------------------
# Graph statistics from the counters of ``snd_graph_stats``
# ---------------------------------------------------------------------------
GS_BINS = 256
KINDS = ("degree", "clustering", "edge_length")


def emd(p, q, width: float = 1.0) -> float:
    """1-D earth mover's distance of two normalised histograms over the same bins of
    width ``width``: sum |cdf_p - cdf_q| * width (the Wasserstein-1 distance of the two
    distributions placed on the bin centres)."""
    p = np.asarray(p, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    if p.shape != q.shape or p.ndim != 1:
        raise ValueError("emd: expected two 1-D histograms over the same bins")
    return float(np.sum(np.abs(np.cumsum(p) - np.cumsum(q))) * width)


def _normalised(h: np.ndarray) -> np.ndarray:
    """Rows of h scaled to sum 1; an empty row stays the zero histogram."""
    h = h.astype(np.float64)
    s = h.sum(axis=-1, keepdims=True)
    return np.divide(h, s, out=np.zeros_like(h), where=s > 0)


class GraphStats:
    """hist [G, 3, 256] and totals [G, 4] of a set of G graphs of n nodes each
    (``layers.graph_stats`` / ``snd_graph_stats``): per graph the histograms of the node
    degree (bin = min(deg, 255)), of the local clustering coefficient (256 bins over
    [0, 1], nodes of degree < 2 in bin 0) and of the edge length (256 bins of width
    max_len / 256, the last one collecting longer edges), and totals = {sum deg,
    sum tri2, sum deg (deg - 1), undirected edges}.

    What the reference hands to ``reconstruct_evaluation`` / ``generation_evaluation``
    (`main.py:423,467`) to answer: do generated graphs look like the data?  Built from
    NumPy arrays or from two int64 torch tensors; device tensors are read back once, on
    first use.  The histograms stay per graph, because the two-sample statistics (``mmd``)
    are over *sets* of graphs; the scalar properties describe the set pooled, and
    ``per_graph()`` gives them per graph.  ``max_len`` None: no edge lengths were binned.
    """

    def __init__(self, hist, totals, n: int, max_len=None):
        self._dev = None
        self._np = None
        self.n = int(n)
        self.max_len = None if max_len is None else float(max_len)
        if self.n < 1:
            raise ValueError("GraphStats: n must be >= 1")
        if self.max_len is not None and not (0.0 < self.max_len < math.inf):
            raise ValueError("GraphStats: max_len must be finite and > 0")
        if _is_tensor(hist):
            if (hist.dim() != 3 or tuple(hist.shape[1:]) != (3, GS_BINS)
                    or tuple(totals.shape) != (hist.shape[0], 4)):
                raise ValueError("GraphStats: expected hist [G, 3, 256] and totals [G, 4]")
            self._dev = (hist, totals)
        else:
            h = np.asarray(hist, dtype=np.int64)
            t = np.asarray(totals, dtype=np.int64)
            if h.ndim == 2:
                h, t = h[None], t.reshape(1, -1)
            if h.ndim != 3 or h.shape[1:] != (3, GS_BINS) or t.shape != (h.shape[0], 4):
                raise ValueError("GraphStats: expected hist [G, 3, 256] and totals [G, 4]")
            self._np = (h, t)

    # ---- storage
    @property
    def tensors(self):
        """The (hist, totals) torch tensors this object was built on, or None."""
        return self._dev

    def invalidate(self) -> None:
        """Forget the host copy: the device tensors were written since it was read."""
        if self._dev is not None:
            self._np = None

    def _arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        if self._np is None:
            import torch
            h, t = self._dev
            both = torch.cat([h.reshape(-1), t.reshape(-1)]).cpu().numpy()     # one read-back
            k = h.numel()
            self._np = (both[:k].reshape(tuple(h.shape)), both[k:].reshape(tuple(t.shape)))
        return self._np

    @property
    def hist(self) -> np.ndarray:
        return self._arrays()[0]

    @property
    def totals(self) -> np.ndarray:
        return self._arrays()[1]

    @property
    def n_graphs(self) -> int:
        return int((self._dev[0] if self._np is None else self._np[0]).shape[0])

    def __eq__(self, other) -> bool:
        return (isinstance(other, GraphStats) and self.n == other.n and self.max_len == other.max_len
                and np.array_equal(self.hist, other.hist) and np.array_equal(self.totals, other.totals))

    __hash__ = None

    @classmethod
    def concat(cls, parts) -> "GraphStats":
        """The graphs of several GraphStats (batches of one dataset) as one set, in order."""
        parts = list(parts)
        if not parts or not all(isinstance(p, GraphStats) for p in parts):
            raise ValueError("GraphStats.concat: expected a non-empty list of GraphStats")
        if any(p.n != parts[0].n or p.max_len != parts[0].max_len for p in parts):
            raise ValueError("GraphStats.concat: the parts differ in n or max_len")
        return cls(np.concatenate([p.hist for p in parts]), np.concatenate([p.totals for p in parts]),
                   parts[0].n, parts[0].max_len)

    def all_gather(self, process_group=None) -> "GraphStats":
        """Every rank's graphs as one set, in rank order (data parallel; each rank holds the
        same number of graphs), as a new GraphStats: the same on every rank."""
        import torch
        import torch.distributed as dist
        dev = self._dev[0].device if self._dev is not None else torch.device("cpu")
        if dev.type == "cpu" and dist.get_backend(process_group) == "nccl":
            dev = torch.device("cuda", torch.cuda.current_device())
        if self._dev is not None and self._dev[0].device == dev:
            h, t = self._dev
        else:
            h = torch.from_numpy(self.hist.copy()).to(dev)
            t = torch.from_numpy(self.totals.copy()).to(dev)
        flat = torch.cat([h.reshape(-1), t.reshape(-1)])
        world = dist.get_world_size(process_group)
        out = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(out, flat, group=process_group)
        k = h.numel()
        hs = torch.cat([o[:k].reshape(h.shape) for o in out])
        ts = torch.cat([o[k:].reshape(t.shape) for o in out])
        return GraphStats(hs, ts, self.n, self.max_len)

    # ---- bins
    def _kind(self, kind: str):
        """(row of hist, bin width in the statistic's own units, default sigma)."""
        if kind == "degree":
            return 0, 1.0, 1.0
        if kind == "clustering":
            return 1, 1.0 / GS_BINS, 0.1
        if kind == "edge_length":
            if self.max_len is None:
                raise ValueError("GraphStats: no edge lengths were binned (max_len is None)")
            return 2, self.max_len / GS_BINS, 0.1 * self.max_len
        raise ValueError(f"GraphStats: kind must be one of {KINDS}, got {kind!r}")

    # ---- scalar properties
    def _scalars(self, h: np.ndarray, t: np.ndarray, graphs) -> dict:
        """Float64 properties of counters summed over their leading axis ``graphs``."""
        n = self.n
        t = t.astype(np.float64)
        pairs = graphs * n * (n - 1.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = {"density": np.where(pairs > 0, t[..., 0] / np.where(pairs > 0, pairs, 1.0), NAN),
                   "mean_degree": t[..., 0] / (graphs * float(n)),
                   "transitivity": np.where(t[..., 2] > 0, t[..., 1] / np.where(t[..., 2] > 0, t[..., 2], 1.0), 0.0),
                   "n_edges": t[..., 3]}
            lower = np.arange(GS_BINS, dtype=np.float64) / GS_BINS
            nodes = h[..., 1, :].sum(axis=-1).astype(np.float64)
            out["mean_clustering"] = np.where(nodes > 0, (h[..., 1, :] * lower).sum(axis=-1)
                                              / np.where(nodes > 0, nodes, 1.0), NAN)
            if self.max_len is not None:
                centres = (np.arange(GS_BINS, dtype=np.float64) + 0.5) * (self.max_len / GS_BINS)
                e = h[..., 2, :].sum(axis=-1).astype(np.float64)
                out["mean_edge_length"] = np.where(e > 0, (h[..., 2, :] * centres).sum(axis=-1)
                                                   / np.where(e > 0, e, 1.0), NAN)
        return out

    def per_graph(self) -> dict:
        """{property: float64 array [G]}: density = sum deg / (n (n - 1)), mean_degree,
        transitivity = sum tri2 / sum deg (deg - 1) (0 without a wedge, as networkx),
        n_edges (entries with column > row), mean_clustering from the bins' lower edges
        (exact for c = 0; in all at most 1/256 below the exact mean) and, when lengths were
        binned, mean_edge_length from the bin centres (nan for a graph without an edge)."""
        return self._scalars(self.hist, self.totals, 1.0)

    def summary(self) -> dict:
        """The same properties of the set pooled, as floats (n_edges: the total)."""
        s = self._scalars(self.hist.sum(axis=0), self.totals.sum(axis=0), float(self.n_graphs))
        return {k: float(v) for k, v in s.items()}

    density = property(lambda self: self.summary()["density"])
    mean_degree = property(lambda self: self.summary()["mean_degree"])
    transitivity = property(lambda self: self.summary()["transitivity"])
    mean_clustering = property(lambda self: self.summary()["mean_clustering"])
    n_edges = property(lambda self: int(self.totals[:, 3].sum()))

    @property
    def mean_edge_length(self) -> float:
        return self.summary().get("mean_edge_length", NAN)

    # ---- two-sample statistics
    def _check_other(self, other, kind):
        if not isinstance(other, GraphStats):
            raise ValueError("GraphStats: expected another GraphStats")
        row, width, sigma = self._kind(kind)
        if kind == "edge_length" and other.max_len != self.max_len:
            raise ValueError("GraphStats: the two sides binned edge lengths with different max_len")
        return row, width, sigma

    def mmd(self, other: "GraphStats", kind: str, sigma=None) -> float:
        """Biased (V-statistic) MMD^2 between two sets of graphs over their per-graph
        normalised histograms of ``kind``: mean k(a, a') + mean k(b, b') - 2 mean k(a, b),
        k = exp(-EMD^2 / (2 sigma^2)), the EMD in the statistic's own units (degrees;
        clustering in [0, 1] with bins of 1/256; length with bins of max_len / 256).
        Default sigma: 1.0, 0.1 and 0.1 max_len.  A graph whose histogram is empty (no
        edge, for "edge_length") enters as the zero histogram: its EMD to a graph with
        edges is that graph's sum of cdf values, to another empty graph 0."""
        row, width, s0 = self._check_other(other, kind)
        sigma = s0 if sigma is None else float(sigma)
        if not sigma > 0.0:
            raise ValueError("GraphStats.mmd: sigma must be > 0")
        ca = np.cumsum(_normalised(self.hist[:, row, :]), axis=1)
        cb = np.cumsum(_normalised(other.hist[:, row, :]), axis=1)
        if ca.shape[0] == 0 or cb.shape[0] == 0:
            return NAN

        def mean_k(x, y):
            tot = 0.0
            step = max(1, (1 << 22) // (y.shape[0] * GS_BINS))          # ~32 MB of float64 per block
            for i in range(0, x.shape[0], step):
                d = np.abs(x[i:i + step, None, :] - y[None, :, :]).sum(axis=2) * width
                tot += float(np.exp(-(d * d) / (2.0 * sigma * sigma)).sum())
            return tot / (x.shape[0] * y.shape[0])

        return mean_k(ca, ca) + mean_k(cb, cb) - 2.0 * mean_k(ca, cb)

    def pooled(self, kind: str) -> np.ndarray:
        """The normalised histogram of ``kind`` over all graphs of the set."""
        row, _, _ = self._kind(kind)
        return _normalised(self.hist[:, row, :].sum(axis=0))

    def kld(self, other: "GraphStats", kind: str, eps: float = 1e-12) -> float:
        """KL(self || other) of the pooled normalised histograms, each smoothed by eps per
        bin and renormalised (scipy.stats.entropy(p + eps, q + eps)).  nan when either side
        has no count."""
        self._check_other(other, kind)
        p, q = self.pooled(kind), other.pooled(kind)
        if p.sum() == 0 or q.sum() == 0:
            return NAN
        p = (p + eps) / (p + eps).sum()
        q = (q + eps) / (q + eps).sum()
        return float(np.sum(p * np.log(p / q)))

    def compare(self, other: "GraphStats") -> dict:
        """mmd_<kind>, kld_<kind> and emd_<kind> (the EMD of the pooled histograms) for the
        three kinds (edge_length only when both sides binned lengths), plus both sides'
        pooled scalars under "self" and "other"."""
        if not isinstance(other, GraphStats):
            raise ValueError("GraphStats.compare: expected another GraphStats")
        out = {}
        for kind in KINDS:
            if kind == "edge_length" and (self.max_len is None or other.max_len is None):
                continue
            _, width, _ = self._check_other(other, kind)
            out[f"mmd_{kind}"] = self.mmd(other, kind)
            out[f"kld_{kind}"] = self.kld(other, kind)
            out[f"emd_{kind}"] = emd(self.pooled(kind), other.pooled(kind), width)
        out["self"] = self.summary()
        out["other"] = other.summary()
        return out

    def __repr__(self) -> str:
        return f"GraphStats(n_graphs={self.n_graphs}, n={self.n}, max_len={self.max_len})"


# ---------------------------------------------------------------------------
# Path statistics from the counters of ``snd_graph_paths``
# ---------------------------------------------------------------------------
PATH_KINDS = ("hops", "detour")


def _emd_mmd(ha: np.ndarray, hb: np.ndarray, width: float, sigma: float) -> float:
    """GraphStats.mmd's statistic on two stacks of histograms [Ga, 256], [Gb, 256]."""
    ca = np.cumsum(_normalised(ha), axis=1)
    cb = np.cumsum(_normalised(hb), axis=1)
    if ca.shape[0] == 0 or cb.shape[0] == 0:
        return NAN

    def mean_k(x, y):
        tot = 0.0
        step = max(1, (1 << 22) // (y.shape[0] * GS_BINS))
        for i in range(0, x.shape[0], step):
            d = np.abs(x[i:i + step, None, :] - y[None, :, :]).sum(axis=2) * width
            tot += float(np.exp(-(d * d) / (2.0 * sigma * sigma)).sum())
        return tot / (x.shape[0] * y.shape[0])

    return mean_k(ca, ca) + mean_k(cb, cb) - 2.0 * mean_k(ca, cb)


class PathStats:
    """hist [G, 2, 256] and totals [G, 6] of a set of G graphs of n nodes each
    (``layers.graph_paths`` / ``snd_graph_paths``): per graph the histogram of the hop count
    of every reachable ordered pair (source, target != source) (bin = min(hops, 255)) and of
    its detour route / straight line - 1 (256 bins of width 1 / detour_scale, the last one
    collecting larger detours), and totals = {weak components, size of the largest, sources
    used, reachable ordered pairs, sum of hops, largest hop count}.

    Does a generated spatial network work as a network: does it hold together, is it as
    wide as the data, does it connect nearby points without a long way round?  (Barthelemy,
    Spatial networks, Phys. Rep. 499 (2011), sections 2.2.2-2.2.3: shortest paths, route
    factor / detour index; the graphs and coordinates are what the reference hands to
    ``generation_evaluation``, `main.py:467`.)  Same storage idiom as GraphStats: NumPy
    arrays or two int64 torch tensors, device tensors read back once, on first use;
    histograms stay per graph for the two-sample statistics.  ``detour_scale`` None: no
    coordinates were given, the detour row is zero.  ``src_step`` > 1: the pairs are those of
    every src_step-th node as source, a sample of the graph's pairs.
    """

    def __init__(self, hist, totals, n: int, detour_scale=None, src_step: int = 1):
        self._dev = None
        self._np = None
        self.n = int(n)
        self.src_step = int(src_step)
        self.detour_scale = None if detour_scale is None else float(detour_scale)
        if self.n < 1 or self.src_step < 1:
            raise ValueError("PathStats: n and src_step must be >= 1")
        if self.detour_scale is not None and not (0.0 < self.detour_scale < math.inf):
            raise ValueError("PathStats: detour_scale must be finite and > 0")
        if _is_tensor(hist):
            if (hist.dim() != 3 or tuple(hist.shape[1:]) != (2, GS_BINS)
                    or tuple(totals.shape) != (hist.shape[0], 6)):
                raise ValueError("PathStats: expected hist [G, 2, 256] and totals [G, 6]")
            self._dev = (hist, totals)
        else:
            h = np.asarray(hist, dtype=np.int64)
            t = np.asarray(totals, dtype=np.int64)
            if h.ndim == 2:
                h, t = h[None], t.reshape(1, -1)
            if h.ndim != 3 or h.shape[1:] != (2, GS_BINS) or t.shape != (h.shape[0], 6):
                raise ValueError("PathStats: expected hist [G, 2, 256] and totals [G, 6]")
            self._np = (h, t)

    # ---- storage
    @property
    def tensors(self):
        """The (hist, totals) torch tensors this object was built on, or None."""
        return self._dev

    def invalidate(self) -> None:
        """Forget the host copy: the device tensors were written since it was read."""
        if self._dev is not None:
            self._np = None

    def _arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        if self._np is None:
            import torch
            h, t = self._dev
            both = torch.cat([h.reshape(-1), t.reshape(-1)]).cpu().numpy()     # one read-back
            k = h.numel()
            self._np = (both[:k].reshape(tuple(h.shape)), both[k:].reshape(tuple(t.shape)))
        return self._np

    @property
    def hist(self) -> np.ndarray:
        return self._arrays()[0]

    @property
    def totals(self) -> np.ndarray:
        return self._arrays()[1]

    @property
    def n_graphs(self) -> int:
        return int((self._dev[0] if self._np is None else self._np[0]).shape[0])

    def _same_binning(self, other) -> bool:
        return (self.n == other.n and self.detour_scale == other.detour_scale
                and self.src_step == other.src_step)

    def __eq__(self, other) -> bool:
        return (isinstance(other, PathStats) and self._same_binning(other)
                and np.array_equal(self.hist, other.hist) and np.array_equal(self.totals, other.totals))

    __hash__ = None

    @classmethod
    def concat(cls, parts) -> "PathStats":
        """The graphs of several PathStats (batches of one dataset) as one set, in order."""
        parts = list(parts)
        if not parts or not all(isinstance(p, PathStats) for p in parts):
            raise ValueError("PathStats.concat: expected a non-empty list of PathStats")
        if any(not p._same_binning(parts[0]) for p in parts):
            raise ValueError("PathStats.concat: the parts differ in n, detour_scale or src_step")
        return cls(np.concatenate([p.hist for p in parts]), np.concatenate([p.totals for p in parts]),
                   parts[0].n, parts[0].detour_scale, parts[0].src_step)

    def all_gather(self, process_group=None) -> "PathStats":
        """Every rank's graphs as one set, in rank order (data parallel; each rank holds the
        same number of graphs), as a new PathStats: the same on every rank."""
        import torch
        import torch.distributed as dist
        dev = self._dev[0].device if self._dev is not None else torch.device("cpu")
        if dev.type == "cpu" and dist.get_backend(process_group) == "nccl":
            dev = torch.device("cuda", torch.cuda.current_device())
        if self._dev is not None and self._dev[0].device == dev:
            h, t = self._dev
        else:
            h = torch.from_numpy(self.hist.copy()).to(dev)
            t = torch.from_numpy(self.totals.copy()).to(dev)
        flat = torch.cat([h.reshape(-1), t.reshape(-1)])
        world = dist.get_world_size(process_group)
        out = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(out, flat, group=process_group)
        k = h.numel()
        hs = torch.cat([o[:k].reshape(h.shape) for o in out])
        ts = torch.cat([o[k:].reshape(t.shape) for o in out])
        return PathStats(hs, ts, self.n, self.detour_scale, self.src_step)

    # ---- bins
    def _kind(self, kind: str):
        """(row of hist, bin width in the statistic's own units, default sigma)."""
        if kind == "hops":
            return 0, 1.0, 1.0
        if kind == "detour":
            if self.detour_scale is None:
                raise ValueError("PathStats: no detours were binned (detour_scale is None)")
            return 1, 1.0 / self.detour_scale, 0.1
        raise ValueError(f"PathStats: kind must be one of {PATH_KINDS}, got {kind!r}")

    # ---- scalar properties
    def per_graph(self) -> dict:
        """{property: float64 array [G]}:

        * n_components = totals[0], the weakly connected components; connected = 1.0 where
          that is 1; lcc_fraction = totals[1] / n, the share of the nodes in the largest one.
        * mean_hops = totals[4] / totals[3]: the average shortest-path length <l> over the
          reachable ordered pairs (Barthelemy 2011, eq. 21, restricted to reachable pairs;
          networkx.average_shortest_path_length on a connected graph), exact; nan without a
          pair.
        * diameter = totals[5]: the largest hop count over the reachable pairs (the diameter
          of a connected graph when every node is a source).
        * global_efficiency = sum_h hist[0][h] / h / (sources (n - 1)): the mean of 1 / d(s, t)
          over ordered pairs, unreachable pairs counting 0 (Latora & Marchiori, Phys. Rev.
          Lett. 87 (2001) 198701, eq. 1; networkx.global_efficiency).  Exact while no pair
          is past 254 hops: bin 255 collects them and enters as 1 / 255.  nan for n = 1.
        * mean_detour = sum_b hist[1][b] (b + 1/2) / detour_scale / sum_b hist[1][b]: the mean
          of route / straight line - 1 (the route factor or detour index minus one,
          Barthelemy 2011, eq. 28) from the bin centres; nan without coordinates or pairs.
        """
        h, t = self.hist.astype(np.float64), self.totals.astype(np.float64)
        out = {"n_components": t[:, 0], "connected": (t[:, 0] == 1).astype(np.float64),
               "lcc_fraction": t[:, 1] / float(self.n), "diameter": t[:, 5]}
        with np.errstate(divide="ignore", invalid="ignore"):
            out["mean_hops"] = np.where(t[:, 3] > 0, t[:, 4] / np.where(t[:, 3] > 0, t[:, 3], 1.0), NAN)
            inv = np.r_[0.0, 1.0 / np.arange(1, GS_BINS, dtype=np.float64)]
            den = t[:, 2] * (self.n - 1.0)
            out["global_efficiency"] = np.where(den > 0, (h[:, 0, :] * inv).sum(axis=1) / np.where(den > 0, den, 1.0),
                                                NAN)
            if self.detour_scale is None:
                out["mean_detour"] = np.full(h.shape[0], NAN)
            else:
                centres = (np.arange(GS_BINS, dtype=np.float64) + 0.5) / self.detour_scale
                cnt = h[:, 1, :].sum(axis=1)
                out["mean_detour"] = np.where(cnt > 0, (h[:, 1, :] * centres).sum(axis=1)
                                              / np.where(cnt > 0, cnt, 1.0), NAN)
        return out

    def summary(self) -> dict:
        """The set as a whole, as floats: n_components and lcc_fraction are means over the
        graphs, connected the share of graphs with one component, diameter the maximum;
        mean_hops, global_efficiency and mean_detour are those of the pooled counters (every
        pair of every graph weighs the same).  nan where per_graph() has no value at all."""
        if self.n_graphs == 0:
            return {k: NAN for k in ("n_components", "connected", "lcc_fraction", "diameter", "mean_hops",
                                     "global_efficiency", "mean_detour")}
        pg = self.per_graph()
        pooled = PathStats(self.hist.sum(axis=0, keepdims=True), self.totals.sum(axis=0, keepdims=True), self.n,
                           self.detour_scale, self.src_step).per_graph()
        return {"n_components": float(pg["n_components"].mean()), "connected": float(pg["connected"].mean()),
                "lcc_fraction": float(pg["lcc_fraction"].mean()), "diameter": float(pg["diameter"].max()),
                "mean_hops": float(pooled["mean_hops"][0]),
                "global_efficiency": float(pooled["global_efficiency"][0]),
                "mean_detour": float(pooled["mean_detour"][0])}

    connected = property(lambda self: self.summary()["connected"])
    mean_hops = property(lambda self: self.summary()["mean_hops"])
    diameter = property(lambda self: self.summary()["diameter"])
    global_efficiency = property(lambda self: self.summary()["global_efficiency"])
    mean_detour = property(lambda self: self.summary()["mean_detour"])

    # ---- two-sample statistics
    def _check_other(self, other, kind):
        if not isinstance(other, PathStats):
            raise ValueError("PathStats: expected another PathStats")
        row, width, sigma = self._kind(kind)
        if kind == "detour" and other.detour_scale != self.detour_scale:
            raise ValueError("PathStats: the two sides binned detours with different detour_scale")
        return row, width, sigma

    def mmd(self, other: "PathStats", kind: str, sigma=None) -> float:
        """Biased (V-statistic) MMD^2 between two sets of graphs over their per-graph
        normalised histograms of ``kind``, with GraphStats.mmd's kernel k = exp(-EMD^2 /
        (2 sigma^2)), the EMD in the statistic's own units (hops; detour with bins of
        1 / detour_scale).  Default sigma: 1.0 hop and 0.1 of detour.  A graph without a
        pair enters as the zero histogram."""
        row, width, s0 = self._check_other(other, kind)
        sigma = s0 if sigma is None else float(sigma)
        if not sigma > 0.0:
            raise ValueError("PathStats.mmd: sigma must be > 0")
        return _emd_mmd(self.hist[:, row, :], other.hist[:, row, :], width, sigma)

    def pooled(self, kind: str) -> np.ndarray:
        """The normalised histogram of ``kind`` over all graphs of the set."""
        row, _, _ = self._kind(kind)
        return _normalised(self.hist[:, row, :].sum(axis=0))

    def kld(self, other: "PathStats", kind: str, eps: float = 1e-12) -> float:
        """KL(self || other) of the pooled normalised histograms, each smoothed by eps per
        bin and renormalised (scipy.stats.entropy(p + eps, q + eps)).  nan when either side
        has no count."""
        self._check_other(other, kind)
        p, q = self.pooled(kind), other.pooled(kind)
        if p.sum() == 0 or q.sum() == 0:
            return NAN
        p = (p + eps) / (p + eps).sum()
        q = (q + eps) / (q + eps).sum()
        return float(np.sum(p * np.log(p / q)))

    def compare(self, other: "PathStats") -> dict:
        """mmd_<kind>, kld_<kind> and emd_<kind> (the EMD of the pooled histograms) for
        "hops" and (when both sides binned detours) "detour", plus both sides' summaries
        under "self" and "other"."""
        if not isinstance(other, PathStats):
            raise ValueError("PathStats.compare: expected another PathStats")
        out = {}
        for kind in PATH_KINDS:
            if kind == "detour" and (self.detour_scale is None or other.detour_scale is None):
                continue
            _, width, _ = self._check_other(other, kind)
            out[f"mmd_{kind}"] = self.mmd(other, kind)
            out[f"kld_{kind}"] = self.kld(other, kind)
            out[f"emd_{kind}"] = emd(self.pooled(kind), other.pooled(kind), width)
        out["self"] = self.summary()
        out["other"] = other.summary()
        return out

    def __repr__(self) -> str:
        return (f"PathStats(n_graphs={self.n_graphs}, n={self.n}, detour_scale={self.detour_scale}, "
                f"src_step={self.src_step})")


# ---------------------------------------------------------------------------
# Graphlet census from the counters of ``snd_graph_motifs``
# ---------------------------------------------------------------------------
MOTIF_NAMES = ("E", "P2", "T", "P3", "S3", "C4", "TT", "D", "K4")
GRAPHLETS4 = ("P3", "S3", "C4", "TT", "D", "K4")       # the six connected 4-node graphlets


class MotifStats:
    """census [G, 10] of a set of G graphs of n nodes each (``layers.graph_motifs`` /
    ``snd_graph_motifs``): per graph the numbers of induced {E edges, P2 open 2-paths, T
    triangles, P3 3-edge paths, S3 claws, C4 chordless 4-cycles, TT tailed triangles, D
    diamonds, K4 4-cliques} of its mutual-edge graph and the one-way arcs that were ignored;
    a graph that was not counted (its work bound exceeded ``work_cap``) holds -1 throughout
    and is left out of every statistic below.

    Same storage idiom as GraphStats / PathStats: a NumPy array or an int64 torch tensor; a
    device tensor is read back once, on first use.
    """

    def __init__(self, census, n: int):
        self._dev = None
        self._np = None
        self.n = int(n)
        if self.n < 1:
            raise ValueError("MotifStats: n must be >= 1")
        if _is_tensor(census):
            if census.dim() != 2 or census.shape[1] != 10:
                raise ValueError("MotifStats: expected census [G, 10]")
            self._dev = census
        else:
            c = np.asarray(census, dtype=np.int64)
            if c.ndim == 1:
                c = c[None]
            if c.ndim != 2 or c.shape[1] != 10:
                raise ValueError("MotifStats: expected census [G, 10]")
            self._np = c

    # ---- storage
    @property
    def tensors(self):
        """The census torch tensor this object was built on, or None."""
        return self._dev

    def invalidate(self) -> None:
        """Forget the host copy: the device tensor was written since it was read."""
        if self._dev is not None:
            self._np = None

    @property
    def census(self) -> np.ndarray:
        if self._np is None:
            self._np = self._dev.cpu().numpy()                                # one read-back
        return self._np

    @property
    def n_graphs(self) -> int:
        """All graphs of the set, skipped ones included."""
        return int((self._dev if self._np is None else self._np).shape[0])

    @property
    def counted(self) -> np.ndarray:
        """[G] bool: the graphs that were counted."""
        return self.census[:, 0] >= 0

    @property
    def n_skipped(self) -> int:
        return int((~self.counted).sum())

    @property
    def one_way(self) -> int:
        """One-way arcs ignored, over the counted graphs."""
        return int(self.census[self.counted, 9].sum())

    def __eq__(self, other) -> bool:
        return isinstance(other, MotifStats) and self.n == other.n and np.array_equal(self.census, other.census)

    __hash__ = None

    @classmethod
    def concat(cls, parts) -> "MotifStats":
        """The graphs of several MotifStats (batches of one dataset) as one set, in order."""
        parts = list(parts)
        if not parts or not all(isinstance(p, MotifStats) for p in parts):
            raise ValueError("MotifStats.concat: expected a non-empty list of MotifStats")
        if any(p.n != parts[0].n for p in parts):
            raise ValueError("MotifStats.concat: the parts differ in n")
        return cls(np.concatenate([p.census for p in parts]), parts[0].n)

    def all_gather(self, process_group=None) -> "MotifStats":
        """Every rank's graphs as one set, in rank order (data parallel; each rank holds the
        same number of graphs), as a new MotifStats: the same on every rank."""
        import torch
        import torch.distributed as dist
        dev = self._dev.device if self._dev is not None else torch.device("cpu")
        if dev.type == "cpu" and dist.get_backend(process_group) == "nccl":
            dev = torch.device("cuda", torch.cuda.current_device())
        if self._dev is not None and self._dev.device == dev:
            c = self._dev.contiguous()
        else:
            c = torch.from_numpy(self.census.copy()).to(dev)
        out = [torch.empty_like(c) for _ in range(dist.get_world_size(process_group))]
        dist.all_gather(out, c, group=process_group)
        return MotifStats(torch.cat(out), self.n)

    # ---- descriptors
    def per_graph(self) -> dict:
        """{name: int64 array over the counted graphs} for the nine counts and "one_way"."""
        c = self.census[self.counted]
        out = {k: c[:, i] for i, k in enumerate(MOTIF_NAMES)}
        out["one_way"] = c[:, 9]
        return out

    def orbits(self) -> np.ndarray:
        """[counted graphs, 15] float64: per graph the mean over its nodes of the fifteen 2- to
        4-node graphlet orbit counts (Przulj's orbits 0-14).  Summed over a graph's nodes
        the orbit counts are multiples of the induced counts: o0 = 2E, o1 = 2P2, o2 = P2,
        o3 = 3T, o4 = o5 = 2P3, o6 = 3S3, o7 = S3, o8 = 4C4, o9 = TT, o10 = 2TT, o11 = TT,
        o12 = o13 = 2D, o14 = 4K4 (a node of each graphlet sits in exactly one orbit); each
        is divided by n."""
        c = self.census[self.counted].astype(np.float64)
        E, P2, T, P3, S3, C4, TT, D, K4 = (c[:, k] for k in range(9))
        o = np.stack([2 * E, 2 * P2, P2, 3 * T, 2 * P3, 2 * P3, 3 * S3, S3, 4 * C4, TT, 2 * TT, TT, 2 * D, 2 * D,
                      4 * K4], axis=1)
        return o / float(self.n)

    def frequencies(self) -> np.ndarray:
        """[counted graphs, 6] float64: the share of each connected 4-node graphlet (GRAPHLETS4:
        P3, S3, C4, TT, D, K4) among the six; nan for a graph that holds none."""
        c = self.census[self.counted][:, 3:9].astype(np.float64)
        tot = c.sum(axis=1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(tot > 0, c / np.where(tot > 0, tot, 1.0), NAN)

    def mean_frequencies(self) -> dict:
        """{graphlet: the mean share over the counted graphs that hold a 4-node graphlet};
        nan when none does."""
        f = self.frequencies()
        f = f[~np.isnan(f[:, 0])] if f.size else f
        return {k: (float(f[:, i].mean()) if f.shape[0] else NAN) for i, k in enumerate(GRAPHLETS4)}

    def summary(self) -> dict:
        """The set as a whole: n_graphs, n_skipped, one_way, the mean of every count over the
        counted graphs ("mean_<name>"; nan without a counted graph) and "frequencies", the
        mean_frequencies()."""
        out = {"n_graphs": self.n_graphs, "n_skipped": self.n_skipped, "one_way": self.one_way}
        pg = self.per_graph()
        for k in MOTIF_NAMES:
            out[f"mean_{k}"] = float(pg[k].mean()) if pg[k].size else NAN
        out["frequencies"] = self.mean_frequencies()
        return out

    # ---- two-sample statistic
    def mmd(self, other: "MotifStats", sigma: float = 30.0) -> float:
        """Biased (V-statistic) MMD^2 between two sets of graphs over their orbit vectors
        ``orbits()`` with the Gaussian kernel k(x, y) = exp(-||x - y||^2 / (2 sigma^2)).

        The statistic is the orbit descriptor of GraphRNN's evaluation (You et al., GraphRNN:
        Generating Realistic Graphs with Deep Auto-regressive Models, ICML 2018, and its
        released evaluation code: per-graph mean orbit counts of the 4-node graphlets,
        compared by a Gaussian-kernel MMD with sigma = 30).  The definition here is this
        project's restatement from that description: the reference project ships no file for
        it, so there is nothing to transcribe, and the numbers are comparable with published
        ones only as far as the restatement agrees.  Skipped graphs are left out; nan when
        either side has no counted graph."""
        if not isinstance(other, MotifStats):
            raise ValueError("MotifStats.mmd: expected another MotifStats")
        sigma = float(sigma)
        if not sigma > 0.0:
            raise ValueError("MotifStats.mmd: sigma must be > 0")
        x, y = self.orbits(), other.orbits()
        if x.shape[0] == 0 or y.shape[0] == 0:
            return NAN

        def mean_k(a, b):
            tot = 0.0
            step = max(1, (1 << 20) // max(1, b.shape[0]))
            for i in range(0, a.shape[0], step):
                d = a[i:i + step, None, :] - b[None, :, :]
                tot += float(np.exp(-(d * d).sum(axis=2) / (2.0 * sigma * sigma)).sum())
            return tot / (a.shape[0] * b.shape[0])

        return mean_k(x, x) + mean_k(y, y) - 2.0 * mean_k(x, y)

    def compare(self, other: "MotifStats") -> dict:
        """{"mmd_orbits": mmd(other), "self": mean_frequencies(), "other": other's}."""
        if not isinstance(other, MotifStats):
            raise ValueError("MotifStats.compare: expected another MotifStats")
        return {"mmd_orbits": self.mmd(other), "self": self.mean_frequencies(), "other": other.mean_frequencies()}

    def __repr__(self) -> str:
        return f"MotifStats(n_graphs={self.n_graphs}, n={self.n})"


# ---------------------------------------------------------------------------
# Spectral density from the Chebyshev moments of ``snd_graph_spectrum``
# ---------------------------------------------------------------------------
def jackson_weights(n_moments: int) -> np.ndarray:
    """g_k, k < K, of the Jackson kernel (Weisse et al., Rev. Mod. Phys. 78, 2006, eq. 71):
    [(K - k + 1) cos(pi k / (K + 1)) + sin(pi k / (K + 1)) cot(pi / (K + 1))] / (K + 1)."""
    K = int(n_moments)
    k = np.arange(K, dtype=np.float64)
    q = np.pi / (K + 1.0)
    return ((K - k + 1.0) * np.cos(q * k) + np.sin(q * k) / np.tan(q)) / (K + 1.0)


class SpectrumStats:
    """moments [G, K] (float64) and info [G, 4] (int64) of a set of G graphs of n nodes each
    (``layers.graph_spectrum`` / ``snd_graph_spectrum``): per graph the Chebyshev moments
    mu_k = tr T_k(L - I) of the normalised Laplacian L of its mutual-edge graph (exact, or a
    Hutchinson estimate over Rademacher probes) and {edges, isolated nodes, one-way arcs,
    probes used}.  ``density`` rebuilds the eigenvalue histogram over [0, 2] by the kernel
    polynomial method with the Jackson kernel: resolution pi / K, non-negative, total mass 1.

    Same storage idiom as GraphStats / PathStats: NumPy arrays or torch tensors; device
    tensors are read back once, on first use.
    """

    def __init__(self, moments, info, n: int):
        self._dev = None
        self._np = None
        self.n = int(n)
        if self.n < 1:
            raise ValueError("SpectrumStats: n must be >= 1")
        if _is_tensor(moments) != _is_tensor(info):
            raise ValueError("SpectrumStats: moments and info must both be tensors or both arrays")
        if _is_tensor(moments):
            if moments.dim() != 2 or moments.shape[1] < 2 or tuple(info.shape) != (moments.shape[0], 4):
                raise ValueError("SpectrumStats: expected moments [G, K >= 2] and info [G, 4]")
            self._dev = (moments, info)
        else:
            m = np.asarray(moments, dtype=np.float64)
            i = np.asarray(info, dtype=np.int64)
            if m.ndim == 1:
                m, i = m[None], i.reshape(1, -1)
            if m.ndim != 2 or m.shape[1] < 2 or i.shape != (m.shape[0], 4):
                raise ValueError("SpectrumStats: expected moments [G, K >= 2] and info [G, 4]")
            self._np = (m, i)

    # ---- storage
    @property
    def tensors(self):
        """The (moments, info) torch tensors this object was built on, or None."""
        return self._dev

    def invalidate(self) -> None:
        """Forget the host copy: the device tensors were written since it was read."""
        if self._dev is not None:
            self._np = None

    def _arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        if self._np is None:
            self._np = (self._dev[0].cpu().numpy().astype(np.float64, copy=False),
                        self._dev[1].cpu().numpy().astype(np.int64, copy=False))
        return self._np

    @property
    def moments(self) -> np.ndarray:
        return self._arrays()[0]

    @property
    def info(self) -> np.ndarray:
        return self._arrays()[1]

    @property
    def n_graphs(self) -> int:
        return int((self._dev[0] if self._np is None else self._np[0]).shape[0])

    @property
    def n_moments(self) -> int:
        return int((self._dev[0] if self._np is None else self._np[0]).shape[1])

    def __eq__(self, other) -> bool:
        return (isinstance(other, SpectrumStats) and self.n == other.n
                and np.array_equal(self.moments, other.moments) and np.array_equal(self.info, other.info))

    __hash__ = None

    @classmethod
    def concat(cls, parts) -> "SpectrumStats":
        """The graphs of several SpectrumStats (batches of one dataset) as one set, in order."""
        parts = list(parts)
        if not parts or not all(isinstance(p, SpectrumStats) for p in parts):
            raise ValueError("SpectrumStats.concat: expected a non-empty list of SpectrumStats")
        if any(p.n != parts[0].n or p.n_moments != parts[0].n_moments for p in parts):
            raise ValueError("SpectrumStats.concat: the parts differ in n or in the number of moments")
        return cls(np.concatenate([p.moments for p in parts]), np.concatenate([p.info for p in parts]), parts[0].n)

    def all_gather(self, process_group=None) -> "SpectrumStats":
        """Every rank's graphs as one set, in rank order (data parallel; each rank holds the
        same number of graphs), as a new SpectrumStats: the same on every rank."""
        import torch
        import torch.distributed as dist
        dev = self._dev[0].device if self._dev is not None else torch.device("cpu")
        if dev.type == "cpu" and dist.get_backend(process_group) == "nccl":
            dev = torch.device("cuda", torch.cuda.current_device())
        world = dist.get_world_size(process_group)
        both = []
        for x in (self.moments, self.info):
            t = torch.from_numpy(x.copy()).to(dev)
            out = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(out, t, group=process_group)
            both.append(torch.cat(out))
        return SpectrumStats(both[0], both[1], self.n)

    # ---- descriptors
    def density(self, bins: int = 200) -> np.ndarray:
        """[G, bins] float64: the Jackson-damped spectral mass of each of ``bins`` equal-width
        bins of lambda in [0, 2], integrated in closed form in theta = arccos(lambda - 1):

            mass(a, b) = [g_0 mu_0 (theta_a - theta_b)
                          + 2 sum_{k >= 1} g_k mu_k (sin k theta_a - sin k theta_b) / k] / (pi mu_0).

        Rows are >= 0 (rounding noise below zero is clipped) and sum to 1."""
        bins = int(bins)
        if bins < 1:
            raise ValueError("SpectrumStats.density: bins must be >= 1")
        m = self.moments
        K = m.shape[1]
        theta = np.arccos(np.clip(np.linspace(0.0, 2.0, bins + 1) - 1.0, -1.0, 1.0))    # pi .. 0
        k = np.arange(1, K, dtype=np.float64)
        coef = m[:, 1:] * (jackson_weights(K)[1:] / k)[None, :]                        # [G, K - 1]
        cum = theta[None, :] * m[:, :1] + 2.0 * coef @ np.sin(k[:, None] * theta[None, :])
        mass = (cum[:, :-1] - cum[:, 1:]) / (np.pi * m[:, :1])
        return np.maximum(mass, 0.0)

    def pooled(self, bins: int = 200) -> np.ndarray:
        """The mean density over the graphs of the set."""
        return self.density(bins).mean(axis=0)

    def second_moment(self) -> np.ndarray:
        """[G]: tr(M^2) / N = (mu_2 + mu_0) / (2 mu_0) (T_2(x) = 2 x^2 - 1); nan with K < 3."""
        m = self.moments
        if m.shape[1] < 3:
            return np.full(m.shape[0], NAN)
        return (m[:, 2] + m[:, 0]) / (2.0 * m[:, 0])

    def summary(self) -> dict:
        """The set as a whole: n_graphs, n_moments, the mean share of isolated nodes, the mean
        number of one-way arcs and the mean of tr(M^2) / N; nan without a graph."""
        i = self.info
        mean = lambda x: float(np.mean(x)) if x.size else NAN
        return {"n_graphs": self.n_graphs, "n_moments": self.n_moments,
                "mean_isolated_share": mean(i[:, 1] / float(self.n)), "mean_one_way": mean(i[:, 2].astype(np.float64)),
                "mean_second_moment": mean(self.second_moment())}

    # ---- two-sample statistics
    def _check_other(self, other):
        if not isinstance(other, SpectrumStats):
            raise ValueError("SpectrumStats: expected another SpectrumStats")

    def mmd(self, other: "SpectrumStats", sigma: float = 1.0, bins: int = 200) -> float:
        """GraphStats.mmd's statistic (biased MMD^2, Gaussian kernel over the EMD in lambda
        units) between the two sets' spectral densities: the spectral descriptor of GRAN's
        evaluation (Liao et al., NeurIPS 2019), restated here on the reconstructed histograms."""
        self._check_other(other)
        sigma = float(sigma)
        if not sigma > 0.0:
            raise ValueError("SpectrumStats.mmd: sigma must be > 0")
        return _emd_mmd(self.density(bins), other.density(bins), 2.0 / bins, sigma)

    def kld(self, other: "SpectrumStats", eps: float = 1e-12, bins: int = 200) -> float:
        """KL(self || other) of the pooled densities, each smoothed by eps per bin and
        renormalised (scipy.stats.entropy(p + eps, q + eps)).  nan when either side is empty."""
        self._check_other(other)
        if self.n_graphs == 0 or other.n_graphs == 0:
            return NAN
        p, q = self.pooled(bins), other.pooled(bins)
        p = (p + eps) / (p + eps).sum()
        q = (q + eps) / (q + eps).sum()
        return float(np.sum(p * np.log(p / q)))

    def compare(self, other: "SpectrumStats") -> dict:
        """{"mmd_spectrum", "kld_spectrum"} and both sides' summaries under "self" and "other"."""
        self._check_other(other)
        return {"mmd_spectrum": self.mmd(other), "kld_spectrum": self.kld(other), "self": self.summary(),
                "other": other.summary()}

    def __repr__(self) -> str:
        return f"SpectrumStats(n_graphs={self.n_graphs}, n={self.n}, n_moments={self.n_moments})"


# ---------------------------------------------------------------------------
# Edge crossings and edge directions from the counters of ``snd_graph_crossings``
# ---------------------------------------------------------------------------
CROSSING_KINDS = ("crossings", "orientation", "cross_angle")
CROSSING_NAMES = ("E", "X", "crossed", "independent", "one_way", "zero_length", "max_c")
ORIENTATION_BINS = 32


def orientation_entropy(h: np.ndarray) -> np.ndarray:
    """Shannon entropy (nats) of the directions hist [..., 256] (bins centred on k pi / 256) over
    ORIENTATION_BINS = 32 bins centred on j pi / 32: fine bin k goes to ((k + 4) mod 256) // 8, so
    axis-aligned and diagonal edges sit in the centre of a coarse bin, as Boeing shifts his bins
    (Urban spatial order, Appl. Netw. Sci. 4 (2019), section 3.2).  nan without an edge."""
    h = np.asarray(h, dtype=np.float64)
    w = GS_BINS // ORIENTATION_BINS
    coarse = np.roll(h, w // 2, axis=-1).reshape(h.shape[:-1] + (ORIENTATION_BINS, w)).sum(axis=-1)
    p = _normalised(coarse)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0).sum(axis=-1)
    return np.where(coarse.sum(axis=-1) > 0, ent, NAN)


def orientation_order(entropy) -> np.ndarray:
    """Boeing's orientation order phi = 1 - ((H - H_g) / (H_max - H_g))^2 (Boeing 2019, eq. 2)
    restated for directions folded to [0, pi): a perfect grid has two of the 32 bins, so
    H_g = ln 2 and H_max = ln 32 (his unfolded bearings: 4 of 36 bins).  1 for a grid, 0 for
    uniform directions."""
    e = np.asarray(entropy, dtype=np.float64)
    return 1.0 - ((e - math.log(2.0)) / (math.log(ORIENTATION_BINS) - math.log(2.0))) ** 2


class CrossingStats:
    """counts [G, 7] and hist [G, 3, 256] of a set of G graphs of n nodes each
    (``layers.graph_crossings`` / ``snd_graph_crossings``): per graph counts = {E edges, X
    crossing pairs, edges with a crossing, independent pairs (the pairs of edges without a
    common node), one-way arcs ignored, zero-length edges, the largest crossing count of one
    edge} and the histograms of the per-edge crossing count (bin = min(c, 255)), of the edge
    direction folded to [0, pi) (256 bins centred on k pi / 256) and of the acute angle of every
    crossing pair (256 bins over [0, pi / 2]).  A graph that was not counted (its E (E - 1) / 2
    pairs exceeded ``work_cap``) holds -1 in counts and is left out of every statistic below.

    Is a generated spatial network drawn like the data: is it planar as embedded, how many of
    its edges cross (Barthelemy, Spatial networks, Phys. Rep. 499 (2011), section 2.1), do its
    edges follow the data's directions (Boeing 2019)?  Same storage idiom as GraphStats: NumPy
    arrays or two int64 torch tensors, device tensors read back once, on first use.
    """

    def __init__(self, counts, hist, n: int):
        self._dev = None
        self._np = None
        self.n = int(n)
        if self.n < 1:
            raise ValueError("CrossingStats: n must be >= 1")
        if _is_tensor(counts):
            if (counts.dim() != 2 or counts.shape[1] != 7
                    or tuple(hist.shape) != (counts.shape[0], 3, GS_BINS)):
                raise ValueError("CrossingStats: expected counts [G, 7] and hist [G, 3, 256]")
            self._dev = (counts, hist)
        else:
            c = np.asarray(counts, dtype=np.int64)
            h = np.asarray(hist, dtype=np.int64)
            if c.ndim == 1:
                c, h = c[None], h[None]
            if c.ndim != 2 or c.shape[1] != 7 or h.shape != (c.shape[0], 3, GS_BINS):
                raise ValueError("CrossingStats: expected counts [G, 7] and hist [G, 3, 256]")
            self._np = (c, h)

    # ---- storage
    @property
    def tensors(self):
        """The (counts, hist) torch tensors this object was built on, or None."""
        return self._dev

    def invalidate(self) -> None:
        """Forget the host copy: the device tensors were written since it was read."""
        if self._dev is not None:
            self._np = None

    def _arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        if self._np is None:
            import torch
            c, h = self._dev
            both = torch.cat([c.reshape(-1), h.reshape(-1)]).cpu().numpy()     # one read-back
            k = c.numel()
            self._np = (both[:k].reshape(tuple(c.shape)), both[k:].reshape(tuple(h.shape)))
        return self._np

    @property
    def counts(self) -> np.ndarray:
        return self._arrays()[0]

    @property
    def hist(self) -> np.ndarray:
        return self._arrays()[1]

    @property
    def n_graphs(self) -> int:
        """All graphs of the set, skipped ones included."""
        return int((self._dev[0] if self._np is None else self._np[0]).shape[0])

    @property
    def counted(self) -> np.ndarray:
        """[G] bool: the graphs that were counted."""
        return self.counts[:, 0] >= 0

    @property
    def n_skipped(self) -> int:
        return int((~self.counted).sum())

    @property
    def one_way(self) -> int:
        """One-way arcs ignored, over the counted graphs."""
        return int(self.counts[self.counted, 4].sum())

    def __eq__(self, other) -> bool:
        return (isinstance(other, CrossingStats) and self.n == other.n
                and np.array_equal(self.counts, other.counts) and np.array_equal(self.hist, other.hist))

    __hash__ = None

    @classmethod
    def concat(cls, parts) -> "CrossingStats":
        """The graphs of several CrossingStats (batches of one dataset) as one set, in order."""
        parts = list(parts)
        if not parts or not all(isinstance(p, CrossingStats) for p in parts):
            raise ValueError("CrossingStats.concat: expected a non-empty list of CrossingStats")
        if any(p.n != parts[0].n for p in parts):
            raise ValueError("CrossingStats.concat: the parts differ in n")
        return cls(np.concatenate([p.counts for p in parts]), np.concatenate([p.hist for p in parts]), parts[0].n)

    def all_gather(self, process_group=None) -> "CrossingStats":
        """Every rank's graphs as one set, in rank order (data parallel; each rank holds the
        same number of graphs), as a new CrossingStats: the same on every rank."""
        import torch
        import torch.distributed as dist
        dev = self._dev[0].device if self._dev is not None else torch.device("cpu")
        if dev.type == "cpu" and dist.get_backend(process_group) == "nccl":
            dev = torch.device("cuda", torch.cuda.current_device())
        if self._dev is not None and self._dev[0].device == dev:
            c, h = self._dev
        else:
            c = torch.from_numpy(self.counts.copy()).to(dev)
            h = torch.from_numpy(self.hist.copy()).to(dev)
        flat = torch.cat([c.reshape(-1), h.reshape(-1)])
        out = [torch.empty_like(flat) for _ in range(dist.get_world_size(process_group))]
        dist.all_gather(out, flat, group=process_group)
        k = c.numel()
        return CrossingStats(torch.cat([o[:k].reshape(c.shape) for o in out]),
                             torch.cat([o[k:].reshape(h.shape) for o in out]), self.n)

    # ---- bins
    def _kind(self, kind: str):
        """(row of hist, bin width in the statistic's own units, default sigma)."""
        if kind == "crossings":
            return 0, 1.0, 1.0                                   # crossings of one edge
        if kind == "orientation":
            return 1, math.pi / GS_BINS, 0.25                    # radians, the histogram cut at 0
        if kind == "cross_angle":
            return 2, math.pi / (2 * GS_BINS), 0.25              # radians
        raise ValueError(f"CrossingStats: kind must be one of {CROSSING_KINDS}, got {kind!r}")

    # ---- scalar properties
    @staticmethod
    def _scalars(c: np.ndarray, h: np.ndarray) -> dict:
        c = c.astype(np.float64)
        E, X = c[:, 0], c[:, 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = lambda a, b: np.where(b > 0, a / np.where(b > 0, b, 1.0), NAN)
            centres = (np.arange(GS_BINS, dtype=np.float64) + 0.5) * (math.pi / (2 * GS_BINS))
            ent = orientation_entropy(h[:, 1, :])
            return {"planar": (X == 0).astype(np.float64), "crossings_per_edge": ratio(X, E),
                    "crossing_ratio": ratio(X, c[:, 3]), "crossed_share": ratio(c[:, 2], E),
                    "orientation_entropy": ent, "orientation_order": orientation_order(ent),
                    "mean_cross_angle": ratio((h[:, 2, :] * centres).sum(axis=1), h[:, 2, :].sum(axis=1))}

    def per_graph(self) -> dict:
        """{name: array over the counted graphs}: the seven counts (int64) and

        * planar = 1.0 where X = 0: planar as drawn (a straight-line drawing without a crossing);
        * crossings_per_edge = X / E; crossing_ratio = X / independent pairs, the share of the
          pairs of edges that could cross that do; crossed_share = crossed edges / E;
        * orientation_entropy H (nats, 32 bins, ``orientation_entropy``) and orientation_order
          phi = 1 - ((H - ln 2) / (ln 32 - ln 2))^2 (``orientation_order``: Boeing 2019, eq. 2,
          restated for folded directions);
        * mean_cross_angle (radians, from the bin centres of the 256 bins over [0, pi / 2]).

        nan where a ratio has no denominator."""
        keep = self.counted
        c, h = self.counts[keep], self.hist[keep]
        out = {k: c[:, i] for i, k in enumerate(CROSSING_NAMES)}
        out.update(self._scalars(c, h))
        return out

    def summary(self) -> dict:
        """The set as a whole, as floats: planar is the share of the counted graphs with X = 0;
        the ratios, the orientation entropy and order and the mean crossing angle are those of
        the pooled counters (every edge of every graph weighs the same); n_skipped and one_way
        are counts.  nan where nothing was counted."""
        keep = self.counted
        out = {"n_skipped": self.n_skipped, "one_way": self.one_way}
        names = ("planar", "crossings_per_edge", "crossing_ratio", "crossed_share", "orientation_entropy",
                 "orientation_order", "mean_cross_angle")
        if not keep.any():
            out.update({k: NAN for k in names})
            return out
        c, h = self.counts[keep], self.hist[keep]
        pooled = self._scalars(c.sum(axis=0, keepdims=True), h.sum(axis=0, keepdims=True))
        out.update({k: float(pooled[k][0]) for k in names})
        out["planar"] = float((c[:, 1] == 0).mean())
        return out

    planar = property(lambda self: self.summary()["planar"])
    crossing_ratio = property(lambda self: self.summary()["crossing_ratio"])

    # ---- two-sample statistics
    def _check_other(self, other, kind):
        if not isinstance(other, CrossingStats):
            raise ValueError("CrossingStats: expected another CrossingStats")
        return self._kind(kind)

    def mmd(self, other: "CrossingStats", kind: str, sigma=None) -> float:
        """Biased (V-statistic) MMD^2 between two sets of graphs over their per-graph normalised
        histograms of ``kind``, with GraphStats.mmd's kernel k = exp(-EMD^2 / (2 sigma^2)), the
        EMD in the statistic's own units (crossings of an edge; radians, the circular direction
        histogram cut at 0).  Default sigma: 1.0 crossing, 0.25 rad.  Skipped graphs are left
        out; a graph without an edge or a crossing enters as the zero histogram."""
        row, width, s0 = self._check_other(other, kind)
        sigma = s0 if sigma is None else float(sigma)
        if not sigma > 0.0:
            raise ValueError("CrossingStats.mmd: sigma must be > 0")
        return _emd_mmd(self.hist[self.counted][:, row, :], other.hist[other.counted][:, row, :], width, sigma)

    def pooled(self, kind: str) -> np.ndarray:
        """The normalised histogram of ``kind`` over the counted graphs of the set."""
        row, _, _ = self._kind(kind)
        return _normalised(self.hist[self.counted][:, row, :].sum(axis=0))

    def kld(self, other: "CrossingStats", kind: str, eps: float = 1e-12) -> float:
        """KL(self || other) of the pooled normalised histograms, smoothed as GraphStats.kld
        (eps per bin, renormalised).  nan when either side has no count."""
        self._check_other(other, kind)
        p, q = self.pooled(kind), other.pooled(kind)
        if p.sum() == 0 or q.sum() == 0:
            return NAN
        p = (p + eps) / (p + eps).sum()
        q = (q + eps) / (q + eps).sum()
        return float(np.sum(p * np.log(p / q)))

    def compare(self, other: "CrossingStats") -> dict:
        """mmd_<kind> and kld_<kind> for "crossings", "orientation" and "cross_angle", both
        sides' summaries under "self" and "other" and the graphs left out under "n_skipped"
        (self, other)."""
        if not isinstance(other, CrossingStats):
            raise ValueError("CrossingStats.compare: expected another CrossingStats")
        out = {}
        for kind in CROSSING_KINDS:
            out[f"mmd_{kind}"] = self.mmd(other, kind)
            out[f"kld_{kind}"] = self.kld(other, kind)
        out["n_skipped"] = (self.n_skipped, other.n_skipped)
        out["self"] = self.summary()
        out["other"] = other.summary()
        return out

    def __repr__(self) -> str:
        return f"CrossingStats(n_graphs={self.n_graphs}, n={self.n}, n_skipped={self.n_skipped})"


class LatentMI:
    """mi [L, K], hz [L] and hf [K] of ``layers.latent_mi`` / ``snd_latent_mi``: the mutual
    information (nats) between every latent dimension and every generative factor and the
    entropies of their binned marginals, the third of the reference's evaluations
    (``disentangle_evaluation``, `main.py:424`).

    The reference's own ``utils/evaluation.py`` is not shipped, so the scores below are this
    project's definitions, each from the paper its docstring cites; all of them are host
    arithmetic on the matrix R[l, k] = mi[l, k] / hf[k] (0 where hf[k] = 0: a factor that
    never varies carries no information).  Built from NumPy arrays or from three float64
    torch tensors; device tensors are read back once, on first use.

    ``groups`` maps group names to the column slices of the latent axis, in display order:
    ``{"s": slice(0, Ls), "g": slice(Ls, Ls + Lg), "sg": slice(Ls + Lg, L)}`` for the
    disentangled model (``DisentangledSGCNModelVAE.latent_means``); None is one group "z".
    """

    def __init__(self, mi, hz, hf, groups=None):
        self._dev = None
        self._np = None
        if _is_tensor(mi):
            if mi.dim() != 2 or tuple(hz.shape) != (mi.shape[0],) or tuple(hf.shape) != (mi.shape[1],):
                raise ValueError("LatentMI: expected mi [L, K], hz [L] and hf [K]")
            self._dev = (mi, hz, hf)
            L = int(mi.shape[0])
        else:
            m, a, b = (np.asarray(x, dtype=np.float64) for x in (mi, hz, hf))
            if m.ndim != 2 or a.shape != (m.shape[0],) or b.shape != (m.shape[1],):
                raise ValueError("LatentMI: expected mi [L, K], hz [L] and hf [K]")
            self._np = (m, a, b)
            L = m.shape[0]
        if L < 1 or (self._dev[0] if self._np is None else self._np[0]).shape[1] < 1:
            raise ValueError("LatentMI: expected at least one latent and one factor")
        if groups is None:
            groups = {"z": slice(0, L)}
        self.groups = {}
        seen = np.zeros(L, np.int64)
        for name, sl in groups.items():
            if not isinstance(sl, slice):
                raise ValueError(f"LatentMI: groups[{name!r}] must be a slice")
            lo, hi, step = sl.indices(L)
            if step != 1 or hi <= lo:
                raise ValueError(f"LatentMI: groups[{name!r}] = {sl} is empty or strided over {L} latents")
            self.groups[str(name)] = slice(lo, hi)
            seen[lo:hi] += 1
        if not np.all(seen == 1):
            raise ValueError(f"LatentMI: the groups must cover each of the {L} latents exactly once")

    # ---- storage
    @property
    def tensors(self):
        """The (mi, hz, hf) torch tensors this object was built on, or None."""
        return self._dev

    def invalidate(self) -> None:
        """Forget the host copy: the device tensors were written since it was read."""
        if self._dev is not None:
            self._np = None

    def _arrays(self):
        if self._np is None:
            import torch
            m, a, b = self._dev
            both = torch.cat([m.reshape(-1), a.reshape(-1), b.reshape(-1)]).cpu().numpy()     # one read-back
            L, K = m.shape
            self._np = (both[:L * K].reshape(L, K), both[L * K:L * K + L], both[L * K + L:])
        return self._np

    @property
    def mi(self) -> np.ndarray:
        return self._arrays()[0]

    @property
    def hz(self) -> np.ndarray:
        return self._arrays()[1]

    @property
    def hf(self) -> np.ndarray:
        return self._arrays()[2]

    @property
    def n_latents(self) -> int:
        return int((self._dev[0] if self._np is None else self._np[0]).shape[0])

    @property
    def n_factors(self) -> int:
        return int((self._dev[0] if self._np is None else self._np[0]).shape[1])

    def __eq__(self, other) -> bool:
        return (isinstance(other, LatentMI) and self.groups == other.groups and np.array_equal(self.mi, other.mi)
                and np.array_equal(self.hz, other.hz) and np.array_equal(self.hf, other.hf))

    __hash__ = None

    # ---- scores
    def normalised(self) -> np.ndarray:
        """R[l, k] = mi[l, k] / hf[k], 0 where hf[k] = 0 (the normalisation of Chen et al.
        2018, eq. 6: I(z_l; v_k) / H(v_k) lies in [0, 1])."""
        hf = self.hf
        return np.divide(self.mi, hf[None, :], out=np.zeros_like(self.mi), where=hf[None, :] > 0)

    def mig(self) -> float:
        """Mutual information gap (Chen et al. 2018, "Isolating Sources of Disentanglement
        in VAEs", eq. 6; this project's statement of it): per factor the largest R[:, k]
        minus the second largest (0 for the second when there is one latent), averaged over
        the factors with hf > 0.  NaN when no factor varies.  Higher is better; 1 when
        every factor is copied by exactly one latent."""
        R, live = self.normalised(), self.hf > 0
        if not live.any():
            return NAN
        top = np.sort(R[:, live], axis=0)[::-1]
        second = top[1] if top.shape[0] > 1 else np.zeros_like(top[0])
        return float(np.mean(top[0] - second))

    def avg_mi(self) -> float:
        """avgMI as the SND-VAE / NED-VAE papers use it (Guo et al. 2020, "Interpretable
        Deep Graph Generation with Node-Edge Co-Disentanglement", and the SND-VAE paper's
        Table; this project's statement): the squared distance of R from the one-to-one
        assignment T, T[l, k] = 1 at l = argmax_l R[l, k] (the lowest index on a tie) and 0
        elsewhere, sum (R - T)^2 / K.  Lower is better; 0 when every factor is copied by one
        latent and known to no other."""
        R = self.normalised()
        T = np.zeros_like(R)
        T[np.argmax(R, axis=0), np.arange(R.shape[1])] = 1.0
        return float(np.sum((R - T) ** 2) / R.shape[1])

    def modularity(self) -> float:
        """Modularity (Ridgeway and Mozer 2018, "Learning Deep Disentangled Embeddings with
        the F-Statistic Loss", eq. 2-3; this project's statement): per latent with
        theta = max_k mi[l, k]^2 > 0 the value 1 - sum_{k != k*} mi[l, k]^2 / (theta (K - 1)),
        averaged over those latents; 1 when K = 1, NaN when no latent has any information.
        1 when every latent knows about one factor only."""
        m2 = self.mi ** 2
        K = m2.shape[1]
        if K == 1:
            return 1.0
        theta = m2.max(axis=1)
        live = theta > 0
        if not live.any():
            return NAN
        rest = m2[live].sum(axis=1) - theta[live]
        return float(np.mean(1.0 - rest / (theta[live] * (K - 1))))

    def group_share(self) -> np.ndarray:
        """[K, groups]: the share of factor k's information held by each latent group,
        sum_{l in group} mi[l, k] / sum_l mi[l, k] (0 where the denominator is 0), columns in
        the order of ``groups``.  For the disentangled model this is the SND-VAE claim in one
        table: does the spatial factor live in z_s, the graph factor in z_g, the joint one in
        z_sg.  This project's definition."""
        mi = self.mi
        tot = mi.sum(axis=0)
        part = np.stack([mi[sl].sum(axis=0) for sl in self.groups.values()], axis=1)
        return np.divide(part, tot[:, None], out=np.zeros_like(part), where=tot[:, None] > 0)

    def best_latent(self):
        """Per factor the (group, index within the group) of the latent with the largest
        R[:, k] (the lowest index on a tie)."""
        out = []
        for l in np.argmax(self.normalised(), axis=0):
            for name, sl in self.groups.items():
                if sl.start <= l < sl.stop:
                    out.append((name, int(l - sl.start)))
        return out

    def summary(self) -> dict:
        return {"mig": self.mig(), "avg_mi": self.avg_mi(), "modularity": self.modularity(),
                "group_share": self.group_share(), "best_latent": self.best_latent(),
                "groups": list(self.groups)}

    def __repr__(self) -> str:
        return f"LatentMI(latents={self.n_latents}, factors={self.n_factors}, groups={list(self.groups)})"
