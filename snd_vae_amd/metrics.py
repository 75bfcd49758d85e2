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
