"""Functional hot-path ops over torch device tensors, backed by libsndvae.so.

Named after the reference layer functions they replace (`layers.py`):
``GraphConvolution`` (:115-125), ``linear`` (:566-576), ``InnerProductDecoder``
(:400-410) fused with the CE of `optimizer.py:142-144`, ``conv1d`` SAME as
used by the decoders (`model_joint.py:115,138`).  The reference versions
create TF variables under a variable_scope; these take the weights
explicitly (the flat parameter buffer owns them, `params.py`).  Forward
only, except where the reference's loss gradient is fused (CE, MSE).
Every call is one or a few HIP launches on the current stream; there is no
CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .model import DTYPES

_P = _lib.ptr
MOTIFS_MAX_N = 16384             # snd_graph_motifs: local ids are 16-bit on chip
# Default work_cap of graph_motifs: the op ran 2.45e11 units of its work bound per second on K512
# (tools/graph_motifs_timing.py), so a graph at this cap takes about a second.
MOTIFS_WORK_CAP = 200_000_000_000
SPECTRUM_MAX_N = 16384           # snd_graph_spectrum
CROSSINGS_MAX_N = 16384          # snd_graph_crossings: local ids are 16-bit on chip
CROSSINGS_TILE = 64              # kGxTile: edges per tile of the all-pairs kernel
# Default work_cap of graph_crossings, in edge pairs: the op ran 3.7e11 pairs per second on 10^5 long
# random edges, where nearly every pair reaches the double predicate and a quarter cross
# (tools/graph_crossings_timing.py, "chords"; 1.6e12 on the bench graphs), so a graph at this cap
# takes about a second at the slower rate.
CROSSINGS_WORK_CAP = 400_000_000_000
SPECTRUM_MAX_MOMENTS = 512
SPECTRUM_EXACT_MAX_N = 256       # graph_spectrum's default: exact traces up to here ...
SPECTRUM_PROBES = 32             # ... and this many Rademacher probes above


def _dt(dtype):
    return DTYPES[dtype] if isinstance(dtype, str) else int(dtype)


def graph_convolution(rowptr, colidx, h, w, gamma=None, beta=None, concat_x=None,
                      enc_gamma=None, enc_beta=None, dtype="f32"):
    """GraphConvolution(adj, h, out) + BN + concat (model.py:107-112).

    Returns (out, preact[, out2]).  Without gamma/beta: plain lrelu(A (h w))
    is not separable from BN in the fused kernel, so gamma=1, beta=0 is used.
    """
    width = w.shape[1]
    xw = linear(h, w, None, dtype)
    if gamma is None:
        gamma = torch.ones(width, device=h.device)
        beta = torch.zeros(width, device=h.device)
    out, pre, out2 = ops.spmm_gcn(rowptr, colidx, xw, gamma, beta, concat_x, enc_gamma, enc_beta)
    return (out, pre, out2) if out2 is not None else (out, pre)


def spmm(rowptr, colidx, h):
    """A @ h on the block-diagonal CSR (tf.matmul(adj, x), layers.py:122)."""
    ops.f32("spmm", h)
    return ops.spmm(rowptr, colidx, h)


def spmm_bf16(rowptr, colidx, h, n_per_graph=0, n_graphs=0, row_order=None):
    """A @ h over bf16 rows, fp32 accumulation (the bf16 path's SpMM, layers.py:122).

    n_per_graph / n_graphs let the kernel keep each graph's row blocks on one XCD;
    row_order (int32 device tensor, data.locality_order) is the processing schedule."""
    if not (h.is_cuda and h.is_contiguous() and h.dtype == torch.bfloat16):
        raise ValueError("spmm_bf16: expected a contiguous bfloat16 device tensor")
    rows, width = h.shape
    out = torch.empty_like(h)
    _lib.check(_lib.lib().snd_csr_spmm_bf16(
        _P(rowptr), _P(colidx), rows, _P(h), width, width, _P(out), width, n_per_graph,
        n_graphs, _P(row_order), _lib.stream_ptr()), "snd_csr_spmm_bf16")
    return out


def spmm_bf16_tiled(rowptr, colidx, tiles, h, n_per_graph=0, n_graphs=0, row_order=None):
    """spmm_bf16 over row tiles (snd_csr_spmm_bf16_tiled): neighbour rows staged in LDS.

    tiles: model.DeviceTiles over the schedule row_order (data.row_tiles);
    bit-identical to spmm_bf16."""
    if not (h.is_cuda and h.is_contiguous() and h.dtype == torch.bfloat16):
        raise ValueError("spmm_bf16_tiled: expected a contiguous bfloat16 device tensor")
    rows, width = h.shape
    out = torch.empty_like(h)
    t = tiles.c_struct()
    _lib.check(_lib.lib().snd_csr_spmm_bf16_tiled(
        _P(rowptr), _P(colidx), rows, C.byref(t), _P(h), width, width, _P(out), width,
        n_per_graph, n_graphs, _P(row_order), _lib.stream_ptr()), "snd_csr_spmm_bf16_tiled")
    return out


class DeviceWindowPlan:
    """data.WindowPlan on the device (meta, slots, rows, order) for spmm_bf16_window."""

    def __init__(self, plan, device="cuda"):
        self.meta = torch.from_numpy(plan.meta).to(device)
        self.slots = torch.from_numpy(plan.slots.view(np.int16)).to(device)
        self.rows = torch.from_numpy(plan.rows).to(device)
        self.order = torch.from_numpy(plan.order).to(device)
        self.beta = plan.beta


def spmm_bf16_window(wplan, h, n_per_graph, n_graphs):
    """spmm_bf16 streamed through an LDS window (snd_csr_spmm_bf16_window; plan:
    data.window_plan): bit-identical to spmm_bf16 on every tested batch.
    wplan: DeviceWindowPlan."""
    if not (h.is_cuda and h.is_contiguous() and h.dtype == torch.bfloat16):
        raise ValueError("spmm_bf16_window: expected a contiguous bfloat16 device tensor")
    rows, width = h.shape
    out = torch.empty_like(h)
    L = _lib.lib()
    fn, name = L.snd_csr_spmm_bf16_window, "snd_csr_spmm_bf16_window"
    _lib.check(fn(_P(wplan.meta), _P(wplan.slots), _P(wplan.rows), _P(wplan.order), rows, n_per_graph, n_graphs,
                  wplan.beta, _P(h), width, width, _P(out), width, _lib.stream_ptr()), name)
    return out


def linear(x, w, b=None, dtype="f32", trans_w=False):
    """x @ w + b (layers.py:566-576) on MFMA (fp32 or bf16 operands, fp32 acc)."""
    ops.f32("linear x", x)
    return ops.gemm(x, w, tb=trans_w, bias=b, dtype=_dt(dtype))


def conv1d_same(x, w, b, n_per_graph, gamma=None, beta=None, dtype="f32"):
    """conv1d(k=5, SAME) [+ BN + lrelu] over each graph's node axis.

    Returns out (and y_pre when BN is applied)."""
    ops.f32("conv1d x", x)
    out, pre = ops.conv1d_same(x, w, b, n_per_graph, gamma, beta, _dt(dtype))
    return (out, pre) if gamma is not None else out


def conv1d_same_bwd(x, w, dy, n_per_graph, dtype="f32"):
    """(dx, dw) of conv1d SAME (TF autodiff of tf.layers.conv1d)."""
    return (ops.conv1d_same_bwd_data(dy, w, n_per_graph, _dt(dtype)),
            ops.conv1d_same_bwd_weight(x, dy, n_per_graph, _dt(dtype)))


def inner_product_ce(z, n_graphs, rowptr, colidx, pos_weight=1.0, norm=1.0, dtype="bf16"):
    """InnerProductDecoder + diagonal rule + softmax CE, fused (no logits in HBM).

    Returns (ce_sum, n_correct, dz) with dz = d(ce_sum)/dz."""
    ops.f32("inner_product_ce z", z)
    rows, d = z.shape
    n = rows // n_graphs
    L = _lib.lib()
    wsb = L.snd_zzt_ce_workspace(n_graphs, n, d, _dt(dtype))
    ws = torch.empty(wsb, dtype=torch.uint8, device=z.device)
    stats = torch.zeros(2, dtype=torch.float64, device=z.device)
    dz = torch.empty_like(z)
    _lib.check(L.snd_zzt_ce(_P(z), n_graphs, n, d, _P(rowptr), _P(colidx), pos_weight, norm,
                            _P(stats), _P(dz), _P(ws), wsb, _dt(dtype), _lib.stream_ptr()),
               "snd_zzt_ce")
    s = stats.cpu()
    return float(s[0]), float(s[1]), dz


def inner_product_ce_rows(z, row0, row1, rowptr, colidx, pos_weight=1.0, norm=1.0, dtype="bf16"):
    """The fused CE of one graph's rows [row0, row1) against all its columns
    (snd_zzt_ce_rows; the row-sharded zz^T of SURVEY §8e): z [n, d] is the WHOLE graph,
    rowptr the range's row pointers (a slice of the graph's CSR), colidx global ids.

    Returns (stats, dz_rows): stats a float64 device tensor [ce_sum, n_correct] over the
    range (left on the device for the caller's all-reduce); dz_rows [row1 - row0, d] is
    d(ce_sum over ALL pairs)/dz for those rows (L symmetric: no reduction needed)."""
    ops.f32("inner_product_ce_rows z", z)
    n, d = z.shape
    L = _lib.lib()
    wsb = L.snd_zzt_ce_rows_workspace(n, d, row0, row1, _dt(dtype))
    if wsb == 0:
        raise _lib.SNDError(f"snd_zzt_ce_rows_workspace: bad shape n={n} d={d} rows [{row0}, {row1})")
    ws = torch.empty(wsb, dtype=torch.uint8, device=z.device)
    stats = torch.zeros(2, dtype=torch.float64, device=z.device)
    dz = torch.empty(row1 - row0, d, dtype=torch.float32, device=z.device)
    _lib.check(L.snd_zzt_ce_rows(_P(z), n, d, row0, row1, _P(rowptr), _P(colidx), pos_weight, norm,
                                 _P(stats), _P(dz), _P(ws), wsb, _dt(dtype), _lib.stream_ptr()),
               "snd_zzt_ce_rows")
    return stats, dz


def zzt_eval(z, rowptr, colidx, n_graphs, n, hist=None, counts=None, accumulate=False):
    """Edge-score counters of the inner-product decoder (snd_zzt_eval): L = z z^T per graph
    on the fp32 matrix cores, binned and classified on chip; no logits in HBM.

    z: float32 device tensor [n_graphs * n, d] with unit column stride (its row stride is
    passed as ldz), 1 <= d <= 128.  Returns (hist, counts): int64 [n_graphs, 2, 2048]
    (label x logit bin of width 1/64 over [-16, 16)) and [n_graphs, 4] = {TP, FP, FN, TN}
    at L > 0 (metrics.EdgeCounts turns them into accuracy / F1 / ROC-AUC / AP).  Given
    ``hist`` / ``counts`` are cleared first, or added to with ``accumulate``.  No host
    synchronisation."""
    if not (z.is_cuda and z.dtype == torch.float32 and z.dim() == 2 and (z.shape[1] == 1 or z.stride(1) == 1)):
        raise ValueError("zzt_eval z: expected a float32 device tensor [rows, d] with unit column stride")
    rows, d = z.shape
    if n_graphs < 1 or n < 1 or rows != n_graphs * n:
        raise ValueError(f"zzt_eval: z has {rows} rows, expected n_graphs * n = {n_graphs} * {n}")
    for t, name, numel in ((rowptr, "rowptr", rows + 1), (colidx, "colidx", 1)):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and t.numel() >= numel):
            raise ValueError(f"zzt_eval {name}: expected a contiguous int32 device tensor of >= {numel} elements")
    if (hist is None) != (counts is None):
        raise ValueError("zzt_eval: pass both hist and counts or neither")
    if hist is None:
        if accumulate:
            raise ValueError("zzt_eval: accumulate needs hist and counts")
        hist = torch.empty(n_graphs, 2, 2048, dtype=torch.int64, device=z.device)
        counts = torch.empty(n_graphs, 4, dtype=torch.int64, device=z.device)
    for t, name, shape in ((hist, "hist", (n_graphs, 2, 2048)), (counts, "counts", (n_graphs, 4))):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int64 and tuple(t.shape) == shape):
            raise ValueError(f"zzt_eval {name}: expected a contiguous int64 device tensor {list(shape)}")
    L = _lib.lib()
    ldz = z.stride(0) if rows > 1 else max(d, z.stride(0))
    wsb = L.snd_zzt_eval_workspace(n_graphs, n, d)
    ws = torch.empty(wsb, dtype=torch.uint8, device=z.device) if wsb else None
    _lib.check(L.snd_zzt_eval(_P(z), ldz, n_graphs, n, d, _P(rowptr), _P(colidx), _P(hist), _P(counts),
                              int(bool(accumulate)), _P(ws), wsb, _lib.stream_ptr()), "snd_zzt_eval")
    return hist, counts


def margin_eval(margin, adj, hist=None, counts=None, accumulate=False):
    """``zzt_eval``'s counters for the e2e structure decoder (snd_margin_eval): the margin
    l1 - l0 of ``disent.structure_decode(..., want_margin=True)`` binned and classified
    against a dense adjacency.

    margin, adj: contiguous float32 device tensors [B, N, N]; the label is adj != 0 and the
    diagonal is skipped by index (counted as TN).  Returns (hist, counts): int64 [B, 2, 2048]
    (label x margin bin of width 1/64 over [-16, 16)) and [B, 4] = {TP, FP, FN, TN} at
    margin > 0, the format metrics.EdgeCounts takes.  Given ``hist`` / ``counts`` are cleared
    first, or added to with ``accumulate``.  No host synchronisation."""
    for t, name in ((margin, "margin"), (adj, "adj")):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.dim() == 3
                and t.shape[1] == t.shape[2] and t.shape[0] >= 1 and t.shape[1] >= 1):
            raise ValueError(f"margin_eval {name}: expected a contiguous float32 device tensor [B, N, N]")
    if margin.shape != adj.shape:
        raise ValueError(f"margin_eval: margin {tuple(margin.shape)} and adj {tuple(adj.shape)} differ")
    n_graphs, n = int(margin.shape[0]), int(margin.shape[1])
    if (hist is None) != (counts is None):
        raise ValueError("margin_eval: pass both hist and counts or neither")
    if hist is None:
        if accumulate:
            raise ValueError("margin_eval: accumulate needs hist and counts")
        hist = torch.empty(n_graphs, 2, 2048, dtype=torch.int64, device=margin.device)
        counts = torch.empty(n_graphs, 4, dtype=torch.int64, device=margin.device)
    for t, name, shape in ((hist, "hist", (n_graphs, 2, 2048)), (counts, "counts", (n_graphs, 4))):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int64 and tuple(t.shape) == shape):
            raise ValueError(f"margin_eval {name}: expected a contiguous int64 device tensor {list(shape)}")
    L = _lib.lib()
    wsb = L.snd_margin_eval_workspace(n_graphs, n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=margin.device) if wsb else None
    _lib.check(L.snd_margin_eval(_P(margin), _P(adj), n_graphs, n, _P(hist), _P(counts), int(bool(accumulate)),
                                 _P(ws), wsb, _lib.stream_ptr()), "snd_margin_eval")
    return hist, counts


def zzt_edges(z, n_graphs, n, threshold=0.0, inclusive=False, capacity=None):
    """The predicted graph of the inner-product decoder as a CSR (snd_zzt_edges): L = z z^T
    per graph on the fp32 matrix cores, thresholded on chip; neither the logits nor a dense
    adjacency reach HBM.

    z as for ``zzt_eval``.  (i, j) is an edge iff i != j and L_ij > threshold (>= with
    ``inclusive``, the rule ``EdgeCounts.best_f1`` reports); +-inf are legal, NaN is not.
    Returns (rowptr, colidx, nnz): the block-diagonal CSR with ascending global column ids,
    as ``DeviceBatch`` / ``zzt_eval`` / ``inner_product_ce`` take it.

    capacity=None: a sizing call, one host read of the total, ``colidx`` allocated exactly
    and the op run again; ``nnz`` is an int.  capacity=k: one call and no host
    synchronisation; ``colidx`` has k elements, ``nnz`` is an int64 device tensor [1] with
    the exact total, and ``colidx`` is left untouched when the total exceeds k."""
    if not (z.dtype == torch.float32 and z.dim() == 2 and (z.shape[1] == 1 or z.stride(1) == 1)):
        raise ValueError("zzt_edges z: expected a float32 device tensor [rows, d] with unit column stride")
    rows, d = z.shape
    if n_graphs < 1 or n < 1 or rows != n_graphs * n:
        raise ValueError(f"zzt_edges: z has {rows} rows, expected n_graphs * n = {n_graphs} * {n}")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("zzt_edges: threshold is NaN")
    if capacity is not None and (int(capacity) != capacity or capacity < 0):
        raise ValueError(f"zzt_edges: capacity must be a non-negative integer or None, got {capacity!r}")
    if not z.is_cuda:
        raise ValueError("zzt_edges z: expected a device tensor (there is no CPU path)")
    L = _lib.lib()
    ldz = z.stride(0) if rows > 1 else max(d, z.stride(0))
    wsb = L.snd_zzt_edges_workspace(n_graphs, n, d)
    ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=z.device)
    rowptr = torch.empty(rows + 1, dtype=torch.int32, device=z.device)
    nnz = torch.empty(1, dtype=torch.int64, device=z.device)

    def run(colidx, cap):
        _lib.check(L.snd_zzt_edges(_P(z), ldz, n_graphs, n, d, threshold, int(bool(inclusive)), _P(rowptr),
                                   _P(colidx), cap, _P(nnz), _P(ws), ws.numel(), _lib.stream_ptr()),
                   "snd_zzt_edges")

    if capacity is not None:
        colidx = torch.empty(max(int(capacity), 1), dtype=torch.int32, device=z.device)[:int(capacity)]
        run(colidx, int(capacity))
        return rowptr, colidx, nnz
    run(None, 0)
    total = int(nnz.item())
    if total >= 2 ** 31:
        raise ValueError(f"zzt_edges: {total} edges exceed the int32 CSR range")
    colidx = torch.empty(max(total, 1), dtype=torch.int32, device=z.device)
    run(colidx, total)
    return rowptr, colidx[:total], total


def graph_stats(rowptr, colidx, n_graphs, n, coords=None, max_len=None, hist=None, totals=None,
                accumulate=False, per_node=False):
    """Degree, triangle, local-clustering and edge-length statistics of a block-diagonal CSR
    (snd_graph_stats), one launch, nothing read back.

    rowptr / colidx: int32 device tensors as ``DeviceBatch`` holds and ``zzt_edges`` returns
    them (entries outside a row's graph block and self loops are ignored).  coords: float32
    device tensor [n_graphs * n, sd] with unit column stride, 1 <= sd <= 3, or None (no
    edge-length histogram); ``max_len`` is the length the 256 bins span (bin width
    max_len / 256, the last bin collects the overflow) and is required with coords.
    Returns (hist, totals): int64 [n_graphs, 3, 256] (degree, clustering, edge length) and
    [n_graphs, 4] = {sum deg, sum tri2, sum deg (deg - 1), entries with column > row}
    (metrics.GraphStats turns them into density, transitivity, MMD ...); with ``per_node``
    also (deg, tri2), int32 [n_graphs * n].  Given ``hist`` / ``totals`` are cleared first,
    or added to with ``accumulate``.  No host synchronisation."""
    if n_graphs < 1 or n < 1:
        raise ValueError(f"graph_stats: expected n_graphs >= 1 and n >= 1, got {n_graphs} and {n}")
    rows = n_graphs * n
    # colidx may be empty (a generated graph without an edge): it is never read then
    for t, name, numel in ((rowptr, "rowptr", rows + 1), (colidx, "colidx", 0)):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and t.numel() >= numel):
            raise ValueError(f"graph_stats {name}: expected a contiguous int32 device tensor of >= {numel} elements")
    ldc = sd = 0
    len_scale = 0.0
    if coords is not None:
        if not (coords.is_cuda and coords.dtype == torch.float32 and coords.dim() == 2
                and coords.shape[0] == rows and 1 <= coords.shape[1] <= 3
                and (coords.shape[1] == 1 or coords.stride(1) == 1)):
            raise ValueError(f"graph_stats coords: expected a float32 device tensor [{rows}, 1..3] with unit "
                             "column stride")
        if max_len is None or not (0.0 < float(max_len) < float("inf")):
            raise ValueError(f"graph_stats: coords need a finite max_len > 0, got {max_len!r}")
        sd = coords.shape[1]
        ldc = coords.stride(0) if rows > 1 else max(sd, coords.stride(0))
        len_scale = 256.0 / float(max_len)
    elif max_len is not None:
        raise ValueError("graph_stats: max_len without coords")
    if (hist is None) != (totals is None):
        raise ValueError("graph_stats: pass both hist and totals or neither")
    dev = rowptr.device
    if hist is None:
        if accumulate:
            raise ValueError("graph_stats: accumulate needs hist and totals")
        hist = torch.empty(n_graphs, 3, 256, dtype=torch.int64, device=dev)
        totals = torch.empty(n_graphs, 4, dtype=torch.int64, device=dev)
    for t, name, shape in ((hist, "hist", (n_graphs, 3, 256)), (totals, "totals", (n_graphs, 4))):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int64 and tuple(t.shape) == shape):
            raise ValueError(f"graph_stats {name}: expected a contiguous int64 device tensor {list(shape)}")
    deg = tri2 = None
    if per_node:
        deg = torch.empty(rows, dtype=torch.int32, device=dev)
        tri2 = torch.empty(rows, dtype=torch.int32, device=dev)
    L = _lib.lib()
    wsb = L.snd_graph_stats_workspace(n_graphs, n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
    _lib.check(L.snd_graph_stats(_P(rowptr), _P(colidx), n_graphs, n, _P(coords), ldc, sd, len_scale,
                                 _P(deg), _P(tri2), _P(hist), _P(totals), int(bool(accumulate)), _P(ws), wsb,
                                 _lib.stream_ptr()), "snd_graph_stats")
    return (hist, totals, deg, tri2) if per_node else (hist, totals)


def graph_paths(rowptr, colidx, n_graphs, n, coords=None, detour_scale=None, src_step=1, hist=None, totals=None,
                per_node=False, per_source=False):
    """Weak components, BFS hop distances and the detour of the shortest route over the
    straight line of a block-diagonal CSR (snd_graph_paths), nothing read back.

    rowptr / colidx: int32 device tensors as ``DeviceBatch`` holds and ``zzt_edges`` returns
    them (entries outside a row's graph block and self loops are ignored, duplicates change
    nothing; arcs are followed row -> column).  The sources of a graph are its local nodes 0,
    src_step, 2 src_step, ...  coords: float32 device tensor [n_graphs * n, sd] with unit
    column stride, 1 <= sd <= 3, or None (no routes, no detour histogram); ``detour_scale`` is
    the number of bins per unit of route / straight line - 1 (the last of the 256 bins collects
    larger detours) and is required with coords.
    Returns (hist, totals): int64 [n_graphs, 2, 256] (hops, detour) and [n_graphs, 6] = {weak
    components, size of the largest, sources, reachable ordered pairs, sum of hops, largest
    hop count} (metrics.PathStats turns them into mean path length, efficiency, MMD ...); with
    ``per_node`` also comp, int32 [n_graphs * n] (the smallest local id of the node's weak
    component); with ``per_source`` also (hops, route): int32 and float32 [n_graphs * n_src, n],
    -1 / inf where unreachable, route None without coords.  Given ``hist`` / ``totals`` are
    cleared first.  No host synchronisation."""
    if n_graphs < 1 or n < 1:
        raise ValueError(f"graph_paths: expected n_graphs >= 1 and n >= 1, got {n_graphs} and {n}")
    if src_step < 1:
        raise ValueError(f"graph_paths: expected src_step >= 1, got {src_step}")
    rows = n_graphs * n
    # colidx may be empty (a generated graph without an edge): it is never read then
    for t, name, numel in ((rowptr, "rowptr", rows + 1), (colidx, "colidx", 0)):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and t.numel() >= numel):
            raise ValueError(f"graph_paths {name}: expected a contiguous int32 device tensor of >= {numel} elements")
    ldc = sd = 0
    scale = 0.0
    if coords is not None:
        if not (coords.is_cuda and coords.dtype == torch.float32 and coords.dim() == 2
                and coords.shape[0] == rows and 1 <= coords.shape[1] <= 3
                and (coords.shape[1] == 1 or coords.stride(1) == 1)):
            raise ValueError(f"graph_paths coords: expected a float32 device tensor [{rows}, 1..3] with unit "
                             "column stride")
        if detour_scale is None or not (0.0 < float(detour_scale) < float("inf")):
            raise ValueError(f"graph_paths: coords need a finite detour_scale > 0, got {detour_scale!r}")
        sd = coords.shape[1]
        ldc = coords.stride(0) if rows > 1 else max(sd, coords.stride(0))
        scale = float(detour_scale)
    elif detour_scale is not None:
        raise ValueError("graph_paths: detour_scale without coords")
    if (hist is None) != (totals is None):
        raise ValueError("graph_paths: pass both hist and totals or neither")
    dev = rowptr.device
    if hist is None:
        hist = torch.empty(n_graphs, 2, 256, dtype=torch.int64, device=dev)
        totals = torch.empty(n_graphs, 6, dtype=torch.int64, device=dev)
    for t, name, shape in ((hist, "hist", (n_graphs, 2, 256)), (totals, "totals", (n_graphs, 6))):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int64 and tuple(t.shape) == shape):
            raise ValueError(f"graph_paths {name}: expected a contiguous int64 device tensor {list(shape)}")
    n_src = (n + src_step - 1) // src_step
    comp = torch.empty(rows, dtype=torch.int32, device=dev) if per_node else None
    hops = route = None
    if per_source:
        hops = torch.empty(n_graphs * n_src, n, dtype=torch.int32, device=dev)
        if coords is not None:
            route = torch.empty(n_graphs * n_src, n, dtype=torch.float32, device=dev)
    L = _lib.lib()
    cap = colidx.numel()
    wsb = L.snd_graph_paths_workspace(n_graphs, n, cap, int(coords is not None))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
    _lib.check(L.snd_graph_paths(_P(rowptr), _P(colidx) if cap else 0, cap, n_graphs, n, _P(coords), ldc, sd, scale,
                                 int(src_step), _P(comp), _P(hops), _P(route), _P(hist), _P(totals), _P(ws), wsb,
                                 _lib.stream_ptr()), "snd_graph_paths")
    out = (hist, totals)
    if per_node:
        out += (comp,)
    if per_source:
        out += (hops, route)
    return out


def graph_motifs(rowptr, colidx, n_graphs, n, work_cap=None):
    """Graphlet census of a block-diagonal CSR (snd_graph_motifs), nothing read back.

    rowptr / colidx: int32 device tensors as ``DeviceBatch`` holds and ``zzt_edges`` /
    ``dense_to_csr`` return them (entries outside a row's graph block and self loops are
    ignored).  The graph that is counted has {i, j} as an edge iff both arcs are present; a
    one-way arc is no edge.  Returns (census, work): int64 device tensors [n_graphs, 10] =
    {E, P2, T, P3, S3, C4, TT, D, K4 induced subgraph counts, one-way arcs} and [n_graphs], the
    bound on the column ids the counting reads per graph (the header has the formula).  A graph
    with work > ``work_cap`` (default MOTIFS_WORK_CAP) is not counted: its census row is -1.
    ``metrics.MotifStats`` turns the census into orbit vectors and their MMD.  No host
    synchronisation."""
    if n_graphs < 1 or n < 1:
        raise ValueError(f"graph_motifs: expected n_graphs >= 1 and n >= 1, got {n_graphs} and {n}")
    if n > MOTIFS_MAX_N:
        raise ValueError(f"graph_motifs: n = {n} > {MOTIFS_MAX_N}")
    work_cap = MOTIFS_WORK_CAP if work_cap is None else int(work_cap)
    if work_cap < 0:
        raise ValueError(f"graph_motifs: expected work_cap >= 0, got {work_cap}")
    rows = n_graphs * n
    # colidx may be empty (a generated graph without an edge): it is never read then
    for t, name, numel in ((rowptr, "rowptr", rows + 1), (colidx, "colidx", 0)):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and t.numel() >= numel):
            raise ValueError(f"graph_motifs {name}: expected a contiguous int32 device tensor of >= {numel} elements")
    dev = rowptr.device
    census = torch.empty(n_graphs, 10, dtype=torch.int64, device=dev)
    work = torch.empty(n_graphs, dtype=torch.int64, device=dev)
    L = _lib.lib()
    cap = colidx.numel()
    wsb = L.snd_graph_motifs_workspace(n_graphs, n, cap)
    if wsb == 0:
        raise _lib.SNDError(f"snd_graph_motifs_workspace: bad shape n_graphs={n_graphs} n={n}")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.snd_graph_motifs(_P(rowptr), _P(colidx) if cap else 0, cap, n_graphs, n, work_cap, _P(census),
                                  _P(work), _P(ws), wsb, _lib.stream_ptr()), "snd_graph_motifs")
    return census, work


def graph_spectrum(rowptr, colidx, n_graphs, n, n_moments=128, n_probes=None, seed=0, force_global=False):
    """Chebyshev moments of the spectral density of the normalised Laplacian of every graph of
    a block-diagonal CSR (snd_graph_spectrum), nothing read back.

    rowptr / colidx: int32 device tensors as ``DeviceBatch`` holds and ``zzt_edges`` /
    ``dense_to_csr`` return them; the graph is ``graph_motifs``' ({i, j} an edge iff both arcs
    are present; out-of-block entries and self loops ignored).  ``n_probes=None``: exact traces
    (0 probes: the n unit vectors) for n <= SPECTRUM_EXACT_MAX_N, SPECTRUM_PROBES Rademacher
    probes above; ``seed`` keys their Philox stream.  ``force_global`` takes the per-step
    kernels at n <= 64 too (the LDS path's counterpart in tests and timing).  Returns
    (moments, info): float64 [n_graphs, n_moments] = tr T_k(L - I) and int64 [n_graphs, 4] =
    {edges, isolated nodes, one-way arcs, probes used}.  ``metrics.SpectrumStats`` rebuilds the
    eigenvalue histogram from them.  No host synchronisation."""
    if n_graphs < 1 or n < 1:
        raise ValueError(f"graph_spectrum: expected n_graphs >= 1 and n >= 1, got {n_graphs} and {n}")
    if n > SPECTRUM_MAX_N:
        raise ValueError(f"graph_spectrum: n = {n} > {SPECTRUM_MAX_N}")
    if not 2 <= n_moments <= SPECTRUM_MAX_MOMENTS:
        raise ValueError(f"graph_spectrum: expected 2 <= n_moments <= {SPECTRUM_MAX_MOMENTS}, got {n_moments}")
    if n_probes is None:
        n_probes = 0 if n <= SPECTRUM_EXACT_MAX_N else SPECTRUM_PROBES
    n_probes, seed = int(n_probes), int(seed)
    if n_probes < 0:
        raise ValueError(f"graph_spectrum: expected n_probes >= 0, got {n_probes}")
    if not 0 <= seed < (1 << 64):
        raise ValueError(f"graph_spectrum: expected a 64-bit seed, got {seed}")
    rows = n_graphs * n
    # colidx may be empty (a generated graph without an edge): it is never read then
    for t, name, numel in ((rowptr, "rowptr", rows + 1), (colidx, "colidx", 0)):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and t.numel() >= numel):
            raise ValueError(f"graph_spectrum {name}: expected a contiguous int32 device tensor of >= {numel} elements")
    dev = rowptr.device
    moments = torch.empty(n_graphs, n_moments, dtype=torch.float64, device=dev)
    info = torch.empty(n_graphs, 4, dtype=torch.int64, device=dev)
    L = _lib.lib()
    cap = colidx.numel()
    wsb = L.snd_graph_spectrum_workspace(n_graphs, n, cap)
    if wsb == 0:
        raise _lib.SNDError(f"snd_graph_spectrum_workspace: bad shape n_graphs={n_graphs} n={n}")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.snd_graph_spectrum(_P(rowptr), _P(colidx) if cap else 0, cap, n_graphs, n, n_moments, n_probes, seed,
                                    1 if force_global else 0, _P(moments), _P(info), _P(ws), wsb, _lib.stream_ptr()),
               "snd_graph_spectrum")
    return moments, info


def graph_crossings(rowptr, colidx, n_graphs, n, coords, work_cap=None, per_edge=False):
    """Edge crossings of a block-diagonal CSR drawn at ``coords`` (snd_graph_crossings), nothing
    read back.

    rowptr / colidx: int32 device tensors as ``DeviceBatch`` holds and ``zzt_edges`` /
    ``dense_to_csr`` return them; the graph is ``graph_motifs``' ({i, j} an edge iff both arcs
    are present; out-of-block entries and self loops ignored).  coords: float32 device tensor
    [n_graphs * n, >= 2] with unit column stride; columns 0 and 1 are read.  Two edges cross iff
    they share no endpoint, their boxes overlap and they straddle each other strictly (the
    header has the predicate: touching and collinear overlap are no crossings).  Returns
    (counts, hist, work[, cross_out]): int64 device tensors [n_graphs, 7] = {E, X crossing
    pairs, crossed edges, independent pairs, one-way arcs, zero-length edges, largest count of
    one edge}, [n_graphs, 3, 256] = {edges by crossing count, edges by direction folded to
    [0, pi), crossing pairs by acute angle} and [n_graphs] = E (E - 1) / 2; with ``per_edge``
    also int32 [colidx.numel()]: c_e at the entry (row a, column b > a) of every edge, 0 at the
    other entries below rowptr[-1].  A graph with work > ``work_cap`` (default
    CROSSINGS_WORK_CAP) is not counted: its counts row and cross_out entries are -1, its hist
    rows 0.  ``metrics.CrossingStats`` turns counts and hist into planarity, crossing ratio and
    orientation entropy.  No host synchronisation."""
    if n_graphs < 1 or n < 1:
        raise ValueError(f"graph_crossings: expected n_graphs >= 1 and n >= 1, got {n_graphs} and {n}")
    if n > CROSSINGS_MAX_N:
        raise ValueError(f"graph_crossings: n = {n} > {CROSSINGS_MAX_N}")
    work_cap = CROSSINGS_WORK_CAP if work_cap is None else int(work_cap)
    if work_cap < 0:
        raise ValueError(f"graph_crossings: expected work_cap >= 0, got {work_cap}")
    rows = n_graphs * n
    # colidx may be empty (a generated graph without an edge): it is never read then
    for t, name, numel in ((rowptr, "rowptr", rows + 1), (colidx, "colidx", 0)):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and t.numel() >= numel):
            raise ValueError(f"graph_crossings {name}: expected a contiguous int32 device tensor of >= {numel} "
                             "elements")
    if not (coords is not None and coords.is_cuda and coords.dtype == torch.float32 and coords.dim() == 2
            and coords.shape[0] == rows and coords.shape[1] >= 2 and coords.stride(1) == 1):
        raise ValueError(f"graph_crossings coords: expected a float32 device tensor [{rows}, >= 2] with unit "
                         "column stride")
    ldc = coords.stride(0) if rows > 1 else max(coords.shape[1], coords.stride(0))
    dev = rowptr.device
    counts = torch.empty(n_graphs, 7, dtype=torch.int64, device=dev)
    hist = torch.empty(n_graphs, 3, 256, dtype=torch.int64, device=dev)
    work = torch.empty(n_graphs, dtype=torch.int64, device=dev)
    cap = colidx.numel()
    cross = torch.zeros(cap, dtype=torch.int32, device=dev) if per_edge else None
    L = _lib.lib()
    wsb = L.snd_graph_crossings_workspace(n_graphs, n, cap)
    if wsb == 0:
        raise _lib.SNDError(f"snd_graph_crossings_workspace: bad shape n_graphs={n_graphs} n={n}")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.snd_graph_crossings(_P(rowptr), _P(colidx) if cap else 0, cap, n_graphs, n, _P(coords), ldc,
                                     work_cap, _P(counts), _P(hist), _P(work), _P(cross), _P(ws), wsb,
                                     _lib.stream_ptr()), "snd_graph_crossings")
    return (counts, hist, work, cross) if per_edge else (counts, hist, work)


def latent_mi(z, factors, n_bins=20, factor_bins=None, want_joint=False):
    """Mutual information between every latent dimension and every generative factor
    (snd_latent_mi), from joint histograms counted on chip; nothing is read back.

    z: float32 device tensor [rows, L] (one row per graph, the encoder means), factors:
    float32 device tensor [rows, K] on the same device (integer-coded factors as floats),
    both with unit column stride; 1 <= L <= 65536, 1 <= K <= 64.  Every column is cut into
    equal-width bins between its minimum and maximum: ``n_bins`` for a latent column,
    ``factor_bins`` (default ``n_bins``) for a factor column, 1 to 32 each; k equally spaced
    factor levels fill k bins at factor_bins = k.  Returns float64 device tensors (mi [L, K]
    in nats, hz [L], hf [K]) (metrics.LatentMI turns them into MIG, avgMI, modularity ...);
    with ``want_joint`` also (joint, range): the int32 counts [L, K, n_bins, factor_bins] and
    the float32 [L + K, 2] {lo, hi} of the columns, latent ones first.  The counts are exact
    and the result is bitwise repeatable.  No host synchronisation."""
    for t, name in ((z, "z"), (factors, "factors")):
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] >= 1 and t.shape[1] >= 1
                and (t.shape[1] == 1 or t.stride(1) == 1)):
            raise ValueError(f"latent_mi {name}: expected a float32 device tensor [rows, columns] with unit "
                             "column stride")
    rows, n_lat = z.shape
    n_fac = factors.shape[1]
    if factors.shape[0] != rows or factors.device != z.device:
        raise ValueError(f"latent_mi: z has {rows} rows on {z.device}, factors {factors.shape[0]} on {factors.device}")
    if n_lat > 65536 or n_fac > 64:
        raise ValueError(f"latent_mi: at most 65536 latent and 64 factor columns, got {n_lat} and {n_fac}")
    nbz = n_bins
    nbf = n_bins if factor_bins is None else factor_bins
    for nb, name in ((nbz, "n_bins"), (nbf, "factor_bins")):
        if int(nb) != nb or not 1 <= nb <= 32:
            raise ValueError(f"latent_mi: {name} must be an integer in [1, 32], got {nb!r}")
    nbz, nbf = int(nbz), int(nbf)
    ldz = z.stride(0) if rows > 1 else max(n_lat, z.stride(0))
    ldf = factors.stride(0) if rows > 1 else max(n_fac, factors.stride(0))
    if ldz < n_lat or ldf < n_fac:
        raise ValueError("latent_mi: rows overlap (row stride below the number of columns)")
    dev = z.device
    out = torch.empty(n_lat * n_fac + n_lat + n_fac, dtype=torch.float64, device=dev)
    mi, hz, hf = out[:n_lat * n_fac].view(n_lat, n_fac), out[n_lat * n_fac:n_lat * n_fac + n_lat], out[-n_fac:]
    joint = rng = None
    if want_joint:
        joint = torch.empty(n_lat, n_fac, nbz, nbf, dtype=torch.int32, device=dev)
        rng = torch.empty(n_lat + n_fac, 2, dtype=torch.float32, device=dev)
    L = _lib.lib()
    wsb = L.snd_latent_mi_workspace(rows, n_lat, n_fac, nbz, nbf)
    if wsb == 0:
        raise _lib.SNDError(f"snd_latent_mi_workspace: bad shape rows={rows} L={n_lat} K={n_fac} bins {nbz}, {nbf}")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.snd_latent_mi(_P(z), ldz, _P(factors), ldf, rows, n_lat, n_fac, nbz, nbf, _P(mi), _P(hz), _P(hf),
                               _P(rng), _P(joint), _P(ws), wsb, _lib.stream_ptr()), "snd_latent_mi")
    return (mi, hz, hf, joint, rng) if want_joint else (mi, hz, hf)


def dense_to_csr(adj):
    """Reference dense adj_truth [B,N,N] -> (rowptr, colidx) on the device."""
    b, n, _ = adj.shape
    L = _lib.lib()
    rowptr = torch.empty(b * n + 1, dtype=torch.int32, device=adj.device)
    nnz = torch.zeros(1, dtype=torch.int32, device=adj.device)
    ws = torch.empty(L.snd_dense_to_csr_workspace(b, n), dtype=torch.uint8, device=adj.device)
    _lib.check(L.snd_dense_to_csr(_P(adj), b, n, _P(rowptr), 0, 0, _P(nnz), _P(ws), ws.numel(),
                                  _lib.stream_ptr()), "snd_dense_to_csr")
    total = int(rowptr[-1].item())
    colidx = torch.empty(max(total, 1), dtype=torch.int32, device=adj.device)
    _lib.check(L.snd_dense_to_csr(_P(adj), b, n, _P(rowptr), _P(colidx), total, _P(nnz), _P(ws),
                                  ws.numel(), _lib.stream_ptr()), "snd_dense_to_csr")
    return rowptr, colidx[:total]
