"""Time the fused edge-extraction op (snd_zzt_edges) against the route it replaces.

Two shapes: C2 (B = 8, N = 4096, d = 64) and C5 (B = 1, N = 16384, d = 128).  Per shape, in
one process and alternating per iteration:

(a) the gate, at threshold 0 on the model's decoder input J:
  * new: ``layers.zzt_edges(J, B, N)`` with ``capacity=None`` (the sizing call, the one host
    read, the exact allocation, the op again), and the preallocated one-call form;
  * old: how a generated graph became a CSR before -- ``generate(want_adj=True)`` minus
    ``generate(want_adj=False)`` (the dense uint8 adjacency through gen_adj_kernel), plus
    uint8 -> float32, plus ``layers.dense_to_csr``.
  The two CSRs must be identical, and the new route's median (``capacity=None``) must not be
  above the old route's median.

(b) reported, not gated: the op alone (one call, preallocated) at the sparse threshold, the
  bin edge of ``evaluate()``'s histogram whose predicted-edge count is closest to the batch's
  true nnz.  Bytes written, and 2 B N^2 d x 2 FLOP (both MFMA passes) over the median as a
  fraction of the 155 TF/s measured fp32-matrix rate; and the sizing call alone (count and
  scan: one MFMA pass).

HIP events around each call, warm-up iterations dropped, medians reported.

    python tools/edges_timing.py --out profiles/edges_timing.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

FP32_MATRIX_TFS = 155.0
SHAPES = (("C2", "C2", 8), ("C5", "C5", 1))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out          # microseconds


def stats(v):
    v = sorted(v)
    return {"median_us": statistics.median(v), "min_us": v[0], "max_us": v[-1], "n": len(v)}


def sparse_threshold(ec, nnz):
    """The bin edge at which "edge iff L >= edge" predicts the count closest to nnz."""
    from snd_vae_amd.metrics import BINS, bin_edge
    per_bin = ec.hist.sum(axis=(0, 1))
    predicted = np.cumsum(per_bin[::-1])[::-1]               # pairs in bins >= b
    b = max(1, int(np.argmin(np.abs(predicted[1:] - nnz))) + 1)
    return bin_edge(b), int(predicted[b]), BINS


def measure(name, preset, B, dtype, iters, warmup):
    from snd_vae_amd import _lib, layers
    from snd_vae_amd.config import PRESETS
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    cfg = PRESETS[preset]
    n, d = cfg.n_nodes, cfg.node_h_size
    db = DeviceBatch(synthetic_batch(cfg, B, seed=3), locality=False)
    model = SGCNModelVAE(cfg, B, dtype=dtype)
    ec = model.evaluate(db, mode="mean")                       # leaves J of the timed op
    J = model.joint_h
    _, _, total = layers.zzt_edges(J, B, n)
    t = {"new": [], "new_one_call": [], "gen_adj": [], "gen_noadj": [], "to_f32": [], "to_csr": [], "old": []}
    new = old = None
    for it in range(warmup + iters):
        tn, new = timed(lambda: layers.zzt_edges(J, B, n))
        t1, one = timed(lambda: layers.zzt_edges(J, B, n, capacity=total))
        ga, out = timed(lambda: model.generate(db, mode="mean", want_adj=True))
        gn, _ = timed(lambda: model.generate(db, mode="mean", want_adj=False))
        tf, adj = timed(lambda: out["generated_adj"].float())
        tc, old = timed(lambda: layers.dense_to_csr(adj))
        del out, adj
        if it >= warmup:
            for k, v in (("new", tn), ("new_one_call", t1), ("gen_adj", ga), ("gen_noadj", gn), ("to_f32", tf),
                         ("to_csr", tc), ("old", ga - gn + tf + tc)):
                t[k].append(v)
    same = bool(torch.equal(new[0], old[0]) and torch.equal(new[1], old[1]) and new[2] == total
                and torch.equal(one[0], old[0]) and torch.equal(one[1], old[1]) and int(one[2].item()) == total)
    del new, old, one
    # (b) the op alone at the sparse threshold
    thr, predicted, _ = sparse_threshold(ec, db.nnz)
    _, _, sparse_total = layers.zzt_edges(J, B, n, thr, True)
    assert sparse_total == predicted, (sparse_total, predicted)      # the histogram's own count
    ts = [timed(lambda: layers.zzt_edges(J, B, n, thr, True, capacity=sparse_total))[0]
          for _ in range(warmup + iters)][warmup:]
    nnz_dev = torch.empty(1, dtype=torch.int64, device="cuda")     # the sizing call alone: one MFMA pass
    rp_dev = torch.empty(B * n + 1, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    ws = torch.empty(L.snd_zzt_edges_workspace(B, n, d), dtype=torch.uint8, device="cuda")
    sizing = lambda: _lib.check(L.snd_zzt_edges(J.data_ptr(), J.stride(0), B, n, d, thr, 1, rp_dev.data_ptr(), None,
                                                0, nnz_dev.data_ptr(), ws.data_ptr(), ws.numel(),
                                                _lib.stream_ptr()), "snd_zzt_edges")
    tz = [timed(sizing)[0] for _ in range(warmup + iters)][warmup:]
    flops = 2.0 * B * n * n * d * 2
    new_med, one_med, old_med = (statistics.median(t[k]) for k in ("new", "new_one_call", "old"))
    sp_med = statistics.median(ts)
    rate = lambda us: flops / (us * 1e-6) / 1e12
    csr_bytes = lambda nnz: 4 * (B * n + 1) + 4 * nnz + 8
    return {"shape": {"name": name, "B": B, "N": n, "d": d, "engine": dtype},
            "flops_two_passes": flops, "pairs": B * n * (n - 1),
            "gate_threshold_0": {
                "nnz": total, "csr_identical": same,
                "new_capacity_none": dict(stats(t["new"]), bytes_written=csr_bytes(total)),
                "new_one_call": dict(stats(t["new_one_call"]), bytes_written=csr_bytes(total),
                                     tf_per_s=rate(one_med), fraction_of_fp32_matrix_rate=rate(one_med) / FP32_MATRIX_TFS),
                "old_route": dict(stats(t["old"]), generate_want_adj=stats(t["gen_adj"]),
                                  generate_no_adj=stats(t["gen_noadj"]), uint8_to_float32=stats(t["to_f32"]),
                                  dense_to_csr=stats(t["to_csr"]),
                                  bytes_written=B * n * n * 5 + csr_bytes(total)),
                "speedup": old_med / new_med, "speedup_one_call": old_med / one_med},
            "sparse_threshold": {
                "threshold": thr, "inclusive": True, "nnz": sparse_total, "batch_nnz": db.nnz,
                "one_call": dict(stats(ts), bytes_written=csr_bytes(sparse_total), tf_per_s=rate(sp_med),
                                 fraction_of_fp32_matrix_rate=rate(sp_med) / FP32_MATRIX_TFS),
                "sizing_call_count_and_scan": dict(stats(tz), tf_per_s=rate(statistics.median(tz)) / 2)},
            "gate_new_not_slower": bool(same and new_med <= old_med)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/edges_timing.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", help="engine of the model whose J is thresholded")
    ap.add_argument("--shapes", default="C2,C5")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("edges_timing needs a ROCm GPU: a time taken elsewhere says nothing")
    want = a.shapes.split(",")
    res = {"device": torch.cuda.get_device_name(0), "fp32_matrix_rate_tf_per_s": FP32_MATRIX_TFS,
           "method": "HIP events per call, routes alternated per iteration in one process, "
                     f"{a.warmup} warm-up + {a.iters} timed iterations, medians; old route = "
                     "generate(want_adj=True) - generate(want_adj=False) + uint8 -> float32 + dense_to_csr; "
                     "the rate counts both MFMA passes (2 B N^2 d x 2 FLOP)",
           "results": []}
    for name, preset, B in SHAPES:
        if name in want:
            r = measure(name, preset, B, a.dtype, a.iters, a.warmup)
            res["results"].append(r)
            g = r["gate_threshold_0"]
            print(json.dumps({"shape": r["shape"], "gate_new_not_slower": r["gate_new_not_slower"],
                              "csr_identical": g["csr_identical"], "new_us": g["new_capacity_none"]["median_us"],
                              "one_call_us": g["new_one_call"]["median_us"], "old_us": g["old_route"]["median_us"],
                              "sparse_us": r["sparse_threshold"]["one_call"]["median_us"],
                              "sparse_nnz": r["sparse_threshold"]["nnz"]}), flush=True)
    res["gate_new_not_slower"] = all(r["gate_new_not_slower"] for r in res["results"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out, "gate", res["gate_new_not_slower"])


if __name__ == "__main__":
    main()
