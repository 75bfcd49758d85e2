"""Time the graph-statistics op (snd_graph_stats) beside the op that produces its input.

Two shapes: C2 (B = 8, N = 4096, d = 64) and C5 (B = 1, N = 16384, d = 128).  Per shape, in
one process and alternating per iteration:

  * edges:      the one-call, preallocated ``layers.zzt_edges`` at the sparse threshold of
                tools/edges_timing.py (the bin edge of ``evaluate()``'s histogram whose
                predicted count is closest to the batch's nnz);
  * generated:  ``layers.graph_stats`` on the CSR that call wrote and ``generated_spatial``;
  * batch:      ``layers.graph_stats`` on the batch's own CSR and ``spatial_truth``.

The gate: the statistics of the generated CSR take no longer (median) than the edge
extraction that produced it, both measured here -- statistics must not become the dominant
cost of generate -> stats.  Reported as measured, pass or fail, with wedges (sum_j deg(j)^2,
the column ids the walk tests) per second and the bytes the op requests.

Once, not gated: the dense regime, threshold 0 on the untrained J at C2, where nearly every
pair is an edge and sum deg^2 ~ B N^3.

HIP events around each call, warm-up iterations dropped, medians reported.

    python tools/gstats_timing.py --out profiles/gstats_timing.json
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

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
    from snd_vae_amd.metrics import bin_edge
    per_bin = ec.hist.sum(axis=(0, 1))
    predicted = np.cumsum(per_bin[::-1])[::-1]               # pairs in bins >= b
    b = max(1, int(np.argmin(np.abs(predicted[1:] - nnz))) + 1)
    return bin_edge(b), int(predicted[b])


def work(layers, rp, ci, B, n, sd):
    """Wedges and requested bytes of one call, from the op's own per-node degrees."""
    _, totals, deg, _ = layers.graph_stats(rp, ci, B, n, per_node=True)
    torch.cuda.synchronize()
    d = deg.cpu().numpy().astype(np.int64)
    entries = int(d.sum())
    wedges = int((d * d).sum())
    edges = int(totals[:, 3].sum().item())
    # the walk's column ids; two passes over the row's own entries; rowptr of the row and of
    # every neighbour; the coordinate rows of the row and of every column > row
    nbytes = 4 * wedges + 8 * entries + 8 * B * n + 8 * entries + 4 * sd * (B * n + edges)
    return {"entries": entries, "undirected_edges": edges, "max_degree": int(d.max()), "wedges": wedges,
            "bytes_read": nbytes}


def with_rates(s, w):
    sec = s["median_us"] * 1e-6
    return dict(s, **w, wedges_per_s=w["wedges"] / sec, bytes_read_per_s=w["bytes_read"] / sec)


def measure(name, preset, B, dtype, iters, warmup, dense):
    from snd_vae_amd import layers
    from snd_vae_amd.config import PRESETS
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    cfg = PRESETS[preset]
    n, d, sd = cfg.n_nodes, cfg.node_h_size, cfg.spatial_dim
    max_len = math.sqrt(sd)
    db = DeviceBatch(synthetic_batch(cfg, B, seed=3), locality=False)
    model = SGCNModelVAE(cfg, B, dtype=dtype)
    ec = model.evaluate(db, mode="mean")                       # leaves J and generated_spatial
    J, xy = model.joint_h, model.generated_spatial.clone()
    thr, predicted = sparse_threshold(ec, db.nnz)
    rp, ci, total = layers.zzt_edges(J, B, n, thr, True)
    assert total == predicted, (total, predicted)
    hist = torch.empty(B, 3, 256, dtype=torch.int64, device="cuda")
    totals = torch.empty(B, 4, dtype=torch.int64, device="cuda")
    gen = lambda: layers.graph_stats(rp, ci, B, n, xy, max_len, hist=hist, totals=totals)
    own = lambda: layers.graph_stats(db.rowptr, db.colidx, B, n, db.spatial_truth, max_len, hist=hist, totals=totals)
    t = {"edges": [], "generated": [], "batch": []}
    for it in range(warmup + iters):
        te, _ = timed(lambda: layers.zzt_edges(J, B, n, thr, True, capacity=total))
        tg, _ = timed(gen)
        tb, _ = timed(own)
        if it >= warmup:
            for k, v in (("edges", te), ("generated", tg), ("batch", tb)):
                t[k].append(v)
    gen()
    torch.cuda.synchronize()
    consistent = int(totals[:, 0].sum().item()) == total       # every entry counted once: no self loops
    e_med, g_med = statistics.median(t["edges"]), statistics.median(t["generated"])
    out = {"shape": {"name": name, "B": B, "N": n, "d": d, "spatial_dim": sd, "engine": dtype},
           "sparse_threshold": {"threshold": thr, "inclusive": True, "nnz": total, "batch_nnz": db.nnz},
           "zzt_edges_one_call": stats(t["edges"]),
           "graph_stats_generated": with_rates(stats(t["generated"]), work(layers, rp, ci, B, n, sd)),
           "graph_stats_batch": with_rates(stats(t["batch"]), work(layers, db.rowptr, db.colidx, B, n, sd)),
           "sum_deg_equals_nnz": consistent,
           "stats_over_edges": g_med / e_med,
           "gate_stats_not_slower_than_edges": bool(consistent and g_med <= e_med)}
    if dense:
        del rp, ci
        rp, ci, total0 = layers.zzt_edges(J, B, n, 0.0, False)
        us, _ = timed(lambda: layers.graph_stats(rp, ci, B, n, xy, max_len, hist=hist, totals=totals))
        w = work(layers, rp, ci, B, n, sd)
        out["dense_threshold_0"] = dict({"nnz": total0, "pairs": B * n * (n - 1), "one_call_us": us, "n": 1}, **w,
                                        wedges_per_s=w["wedges"] / (us * 1e-6), b_n_cubed=B * n ** 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/gstats_timing.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", help="engine of the model whose J is thresholded")
    ap.add_argument("--shapes", default="C2,C5")
    ap.add_argument("--no-dense", action="store_true", help="skip the dense-regime call at C2")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gstats_timing needs a ROCm GPU: a time taken elsewhere says nothing")
    want = a.shapes.split(",")
    res = {"device": torch.cuda.get_device_name(0),
           "method": "HIP events per call, routes alternated per iteration in one process, "
                     f"{a.warmup} warm-up + {a.iters} timed iterations, medians; the gate compares "
                     "graph_stats on the generated CSR with the one-call preallocated zzt_edges that "
                     "wrote it; wedges = sum_j deg(j)^2; bytes_read = requested bytes, not HBM traffic; "
                     "dense_threshold_0 is one call, not gated",
           "results": []}
    for name, preset, B in SHAPES:
        if name in want:
            r = measure(name, preset, B, a.dtype, a.iters, a.warmup, dense=(name == "C2" and not a.no_dense))
            res["results"].append(r)
            print(json.dumps({"shape": r["shape"], "gate": r["gate_stats_not_slower_than_edges"],
                              "edges_us": r["zzt_edges_one_call"]["median_us"],
                              "stats_generated_us": r["graph_stats_generated"]["median_us"],
                              "stats_batch_us": r["graph_stats_batch"]["median_us"],
                              "max_degree_generated": r["graph_stats_generated"]["max_degree"],
                              "dense_us": r.get("dense_threshold_0", {}).get("one_call_us")}), flush=True)
    res["gate_stats_not_slower_than_edges"] = all(r["gate_stats_not_slower_than_edges"] for r in res["results"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out, "gate", res["gate_stats_not_slower_than_edges"])


if __name__ == "__main__":
    main()
