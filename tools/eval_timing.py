"""Time the fused evaluation op (snd_zzt_eval) against the route it replaces.

Two shapes: C2 (B = 8, N = 4096, d = 64) and C5 (B = 1, N = 16384, d = 128).  Per shape, in
one process and alternating per iteration:

* new: ``layers.zzt_eval`` on the model's decoder input J into preallocated counters;
* old: what answered "how good is the predicted adjacency" before --
  ``generate(want_adj=True)`` minus ``generate(want_adj=False)`` (the dense uint8 adjacency
  through gen_adj_kernel) plus ``adj_accuracy`` on it.

HIP events around each call, warm-up iterations dropped, medians reported.  The rate is
2 B N^2 d over the op's median, as a fraction of the 155 TF/s measured fp32-matrix rate.
The gate: the op's median is not above the old route's median.  The two routes must also
agree at the timed size (TP + FP = generated ones, accuracy = adj_accuracy).

    python tools/eval_timing.py --out profiles/eval_timing.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

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


def measure(name, preset, B, dtype, iters, warmup):
    from snd_vae_amd import layers
    from snd_vae_amd.config import PRESETS
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.metrics import EdgeCounts
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE, adj_accuracy
    cfg = PRESETS[preset]
    n, d = cfg.n_nodes, cfg.node_h_size
    db = DeviceBatch(synthetic_batch(cfg, B, seed=3), locality=False)
    model = SGCNModelVAE(cfg, B, dtype=dtype)
    hist = torch.zeros(B, 2, 2048, dtype=torch.int64, device="cuda")
    counts = torch.zeros(B, 4, dtype=torch.int64, device="cuda")
    model.generate(db, mode="mean", want_adj=False)            # J of the timed op
    J = model.joint_h
    t = {"new": [], "gen_adj": [], "gen_noadj": [], "acc": [], "old": []}
    acc = gen = None
    for it in range(warmup + iters):
        new, _ = timed(lambda: layers.zzt_eval(J, db.rowptr, db.colidx, B, n, hist, counts))
        ga, out = timed(lambda: model.generate(db, mode="mean", want_adj=True))
        gn, _ = timed(lambda: model.generate(db, mode="mean", want_adj=False))
        gen = out["generated_adj"]
        ac, acc = timed(lambda: adj_accuracy(gen, db))
        if it >= warmup:
            for k, v in (("new", new), ("gen_adj", ga), ("gen_noadj", gn), ("acc", ac), ("old", ga - gn + ac)):
                t[k].append(v)
    ec = EdgeCounts(hist, counts)
    ones = int(gen.sum(dtype=torch.int64).item())
    assert ec.tp + ec.fp == ones, (ec.tp + ec.fp, ones)
    assert ec.accuracy == acc, (ec.accuracy, acc)
    # the op alone on Gaussian z of three scales: logits within a few bins of 0, spread over
    # hundreds of bins, and mostly in the two end bins (its time depends on the clustering)
    other = {}
    h2, c2 = torch.empty_like(hist), torch.empty_like(counts)
    gen_ = torch.Generator(device="cuda").manual_seed(5)
    for label, scale in (("clustered_std_0.02", 0.02), ("spread_std_0.35", 0.35), ("saturated_std_3", 3.0)):
        zs = scale * torch.randn(B * n, d, device="cuda", generator=gen_)
        ts = [timed(lambda: layers.zzt_eval(zs, db.rowptr, db.colidx, B, n, h2, c2))[0]
              for _ in range(warmup + iters)][warmup:]
        e2 = EdgeCounts(h2.clone(), c2.clone())
        other[label] = dict(stats(ts), occupied_bins=int((e2.hist.sum(axis=(0, 1)) > 0).sum()),
                            tf_per_s=2.0 * B * n * n * d / (statistics.median(ts) * 1e-6) / 1e12)
    flops = 2.0 * B * n * n * d
    new_med, old_med = statistics.median(t["new"]), statistics.median(t["old"])
    tfs = flops / (new_med * 1e-6) / 1e12
    return {"shape": {"name": name, "B": B, "N": n, "d": d, "engine": dtype}, "flops": flops,
            "new_op": dict(stats(t["new"]), tf_per_s=tfs, fraction_of_fp32_matrix_rate=tfs / FP32_MATRIX_TFS,
                           bytes_written=int(hist.numel() + counts.numel()) * 8),
            "old_route": dict(stats(t["old"]), generate_want_adj=stats(t["gen_adj"]),
                              generate_no_adj=stats(t["gen_noadj"]), adj_accuracy=stats(t["acc"]),
                              tf_per_s=flops / (old_med * 1e-6) / 1e12, bytes_written=B * n * n),
            "new_op_other_logits": other,
            # how clustered the timed logits are (clustered logits contend for few LDS cells)
            "logit_spread": {"occupied_bins": int((ec.hist.sum(axis=(0, 1)) > 0).sum()),
                             "largest_bin_share": float(ec.hist.sum(axis=(0, 1)).max() / ec.hist.sum())},
            "agreement": {"tp_plus_fp": ec.tp + ec.fp, "generated_ones": ones, "accuracy": acc,
                          "roc_auc": ec.roc_auc, "average_precision": ec.average_precision},
            "speedup": old_med / new_med, "gate_new_not_slower": bool(new_med <= old_med)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/eval_timing.json")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", help="engine of the model whose J is evaluated")
    ap.add_argument("--shapes", default="C2,C5")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_timing needs a ROCm GPU: a time taken elsewhere says nothing")
    want = a.shapes.split(",")
    res = {"device": torch.cuda.get_device_name(0), "fp32_matrix_rate_tf_per_s": FP32_MATRIX_TFS,
           "method": "HIP events per call, routes alternated per iteration in one process, "
                     f"{a.warmup} warm-up + {a.iters} timed iterations, medians; "
                     "old route = generate(want_adj=True) - generate(want_adj=False) + adj_accuracy",
           "results": []}
    for name, preset, B in SHAPES:
        if name in want:
            r = measure(name, preset, B, a.dtype, a.iters, a.warmup)
            res["results"].append(r)
            print(json.dumps({k: r[k] for k in ("shape", "speedup", "gate_new_not_slower")}),
                  r["new_op"]["median_us"], r["old_route"]["median_us"], r["new_op"]["tf_per_s"], flush=True)
    res["gate_new_not_slower"] = all(r["gate_new_not_slower"] for r in res["results"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out, "gate", res["gate_new_not_slower"])


if __name__ == "__main__":
    main()
