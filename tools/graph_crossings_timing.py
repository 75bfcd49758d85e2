"""Time the edge-crossing op (snd_graph_crossings) beside the only other route to its numbers.

Shapes:

  * ref:    the reference's scale, N = 25, B = 1500 graphs;
  * C2:     the node-latent scale, N = 4096, B = 8 from ``data.synthetic_batch`` (the bench RGG);
  * chords: one graph of N = 2048 nodes at random points with 10^5 random edges: long edges whose
            boxes nearly all overlap, so nearly every pair reaches the double predicate and about
            a quarter cross.  The op alone; its pairs per second is the rate the default
            ``work_cap`` (``layers.CROSSINGS_WORK_CAP``) is derived from.

Per shape, in one process and alternating per iteration:

  * op:    ``layers.graph_crossings`` on the batch's own CSR and coordinates (HIP events around
           the call);
  * host:  the route without the op: read the CSR and the coordinates back (timed on its own),
           then the NumPy pair test of tests/graph_crossings_ref.py (wall clock).  At C2 the host
           leg runs on the first graph alone, chunked, three times (5e8 pairs take tens of
           seconds); its time is reported per graph and scaled by B for the ratio.

Medians with min-max; the counts of both routes must agree exactly.  No ratio is a gate: the
numbers are reported as measured.

    python tools/graph_crossings_timing.py --out profiles/graph_crossings_timing.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


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


def read_back(rowptr, colidx, coords):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rp, ci, xy = rowptr.cpu().numpy(), colidx.cpu().numpy(), coords.cpu().numpy()
    return (time.perf_counter() - t0) * 1e6, (rp, ci, xy)


_host_calls = [0]


def host_counts(rp, ci, xy, B, n, graphs=None):
    """counts [graphs, 7] by the NumPy reference; returns (microseconds, counts)."""
    import graph_crossings_ref as X
    t0 = time.perf_counter()
    if graphs is not None:                                       # the first ``graphs`` graphs only
        B = graphs
        rp, xy = rp[:B * n + 1], xy[:B * n]
    _host_calls[0] += 1
    c = X.Case(f"timing_{_host_calls[0]}", B, n, np.array(rp[:B * n + 1]), np.array(ci[:max(int(rp[B * n]), 1)]),
               np.array(xy[:, :2]))
    out = X.reference(c)
    X._ref_cache.clear()
    return (time.perf_counter() - t0) * 1e6, np.array(out["counts"])


def op_times(op, iters, warmup):
    t, out = [], None
    for it in range(warmup + iters):
        us, out = timed(op)
        if it >= warmup:
            t.append(us)
    torch.cuda.synchronize()
    return t, out


def measure(name, cfg, B, iters, warmup, host_iters, host_graphs):
    from snd_vae_amd import layers
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.model import DeviceBatch
    n = cfg.n_nodes
    db = DeviceBatch(synthetic_batch(cfg, B, seed=3), locality=False)
    xy = db.spatial_truth
    op = lambda: layers.graph_crossings(db.rowptr, db.colidx, B, n, xy, work_cap=1 << 62)
    t, outs = op_times(op, iters, warmup)
    cnt = outs[0].cpu().numpy()
    wk = outs[2].cpu().numpy()
    th = {"read_back": [], "host": []}
    host_cnt = None
    for _ in range(host_iters):
        timed(op)                                                # alternate with the op
        rb, arrays = read_back(db.rowptr, db.colidx, xy)
        hu, host_cnt = host_counts(*arrays, B, n, host_graphs)
        th["read_back"].append(rb)
        th["host"].append(hu)
    hg = B if host_graphs is None else host_graphs
    out = {"shape": {"name": name, "B": B, "N": n, "entries": int(db.nnz)},
           "counts_sum": dict(zip(("E", "X", "crossed", "independent", "one_way", "zero_length"),
                                  (int(x) for x in cnt[:, :6].sum(axis=0)))),
           "pairs": int(wk.sum()), "pairs_max": int(wk.max()), "skipped": int((cnt[:, 0] < 0).sum()),
           "planar_graphs": int((cnt[:, 1] == 0).sum()),
           "host_graphs": hg, "counts_agree_with_host": bool(np.array_equal(cnt[:hg], host_cnt)),
           "graph_crossings_op": stats(t),
           "host_read_back": stats(th["read_back"]), "host_numpy": stats(th["host"])}
    med = out["graph_crossings_op"]["median_us"]
    out["pairs_per_second"] = out["pairs"] / (med * 1e-6)
    host = out["host_numpy"]["median_us"] * (B / hg) + out["host_read_back"]["median_us"]
    out["host_over_op"] = host / med
    return out


def chords_rate(n, edges, iters, warmup):
    """The op alone on one graph of long random edges: pairs per second where nearly every pair
    reaches the double predicate."""
    from snd_vae_amd import layers
    rng = np.random.default_rng(7)
    p = rng.integers(0, n, (edges * 2, 2))
    p = p[p[:, 0] != p[:, 1]]
    p = np.unique(np.sort(p, axis=1), axis=0)[:edges]
    r = np.concatenate([p[:, 0], p[:, 1]])
    c = np.concatenate([p[:, 1], p[:, 0]])
    order = np.lexsort((c, r))
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rp[1:])
    rowptr = torch.from_numpy(rp.astype(np.int32)).cuda()
    colidx = torch.from_numpy(c[order].astype(np.int32)).cuda()
    xy = torch.from_numpy(rng.random((n, 2)).astype(np.float32)).cuda()
    op = lambda: layers.graph_crossings(rowptr, colidx, 1, n, xy, work_cap=1 << 62)
    t, outs = op_times(op, iters, warmup)
    cnt, wk = outs[0].cpu().numpy(), int(outs[2][0].item())
    res = {"n": n, "E": int(cnt[0, 0]), "X": int(cnt[0, 1]), "pairs": wk, "op": stats(t)}
    res["pairs_per_second"] = wk / (res["op"]["median_us"] * 1e-6)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/graph_crossings_timing.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--shapes", default="ref,C2")
    ap.add_argument("--chords", default="2048x100000", help="NxE of the rate graph, empty to skip")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("graph_crossings_timing needs a ROCm GPU: a time taken elsewhere says nothing")
    from snd_vae_amd import layers
    from snd_vae_amd.config import PRESETS, tscale
    want = a.shapes.split(",")
    runs = []
    if "ref" in want:
        runs.append(("ref", tscale(25, 16, mean_degree=4.0), 1500, a.host_iters, None))
    if "C2" in want:
        runs.append(("C2", PRESETS["C2"], 8, min(3, a.host_iters), 1))
    res = {"device": torch.cuda.get_device_name(0),
           "method": f"op: HIP events per call, {a.warmup} warm-up + {a.iters} timed iterations; host: wall clock of the read-back of CSR and coordinates and of the NumPy pair "
                     "test of tests/graph_crossings_ref.py (per graph: mutual edges, fp32 box reject, float64 "
                     "orientations, in chunks of 512 edges), one process, alternated with the op; at C2 the host leg "
                     "runs on the first graph alone, three times, and is scaled by B in host_over_op; medians with "
                     "min-max; pairs_per_second = sum of work / median op time; no ratio is a gate",
           "default_work_cap": layers.CROSSINGS_WORK_CAP, "results": []}
    for name, cfg, B, hi, hg in runs:
        r = measure(name, cfg, B, a.iters, a.warmup, hi, hg)
        res["results"].append(r)
        print(json.dumps({"shape": r["shape"], "op_us": r["graph_crossings_op"]["median_us"],
                          "host_us": r["host_numpy"]["median_us"], "host_graphs": r["host_graphs"],
                          "read_back_us": r["host_read_back"]["median_us"], "pairs_per_second": r["pairs_per_second"],
                          "host_over_op": r["host_over_op"], "agree": r["counts_agree_with_host"],
                          "counts_sum": r["counts_sum"]}), flush=True)
    if a.chords:
        n, e = (int(x) for x in a.chords.split("x"))
        r = chords_rate(n, e, max(3, a.iters // 4), 1)
        res["chords"] = r
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
