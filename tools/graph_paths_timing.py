"""Time the path-statistics op (snd_graph_paths) beside the only other route to its numbers.

Two shapes, three measurements:

  * ref:  the reference's scale, N = 25, B = 1500 graphs, every node a source;
  * C2:   the node-latent scale, N = 4096, B = 8 from ``data.synthetic_batch``, with
          ``src_step`` 1 (every node a source) and 16.

Per measurement, in one process and alternating per iteration:

  * op:    ``layers.graph_paths`` on the batch's own CSR and ``spatial_truth`` into preallocated
           counters (HIP events around the call);
  * host:  the route without the op: read the CSR and the coordinates back (timed on its own),
           then per graph ``scipy.sparse.csgraph.connected_components`` +
           ``shortest_path(unweighted=True)`` + ``dijkstra`` from the same sources (wall clock).

Medians with min-max.  The host route at C2 with every node a source takes most of a minute per
iteration, so it is timed ``--host-iters-big`` times (default 3), not ``--iters``; every entry
carries its own n.  No ratio is a gate: the numbers are reported as measured.

    python tools/graph_paths_timing.py --out profiles/graph_paths_timing.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

DETOUR_SCALE = 64.0


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


def read_back(db):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rp, ci, xy = db.rowptr.cpu().numpy(), db.colidx.cpu().numpy(), db.spatial_truth.cpu().numpy()
    return (time.perf_counter() - t0) * 1e6, (rp, ci, xy)


def host_route(rp, ci, xy, B, n, src_step):
    """The statistics' raw material per graph with scipy: component labels, hop counts and
    float64 route lengths from the sources.  Returns (microseconds, reachable ordered pairs)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components, dijkstra, shortest_path
    t0 = time.perf_counter()
    src = np.arange(0, n, src_step)
    pairs = 0
    x = xy.astype(np.float64)
    for g in range(B):
        lo, hi = rp[g * n], rp[(g + 1) * n]
        cols = ci[lo:hi].astype(np.int64) - g * n
        rows = np.repeat(np.arange(n), np.diff(rp[g * n:(g + 1) * n + 1]))
        keep = (cols >= 0) & (cols < n) & (cols != rows)
        rows, cols = rows[keep], cols[keep]
        d = x[g * n + rows] - x[g * n + cols]
        W = sp.csr_matrix((np.sqrt((d * d).sum(axis=1)), (rows, cols)), shape=(n, n))
        connected_components(W, directed=False)
        hops = shortest_path(W, unweighted=True, directed=True, indices=src)
        dijkstra(W, directed=True, indices=src)
        pairs += int(np.isfinite(hops).sum()) - len(src)
    return (time.perf_counter() - t0) * 1e6, pairs


def measure(name, cfg, B, src_step, iters, warmup, host_iters):
    from snd_vae_amd import layers
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.model import DeviceBatch
    n = cfg.n_nodes
    db = DeviceBatch(synthetic_batch(cfg, B, seed=3), locality=False)
    hist = torch.empty(B, 2, 256, dtype=torch.int64, device="cuda")
    totals = torch.empty(B, 6, dtype=torch.int64, device="cuda")
    op = lambda: layers.graph_paths(db.rowptr, db.colidx, B, n, db.spatial_truth, DETOUR_SCALE, src_step,
                                    hist=hist, totals=totals)
    t = {"op": [], "read_back": [], "host": []}
    host_pairs = None
    for it in range(warmup + iters):
        us, _ = timed(op)
        if it >= warmup:
            t["op"].append(us)
            if len(t["host"]) < host_iters:
                rb, arrays = read_back(db)
                hu, host_pairs = host_route(*arrays, B, n, src_step)
                t["read_back"].append(rb)
                t["host"].append(hu)
                print(f"{name} src_step={src_step} host iteration {len(t['host'])}: {hu * 1e-6:.2f} s", file=sys.stderr,
                      flush=True)
    op()
    torch.cuda.synchronize()
    tot = totals.cpu().numpy()
    n_src = -(-n // src_step)
    out = {"shape": {"name": name, "B": B, "N": n, "src_step": src_step, "sources_per_graph": n_src,
                     "entries": db.nnz, "spatial_dim": cfg.spatial_dim},
           "work_sources_x_arcs": int(n_src) * int(db.nnz),
           "reachable_pairs": int(tot[:, 3].sum()), "pairs_agree_with_host": bool(int(tot[:, 3].sum()) == host_pairs),
           "components_per_graph_mean": float(tot[:, 0].mean()), "max_hops": int(tot[:, 5].max()),
           "graph_paths_op": stats(t["op"]), "host_read_back": stats(t["read_back"]),
           "host_scipy": stats(t["host"])}
    host = out["host_scipy"]["median_us"] + out["host_read_back"]["median_us"]
    out["host_over_op"] = host / out["graph_paths_op"]["median_us"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/graph_paths_timing.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters-big", type=int, default=3, help="host iterations at C2 with every node a source")
    ap.add_argument("--shapes", default="ref,C2")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("graph_paths_timing needs a ROCm GPU: a time taken elsewhere says nothing")
    from snd_vae_amd.config import PRESETS, tscale
    want = a.shapes.split(",")
    runs = []
    if "ref" in want:
        runs.append(("ref", tscale(25, 16, mean_degree=4.0), 1500, 1, a.iters))
    if "C2" in want:
        runs += [("C2", PRESETS["C2"], 8, 1, a.host_iters_big), ("C2", PRESETS["C2"], 8, 16, a.iters)]
    res = {"device": torch.cuda.get_device_name(0),
           "method": f"op: HIP events per call, {a.warmup} warm-up + {a.iters} timed iterations; host: wall clock "
                     "of the read-back (CSR and coordinates) and of scipy.sparse.csgraph connected_components + "
                     "shortest_path(unweighted) + dijkstra per graph from the same sources, one process, "
                     "alternated with the op per iteration, n as stated per entry; medians with min-max; "
                     "host_over_op = (host_scipy + host_read_back) / graph_paths_op medians; no ratio is a gate",
           "results": []}
    for name, cfg, B, step, host_iters in runs:
        r = measure(name, cfg, B, step, a.iters, a.warmup, host_iters)
        res["results"].append(r)
        print(json.dumps({"shape": r["shape"], "op_us": r["graph_paths_op"]["median_us"],
                          "host_us": r["host_scipy"]["median_us"], "read_back_us": r["host_read_back"]["median_us"],
                          "host_over_op": r["host_over_op"], "pairs_agree": r["pairs_agree_with_host"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
