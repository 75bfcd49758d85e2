"""Time the graphlet census (snd_graph_motifs) beside the only other route to its numbers.

Two shapes:

  * ref:  the reference's scale, N = 25, B = 1500 graphs;
  * C2:   the node-latent scale, N = 4096, B = 8 from ``data.synthetic_batch`` (the bench RGG).

Per shape, in one process and alternating per iteration:

  * op:    ``layers.graph_motifs`` on the batch's own CSR (HIP events around the call);
  * host:  the route without the op: read the CSR back (timed on its own), then the header's
           formulas with ``scipy.sparse`` on the block-diagonal matrix (degrees, codegrees M M,
           per-edge triangles (M M) o M, 4-cliques as the triangles among the higher neighbours
           of every node) (wall clock).  networkx, where it is exact (triangles; 4-cliques by
           ``enumerate_all_cliques`` up to size 4), is run once per shape and checked, with its
           own wall clock.

Medians with min-max; both routes' census must agree exactly.  Then the op alone on complete
graphs K_n, whose work bound and clique count are known: work / time is the rate from which the
default ``work_cap`` (``layers.MOTIFS_WORK_CAP``) is chosen.  No ratio is a gate: the numbers are
reported as measured.

    python tools/graph_motifs_timing.py --out profiles/graph_motifs_timing.json
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


def read_back(rowptr, colidx):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rp, ci = rowptr.cpu().numpy(), colidx.cpu().numpy()
    return (time.perf_counter() - t0) * 1e6, (rp, ci)


def mutual_matrix(rp, ci, B, n):
    """(M, one-way arcs per graph): the mutual-edge 0/1 matrix of the whole batch."""
    import scipy.sparse as sp
    R = B * n
    rp = rp.astype(np.int64)
    ci = ci[:rp[-1]].astype(np.int64)
    rows = np.repeat(np.arange(R, dtype=np.int64), np.diff(rp))
    base = rows // n * n
    ok = (ci >= base) & (ci < base + n) & (ci != rows)
    A = sp.csr_matrix((np.ones(int(ok.sum()), np.int64), (rows[ok], ci[ok])), shape=(R, R))
    A.sum_duplicates()
    A.data[:] = 1
    M = A.multiply(A.T).tocsr()
    M.data[:] = 1
    arcs = np.bincount(A.tocoo().row // n, minlength=B)
    return M, arcs - np.bincount(M.tocoo().row // n, minlength=B)


def host_census(rp, ci, B, n):
    """census [B, 10] by the header's formulas on scipy.sparse; returns (microseconds, census)."""
    import scipy.sparse as sp
    t0 = time.perf_counter()
    M, one = mutual_matrix(rp, ci, B, n)
    R = B * n
    per = lambda v: np.add.reduceat(np.asarray(v, np.int64), np.arange(0, R, n))      # sums per graph
    d = np.asarray(M.sum(axis=1)).ravel().astype(np.int64)
    C = (M @ M).tocsr()
    t = C.multiply(M).tocsr()
    tv = np.asarray(t.sum(axis=1)).ravel().astype(np.int64)
    E = per(d) // 2
    T = per(tv) // 6
    W = per(d * (d - 1) // 2)
    S3p = per(d * (d - 1) * (d - 2) // 6)
    P3p = per((d - 1) * (M @ (d - 1))) // 2 - 3 * T
    TTp = per(tv // 2 * (d - 2))
    cu = sp.triu(C, k=1).tocoo()
    C4p = np.bincount(cu.row // n, weights=(cu.data * (cu.data - 1) // 2).astype(np.float64), minlength=B)
    C4p = np.rint(C4p).astype(np.int64) // 2
    tu = sp.triu(t, k=1).tocoo()
    Dp = np.rint(np.bincount(tu.row // n, weights=(tu.data * (tu.data - 1) // 2).astype(np.float64),
                             minlength=B)).astype(np.int64)
    K4 = np.zeros(B, np.int64)
    U = sp.triu(M, k=1).tocsr()
    for u in np.nonzero(np.diff(U.indptr) >= 3)[0]:
        nb = U.indices[U.indptr[u]:U.indptr[u + 1]]
        S = M[nb][:, nb].toarray().astype(np.float64)
        K4[u // n] += int(round(((S @ S) * S).sum())) // 6
    D = Dp - 6 * K4
    C4 = C4p - D - 3 * K4
    TT = TTp - 4 * D - 12 * K4
    S3 = S3p - TT - 2 * D - 4 * K4
    P3 = P3p - 2 * TT - 4 * C4 - 6 * D - 12 * K4
    cen = np.stack([E, W - 3 * T, T, P3, S3, C4, TT, D, K4, one.astype(np.int64)], axis=1)
    return (time.perf_counter() - t0) * 1e6, cen


def networkx_check(rp, ci, B, n, census):
    """Triangles and 4-cliques per graph with networkx; (microseconds, agree)."""
    import networkx as nx
    t0 = time.perf_counter()
    M, _ = mutual_matrix(rp, ci, B, n)
    ok = True
    for g in range(B):
        H = nx.from_scipy_sparse_array(M[g * n:(g + 1) * n][:, g * n:(g + 1) * n])
        tri = sum(nx.triangles(H).values()) // 3
        k4 = 0
        for q in nx.enumerate_all_cliques(H):
            if len(q) > 4:
                break
            k4 += len(q) == 4
        ok = ok and tri == census[g, 2] and k4 == census[g, 8]
    return (time.perf_counter() - t0) * 1e6, bool(ok)


def measure(name, cfg, B, iters, warmup, host_iters):
    from snd_vae_amd import layers
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.model import DeviceBatch
    n = cfg.n_nodes
    db = DeviceBatch(synthetic_batch(cfg, B, seed=3), locality=False)
    op = lambda: layers.graph_motifs(db.rowptr, db.colidx, B, n)
    t = {"op": [], "read_back": [], "host": []}
    host_cen = None
    for it in range(warmup + iters):
        us, _ = timed(op)
        if it >= warmup:
            t["op"].append(us)
            if len(t["host"]) < host_iters:
                rb, arrays = read_back(db.rowptr, db.colidx)
                hu, host_cen = host_census(*arrays, B, n)
                t["read_back"].append(rb)
                t["host"].append(hu)
    census, work = op()
    torch.cuda.synchronize()
    cen, wk = census.cpu().numpy(), work.cpu().numpy()
    nx_us, nx_ok = networkx_check(*read_back(db.rowptr, db.colidx)[1], B, n, cen)
    out = {"shape": {"name": name, "B": B, "N": n, "entries": db.nnz},
           "census_sum": dict(zip(("E", "P2", "T", "P3", "S3", "C4", "TT", "D", "K4", "one_way"),
                                  (int(x) for x in cen.sum(axis=0)))),
           "work_max": int(wk.max()), "work_sum": int(wk.sum()), "skipped": int((cen[:, 0] < 0).sum()),
           "census_agrees_with_host": bool(np.array_equal(cen, host_cen)),
           "networkx_triangles_and_cliques_agree": nx_ok, "networkx_us_once": nx_us,
           "graph_motifs_op": stats(t["op"]), "host_read_back": stats(t["read_back"]),
           "host_scipy": stats(t["host"])}
    host = out["host_scipy"]["median_us"] + out["host_read_back"]["median_us"]
    out["host_over_op"] = host / out["graph_motifs_op"]["median_us"]
    return out


def complete_rate(n, iters, warmup):
    """The op on one complete graph K_n without a cap: its work bound per second."""
    from snd_vae_amd import layers
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    col = idx.repeat(n, 1)
    colidx = col[col != idx[:, None]].contiguous()
    rowptr = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * (n - 1)).to(torch.int32)
    op = lambda: layers.graph_motifs(rowptr, colidx, 1, n, work_cap=1 << 62)
    t = []
    for it in range(warmup + iters):
        us, (census, work) = timed(op)
        if it >= warmup:
            t.append(us)
    k4, wk = int(census[0, 8].item()), int(work[0].item())
    s = stats(t)
    return {"n": n, "work": wk, "K4": k4, "K4_expected": n * (n - 1) * (n - 2) * (n - 3) // 24, "op": s,
            "work_per_second": wk / (s["median_us"] * 1e-6)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/graph_motifs_timing.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--shapes", default="ref,C2")
    ap.add_argument("--complete", default="128,256,512", help="complete graphs for the work rate")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("graph_motifs_timing needs a ROCm GPU: a time taken elsewhere says nothing")
    from snd_vae_amd import layers
    from snd_vae_amd.config import PRESETS, tscale
    want = a.shapes.split(",")
    runs = []
    if "ref" in want:
        runs.append(("ref", tscale(25, 16, mean_degree=4.0), 1500))
    if "C2" in want:
        runs.append(("C2", PRESETS["C2"], 8))
    res = {"device": torch.cuda.get_device_name(0),
           "method": f"op: HIP events per call, {a.warmup} warm-up + {a.iters} timed iterations; host: wall clock "
                     "of the CSR read-back and of the header's formulas on scipy.sparse over the block-diagonal "
                     "matrix, one process, alternated with the op per iteration; medians with min-max; "
                     "host_over_op = (host_scipy + host_read_back) / graph_motifs_op medians; complete graphs: the "
                     "op alone, work / median time; no ratio is a gate",
           "default_work_cap": layers.MOTIFS_WORK_CAP, "results": [], "complete_graphs": []}
    for name, cfg, B in runs:
        r = measure(name, cfg, B, a.iters, a.warmup, a.host_iters)
        res["results"].append(r)
        print(json.dumps({"shape": r["shape"], "op_us": r["graph_motifs_op"]["median_us"],
                          "host_us": r["host_scipy"]["median_us"], "read_back_us": r["host_read_back"]["median_us"],
                          "host_over_op": r["host_over_op"], "agree": r["census_agrees_with_host"],
                          "networkx_agree": r["networkx_triangles_and_cliques_agree"]}), flush=True)
    for n in (int(x) for x in a.complete.split(",") if x):
        r = complete_rate(n, max(3, a.iters // 4), 1)
        res["complete_graphs"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
