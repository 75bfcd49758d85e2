"""Time the spectral density op (snd_graph_spectrum) beside the only other route to a spectrum.

Two shapes:

  * ref:  the reference's scale, N = 25, B = 1500 graphs, exact traces, K = 128 moments;
  * C2:   the node-latent scale, N = 4096, B = 8 from ``data.synthetic_batch`` (the bench RGG),
          32 Rademacher probes, K = 128.

Per shape, in one process and alternating per iteration:

  * op:    ``layers.graph_spectrum`` on the batch's own CSR (HIP events around the call); at
           ``ref`` both the LDS path and the forced global path (``force_global=True``), one
           after the other in every iteration;
  * host:  the route without the op: read the CSR back (timed on its own), then per graph the
           dense M = L - I and ``numpy.linalg.eigvalsh`` (wall clock; ``--host-iters-large``
           runs at C2, where one iteration takes many seconds).

Medians with min-max.  The op's moments are compared with the moments of the host's eigenvalues
(exact mode: the difference; probe mode: the EMD in lambda units between the two 200-bin
densities, the error of 32 probes).  No ratio is a gate: the numbers are reported as measured.

    python tools/graph_spectrum_timing.py --out profiles/graph_spectrum_timing.json
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


def host_spectra(rp, ci, B, n):
    """Eigenvalues of L per graph by dense eigvalsh; returns (microseconds, [B, n])."""
    t0 = time.perf_counter()
    rp = rp.astype(np.int64)
    out = np.empty((B, n))
    for g in range(B):
        A = np.zeros((n, n), bool)
        lo, hi = rp[g * n], rp[(g + 1) * n]
        rows = np.repeat(np.arange(n), np.diff(rp[g * n:(g + 1) * n + 1]))
        cols = ci[lo:hi].astype(np.int64) - g * n
        ok = (cols >= 0) & (cols < n) & (cols != rows)
        A[rows[ok], cols[ok]] = True
        A = (A & A.T).astype(np.float64)
        d = A.sum(axis=1)
        s = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
        M = -(s[:, None] * A * s[None, :])
        M[d == 0, d == 0] = -1.0
        out[g] = np.linalg.eigvalsh(M) + 1.0
    return (time.perf_counter() - t0) * 1e6, out


def measure(name, cfg, B, K, probes, iters, warmup, host_iters, both_paths):
    from snd_vae_amd import layers
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.metrics import SpectrumStats, emd
    from snd_vae_amd.model import DeviceBatch
    n = cfg.n_nodes
    db = DeviceBatch(synthetic_batch(cfg, B, seed=3), locality=False)
    op = lambda: layers.graph_spectrum(db.rowptr, db.colidx, B, n, n_moments=K, n_probes=probes, seed=1)
    glob = lambda: layers.graph_spectrum(db.rowptr, db.colidx, B, n, n_moments=K, n_probes=probes, seed=1,
                                         force_global=True)
    t = {"op": [], "forced_global": [], "read_back": [], "host": []}
    lam = None
    for it in range(warmup + iters):
        us, _ = timed(op)
        gus = timed(glob)[0] if both_paths else None
        if it >= warmup:
            t["op"].append(us)
            if both_paths:
                t["forced_global"].append(gus)
            if len(t["host"]) < host_iters:
                rb, arrays = read_back(db.rowptr, db.colidx)
                hu, lam = host_spectra(*arrays, B, n)
                t["read_back"].append(rb)
                t["host"].append(hu)
    moments, info = op()
    torch.cuda.synchronize()
    st = SpectrumStats(moments, info, n)
    theta = np.arccos(np.clip(lam - 1.0, -1.0, 1.0))
    host_m = np.cos(np.arange(K)[None, :, None] * theta[:, None, :]).sum(axis=2)
    host_st = SpectrumStats(host_m, st.info, n)
    d_op, d_host = st.density(200), host_st.density(200)
    out = {"shape": {"name": name, "B": B, "N": n, "entries": db.nnz, "n_moments": K, "n_probes": probes},
           "path": "lds" if n <= 64 else "global",
           "max_moment_difference_from_eigvalsh": float(np.abs(st.moments - host_m).max()),
           "max_density_emd_from_eigvalsh": max(emd(d_op[g], d_host[g], 2.0 / 200) for g in range(B)),
           "graph_spectrum_op": stats(t["op"]), "host_read_back": stats(t["read_back"]),
           "host_eigvalsh": stats(t["host"])}
    if both_paths:
        out["graph_spectrum_forced_global"] = stats(t["forced_global"])
        out["global_over_lds"] = out["graph_spectrum_forced_global"]["median_us"] / out["graph_spectrum_op"]["median_us"]
    host = out["host_eigvalsh"]["median_us"] + out["host_read_back"]["median_us"]
    out["host_over_op"] = host / out["graph_spectrum_op"]["median_us"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/graph_spectrum_timing.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--host-iters-large", type=int, default=3)
    ap.add_argument("--moments", type=int, default=128)
    ap.add_argument("--shapes", default="ref,C2")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("graph_spectrum_timing needs a ROCm GPU: a time taken elsewhere says nothing")
    from snd_vae_amd import layers
    from snd_vae_amd.config import PRESETS, tscale
    want = a.shapes.split(",")
    res = {"device": torch.cuda.get_device_name(0),
           "method": f"op: HIP events per call, {a.warmup} warm-up + {a.iters} timed iterations; at ref the LDS path "
                     "and the forced global path alternate in every iteration; host: wall clock of the CSR "
                     "read-back and of a dense numpy.linalg.eigvalsh per graph, one process, alternated with the "
                     "op; medians with min-max, every entry carries its n; host_over_op = (host_eigvalsh + "
                     "host_read_back) / graph_spectrum_op medians; no ratio is a gate",
           "probe_block_width": 32, "results": []}
    runs = []
    if "ref" in want:
        runs.append(("ref", tscale(25, 16, mean_degree=4.0), 1500, 0, a.host_iters, True))
    if "C2" in want:
        runs.append(("C2", PRESETS["C2"], 8, layers.SPECTRUM_PROBES, a.host_iters_large, False))
    for name, cfg, B, probes, host_iters, both in runs:
        r = measure(name, cfg, B, a.moments, probes, a.iters, a.warmup, host_iters, both)
        res["results"].append(r)
        print(json.dumps({k: r[k] for k in r if not k.startswith("host_") or k == "host_over_op"}), flush=True)
        print(json.dumps({"host_eigvalsh": r["host_eigvalsh"], "host_read_back": r["host_read_back"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
