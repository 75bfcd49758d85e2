"""Time the latent-factor mutual-information op (snd_latent_mi) against the only other route.

One shape, the reference's scale: a [2500, 400] matrix of encoder means on the device, 3
integer-coded factors of 5 levels, 20 bins each.  In one process, alternating per iteration:

  * new: ``layers.latent_mi(z, f, 20)`` -- HIP events around the call (the op: a memset and
    four kernels), and the wall time of the call plus the one read-back of mi, hz, hf
    (``metrics.LatentMI``), which is what an evaluation waits for;
  * host: read the means back (``z.cpu()``), then ``np.histogram2d`` per (latent, factor) and
    the same sums in NumPy -- wall time, split into the read-back and the arithmetic.

Warm-up iterations dropped; medians with min and max.  The two routes' mi are compared and the
largest difference is reported (np.histogram2d places its interior edges by its own rule, so
a value on an edge may land one bin over; nothing is gated on it).  No ratio is promised.

    python tools/latent_mi_timing.py --out profiles/latent_mi_timing.json
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

ROWS, LATENTS, FACTORS, LEVELS, BINS = 2500, 400, 3, 5, 20


def stats(v):
    v = sorted(v)
    return {"median_us": statistics.median(v), "min_us": v[0], "max_us": v[-1], "n": len(v)}


def host_mi(z, f, nb):
    """mi [L, K] through np.histogram2d, one call per (latent, factor)."""
    rows, L = z.shape
    K = f.shape[1]
    mi = np.zeros((L, K))
    for l in range(L):
        for k in range(K):
            c, _, _ = np.histogram2d(z[:, l], f[:, k], bins=(nb, nb))
            r, s = c.sum(axis=1, keepdims=True), c.sum(axis=0, keepdims=True)
            nz = c > 0
            mi[l, k] = np.sum(c[nz] / rows * np.log(c[nz] * rows / (r * s)[nz]))
    return mi


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/latent_mi_timing.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("latent_mi_timing needs a ROCm GPU: a time taken elsewhere says nothing")
    from snd_vae_amd import layers
    from snd_vae_amd.metrics import LatentMI

    rng = np.random.default_rng(0)
    fh = rng.integers(0, LEVELS, size=(ROWS, FACTORS)).astype(np.float32)
    zh = rng.standard_normal((ROWS, LATENTS)).astype(np.float32)
    zh[:, :FACTORS] += fh                                    # a few latents that know a factor
    z, f = torch.from_numpy(zh).cuda(), torch.from_numpy(fh).cuda()
    t = {"op_events": [], "new_wall": [], "host_wall": [], "host_readback": [], "host_arithmetic": []}
    new_mi = old_mi = None
    for it in range(a.warmup + a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        out = layers.latent_mi(z, f, BINS)
        e1.record()
        new_mi = LatentMI(*out).mi                           # the one read-back
        w1 = time.perf_counter()
        e1.synchronize()
        op = e0.elapsed_time(e1) * 1e3
        h0 = time.perf_counter()
        zc, fc = z.cpu().numpy(), f.cpu().numpy()
        h1 = time.perf_counter()
        old_mi = host_mi(zc, fc, BINS)
        h2 = time.perf_counter()
        if it >= a.warmup:
            for k, v in (("op_events", op), ("new_wall", (w1 - w0) * 1e6), ("host_wall", (h2 - h0) * 1e6),
                         ("host_readback", (h1 - h0) * 1e6), ("host_arithmetic", (h2 - h1) * 1e6)):
                t[k].append(v)
    res = {"device": torch.cuda.get_device_name(0),
           "shape": {"rows": ROWS, "latents": LATENTS, "factors": FACTORS, "levels": LEVELS, "n_bins": BINS,
                     "factor_bins": BINS},
           "method": "one process, routes alternated per iteration, "
                     f"{a.warmup} warm-up + {a.iters} timed iterations, medians with min and max; op_events = HIP "
                     "events around layers.latent_mi (memset + four kernels); new_wall = that call plus the one "
                     "read-back of mi, hz, hf, wall clock; host_wall = z.cpu() + np.histogram2d per (latent, "
                     "factor) + the sums in NumPy, wall clock",
           "bytes_read_by_the_op": 4 * ROWS * (LATENTS + FACTORS),
           "bytes_read_back_new": 8 * (LATENTS * FACTORS + LATENTS + FACTORS),
           "bytes_read_back_host": 4 * ROWS * (LATENTS + FACTORS),
           "new": {"op_events": stats(t["op_events"]), "wall_with_read_back": stats(t["new_wall"])},
           "host": {"wall": stats(t["host_wall"]), "read_back": stats(t["host_readback"]),
                    "histogram2d_and_sums": stats(t["host_arithmetic"])},
           "max_abs_mi_difference_between_routes": float(np.max(np.abs(new_mi - old_mi)))}
    res["host_wall_over_new_wall"] = res["host"]["wall"]["median_us"] / res["new"]["wall_with_read_back"]["median_us"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
    print(json.dumps({"op_us": res["new"]["op_events"]["median_us"],
                      "new_wall_us": res["new"]["wall_with_read_back"]["median_us"],
                      "host_wall_us": res["host"]["wall"]["median_us"],
                      "mi_diff": res["max_abs_mi_difference_between_routes"]}), flush=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
