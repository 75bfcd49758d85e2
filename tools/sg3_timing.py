"""Time one three-hop spatial-graph layer (snd_sg3_layer_fwd + snd_sg3_layer_bwd,
SpatialGraphConvolution_3D of `layers.py:200-277`) on spanning trees.

Shapes: the protein widths of the reference (`main.py:223`): layer 1 (F = 1, [10]*4) and
layer 2 (F = 10, [20]*4), over C = B * sampling_num tree copies of N nodes, for (C, N) =
(100, 25), the reference's batch of 10 graphs x 10 trees, and (100, 100).  Trees are uniform
random recursive trees, rel the 3-D Euclidean distances of points in the unit cube.  Per
shape, in one process and alternating per iteration:

  * sg3_fwd, sg3_bwd: the three-hop layer with BN + lrelu, dx requested;
  * sg_fwd, sg_bwd:   the two-hop layer (snd_sg_layer_*) at the first three widths on the
                      same graph, for scale.

There is no pass bar: the kernels are latency- and gather-bound and this is their first
measurement.  Reported with the directed 2-paths P2 = sum_j d_j^2 the path kernels walk and
the workspace bytes the layer asks for.

HIP events around each call, warm-up iterations dropped, medians reported.

    python tools/sg3_timing.py --out profiles/sg3_timing.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = ((100, 25), (100, 100))
LAYERS = (("layer1", 1, (10, 10, 10, 10)), ("layer2", 10, (20, 20, 20, 20)))


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


def trees(C, N, rng):
    """Block-diagonal symmetric CSR of C random recursive trees and rel [C, N, N]."""
    from snd_vae_amd.data import csr_from_pairs, stack_csr
    parts = []
    for _ in range(C):
        order = rng.permutation(N)
        pairs = np.array([(order[t], order[rng.integers(t)]) for t in range(1, N)], np.int64)
        parts.append(csr_from_pairs(N, pairs))
    rp, ci = stack_csr(parts, N)
    pos = rng.random((C, N, 3))
    rel = np.linalg.norm(pos[:, :, None] - pos[:, None], axis=-1).astype(np.float32)
    return rp, ci, rel


def measure(C, N, name, F, hid, iters, warmup, seed):
    from snd_vae_amd import _lib
    from snd_vae_amd.sg import (SGGraph, SpatialGraphConvolution, SpatialGraphConvolution3D, init_sg3_layer,
                                init_sg_layer, sg3_pack, sg_pack)
    rng = np.random.default_rng(seed)
    rp, ci, rel = trees(C, N, rng)
    g = SGGraph(rp, ci, N, torch.from_numpy(rel).cuda())
    R = C * N
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    l3 = SpatialGraphConvolution3D(F, hid, up(sg3_pack(F, hid, init_sg3_layer(F, hid, rng))))
    l2 = SpatialGraphConvolution(F, hid[:3], up(sg_pack(F, hid[:3], init_sg_layer(F, hid[:3], rng))))
    x = up(rng.random((R, F)))
    d3, d2 = up(rng.normal(size=(R, hid[3]))), up(rng.normal(size=(R, hid[2])))
    t = {"sg3_fwd": [], "sg3_bwd": [], "sg_fwd": [], "sg_bwd": []}
    for it in range(warmup + iters):
        row = (timed(lambda: l3.forward(g, x))[0], timed(lambda: l3.backward(d3))[0],
               timed(lambda: l2.forward(g, x))[0], timed(lambda: l2.backward(d2))[0])
        if it >= warmup:
            for k, v in zip(t, row):
                t[k].append(v)
    med = {k: statistics.median(v) for k, v in t.items()}
    ws = int(_lib.lib().snd_sg3_workspace(R, g.nnz, g.n_paths, F, *hid))
    return {"shape": {"copies": C, "N": N, "rows": R, "layer": name, "F": F, "widths": list(hid)},
            "directed_edges": g.nnz, "directed_2_paths": g.n_paths,
            "max_degree": int(np.diff(np.asarray(rp)).max()), "workspace_bytes": ws,
            **{k: stats(v) for k, v in t.items()},
            "sg3_fwd_bwd_us": med["sg3_fwd"] + med["sg3_bwd"], "sg_fwd_bwd_us": med["sg_fwd"] + med["sg_bwd"],
            "paths_per_s": g.n_paths / ((med["sg3_fwd"] + med["sg3_bwd"]) * 1e-6)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/sg3_timing.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sg3_timing needs a ROCm GPU: a time taken elsewhere says nothing")
    res = {"device": torch.cuda.get_device_name(0),
           "method": "HIP events per call (host launches included: the calls are launch sequences, not "
                     f"captured graphs), routes alternated per iteration in one process, {a.warmup} warm-up + "
                     f"{a.iters} timed iterations, medians; no pass bar; sg_* is the two-hop layer at the "
                     "first three widths on the same trees",
           "results": []}
    for C, N in SHAPES:
        for name, F, hid in LAYERS:
            r = measure(C, N, name, F, hid, a.iters, a.warmup, a.seed)
            res["results"].append(r)
            print(json.dumps({"shape": r["shape"], "paths": r["directed_2_paths"],
                              "sg3_fwd_us": r["sg3_fwd"]["median_us"], "sg3_bwd_us": r["sg3_bwd"]["median_us"],
                              "sg_fwd_us": r["sg_fwd"]["median_us"], "sg_bwd_us": r["sg_bwd"]["median_us"]}),
                  flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
