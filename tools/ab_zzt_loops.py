"""A/B of the d = 64 zz^T kernel's tile loops in alternating processes (HIP events over
captured back-to-back launches; each process's first timing is discarded).

    python tools/ab_zzt_loops.py [--rounds 3] [--shapes C2,C3,C4] [--skips] > table.txt
    python tools/ab_zzt_loops.py --one zzt_dense_v12 --shape C2,C3   # one process, a JSON line per shape

Variants: zzt_dense (the shipped loop), zzt_dense_v9 (round 5's loop), v10 (-z_i in
registers), v11 (+ DMA two tiles ahead), v12 (+ two-tile stages).  --skips adds the
measurement build's rows for v9 and v12: full / no epilogue (1) / no backward MFMAs (4) /
skeleton only (2: DMAs, waits, barriers and LDS reads) / no tile DMA (8) / both (10) / no tile loop (64),
variant = loop | bits << 8.
Shapes: C2 (N 4096, d 64, 8 graphs), C3 per rank (1 graph: column splits), C4 (graph
latent, 8 graphs).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOOPS = ["zzt_dense_v9", "zzt_dense_v10", "zzt_dense_v11", "zzt_dense_v12"]
SKIPS = [("full", 0), ("no epilogue", 1), ("no backward MFMAs", 4), ("skeleton only", 2),
         ("no tile DMA", 8), ("skeleton, no tile DMA", 10), ("no tile loop", 64)]


def one(name, shapes, reps, timings):
    for shape in shapes.split(","):
        one_shape(name, shape, reps, timings)


def one_shape(name, shape, reps, timings):
    import torch
    from snd_vae_amd import _lib
    from snd_vae_amd.config import PRESETS
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    from snd_vae_amd.optimizer import OptimizerVAE
    cfg, B = PRESETS[shape], {"C2": 8, "C3": 1, "C4": 8}[shape]
    db = DeviceBatch(synthetic_batch(cfg, B, seed=1000))
    model = SGCNModelVAE(cfg, B, dtype="bf16")
    OptimizerVAE(model).step(db)
    bc, L = db.c_struct(), _lib.lib()

    def launch(sp):
        _lib.check(L.snd_plan_launch(model.plan, bc, model.workspace.data_ptr(), name.encode(), sp))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        launch(_lib.stream_ptr(side))
        with torch.cuda.graph(g, stream=side):
            for _ in range(reps):
                launch(_lib.stream_ptr(side))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(timings + 1)]
    with torch.cuda.stream(side):
        for e0, e1 in ev:
            e0.record(side)
            g.replay()
            e1.record(side)
    ev[-1][1].synchronize()
    us = sorted(1e3 * e0.elapsed_time(e1) / reps for e0, e1 in ev[1:])   # the first one discarded
    print(json.dumps({"variant": name, "shape": shape, "us_median": round(us[len(us) // 2], 3),
                      "us_min": round(us[0], 3), "us_max": round(us[-1], 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--shape", default="C2")
    ap.add_argument("--shapes", default="C2,C3,C4")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--timings", type=int, default=7)
    ap.add_argument("--skips", action="store_true")
    ap.add_argument("--timeout", type=int, default=120)
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.shape, args.reps, args.timings)
    jobs = [(args.shapes, v, v, args.rounds) for v in LOOPS if args.rounds]
    if args.skips:
        for loop in (9, 12):
            jobs += [("C2", f"zzt_dense_v{loop | bits << 8}", f"v{loop} MEAS {label}", args.skip_rounds)
                     for label, bits in SKIPS]
    res = {}
    for rnd in range(max(args.rounds, args.skip_rounds)):   # alternating: every variant once per round
        for shapes, name, label, rounds in jobs:
            if rnd >= rounds:
                continue
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--shape", shapes,
                                "--reps", str(args.reps), "--timings", str(args.timings)],
                               capture_output=True, text=True, timeout=args.timeout)
            if r.returncode != 0:           # no further GPU process after an abnormal exit
                sys.exit(f"{name} at {shapes}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
            for line in r.stdout.strip().splitlines()[-len(shapes.split(",")):]:
                j = json.loads(line)
                res.setdefault((j["shape"], label), []).append(j["us_median"])
                print(f"# round {rnd} {j['shape']} {label}: {j['us_median']:.2f} us", flush=True)
    print(f"{'shape':5s} {'variant':28s} {'median us':>10s} {'min':>8s} {'max':>8s} {'spread':>7s}  rounds")
    for (shape, label), v in res.items():
        s = sorted(v)
        print(f"{shape:5s} {label:28s} {s[len(s) // 2]:10.2f} {s[0]:8.2f} {s[-1]:8.2f} {s[-1] - s[0]:7.2f}  "
              + " ".join(f"{x:.2f}" for x in v))


if __name__ == "__main__":
    main()
