"""Time the forward-only e2e structure decoder (snd_e2e_decode, ABI 22) against the only
other route to the same adjacency, the forward half of the training decoder
(`disent.structure_decoder`): snd_e2e_pair_fwd, then snd_e2e_fwd / snd_bn_relu_fwd per
layer, then snd_e2e_head_ce -- which also computes the CE and every gradient of the head;
the training route has no cheaper way to its argmax.

Shapes: the synthetic2 widths of the reference (N = 25, D = 2 node_h = 40, e_d_hidden
(50, 20); `main.py:173-217`) at B = 10, a reference batch, and B = 1500, a full latent
traversal (visualize_length 5 x 300 latent dimensions, `main.py:121-123`).  Both routes read
the same operands, with every buffer allocated before the timed window; per iteration the
routes alternate in one process.  HIP events around each route (host launches included:
both are launch sequences), warm-up iterations dropped, medians with the min-max spread.

Condition at B = 1500: the new op's slowest run is below the old route's fastest.  B = 10
carries no condition (both are launch-bound there; the figure says which is shorter).

The adjacency of the two routes is compared at the timed sizes through the training
route's ``correct`` count against a random target.

    python tools/e2e_decode_timing.py --out profiles/e2e_decode_timing.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, D, HIDDEN = 25, 40, (50, 20)
BATCHES = (10, 1500)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3          # microseconds


def stats(v):
    v = sorted(v)
    return {"median_us": statistics.median(v), "min_us": v[0], "max_us": v[-1], "n": len(v)}


def operands(B, seed):
    rng = np.random.default_rng(seed)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    z = up(rng.standard_normal((B, N, D)))
    layers, cin = [], 2 * D
    for co in HIDDEN:
        layers.append({"gamma": up(1 + 0.3 * rng.standard_normal(cin)), "beta": up(0.3 * rng.standard_normal(cin)),
                       "w": up(rng.standard_normal((N, cin, co)) / np.sqrt(2 * N * cin)),
                       "b": up(0.3 * rng.standard_normal(co))})
        cin = co
    head = {"gamma": up(1 + 0.3 * rng.standard_normal(cin)), "beta": up(0.3 * rng.standard_normal(cin)),
            "w": up(rng.standard_normal((cin, 2)) / np.sqrt(cin)), "b": up(np.zeros(2))}
    target = up(rng.random((B, N, N)) < 0.4)
    return z, layers, head, target


def measure(B, iters, warmup, seed):
    from snd_vae_amd import _lib
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    z, layers, head, target = operands(B, seed)
    E = lambda *shape: torch.empty(*shape, device="cuda")
    # the new op
    n = len(layers)
    couts = (ctypes.c_int * n)(*HIDDEN)
    arr = (_lib.E2ELayer * n)(*[_lib.E2ELayer(P(l["gamma"]), P(l["beta"]), P(l["w"]), P(l["b"]), co)
                                for l, co in zip(layers, HIDDEN)])
    need = int(L.snd_e2e_decode_workspace(B, N, D, couts, n))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    adj = torch.empty(B, N, N, dtype=torch.uint8, device="cuda")

    def new():
        _lib.check(L.snd_e2e_decode(P(z), D, B, N, D, arr, n, P(head["gamma"]), P(head["beta"]), P(head["w"]),
                                    P(head["b"]), P(adj), None, P(ws), need, S), "snd_e2e_decode")
    # the training route's forward
    x0 = E(B, N, N, 2 * D)
    ys = [E(B, N, N, co) for co in HIDDEN]
    xs = [E(B, N, N, co) for co in HIDDEN[:-1]]
    dy = E(B, N, N, HIDDEN[-1])
    hg = {k: torch.empty_like(v) for k, v in head.items()}
    out = torch.empty(2, dtype=torch.float64, device="cuda")

    def old():
        _lib.check(L.snd_e2e_pair_fwd(P(z), B, N, D, P(layers[0]["gamma"]), P(layers[0]["beta"]), P(x0), S),
                   "snd_e2e_pair_fwd")
        x, cin = x0, 2 * D
        for i, (l, co) in enumerate(zip(layers, HIDDEN)):
            _lib.check(L.snd_e2e_fwd(P(x), B, N, cin, P(l["w"]), P(l["b"]), N, co, P(ys[i]), S), "snd_e2e_fwd")
            if i + 1 < n:
                nx = layers[i + 1]
                _lib.check(L.snd_bn_relu_fwd(P(ys[i]), B * N * N, co, P(nx["gamma"]), P(nx["beta"]), P(xs[i]), S),
                           "snd_bn_relu_fwd")
                x = xs[i]
            cin = co
        _lib.check(L.snd_e2e_head_ce(P(ys[-1]), P(target), B, N, HIDDEN[-1], P(head["gamma"]), P(head["beta"]),
                                     P(head["w"]), P(head["b"]), P(dy), P(hg["w"]), P(hg["b"]), P(hg["gamma"]),
                                     P(hg["beta"]), P(out), S), "snd_e2e_head_ce")
    t = {"new": [], "old": []}
    for it in range(warmup + iters):
        row = (timed(new), timed(old))
        if it >= warmup:
            t["new"].append(row[0])
            t["old"].append(row[1])
    torch.cuda.synchronize()
    correct_old = float(out.cpu()[1])
    correct_new = float((adj.float() == target).sum().cpu())
    r = {"shape": {"B": B, "N": N, "D": D, "hidden": list(HIDDEN)},
         "workspace_bytes": need,
         "old_route_bytes": 4 * (x0.numel() + sum(y.numel() for y in ys) + sum(x.numel() for x in xs) + dy.numel()),
         "snd_e2e_decode": stats(t["new"]), "training_route_forward": stats(t["old"]),
         "ratio_old_over_new": statistics.median(t["old"]) / statistics.median(t["new"]),
         "new_max_below_old_min": max(t["new"]) < min(t["old"]),
         "correct_vs_random_target": {"training_route": correct_old, "snd_e2e_decode": correct_new,
                                      "entries": B * N * N}}
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/e2e_decode_timing.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("e2e_decode_timing needs a ROCm GPU: a time taken elsewhere says nothing")
    res = {"device": torch.cuda.get_device_name(0),
           "method": "HIP events per route (host launches included: both are launch sequences, not captured "
                     f"graphs), same operands, routes alternated per iteration in one process, {a.warmup} warm-up + "
                     f"{a.iters} timed iterations, medians with min and max.  training_route_forward = "
                     "snd_e2e_pair_fwd + snd_e2e_fwd / snd_bn_relu_fwd per layer + snd_e2e_head_ce; the last call "
                     "also computes the CE and the head's gradients (dy, dW, db, dgamma, dbeta): the training "
                     "route has no forward-only head.  Condition at B = 1500: the new op's max below the old "
                     "route's min; none at B = 10",
           "results": []}
    for B in BATCHES:
        r = measure(B, a.iters, a.warmup, a.seed)
        res["results"].append(r)
        print(json.dumps({"B": B, "new_us": r["snd_e2e_decode"]["median_us"],
                          "old_us": r["training_route_forward"]["median_us"], "ratio": r["ratio_old_over_new"],
                          "new_max_below_old_min": r["new_max_below_old_min"],
                          "correct": r["correct_vs_random_target"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    big = res["results"][-1]
    if not big["new_max_below_old_min"]:
        sys.exit(f"B = {big['shape']['B']}: snd_e2e_decode max {big['snd_e2e_decode']['max_us']:.0f} us is not below "
                 f"the training route's min {big['training_route_forward']['min_us']:.0f} us")


if __name__ == "__main__":
    main()
