"""Time the training e2e structure decoder, forward + backward, under both engines on the
same operands: the direct launch sequence of `disent.structure_decoder` (snd_e2e_pair_fwd,
snd_e2e_fwd / snd_bn_relu_fwd per layer, snd_e2e_head_ce, then snd_e2e_bwd /
snd_bn_relu_bwd per layer and snd_e2e_pair_bwd) against one call of the factorised engine
(snd_e2e_train, ABI 24).

Shape: the synthetic2 widths of the reference (N = 25, D = 2 node_h = 40, e_d_hidden
(50, 20)) at B = 10, a reference batch, and B = 50.  Every buffer is allocated before the
timed window; per iteration the routes alternate in one process.  HIP events around each
route (host launches included: both are launch sequences), warm-up iterations dropped,
medians of 20 with the min-max spread.  Each engine's error against the float64 oracle
(autograd on the literal model) is recorded per block, as max |got - ref| / max |ref|.

Condition at both sizes: the factorised engine's slowest run is below the direct engine's
fastest.

    python tools/e2e_train_timing.py --out profiles/e2e_train_timing.json
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
BATCHES = (10, 50)
KEYS = ("gamma", "beta", "w", "b")


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
    f = lambda a: np.ascontiguousarray(a, np.float32)
    z = f(rng.standard_normal((B, N, D)))
    layers, cin = [], 2 * D
    for co in HIDDEN:
        layers.append({"gamma": f(1 + 0.3 * rng.standard_normal(cin)), "beta": f(0.3 * rng.standard_normal(cin)),
                       "w": f(rng.standard_normal((N, cin, co)) / np.sqrt(2 * N * cin)),
                       "b": f(0.3 * rng.standard_normal(co))})
        cin = co
    head = {"gamma": f(1 + 0.3 * rng.standard_normal(cin)), "beta": f(0.3 * rng.standard_normal(cin)),
            "w": f(rng.standard_normal((cin, 2)) / np.sqrt(cin)), "b": f(np.zeros(2))}
    up = np.triu(rng.random((B, N, N)) < 0.4, 1)
    return z, layers, head, f(up | up.transpose(0, 2, 1))


def block_errors(got, ref):
    """{block: max |got - ref| / max |ref|}; got / ref = (dz, layer grads, head grads)."""
    blocks = [("dz", got[0], ref[0])]
    for i, (a, b) in enumerate(zip(got[1], ref[1])):
        blocks += [(f"l{i}_{k}", a[k], b[k]) for k in KEYS]
    blocks += [(f"head_{k}", got[2][k], ref[2][k]) for k in KEYS]
    return {name: float(np.abs(np.asarray(a, np.float64).reshape(-1) - np.asarray(b).reshape(-1)).max()
                        / np.abs(b).max()) for name, a, b in blocks}


def measure(B, iters, warmup, seed):
    from oracle import ref_disent as RD
    from snd_vae_amd import _lib
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    hz, hlayers, hhead, hadj = operands(B, seed)
    cu = lambda a: torch.from_numpy(a).cuda()
    z, adj = cu(hz), cu(hadj)
    layers = [{k: cu(v) for k, v in l.items()} for l in hlayers]
    head = {k: cu(v) for k, v in hhead.items()}
    E = lambda *shape: torch.empty(*shape, device="cuda")
    n, rows = len(layers), B * N * N
    cins = (2 * D,) + HIDDEN[:-1]
    # one set of outputs per engine
    outs = {e: {"dz": torch.empty_like(z), "layers": [{k: torch.empty_like(v) for k, v in l.items()} for l in layers],
                "head": {k: torch.empty_like(v) for k, v in head.items()},
                "out": torch.empty(2, dtype=torch.float64, device="cuda")} for e in ("direct", "factorised")}
    # the factorised engine
    couts = (ctypes.c_int * n)(*HIDDEN)
    arr = (_lib.E2ELayer * n)(*[_lib.E2ELayer(*[P(l[k]) for k in KEYS], co) for l, co in zip(layers, HIDDEN)])
    fo = outs["factorised"]
    garr = (_lib.E2ELayerGrad * n)(*[_lib.E2ELayerGrad(*[P(g[k]) for k in KEYS]) for g in fo["layers"]])
    need = int(L.snd_e2e_train_workspace(B, N, D, couts, n))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def factorised():
        _lib.check(L.snd_e2e_train(P(z), D, P(adj), B, N, D, arr, n, P(head["gamma"]), P(head["beta"]), P(head["w"]),
                                   P(head["b"]), P(fo["dz"]), D, garr, P(fo["head"]["gamma"]), P(fo["head"]["beta"]),
                                   P(fo["head"]["w"]), P(fo["head"]["b"]), P(fo["out"]), P(ws), need, S),
                   "snd_e2e_train")
    # the direct engine's launch sequence (disent.structure_decoder), buffers allocated once
    do = outs["direct"]
    xs = [E(B, N, N, c) for c in cins]
    ys = [E(B, N, N, co) for co in HIDDEN]
    dys = [E(B, N, N, co) for co in HIDDEN]
    dxs = [E(B, N, N, c) for c in cins]
    pws = torch.empty(int(L.snd_e2e_pair_bwd_workspace(B, N, D)) // 4 + 1, device="cuda")

    def direct():
        l0 = layers[0]
        _lib.check(L.snd_e2e_pair_fwd(P(z), B, N, D, P(l0["gamma"]), P(l0["beta"]), P(xs[0]), S), "snd_e2e_pair_fwd")
        for i, (l, co) in enumerate(zip(layers, HIDDEN)):
            _lib.check(L.snd_e2e_fwd(P(xs[i]), B, N, cins[i], P(l["w"]), P(l["b"]), N, co, P(ys[i]), S), "snd_e2e_fwd")
            if i + 1 < n:
                nx = layers[i + 1]
                _lib.check(L.snd_bn_relu_fwd(P(ys[i]), rows, co, P(nx["gamma"]), P(nx["beta"]), P(xs[i + 1]), S),
                           "snd_bn_relu_fwd")
        hg = do["head"]
        _lib.check(L.snd_e2e_head_ce(P(ys[-1]), P(adj), B, N, HIDDEN[-1], P(head["gamma"]), P(head["beta"]),
                                     P(head["w"]), P(head["b"]), P(dys[-1]), P(hg["w"]), P(hg["b"]), P(hg["gamma"]),
                                     P(hg["beta"]), P(do["out"]), S), "snd_e2e_head_ce")
        for i in range(n - 1, -1, -1):
            g = do["layers"][i]
            _lib.check(L.snd_e2e_bwd(P(xs[i]), B, N, cins[i], P(layers[i]["w"]), N, HIDDEN[i], P(dys[i]), P(dxs[i]),
                                     P(g["w"]), P(g["b"]), S), "snd_e2e_bwd")
            if i > 0:
                _lib.check(L.snd_bn_relu_bwd(P(dxs[i]), P(ys[i - 1]), rows, cins[i], P(layers[i]["gamma"]),
                                             P(layers[i]["beta"]), P(dys[i - 1]), P(g["gamma"]), P(g["beta"]), S),
                           "snd_bn_relu_bwd")
            else:
                _lib.check(L.snd_e2e_pair_bwd(P(dxs[0]), P(z), B, N, D, P(l0["gamma"]), P(l0["beta"]), P(do["dz"]),
                                              P(g["gamma"]), P(g["beta"]), P(pws), S), "snd_e2e_pair_bwd")
    t = {"factorised": [], "direct": []}
    for it in range(warmup + iters):
        row = (timed(factorised), timed(direct))
        if it >= warmup:
            t["factorised"].append(row[0])
            t["direct"].append(row[1])
    torch.cuda.synchronize()
    rce, rcorrect, rdz, rlg, rhg = RD.structure_decoder_grads(hz, hadj, hlayers, hhead)
    r = {"shape": {"B": B, "N": N, "D": D, "hidden": list(HIDDEN)},
         "workspace_bytes": {"factorised": need,
                             "direct": 4 * sum(x.numel() for x in xs + ys + dys + dxs) + 4 * pws.numel()},
         "factorised": stats(t["factorised"]), "direct": stats(t["direct"]),
         "ratio_direct_over_factorised": statistics.median(t["direct"]) / statistics.median(t["factorised"]),
         "factorised_max_below_direct_min": max(t["factorised"]) < min(t["direct"]),
         "error_vs_float64": {}}
    for e, o in outs.items():
        cpu = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
        errs = block_errors((o["dz"].cpu().numpy(), [cpu(g) for g in o["layers"]], cpu(o["head"])), (rdz, rlg, rhg))
        v = o["out"].cpu().tolist()
        errs["ce_rel"] = abs(v[0] / rows - rce) / abs(rce)
        errs["correct_minus_ref"] = v[1] - rcorrect
        r["error_vs_float64"][e] = errs
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/e2e_train_timing.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("e2e_train_timing needs a ROCm GPU: a time taken elsewhere says nothing")
    res = {"device": torch.cuda.get_device_name(0),
           "method": "HIP events per route (host launches included: both are launch sequences, not captured "
                     f"graphs), same operands, routes alternated per iteration in one process, {a.warmup} warm-up + "
                     f"{a.iters} timed iterations, medians with min and max.  direct = snd_e2e_pair_fwd + snd_e2e_fwd "
                     "/ snd_bn_relu_fwd per layer + snd_e2e_head_ce + snd_e2e_bwd / snd_bn_relu_bwd per layer + "
                     "snd_e2e_pair_bwd on preallocated buffers; factorised = one snd_e2e_train.  Condition at both "
                     "sizes: the factorised max below the direct min",
           "results": []}
    for B in BATCHES:
        r = measure(B, a.iters, a.warmup, a.seed)
        res["results"].append(r)
        print(json.dumps({"B": B, "factorised_us": r["factorised"], "direct_us": r["direct"],
                          "ratio": r["ratio_direct_over_factorised"],
                          "factorised_max_below_direct_min": r["factorised_max_below_direct_min"],
                          "worst_error": {e: max(v for k, v in d.items() if k != "correct_minus_ref")
                                          for e, d in r["error_vs_float64"].items()}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    slow = [r["shape"]["B"] for r in res["results"] if not r["factorised_max_below_direct_min"]]
    if slow:
        sys.exit(f"B = {slow}: the factorised engine's slowest run is not below the direct engine's fastest")


if __name__ == "__main__":
    main()
