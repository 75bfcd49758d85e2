#!/usr/bin/env python3
"""Benchmark: SND-VAE training graphs/sec + ELBO-step ms (BASELINE.json metric).

Workload (BASELINE.json configs[1], "C2"): synthetic random-geometric spatial
graphs, N=4096 nodes, d=64, bf16 MFMA operands (fp32 accumulation/params),
node-latent SND-VAE (SURVEY.md §8 composed step).  A "step" is one full
training iteration over the device batch: forward, hand-derived backward,
(data parallel) one RCCL all-reduce of the flat gradient, TF1 Adam --
captured in one HIP graph and replayed.  Inputs are resident in HBM.

    python bench.py [--gpus N --steps K --warmup W --graphs-per-gpu B]
    python bench.py --full ...           (everything beside the headline, below)
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 \
        bench.py --gpus N ...            (one rank per GPU, RCCL over xGMI)

Prints ONE JSON line on rank 0.  value = graphs/sec over all ranks (weak
scaling: B graphs per GPU); ms_per_step = the median timed step.  A plain run
sets up, warms up, times the K steps and prints that line.  --dump-outputs DIR
also writes what the last timed step left its caller (loss terms, parameters,
gradient, Adam moments) as DIR/<name>.npy; the inputs are the same in every
run with the same arguments, so two builds compare output for output.

--full adds what takes runs of its own: roofline = the dominant kernel (fused
zz^T + CE, MFMA-bound), timed with HIP events on the launch stream, the SpMM
secondary roofline, the fp32 mode, the one-graph (C3 per-rank) step, the batch
sweep, the C4 / C5 workloads, and cpu_baseline = the reference formulation
(dense A, materialised [N,N,2] logits, autograd, TF1 Adam) in torch-CPU fp32
on the host cores (TensorFlow is unavailable).
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "training graphs/sec + ELBO-step ms, N=4096 d=64, at 1/2/4/8 MI355X"
PEAK_TFLOPS = {"bf16": 2500.0, "f32": 157.3}      # MI355X dense MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def _cpu_quota():
    """CPUs the cgroup grants this process (cpu.max), or None when unlimited/unknown."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else round(int(q) / int(per), 2)
    except (OSError, ValueError):
        return None


def cpu_leg(cfg, budget_s, max_steps=1000):
    """Reference-formula CPU path (oracle/ref_torch.py) on one graph of `cfg` per step:
    2 warm-up steps, then steps for ~budget_s; median and mean step time."""
    import numpy as np
    import torch

    from oracle import ref_torch as T
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.params import init_blocks

    n, lat = cfg.n_nodes, cfg.latent
    b = synthetic_batch(cfg, 1, seed=777)
    eps_rows = 1 if cfg.topology == "tref" else n
    eps = np.random.default_rng(0).standard_normal((eps_rows, lat))
    tensors = T.to_tensors(([b.dense_adj(0)], b.features, b.feature_truth, b.spatial_truth, eps),
                           cfg, torch.float32)
    p = T.build_params(init_blocks(cfg, 0), torch.float32)
    opt = T.TF1Adam(p, cfg.learning_rate)

    def step():
        cost, _ = T.loss_fn(p, *tensors, cfg)
        cost.backward()
        opt.step()

    t0 = time.perf_counter()
    for i in range(2):                      # warm-up (allocations), BASELINE.md
        step()
        log(f"  cpu warm-up step {i + 1} (N={n}) done")
    first = (time.perf_counter() - t0) / 2
    times = []
    t0 = time.perf_counter()
    while len(times) < max_steps and (len(times) < 5 or time.perf_counter() - t0 + first < budget_s):
        t1 = time.perf_counter()
        step()
        times.append(time.perf_counter() - t1)
        log(f"  cpu step {len(times)}: {1000 * times[-1]:.1f} ms")
    med = float(np.median(times))
    return {"graphs_per_s": round(1.0 / med, 4), "ms_per_graph_median": round(1000 * med, 3),
            "ms_per_graph_mean": round(1000 * float(np.mean(times)), 3), "steps": len(times)}


def cpu_baseline(n_nodes, latent, budget_s):
    """The reference-formula CPU path on a bounded sample, threads =
    len(os.sched_getaffinity(0)): C2 (the headline's N, d) and C1."""
    import torch

    from snd_vae_amd.config import PRESETS, tscale
    affinity = len(os.sched_getaffinity(0))
    quota = _cpu_quota()
    # threads = len(os.sched_getaffinity(0)) -- capped by the cgroup's CPU
    # quota when one is set (the CPUs this process may actually run on at once)
    cores = min(affinity, max(1, int(quota + 0.5))) if quota else affinity
    torch.set_num_threads(cores)
    c2 = cpu_leg(tscale(n_nodes, latent), budget_s)
    c1 = cpu_leg(PRESETS["C1"], min(budget_s, 5.0))
    return {"value": c2["graphs_per_s"], "unit": "graphs/s", "cores": cores, "kind": "port",
            "affinity_cpus": affinity, "cgroup_cpu_quota": quota,
            "sample": f"{c2['steps']} train steps x 1 graph (N={n_nodes}, d={latent}) after 2 warm-up, "
                      "median step; reference-formula CPU path (TF unavailable): torch-CPU fp32, dense "
                      "A@(XW), [N,N,2] logits + softmax-CE, autograd, TF1 Adam",
            "ms_per_graph": c2["ms_per_graph_median"], "C2": c2,
            "C1": dict(c1, config="N=200, d=16, graph latent (tref), F_in=1")}


def load_traffic(n, d, B, dtype):
    """HBM bytes per zz^T launch from the newest committed rocprofv3 PMC summary, if any."""
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_zzt*.json")), reverse=True):
        try:
            j = json.load(open(f))
        except Exception:
            continue
        if (j.get("n_nodes"), j.get("latent"), j.get("graphs"), j.get("dtype")) == (n, d, B, dtype):
            return j.get("hbm_bytes_per_launch")
    return None


def load_spmm_traffic(kern, nnz):
    """HBM bytes per window-SpMM launch (FETCH x2 + WRITE) from the committed rocprofv3
    PMC summary of the same batch, if any (profiles/*pmc_spmm_win*.json)."""
    if not kern.startswith("csr_spmm_bf16_window"):
        return None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_spmm_win.json")), reverse=True):
        try:
            j = json.load(open(f))
        except Exception:
            continue
        if f"{nnz} nnz" in j.get("workload", ""):
            return j.get("hbm_bytes_per_launch")
    return None


def run_workload(cfg, B, args, info, steps=None, warmup=None, dtype=None, reset_state=False,
                 options=None):
    """Build B graphs per GPU, capture one full step in a HIP graph, time `steps` replays.

    reset_state: every timed replay starts from the initial state (parameters, Adam
    moments, step counter copied back on the stream before the replay; the replay
    alone is timed by HIP events around it), i.e. each timed step is step 1.  For C4, whose
    reference dynamics overflow within a few steps at N = 4096: the
    timed steps then run on finite losses, the kernels' common path."""
    import torch

    from snd_vae_amd.data import default_tile_rows, synthetic_batch
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    from snd_vae_amd.optimizer import OptimizerVAE
    from snd_vae_amd.parallel import max_over_ranks
    steps = args.steps if steps is None else steps
    warmup = args.warmup if warmup is None else warmup
    log(f"[rank {info.rank}] building {B} RGG graphs N={cfg.n_nodes} ({cfg.topology}, node_h "
        f"{cfg.node_h_size}, latent {cfg.latent})")
    host = synthetic_batch(cfg, B, seed=1000 + info.rank * B)
    db = DeviceBatch(host, tile_rows=0 if args.no_tiles else default_tile_rows(cfg.g_conv_hidden[1]))
    model = SGCNModelVAE(cfg, B, dtype=args.dtype if dtype is None else dtype)
    for k, v in (options or {}).items():
        if not model.set_option(k, v) and v > 0:
            log(f"[rank {info.rank}] plan option {k}={v} not in effect for this plan")
    opt = OptimizerVAE(model, process_group=info.group,
                       bucketed=bool(getattr(args, "buckets", False)))
    if reset_state:
        state = [t.clone() for t in (model.params, opt.m, opt.v, opt.step_counter)]
    opt.step(db)          # first step (counts as warm-up): the ELBO of the initial weights
    torch.cuda.synchronize()
    opt.first_losses = {k: round(v, 6) for k, v in opt.loss_dict().items()}
    if args.no_graph:
        run = lambda: opt.step(db)
    else:
        opt.capture(db, warmup=2)
        run = opt.replay
    _LIVE.append((model, opt, db))
    if reset_state:
        def restore():
            for dst, src in zip((model.params, opt.m, opt.v, opt.step_counter), state):
                dst.copy_(src, non_blocking=True)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(steps)]
        for _ in range(warmup):
            restore()
            run()
        for e0, e1 in ev:
            restore()          # ~the parameter bytes of copies: the replay is queued behind them
            e0.record()
            run()
            e1.record()
        torch.cuda.synchronize()
        dt = sum(e0.elapsed_time(e1) for e0, e1 in ev) / 1000.0
        dt = max_over_ranks(dt, info, device=f"cuda:{info.local_rank}")
        log(f"[rank {info.rank}] state-reset timing done, loss terms {opt.loss_dict()}")
        return B * info.world * steps / dt, 1000.0 * dt / steps, model, opt, db, host
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    log(f"[rank {info.rank}] warm-up done, loss terms {opt.loss_dict()}")

    def barrier():
        if info.group is not None:
            import torch.distributed as dist
            dist.barrier()

    # the timed K steps: wall clock between barrier + synchronize on both sides
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    barrier()
    dev = f"cuda:{info.local_rank}"
    dt = max_over_ranks(time.perf_counter() - t0, info, device=dev)
    # then K more steps with HIP events around every replay on the stream they run on
    # (the median step; event records between replays cost wall time, so
    # they stay out of the wall-clock pass)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(steps)]
    for e0, e1 in ev:
        e0.record()
        run()
        e1.record()
    torch.cuda.synchronize()
    per = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    med = max_over_ranks(per[len(per) // 2] if len(per) % 2 else 0.5 * (per[len(per) // 2 - 1] + per[len(per) // 2]),
                         info, device=dev)
    TIMING.update(ms_step_median_events=round(med, 5), ms_step_wall_mean=round(1000.0 * dt / steps, 5),
                  ms_step_min_events=round(per[0], 5), ms_step_max_events=round(per[-1], 5))
    return B * info.world * steps / dt, med, model, opt, db, host


TIMING = {}


_LIVE = []


def del_models():
    import torch
    _LIVE.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def time_launches(launch, reps):
    """ms per launch: `reps` launches captured in one HIP graph (times the GPU, not the
    host launch path), replayed between HIP events recorded on the stream the kernels
    run on; the best of 3 rounds of 3 replays after 3 warm replays (the first
    measurement of a process otherwise reads high while the clocks ramp up).
    launch(stream_ptr) enqueues one launch."""
    import torch

    from snd_vae_amd import _lib
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        launch(_lib.stream_ptr(side))
        with torch.cuda.graph(g, stream=side):
            for _ in range(reps):
                launch(_lib.stream_ptr(side))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(3)]
    with torch.cuda.stream(side):      # warm replays (clocks up) + 3 timed rounds, all on `side`
        for _ in range(3):
            g.replay()
        for e0, e1 in ev:
            e0.record(side)
            for _ in range(3):
                g.replay()
            e1.record(side)
    ev[-1][1].synchronize()
    torch.cuda.current_stream().wait_stream(side)
    return min(e0.elapsed_time(e1) for e0, e1 in ev) / (3 * reps)


def allreduce_cost_ms(numel, reps=20):
    """One RCCL all-reduce of `numel` floats in a world-1 group initialised in this
    process, timed eagerly between HIP events on the current stream (the collective's
    launch and local cost; at world 1 RCCL moves no data over xGMI, and a HIP-graph
    capture of it records an empty graph)."""
    import socket

    import torch
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", torch.cuda.current_device()))
    try:
        t = torch.zeros(numel, dtype=torch.float32, device="cuda")
        for _ in range(3):
            dist.all_reduce(t)
        torch.cuda.synchronize()
        best = None
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                dist.all_reduce(t)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / reps
            best = ms if best is None else min(best, ms)
        return best
    finally:
        dist.destroy_process_group()


def kernel_timer(model, bc, reps):
    """ms per launch of one kernel of the plan (snd_plan_launch) on the step's workspace."""
    from snd_vae_amd import _lib
    L = _lib.lib()

    def kernel_ms(name):   # "a+b": the plan kernels a and b back to back, per launch pair
        def launch(sp):
            for part in name.split("+"):
                _lib.check(L.snd_plan_launch(model.plan, bc, model.workspace.data_ptr(), part.encode(), sp))
        return time_launches(launch, reps)

    return kernel_ms


def kernel_timer_rot(replicas, reps):
    """ms per launch of one plan kernel rotated over distinct replicas (model, batch
    struct): each launch streams another replica's weights, so with >= 3 replicas of
    the 114-237 MB weight streams no launch finds its bytes in the 256 MB Infinity
    Cache (MALL) -- the honest HBM time of an in-step launch."""
    from snd_vae_amd import _lib
    L = _lib.lib()

    def kernel_ms(name):
        def launch(sp):
            for model, bc in replicas:
                _lib.check(L.snd_plan_launch(model.plan, bc, model.workspace.data_ptr(),
                                             name.encode(), sp))
        return time_launches(launch, reps) / len(replicas)

    return kernel_ms


def spmm_batched(host, width, copies, reps):
    """The bf16 SpMM on `copies` x the bench batch stacked block-diagonally (8 x copies
    graphs): a working set above the 256 MB Infinity Cache, so the HBM fraction is not
    a cache artefact.  Headline: the sliding-window kernel
    (snd_csr_spmm_bf16_window, every h row DMA'd once into an LDS ring);
    previous_variant: the row-tile kernel (snd_csr_spmm_bf16_tiled) and, under it, the
    register-gather kernel (snd_csr_spmm_bf16) on the same input."""
    import ctypes

    import numpy as np
    import torch

    from snd_vae_amd import _lib
    from snd_vae_amd.data import GraphBatch, default_tile_rows, locality_order, row_tiles
    rp0, ci0 = host.rowptr.astype(np.int64), host.colidx.astype(np.int64)
    nnz0, R0 = int(rp0[-1]), host.n_graphs * host.n_nodes
    rp = np.concatenate([rp0[:-1] + c * nnz0 for c in range(copies)] + [np.array([copies * nnz0])])
    ci = np.concatenate([ci0 + c * R0 for c in range(copies)])
    o0 = locality_order(host).astype(np.int64)
    order = np.concatenate([o0 + c * R0 for c in range(copies)])
    R = R0 * copies
    z = np.zeros((1, 1), np.float32)
    big = GraphBatch(host.n_graphs * copies, host.n_nodes, rp.astype(np.int32), ci.astype(np.int32), z, z, z)
    tr = default_tile_rows(width)
    from snd_vae_amd.model import DeviceTiles
    rt = row_tiles(big, order.astype(np.int32), tr)
    dt = DeviceTiles(rt)
    d_rp = torch.from_numpy(rp.astype(np.int32)).cuda()
    d_ci = torch.from_numpy(ci.astype(np.int32)).cuda()
    d_order = torch.from_numpy(order.astype(np.int32)).cuda()
    tiles = dt.c_struct()
    h = torch.randn(R, width, device="cuda").to(torch.bfloat16)
    out = torch.empty_like(h)
    L = _lib.lib()
    ng = host.n_graphs * copies
    ms_tiled = time_launches(lambda sp: _lib.check(L.snd_csr_spmm_bf16_tiled(
        d_rp.data_ptr(), d_ci.data_ptr(), R, ctypes.byref(tiles), h.data_ptr(), width, width,
        out.data_ptr(), width, host.n_nodes, ng, d_order.data_ptr(), sp)), reps)
    ms_reg = time_launches(lambda sp: _lib.check(L.snd_csr_spmm_bf16(
        d_rp.data_ptr(), d_ci.data_ptr(), R, h.data_ptr(), width, width, out.data_ptr(), width,
        host.n_nodes, ng, d_order.data_ptr(), sp)), reps)
    byts = 4 * (R + 1) + 4 * len(ci) + 2 * 2 * R * width
    frac = lambda t: round(byts / (t * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)
    tiled = {"kernel": f"csr_spmm_bf16_tiled ({tr}-row tiles, sets <= {rt.ustride} rows)",
             "avg_launch_ms": round(ms_tiled, 5), "frac": frac(ms_tiled)}
    reg = {"kernel": "csr_spmm_bf16 (register gathers)", "avg_launch_ms": round(ms_reg, 5),
           "frac": frac(ms_reg)}
    # headline: the sliding-window kernel (h rows DMA'd once into an LDS ring) when the
    # schedule's bandwidth fits its ring, else the row-tile kernel
    from snd_vae_amd.data import window_plan
    from snd_vae_amd.layers import DeviceWindowPlan
    wp = window_plan(big, order.astype(np.int32))
    if (wp.beta + 7) // 8 * 8 <= 352 and width == 64:
        dw = DeviceWindowPlan(wp)
        ms = time_launches(lambda sp: _lib.check(L.snd_csr_spmm_bf16_window(
            dw.meta.data_ptr(), dw.slots.data_ptr(), dw.rows.data_ptr(), dw.order.data_ptr(), R, host.n_nodes, ng, wp.beta,
            h.data_ptr(), width, width, out.data_ptr(), width, sp)), reps)
        kern = (f"csr_spmm_bf16_window (A @ H, width {width}, {ng} graphs block-diagonal, {len(ci)} nnz, "
                f"RCM schedule, beta {wp.beta}, 1096-row LDS ring; the kernel snd_train_step launches "
                f"for the GraphConvolution backward A @ dP1)")
        prev = dict(tiled, previous_variant=reg)
    else:
        ms, kern, prev = ms_tiled, "csr_spmm_bf16_tiled (A @ H, width %d, %d graphs)" % (width, ng), reg
    gbs = byts / (ms * 1e-3) / 1e9
    return {"kernel": kern, "bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": round(gbs / PEAK_HBM_GBS, 4), "avg_launch_ms": round(ms, 5),
            "bytes_per_launch": byts, "traffic": load_spmm_traffic(kern, len(ci)), "previous_variant": prev}


def extra_workload(name, args, info):
    """Time another BASELINE config (C4: graph latent + model_joint decoders; C5: the
    N=16384 d=128 zz^T stress) with its dominant kernels' rooflines."""
    from snd_vae_amd.config import PRESETS
    cfg = PRESETS[name]
    B = {"C4": args.graphs_per_gpu, "C5": 1}[name]
    steps = max(5, args.steps // 5)
    value, ms, model, opt, db, host = run_workload(cfg, B, args, info, steps=steps,
                                                   warmup=min(args.warmup, 5),
                                                   reset_state=cfg.topology == "tref")
    kms = kernel_timer(model, db.c_struct(), max(4, args.kernel_reps // 4))
    N, dj = cfg.n_nodes, cfg.node_h_size
    res = {"value": round(value, 3), "unit": "graphs/s", "ms_per_step": round(ms, 4),
           "graphs_per_gpu": B, "steps": steps, "n_nodes": N, "node_h": dj,
           "topology": cfg.topology, "param_count": model.param_count,
           "losses_first_step": opt.first_losses,
           "losses": {k: round(v, 6) for k, v in opt.loss_dict().items()}}
    if cfg.topology == "tref":
        res["timing"] = ("STEP-1, RESET-STATE: each timed HIP-graph replay is step 1: it starts "
                         "from the initial state (params, Adam moments, step counter copied back "
                         "outside the HIP events), so the timed steps run on finite losses; "
                         "steady_state below times consecutive steps")
        res["losses_note"] = ("reference dynamics: TF1 Adam (lr 1e-3) moves all N*W = "
                              f"{cfg.n_nodes * cfg.enc_width} fan-in weights of the graph-latent head by ~lr per step, "
                              "so h and logstd grow by O(100) per step and the KL overflows within a few "
                              "steps at N = 4096 (the reference model was built for N ~ 25); 'losses' is "
                              "the last timed step (step 1 again, from the reset state)")
    if cfg.topology == "tref":
        # a short steady-state run from where the timed steps left off (no reset): the
        # reference dynamics overflow here, which times the overflow path
        import torch
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(steps)]
        for e0, e1 in ev:
            e0.record()
            opt.replay()
            e1.record()
        torch.cuda.synchronize()
        per = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        res["steady_state"] = {"ms_per_step_median": round(per[len(per) // 2], 4),
                               "steps": steps, "losses": {k: round(v, 6) for k, v in opt.loss_dict().items()},
                               "note": "consecutive replays without the state reset (steps 2.., "
                                       "the overflowing dynamics of DESIGN §2)"}
    kern = {}
    zms = kms("zzt_dense")
    zfl = 4.0 * N * N * dj * B
    kern["zzt_dense"] = {"bound": "mfma", "avg_launch_ms": round(zms, 5), "flops_per_launch": zfl,
                         "achieved": round(zfl / (zms * 1e-3) / 1e12, 2), "peak": PEAK_TFLOPS[args.dtype],
                         "unit": "TFLOP/s", "frac": round(zfl / (zms * 1e-3) / 1e12 / PEAK_TFLOPS[args.dtype], 4)}
    if cfg.topology == "tref":
        W = cfg.enc_width
        K, gh, L, Cp = N * W, cfg.g_hidden_size, cfg.latent, N * dj
        # algorithmic bytes: weight read (+ weight-gradient write) + activations in / out
        units = {"tref_head_fwd": 4 * (K * gh + B * K),
                 "tref_head_bwd": 4 * (2 * K * gh + 2 * B * K + B * gh),
                 "tref_proj_fwd": 4 * (L * Cp + Cp + B * Cp + B * L),
                 "tref_proj_bwd": 4 * (2 * L * Cp + Cp + 3 * B * Cp + B * L)}
        # MALL-proof: two more replicas (own weights, workspace, batch), launches rotated
        # over the three, so every launch streams weights the previous two evicted
        from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
        from snd_vae_amd.optimizer import OptimizerVAE
        reps_ = [(model, db.c_struct())]
        for r in range(2):
            m2 = SGCNModelVAE(cfg, B, dtype=args.dtype)
            o2 = OptimizerVAE(m2)
            d2 = DeviceBatch(host)
            o2.step(d2)
            _LIVE.append((m2, o2, d2))
            reps_.append((m2, d2.c_struct()))
        krot = kernel_timer_rot(reps_, max(4, args.kernel_reps // 4))
        for k, byts in units.items():
            t = krot(k)
            tc = kms(k)
            kern[k] = {"bound": "hbm", "avg_launch_ms": round(t, 5), "bytes_per_launch": byts,
                       "timing": "rotated over 3 replicas' weights (>= 342 MB per kernel "
                                 "stream: not Infinity-Cache resident)",
                       "same_weights_back_to_back_ms": round(tc, 5),
                       "achieved": round(byts / (t * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS,
                       "unit": "GB/s", "frac": round(byts / (t * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)}
    res["kernels"] = kern
    log(f"[{name}] {value:.1f} graphs/s, {ms:.3f} ms/step, kernels {kern}")
    return res


def rooflines(args, cfg, model, db, host):
    """--full: the dominant kernels of the headline step, each timed in runs of its own
    (time_launches) on the step's workspace: `roofline` (fused zz^T + CE) and
    `secondary_roofline` (the SpMM)."""
    B, N, d = args.graphs_per_gpu, args.nodes, args.latent
    bc = db.c_struct()
    kernel_ms = kernel_timer(model, bc, args.kernel_reps)

    # ---- dominant kernel: fused zz^T + CE, HIP events on the launch stream
    zzt_ms = kernel_ms("zzt_dense")
    zzt_v1_ms = kernel_ms("zzt_dense_v1") if args.dtype == "bf16" else None
    fast = args.dtype == "bf16"
    spmm_ms = kernel_ms("spmm_bf16" if fast else "spmm_dxw1")
    spmm_tiled_ms = kernel_ms("spmm_bf16_tiled") if fast and db.tiles else None
    flops = 4.0 * N * N * d * B                       # 2N^2 d fwd + 2N^2 d bwd per graph
    achieved = flops / (zzt_ms * 1e-3) / 1e12
    peak = PEAK_TFLOPS[args.dtype]
    h1 = cfg.g_conv_hidden[1]
    # SURVEY 8d SpMM units: rowptr + colidx + feature rows in + out (bf16 on the fast path)
    fb = 2 if fast else 4
    spmm_bytes = 4 * (B * N + 1) + 4 * host.nnz + 2 * fb * B * N * h1
    spmm_gbs = spmm_bytes / (spmm_ms * 1e-3) / 1e9

    return {
        "roofline": {"kernel": "zzt_dense (fused z z^T + CE fwd+bwd; " +
                               ("zzt_dense_bf16_v9: two 512-thread workgroups per CU" if fast and d <= 64 and d > 32
                                else "zzt_dense_bf16_v7" if fast and d > 64 else "v4 / fp32") + ")",
                     "bound": "mfma",
                     "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                     "frac": round(achieved / peak, 4),
                     "traffic": load_traffic(N, d, B, args.dtype),
                     "avg_launch_ms": round(zzt_ms, 5), "flops_per_launch": flops,
                     "previous_variant_ms": None if zzt_v1_ms is None else round(zzt_v1_ms, 5)},
        "secondary_roofline": dict(
            spmm_batched(host, h1, args.spmm_copies, max(4, args.kernel_reps // 2)) if fast else {},
            in_step={"kernel": f"csr_spmm (A @ dP1, width {h1}, {'bf16' if fast else 'fp32'}, "
                               f"{B} graphs, "
                               f"{'window' if fast and db.window else ('row tiles' if fast and db.tiles else 'register gathers')})",
                     "achieved": round(spmm_gbs, 1), "frac": round(spmm_gbs / PEAK_HBM_GBS, 4),
                     "avg_launch_ms": round(spmm_ms, 5), "bytes_per_launch": spmm_bytes,
                     "row_tiles_ms": None if spmm_tiled_ms is None else round(spmm_tiled_ms, 5),
                     "note": "8 graphs: a 4 MB working set, L2-resident; the HBM fraction is the 256-graph line"}),
    }


DUMP_BYTES = 64 << 20      # --dump-outputs: at most this much in all


def dump_outputs(path, model, opt):
    """What the step just run left its caller, as path/<name>.npy: the loss terms
    (float64, optimizer.LOSS_NAMES order) and the flat parameters, gradient and Adam
    moments (float32, params.flat_layout order).  An array above its share of
    DUMP_BYTES is written as a fixed sample: the elements at the sorted indices
    numpy's default_rng(0) draws for its size."""
    import numpy as np
    pc = model.param_count
    arrays = {"losses": opt.losses, "params": model.params[:pc], "grads": opt.grads[:pc],
              "adam_m": opt.m[:pc], "adam_v": opt.v[:pc]}
    share = DUMP_BYTES // len(arrays)
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32, copy=False)
        if a.nbytes > share:
            a = a[np.sort(np.random.default_rng(0).integers(0, a.size, share // a.itemsize))]
        np.save(os.path.join(path, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--graphs-per-gpu", type=int, default=8)
    ap.add_argument("--nodes", type=int, default=4096)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: kernel rooflines, fp32 and one-graph modes, batch "
                         "sweep, the C4 / C5 workloads and the CPU baseline (each takes runs of "
                         "its own; the options below them apply with --full only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed (loss terms, "
                         "parameters, gradient, Adam moments) as DIR/<name>.npy")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of HIP graph")
    ap.add_argument("--no-tiles", action="store_true", help="register-gather SpMM instead of LDS row tiles")
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--cpu-baseline-seconds", type=float, default=20.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--force-dist", action="store_true",
                    help="under torchrun with one rank: init RCCL and run the gradient all-reduce "
                         "(the N>1 step, captured in the HIP graph) anyway")
    ap.add_argument("--buckets", action="store_true",
                    help="data parallel: the bucketed exchange (opt-in; verified at world 1 "
                         "and on gloo only) instead of one all-reduce + one Adam pass")
    ap.add_argument("--spmm-copies", type=int, default=32,
                    help="secondary roofline: SpMM over this many copies of the batch (8 x 32 graphs)")
    ap.add_argument("--batch-sweep", default="16,32",
                    help="extra per-GPU batch sizes timed after the headline (1 GPU only)")
    ap.add_argument("--no-modes", action="store_true",
                    help="skip the fp32-mode and 1-graph (C3 per-rank) step timings")
    ap.add_argument("--extra", default="C4,C5",
                    help="other BASELINE configs timed after the headline (1 GPU only): C4,C5")
    args = ap.parse_args()

    import torch

    from snd_vae_amd.config import tscale
    from snd_vae_amd.parallel import init_from_env

    info = init_from_env("nccl", force=args.force_dist)
    if info.world != args.gpus:
        log(f"warning: --gpus {args.gpus} but WORLD_SIZE {info.world}")
    torch.cuda.set_device(info.local_rank)
    B, N, d = args.graphs_per_gpu, args.nodes, args.latent
    cfg = tscale(N, d)
    value, ms, model, opt, db, host = run_workload(cfg, B, args, info)
    timing = dict(TIMING)
    losses = opt.loss_dict(global_mean=True)
    log(f"[rank {info.rank}] {value:.1f} graphs/s, {ms:.3f} ms/step")
    if args.dump_outputs and info.rank == 0:
        dump_outputs(args.dump_outputs, model, opt)

    out = {
        "metric": METRIC,
        "value": round(value, 3),
        "unit": "graphs/s",
        "n_gpus": info.world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms, 4),
        "elbo_step_ms": round(ms, 4),
        "ms_per_step_wall_mean": timing.get("ms_step_wall_mean"),
        "timing": dict(timing, method="value = graphs over the barrier-bracketed wall clock of the K "
                                      "timed steps; ms_per_step = median over K further steps of "
                                      "HIP-event pairs around each graph replay (max over ranks)"),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.dtype,
        "data": "synthetic random-geometric graphs (U[0,1)^2 nodes, r=sqrt(16/(pi N))), random-init weights",
        "config": {"workload": f"C2: node-latent SND-VAE train step, N={N}, d={d}, "
                               f"{B} graphs/GPU, HIP-graph replay",
                   "n_nodes": N, "latent": d, "graphs_per_gpu": B, "global_batch": B * info.world,
                   "nnz_per_graph": round(host.nnz / B, 1), "parallelism": f"dp{info.world}",
                   "hip_graph": not args.no_graph},
        "losses": {k: round(v, 6) for k, v in losses.items()},
    }
    from snd_vae_amd.build import lib_status
    out["build"] = lib_status()
    if args.full:
        out.update(rooflines(args, cfg, model, db, host))
    if args.full and info.world == 1 and not args.no_modes:
        # the same step in the fp32 parity mode (generic engine), and C3's per-rank work:
        # one N=4096 graph per GPU (global batch 8 over 8 GPUs = strong scaling)
        del_models()
        v32, ms32, *_ = run_workload(cfg, B, args, info, steps=max(5, args.steps // 5),
                                     warmup=min(args.warmup, 3), dtype="f32")
        out["fp32_mode"] = {"value": round(v32, 3), "unit": "graphs/s", "ms_per_step": round(ms32, 4),
                            "graphs_per_gpu": B, "note": "the parity mode (fp32 operands, generic engine)"}
        del_models()
        v1, ms1, m1, *_ = run_workload(cfg, 1, args, info, steps=args.steps, warmup=args.warmup,
                                       options={"conc_decoder": 0})
        out["strong"] = {"workload": "C3 per rank: 1 graph (N=4096, d=64) per GPU, bf16, HIP-graph replay; "
                                     "serial (conc_decoder 0) here, the default concurrent decoder below",
                         "graphs_per_gpu": 1, "value": round(v1, 3), "unit": "graphs/s",
                         "ms_per_step": round(ms1, 4), "timing": dict(TIMING)}
        del_models()
        # the same one-graph step with the fused decoder on a side stream beside zz^T
        # (snd_plan_set_option "conc_decoder"): at one graph neither kernel fills the chip
        v1c, ms1c, *_ = run_workload(cfg, 1, args, info, steps=args.steps, warmup=args.warmup,
                                     options={"conc_decoder": 1})
        out["strong"]["conc_decoder"] = {"value": round(v1c, 3), "ms_per_step": round(ms1c, 4),
                                         "timing": dict(TIMING)}
        try:   # C3 = 8 graphs on 8 ranks: (8-graph step) / (1-graph step + the all-reduce)
            ar = allreduce_cost_ms(m1.param_count + 8)
            out["strong"]["allreduce_world1_ms"] = round(ar, 5)
            out["strong"]["projected_speedup_8"] = round(ms / (min(ms1, ms1c) + ar), 3)
            out["strong"]["projection"] = ("8-graph step on 1 GPU / (faster 1-graph step + one "
                                           "eager world-1 RCCL all-reduce of the gradient): the "
                                           "xGMI transfer of the ~245 KB ring at 8 ranks is not "
                                           "included (unmeasurable on one GPU)")
        except Exception as e:   # no RCCL on this box: report the step alone
            out["strong"]["projected_speedup_8"] = None
            out["strong"]["projection_error"] = repr(e)[:200]
        del_models()
        # the same step at larger per-GPU batches (the headline stays at 8 graphs per GPU,
        # C3's global batch per rank count): how far the machine is from filled at 8
        out["batch_sweep"] = {}
        for bs in [int(t) for t in args.batch_sweep.split(",") if t]:
            vb, msb, *_ = run_workload(cfg, bs, args, info, steps=max(5, args.steps // 2),
                                       warmup=min(args.warmup, 5))
            out["batch_sweep"][str(bs)] = {"value": round(vb, 3), "unit": "graphs/s", "ms_per_step": round(msb, 4)}
            del_models()
    extra = [w for w in args.extra.split(",") if w] if args.full and info.world == 1 else []
    if extra:
        out["workloads"] = {}
        for w in extra:
            out["workloads"][w] = extra_workload(w, args, info)
            del_models()
    if args.full and info.rank == 0 and info.world == 1 and not args.no_cpu_baseline:
        log("cpu baseline ...")
        out["cpu_baseline"] = cpu_baseline(N, d, args.cpu_baseline_seconds)
    if info.rank == 0:
        print(json.dumps(out), flush=True)
    if info.group is not None:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
