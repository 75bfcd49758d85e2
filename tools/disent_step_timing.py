"""Time one training step of the disentangled model at the reference's scale: the synthetic2
widths (``DisentangledConfig()``), N = 25, S = 10 spanning trees, B = 10 graphs
(`main.py:100,173-217`), a seeded ``sgjoint_batch``.

Routes, each on its own model built from the same blocks, each step drawing its normals
with ``disent_trainer.draw_step_eps`` first (every training loop has to):

* ``eager``:        ``model.step()``, which reads its loss terms back in six places -- the
                    only route before ``step_device``; the host stalls are part of its cost;
* ``eager_device``: ``model.step_device()``, the same launches without a read-back;
* ``replay``:       one replay of the HIP graph captured from ``step_device`` (what
                    ``DisentTrainer`` does with ``use_graphs``).

All routes are warmed, then run in alternating blocks of ``--steps`` steps; the wall clock
is taken around each block, which ends in a device synchronise, and divided by the steps.
For ``replay`` HIP events around every replay give the device-side time as well.  Medians
with the min-max spread over the blocks.  ``--route NAME`` runs one route alone (for a
kernel trace: ``rocprofv3 --kernel-trace --stats -- python tools/disent_step_timing.py
--route replay``).  ``--e2e-engine factorised`` times the model with the factorised training
structure decoder (``snd_e2e_train``); ``--e2e-engine both`` alternates every route under
both engines in one process (names ``route:engine``).

    python tools/disent_step_timing.py --out profiles/disent_step_timing.json
    python tools/disent_step_timing.py --e2e-engine both --out profiles/disent_step_timing_engines.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

N, S, B = 25, 10, 10
ROUTES = ("eager", "eager_device", "replay")


def stats(v):
    v = sorted(v)
    return {"median_us": statistics.median(v), "min_us": v[0], "max_us": v[-1], "n": len(v)}


class Route:
    def __init__(self, name, cfg, blocks, batch, seed, engine="direct", label=None):
        from snd_vae_amd.disent_model import DisentangledSGCNModelVAE
        from snd_vae_amd.disent_trainer import eps_shapes
        self.name, self.seed, self.t, self.batch = name, seed, 0, batch
        self.engine, self.label = engine, label or name
        self.model = DisentangledSGCNModelVAE(cfg, B, blocks=blocks, e2e_engine=engine)
        self.eps = {k: torch.empty(*s, device="cuda") for k, s in eps_shapes(cfg, B).items()}
        self.graph, self.events = None, []
        if name == "replay":
            from snd_vae_amd.disent_trainer import draw_step_eps
            m = self.model
            state = (m.params, m.m, m.v, m.step_counter, m.grads, m.losses)
            saved = [x.clone() for x in state]
            draw_step_eps(seed, 0, self.eps)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                m.step_device(batch, self.eps)                      # the layers' workspaces
            torch.cuda.current_stream().wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                m.step_device(batch, self.eps)
            torch.cuda.synchronize()
            for dst, src in zip(state, saved):                      # the warm-up step is not counted
                dst.copy_(src)

    def step(self, events=False):
        from snd_vae_amd.disent_trainer import draw_step_eps
        draw_step_eps(self.seed, self.t, self.eps)
        self.t += 1
        if self.name == "eager":
            self.model.step(self.batch, self.eps)
        elif self.name == "eager_device":
            self.model.step_device(self.batch, self.eps)
        elif events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            self.graph.replay()
            b.record()
            self.events.append((a, b))
        else:
            self.graph.replay()

    def block(self, steps, events=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step(events)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e6              # microseconds per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=ROUTES, default=None, help="one route alone (kernel traces)")
    ap.add_argument("--steps", type=int, default=20, help="steps per block")
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per route")
    ap.add_argument("--warmup", type=int, default=2, help="untimed blocks per route")
    ap.add_argument("--e2e-engine", choices=("direct", "factorised", "both"), default="direct",
                    help="the training structure decoder of the timed model")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("disent_step_timing: needs a ROCm GPU (there is nothing to time without one)")
    from snd_vae_amd.config import sgjoint
    from snd_vae_amd.data import sgjoint_batch
    from snd_vae_amd.disent_model import LOSS_NAMES, DeviceDisentBatch, DisentangledConfig, init_blocks
    cfg = DisentangledConfig()
    assert (cfg.n_nodes, cfg.sampling_num) == (N, S)
    batch = DeviceDisentBatch(sgjoint_batch(sgjoint(N, cfg.node_h, mean_degree=4.0, sampling_num=S), B, seed=3))
    blocks = init_blocks(cfg, 0)
    engines = ("direct", "factorised") if a.e2e_engine == "both" else (a.e2e_engine,)
    routes = [Route(r, cfg, blocks, batch, seed=1234, engine=e, label=r if a.e2e_engine == "direct" else f"{r}:{e}")
              for r in (ROUTES if a.route is None else (a.route,)) for e in engines]
    for _ in range(a.warmup):
        for r in routes:
            r.block(a.steps)
    wall = {r.label: [] for r in routes}
    for _ in range(a.blocks):
        for r in routes:                                             # alternating
            wall[r.label].append(r.block(a.steps, events=True))
    res = {"shape": {"n_nodes": N, "sampling_num": S, "n_graphs": B, "model_type": cfg.model_type,
                     "param_count": routes[0].model.param_count},
           "steps_per_block": a.steps, "blocks": a.blocks, "device": torch.cuda.get_device_name(0),
           "wall_us_per_step": {k: stats(v) for k, v in wall.items()}}
    for r in routes:
        if r.events:
            key = "replay_event_us" if a.e2e_engine == "direct" else f"replay_event_us:{r.engine}"
            res[key] = stats([x.elapsed_time(y) * 1e3 for x, y in r.events])
    # the device routes took the same steps from the same blocks and normals: the same last loss
    # (per engine: the two engines sum in different orders)
    res["last_cost"] = {r.label: float(r.model.losses[LOSS_NAMES.index("cost")]) for r in routes
                        if r.name != "eager"}
    for e in engines:
        same = {v for r, v in zip(routes, [res["last_cost"].get(r.label) for r in routes])
                if r.engine == e and r.name != "eager"}
        assert len(same) <= 1, res["last_cost"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
