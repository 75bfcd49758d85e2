"""snd_graph_paths (components, hop distances, detour) on the GPU, through the raw entry point on
the guarded buffers of tests/abi_ops.py: every operand, every output and the workspace of exactly
the queried bytes sits between NaN-pattern guards, and outputs start at the pattern, so a store
outside an output or a missed store shows.

comp, hops_out, the hop histogram and totals are compared exactly with tests/graph_paths_ref.py;
route_out within the derived bound (K + 6) 2^-23 route64 per element, inf exactly where
unreachable; the detour histogram under the envelope rule, whose condition (at most 1 % of a
case's pairs ambiguous) ``reference`` asserts on the CPU before any launch.  Then the layers,
model and trainer levels at N = 25.
"""
import numpy as np
import pytest
import torch

import abi_ops as A
import graph_paths_ref as P
import graph_stats_ref as G

pytestmark = pytest.mark.gpu

I64_PAT = np.uint64(A.PATTERN["f64"][2]).astype(np.int64)       # int64 outputs ride in 8-byte "f64" buffers
I32_PAT = np.int32(A.PATTERN["i32"][2])
F32_PAT = np.uint32(A.PATTERN["f32"][2])
ERR_ARG = -1
SCALE = P.DETOUR_SCALE


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def run_raw(c, x, step, want=("comp", "hops", "route"), expect_rc=0, override=None):
    """One call on fresh guarded buffers; x None: coords = NULL.  ``want``: the optional outputs
    that are passed (the others are NULL and must keep the pattern).  Returns the outputs after
    the call, with every guard, padding element and input checked."""
    from snd_vae_amd import _lib
    L = _lib.lib()
    R, S = c.B * c.n, len(P.sources(c.n, step))
    cap = len(c.ci)
    bufs = {"rowptr": A.guarded(1, R + 1, None, "i32", 0, c.rp, "rowptr"),
            "colidx": A.guarded(1, cap, None, "i32", 0, c.ci, "colidx"),
            "comp": A.guarded(1, R, None, "i32", 0, None, "comp"),
            "hops": A.guarded(c.B * S, c.n, None, "i32", 0, None, "hops_out"),
            "route": A.guarded(c.B * S, c.n, None, "f32", 0, None, "route_out"),
            "hist": A.guarded(1, c.B * 2 * P.BINS, None, "f64", 0, None, "hist"),
            "totals": A.guarded(1, c.B * 6, None, "f64", 0, None, "totals")}
    sd = 0
    if x is not None:
        sd = x.shape[1]
        bufs["coords"] = A.guarded(R, sd, sd + 3, "f32", 1, x, "coords")      # base 4 bytes off 16
    wsb = L.snd_graph_paths_workspace(c.B, c.n, cap, int(x is not None))
    assert wsb % 4 == 0 and (wsb >= cap * 4 if x is not None else wsb == 0)
    bufs["ws"] = A.guarded(1, max(wsb // 4, 4), None, "f32", 0, None, "workspace")   # exactly the queried bytes
    dev = {k: torch.from_numpy(g.arr).cuda() for k, g in bufs.items()}
    ptr = {k: dev[k].data_ptr() + g.off * g.arr.itemsize for k, g in bufs.items()}
    args = dict(rowptr=ptr["rowptr"], colidx=ptr["colidx"], nnz_cap=cap, n_graphs=c.B, n=c.n,
                coords=ptr.get("coords"), ldc=0 if x is None else sd + 3, sd=sd, detour_scale=float(SCALE),
                src_step=step, comp=ptr["comp"] if "comp" in want else None,
                hops_out=ptr["hops"] if "hops" in want else None,
                route_out=ptr["route"] if "route" in want and x is not None else None,
                hist=ptr["hist"], totals=ptr["totals"], workspace=ptr["ws"] if wsb else None, workspace_bytes=wsb)
    args.update(override or {})
    rc = L.snd_graph_paths(*args.values(), _lib.stream_ptr())
    assert rc == expect_rc, (rc, _lib.last_error())
    err = _lib.last_error() if rc else ""
    torch.cuda.synchronize()
    after = {k: t.cpu().numpy() for k, t in dev.items()}
    for k, g in bufs.items():
        if k != "ws" or not wsb:                                              # the workspace is scratch
            g.check_untouched(after[k])
    if wsb:
        bufs["ws"].check_untouched(_guards_only(bufs["ws"], after["ws"]))
    for k in ("rowptr", "colidx", "coords"):                                  # inputs bitwise intact
        if k in bufs:
            assert np.array_equal(after[k].view(np.uint32), bufs[k].arr.view(np.uint32)), k
    i64 = lambda k: np.ascontiguousarray(bufs[k].block(after[k])).view(np.int64).ravel()
    return {"comp": bufs["comp"].block(after["comp"]).ravel(), "hops": bufs["hops"].block(after["hops"]),
            "route": bufs["route"].block(after["route"]), "hist": i64("hist").reshape(c.B, 2, P.BINS),
            "totals": i64("totals").reshape(c.B, 6), "err": err,
            "raw": {k: after[k] for k in ("comp", "hops", "route", "hist", "totals")}}


def _guards_only(g, after):
    """``after`` with the block itself put back to the pattern: only the guards are checked."""
    a = np.array(after)
    g.block(a).view(np.uint32)[...] = F32_PAT
    return a


def check(c, x, step, out, want=("comp", "hops", "route"), what=""):
    ref = P.reference(c, x, None if x is None else SCALE, step)
    got = {"hist": out["hist"], "totals": out["totals"], "comp": out["comp"] if "comp" in want else None,
           "hops": out["hops"] if "hops" in want else None,
           "route": out["route"] if "route" in want and x is not None else None}
    worst = P.assert_paths(got, ref, c.n, f"{c.name} {what}")
    if "comp" not in want:
        assert (out["comp"] == I32_PAT).all()
    if "hops" not in want:
        assert (out["hops"] == I32_PAT).all()
    if "route" not in want or x is None:
        assert (out["route"].view(np.uint32) == F32_PAT).all()
    if x is None:
        assert not out["hist"][:, 1].any()
    return ref, worst


@pytest.mark.parametrize("name", list(P.CASES))
def test_cases(name):
    """Every case with coords (sd = 2, ldc = 5, base 4 bytes off 16-byte alignment) and with
    coords = NULL; two runs bitwise equal."""
    c, x, step = P.build_case(name)
    refs = [P.reference(c, x, SCALE, step), P.reference(c, None, None, step)]     # the condition, before any launch
    assert refs[0]["ambiguous_share"] <= P.AMBIGUOUS_CAP
    out = run_raw(c, x, step)
    ref, worst = check(c, x, step, out)
    print(f"GPATHS {name} pairs {int(ref['totals'][:, 3].sum())} components {ref['totals'][:, 0].tolist()} "
          f"max_hops {int(ref['totals'][:, 5].max())} ambiguous_share {ref['ambiguous_share']:.2e} "
          f"worst_err_over_bound {worst:.3f}")
    check(c, None, step, run_raw(c, None, step))
    again = run_raw(c, x, step)
    for k, v in out["raw"].items():
        assert np.array_equal(v.view(np.uint8), again["raw"][k].view(np.uint8)), (name, k)


@pytest.mark.parametrize("name,sd", [("b2n70", 1), ("b2n70", 3), ("b3n33", 3)])
def test_other_dimensions(name, sd):
    c, x, step = P.build_case(name, sd)
    P.reference(c, x, SCALE, step)
    check(c, x, step, run_raw(c, x, step), what=f"sd={sd}")


@pytest.mark.parametrize("want", [(), ("comp",), ("hops",), ("route",), ("hops", "route")])
def test_null_optional_outputs(want):
    c, x, step = P.build_case("b2n70")
    check(c, x, step, run_raw(c, x, step, want), want)


def test_source_step():
    c, x, _ = P.build_case("b1n257")
    for step in (2, 16, 256, 257, 1000):
        P.reference(c, x, SCALE, step)
        check(c, x, step, run_raw(c, x, step), what=f"src_step={step}")


def test_rejected_calls_touch_nothing():
    """Every SND_ERR_ARG call returns the code with a message naming the entry point, and all
    buffers (outputs included: they keep the guard pattern) are bitwise intact."""
    c, x, step = P.build_case("b2n70")
    nan, inf = float("nan"), float("inf")
    wsb = len(c.ci) * 4
    bad = [dict(n_graphs=0), dict(n=0), dict(n=16385), dict(src_step=0), dict(sd=0), dict(sd=4), dict(ldc=1),
           dict(detour_scale=nan), dict(detour_scale=0.0), dict(detour_scale=-1.0), dict(detour_scale=inf),
           dict(rowptr=None), dict(hist=None), dict(totals=None), dict(workspace_bytes=wsb - 1),
           dict(workspace=None), dict(coords=None)]                          # the last: route_out without coords
    for kw in bad:
        out = run_raw(c, x, step, expect_rc=ERR_ARG, override=kw)
        assert "snd_graph_paths" in out["err"], (kw, out["err"])
        assert (out["comp"] == I32_PAT).all() and (out["hops"] == I32_PAT).all(), kw
        assert (out["route"].view(np.uint32) == F32_PAT).all(), kw
        assert (out["hist"] == I64_PAT).all() and (out["totals"] == I64_PAT).all(), kw
    # coords = NULL: sd, ldc and detour_scale are not looked at
    check(c, None, step, run_raw(c, None, step, override=dict(sd=9, ldc=-3, detour_scale=nan)))


def test_layers_graph_paths_and_graph_replay():
    """The torch-level op: fresh and given buffers, the optional outputs, and a captured graph
    whose replay equals the eager call bitwise."""
    from snd_vae_amd import layers
    from snd_vae_amd.metrics import PathStats
    c, x, _ = P.build_case("b2n70")
    step = 3
    ref = P.reference(c, x, SCALE, step)
    rp, ci, xt = (torch.from_numpy(np.array(a)).cuda() for a in (c.rp, c.ci, x))
    hist, totals, comp, hops, route = layers.graph_paths(rp, ci, c.B, c.n, xt, float(SCALE), step, per_node=True,
                                                         per_source=True)
    got = {"hist": hist.cpu().numpy(), "totals": totals.cpu().numpy(), "comp": comp.cpu().numpy(),
           "hops": hops.cpu().numpy(), "route": route.cpu().numpy()}
    P.assert_paths(got, ref, c.n, "layers")
    hist.fill_(7)
    h2, t2 = layers.graph_paths(rp, ci, c.B, c.n, xt, float(SCALE), step, hist=hist, totals=totals)   # cleared first
    assert h2 is hist and np.array_equal(hist.cpu().numpy(), got["hist"])
    h3, t3, hops3, route3 = layers.graph_paths(rp, ci, c.B, c.n, src_step=step, per_source=True)
    assert route3 is None and torch.equal(hops3, hops) and torch.equal(t3, totals) and not h3[:, 1].any()
    ps = PathStats(hist, totals, c.n, float(SCALE), step)
    assert ps == PathStats(got["hist"], got["totals"], c.n, float(SCALE), step) and ps.tensors is not None
    assert ps.per_graph()["n_components"].tolist() == ref["totals"][:, 0].tolist()

    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        layers.graph_paths(rp, ci, c.B, c.n, xt, float(SCALE), step, per_node=True, per_source=True)      # warm-up
        with torch.cuda.graph(g, stream=s):
            outs = layers.graph_paths(rp, ci, c.B, c.n, xt, float(SCALE), step, per_node=True, per_source=True)
    torch.cuda.current_stream().wait_stream(s)
    for o in outs:
        o.fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, (hist, totals, comp, hops, route)):
        assert torch.equal(o.view(torch.uint8), e.view(torch.uint8))

    with pytest.raises(ValueError, match="detour_scale"):
        layers.graph_paths(rp, ci, c.B, c.n, xt)
    with pytest.raises(ValueError, match="detour_scale"):
        layers.graph_paths(rp, ci, c.B, c.n, detour_scale=64.0)
    with pytest.raises(ValueError, match="coords"):
        layers.graph_paths(rp, ci, c.B, c.n, xt[:-1], 64.0)
    with pytest.raises(ValueError, match="hist"):
        layers.graph_paths(rp, ci, c.B, c.n, hist=hist[:1], totals=totals)


# ---------------------------------------------------------------- model and trainers, N = 25
N, B = 25, 2


def _same(a, b):
    """Equality through dicts, lists and tensors, nan equal to nan."""
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, float) and a != a:
        return b != b
    return a == b


def _ref_of(name, rp, ci, coords, step=1):
    c = G.Case(name, B, N, np.array(rp, np.int32), np.array(ci, np.int32))
    return c, P.reference(c, np.asarray(coords, np.float32), SCALE, step)


def _equals_ref(ps, ref, step, what):
    from snd_vae_amd.metrics import PathStats
    assert isinstance(ps, PathStats) and ps.n == N and ps.detour_scale == float(SCALE) and ps.src_step == step
    P.assert_paths({"hist": ps.hist, "totals": ps.totals}, ref, N, what)


def test_model_graph_paths_and_generate():
    from snd_vae_amd import layers
    from snd_vae_amd.config import tscale
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    cfg = tscale(N, 16, mean_degree=4.0)
    batch = synthetic_batch(cfg, B, seed=31)
    model = SGCNModelVAE(cfg, B, dtype="f32", seed=4)
    assert model.PATH_DETOUR_SCALE == float(SCALE)
    db = DeviceBatch(batch)
    for step in (1, 4):
        _, ref = _ref_of(f"model_batch_{step}", batch.rowptr, batch.colidx, batch.spatial_truth, step)
        _equals_ref(model.graph_paths(db, step), ref, step, f"batch src_step={step}")

    plain = model.generate(db, mode="mean", adj_format="csr")
    out = model.generate(db, mode="mean", adj_format="csr", paths=True)
    assert set(out) == set(plain) | {"generated_paths"}
    for k in ("generated_rowptr", "generated_colidx", "generated_spatial"):
        assert torch.equal(out[k], plain[k]), k
    h, t = layers.graph_paths(out["generated_rowptr"], out["generated_colidx"], B, N, out["generated_spatial"],
                              float(SCALE))
    gp = out["generated_paths"]
    assert torch.equal(gp.tensors[0], h) and torch.equal(gp.tensors[1], t) and gp.totals[:, 2].tolist() == [N] * B
    both = model.generate(db, mode="mean", adj_format="csr", stats=True, paths=True, src_step=5)
    assert both["generated_paths"].totals[:, 2].tolist() == [5] * B and "generated_stats" in both
    with pytest.raises(ValueError, match="paths"):
        model.generate(db, mode="mean", paths=True)


def test_trainer_evaluate_generation_paths(tmp_path):
    from snd_vae_amd.config import tscale
    from snd_vae_amd.input_data import load_data_syn, write_synthetic_dataset
    from snd_vae_amd.metrics import PathStats
    from snd_vae_amd.trainer import Trainer
    cfg = tscale(N, 16, mean_degree=4.0)
    write_synthetic_dataset(str(tmp_path), cfg, 4, seed=11)
    np.random.seed(1)
    ds = load_data_syn("train", str(tmp_path), sampling_num=2)
    t = Trainer(cfg, ds, batch_size=B, dtype="f32")
    t.train_epoch()
    o = t.opt
    state = [x.clone() for x in (t.model.params, o.m, o.v, o.step_counter)]
    base = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False)
    res = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False, paths=True, src_step=2)
    assert set(res) == set(base) | {"paths"} and "paths" not in base
    for k in base:                                                            # unchanged key for key
        assert _same(res[k], base[k]), k
    data = PathStats.concat([t.model.graph_paths(b, 2) for b in t.batches])
    gen = PathStats.concat([t.model.generate(b, mode="mean", step=i, adj_format="csr", threshold=0.0, paths=True,
                                             src_step=2)["generated_paths"] for i, b in enumerate(t.batches)])
    p = res["paths"]
    assert p["dataset"] == data and p["generated"] == gen and data.n_graphs == 4
    want = data.compare(gen)
    assert set(p) == set(want) | {"dataset", "generated"}
    for k, v in want.items():
        assert _same(p[k], v), k
    for x, y in zip(state, (t.model.params, o.m, o.v, o.step_counter)):
        assert torch.equal(x, y)
    t.train_epoch()                                                           # the captured graphs still replay
    assert o.global_step == 4


def test_disent_trainer_evaluate_generation_paths(tmp_path):
    from test_gpu_disent_trainer import data_cfg, same_state, state, trainer
    from snd_vae_amd import layers
    from snd_vae_amd.input_data import load_data_syn, write_synthetic_dataset
    from snd_vae_amd.metrics import PathStats
    write_synthetic_dataset(str(tmp_path), data_cfg(), 4, seed=3, with_rel=True)
    ds = load_data_syn("train", str(tmp_path), sampling_num=3, rng=np.random.RandomState(1))
    t = trainer(ds)
    t.train(1)
    before = state(t.model)
    base = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False)
    res = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False, paths=True)
    same_state(before, state(t.model), "evaluate_generation(paths=True)")
    assert set(res) == set(base) | {"paths"}
    for k in base:
        assert _same(res[k], base[k]), k
    scale = t.PATH_DETOUR_SCALE
    assert scale == float(SCALE)
    data, gen = [], []
    for i, b in enumerate(t.batches):
        _, ref = _ref_of(f"disent_batch_{i}", b.rowptr.cpu().numpy(), b.colidx.cpu().numpy(), b.spatial.cpu().numpy())
        ps = PathStats(*layers.graph_paths(b.rowptr, b.colidx, B, N, b.spatial, scale), N, scale)
        _equals_ref(ps, ref, 1, f"disent batch {i}")
        data.append(ps)
        rp, ci = res["generated_csr"][i]
        xy = t.model.generate(b, z="mean")["generated_spatial"].reshape(B * N, 2)
        gen.append(PathStats(*layers.graph_paths(rp, ci, B, N, xy, scale), N, scale))
    data, gen = PathStats.concat(data), PathStats.concat(gen)
    p = res["paths"]
    assert p["dataset"] == data and p["generated"] == gen
    for k, v in data.compare(gen).items():
        assert _same(p[k], v), k
    t.train(1)                                                                # the captured graphs still replay
