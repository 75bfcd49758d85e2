"""snd_graph_motifs (graphlet census) on the GPU, through the raw entry point on the guarded buffers
of tests/abi_ops.py: every operand, both outputs and the workspace of exactly the queried bytes
sit between NaN-pattern guards, outputs and workspace start at the pattern, so a store outside an
output or a missed store shows.  census and work are compared for exact equality with
tests/graph_motifs_ref.py.  Then the layers, model and trainer levels at N = 25.
"""
import numpy as np
import pytest
import torch

import abi_ops as A
import graph_motifs_ref as M
import graph_stats_ref as G

pytestmark = pytest.mark.gpu

I64_PAT = np.uint64(A.PATTERN["f64"][2]).astype(np.int64)       # int64 outputs ride in 8-byte "f64" buffers
F32_PAT = np.uint32(A.PATTERN["f32"][2])
ERR_ARG = -1
NO_CAP = (1 << 62)


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def run_raw(c, work_cap=NO_CAP, expect_rc=0, override=None):
    """One call on fresh guarded buffers.  Returns census [B, 10], work [B] after the call, with
    every guard and input checked."""
    from snd_vae_amd import _lib
    L = _lib.lib()
    R, cap = c.B * c.n, len(c.ci)
    bufs = {"rowptr": A.guarded(1, R + 1, None, "i32", 0, c.rp, "rowptr"),
            "colidx": A.guarded(1, cap, None, "i32", 0, c.ci, "colidx"),
            "census": A.guarded(1, c.B * 10, None, "f64", 0, None, "census"),
            "work": A.guarded(1, c.B, None, "f64", 0, None, "work")}
    wsb = L.snd_graph_motifs_workspace(c.B, c.n, cap)
    assert wsb % 16 == 0 and wsb >= c.B * 80 + R * 4 + cap * 4
    bufs["ws"] = A.guarded(1, wsb // 4, None, "f32", 0, None, "workspace")    # exactly the queried bytes
    dev = {k: torch.from_numpy(g.arr).cuda() for k, g in bufs.items()}
    ptr = {k: dev[k].data_ptr() + g.off * g.arr.itemsize for k, g in bufs.items()}
    args = dict(rowptr=ptr["rowptr"], colidx=ptr["colidx"], nnz_cap=cap, n_graphs=c.B, n=c.n, work_cap=work_cap,
                census=ptr["census"], work=ptr["work"], workspace=ptr["ws"], workspace_bytes=wsb)
    args.update(override or {})
    rc = L.snd_graph_motifs(*args.values(), _lib.stream_ptr())
    assert rc == expect_rc, (rc, _lib.last_error())
    err = _lib.last_error() if rc else ""
    torch.cuda.synchronize()
    after = {k: t.cpu().numpy() for k, t in dev.items()}
    for k, g in bufs.items():
        if k != "ws" or rc:                                                   # the workspace is scratch
            g.check_untouched(after[k])
    guards = np.array(after["ws"])
    bufs["ws"].block(guards).view(np.uint32)[...] = F32_PAT
    bufs["ws"].check_untouched(guards)
    for k in ("rowptr", "colidx"):                                            # inputs bitwise intact
        assert np.array_equal(after[k].view(np.uint32), bufs[k].arr.view(np.uint32)), k
    i64 = lambda k: np.ascontiguousarray(bufs[k].block(after[k])).view(np.int64).ravel()
    return {"census": i64("census").reshape(c.B, 10), "work": i64("work"), "err": err,
            "raw": {k: after[k] for k in ("census", "work")}}


@pytest.mark.parametrize("name", list(M.CASES))
def test_cases(name):
    c = M.build_case(name)
    cap = M.case_work_cap(name)
    want_c, want_w = M.reference(c, cap)
    full, _ = M.reference(c)
    for g, kv in M.known_counts(name).items():                                # the reference's own closed forms
        for k, v in kv.items():
            assert full[g, M.NAMES.index(k)] == v, (name, g, k)
    out = run_raw(c, NO_CAP if cap is None else cap)
    print(f"GMOTIFS {name} B {c.B} n {c.n} work {want_w.tolist()[:4]} census[0] {want_c[0].tolist()}")
    M.assert_census(out["census"], out["work"], want_c, want_w, name)
    if name == "k200_middle":
        assert (out["census"][1] == -1).all() and (out["census"][[0, 2]] >= 0).all()
    if name == "cap0":
        assert (out["census"][[0, 2]] == -1).all() and out["census"][1].tolist() == [0] * 10
    if name == "one_way":
        assert (out["census"][:, 9] > 0).all()


def test_k200_counted():
    """The middle graph of the work_cap case without a cap: 6.5e7 4-cliques."""
    c = M.build_case("k200_middle")
    out = run_raw(c)
    M.assert_census(out["census"], out["work"], *M.reference(c), "k200 uncapped")
    assert out["census"][1, 8] == 64684950


def test_two_runs_and_a_graph_replay_are_bitwise_equal():
    from snd_vae_amd import layers
    c = M.build_case("b70_mixed")
    a, b = run_raw(c), run_raw(c)
    for k in a["raw"]:
        assert np.array_equal(a["raw"][k].view(np.uint8), b["raw"][k].view(np.uint8)), k
    want_c, want_w = M.reference(c)
    rp, ci = (torch.from_numpy(np.array(x)).cuda() for x in (c.rp, c.ci))
    census, work = layers.graph_motifs(rp, ci, c.B, c.n, work_cap=NO_CAP)
    M.assert_census(census.cpu().numpy(), work.cpu().numpy(), want_c, want_w, "layers")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        layers.graph_motifs(rp, ci, c.B, c.n, work_cap=NO_CAP)                # warm-up
        with torch.cuda.graph(g, stream=s):
            outs = layers.graph_motifs(rp, ci, c.B, c.n, work_cap=NO_CAP)
    torch.cuda.current_stream().wait_stream(s)
    for o in outs:
        o.fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, (census, work)):
        assert torch.equal(o.view(torch.uint8), e.view(torch.uint8))
    # the default cap counts these graphs; a cap of 0 skips all but the empty ones
    c0, w0 = layers.graph_motifs(rp, ci, c.B, c.n)
    assert torch.equal(c0, census) and torch.equal(w0, work)
    c1, _ = layers.graph_motifs(rp, ci, c.B, c.n, work_cap=0)
    assert torch.equal(c1.cpu(), torch.from_numpy(M.reference(c, 0)[0]))


def test_rejected_calls_touch_nothing():
    """Every SND_ERR_ARG call returns the code with a message naming the entry point, and all
    buffers (outputs and workspace included: they keep the guard pattern) are bitwise intact."""
    c = M.build_case("r33")
    need = None
    from snd_vae_amd import _lib
    need = _lib.lib().snd_graph_motifs_workspace(c.B, c.n, len(c.ci))
    bad = [dict(n_graphs=0), dict(n=0), dict(n=M.MAX_N + 1), dict(n=M.MAX_N, n_graphs=1 << 17), dict(nnz_cap=-1),
           dict(work_cap=-1), dict(rowptr=None), dict(census=None), dict(work=None), dict(colidx=None),
           dict(workspace_bytes=need - 1), dict(workspace=None)]
    for kw in bad:
        out = run_raw(c, expect_rc=ERR_ARG, override=kw)
        assert "snd_graph_motifs" in out["err"], (kw, out["err"])
        assert (out["census"] == I64_PAT).all() and (out["work"] == I64_PAT).all(), kw


def test_identities_against_graph_stats():
    """On symmetric CSRs: E = totals[3], 6T = totals[1], 2(P2 + 3T) = totals[2] of snd_graph_stats."""
    from snd_vae_amd import layers
    for name in ("r257", "k40", "lattice12", "star200", "unsorted", "isolated"):
        c = M.build_case(name)
        rp, ci = (torch.from_numpy(np.array(x)).cuda() for x in (c.rp, c.ci))
        census, _ = layers.graph_motifs(rp, ci, c.B, c.n, work_cap=NO_CAP)
        _, totals = layers.graph_stats(rp, ci, c.B, c.n)
        cen, tot = census.cpu().numpy(), totals.cpu().numpy()
        if name == "r257":                                                    # its planted one-way arcs break symmetry
            assert (cen[:, 9] > 0).all()
            continue
        assert (cen[:, 9] == 0).all(), name
        assert np.array_equal(cen[:, 0], tot[:, 3]), name
        assert np.array_equal(6 * cen[:, 2], tot[:, 1]), name
        assert np.array_equal(2 * (cen[:, 1] + 3 * cen[:, 2]), tot[:, 2]), name


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


def _ref_census(name, rp, ci):
    c = G.Case(name, B, N, np.array(rp, np.int32), np.array(ci, np.int32))
    return M.reference(c)[0]


def test_model_graph_motifs_and_generate():
    from snd_vae_amd import layers
    from snd_vae_amd.config import tscale
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.metrics import MotifStats
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    cfg = tscale(N, 16, mean_degree=4.0)
    batch = synthetic_batch(cfg, B, seed=31)
    model = SGCNModelVAE(cfg, B, dtype="f32", seed=4)
    db = DeviceBatch(batch)
    ms = model.graph_motifs(db)
    assert isinstance(ms, MotifStats) and ms.n == N and ms.n_skipped == 0
    assert np.array_equal(ms.census, _ref_census("model_batch", batch.rowptr, batch.colidx))

    plain = model.generate(db, mode="mean", adj_format="csr")
    out = model.generate(db, mode="mean", adj_format="csr", motifs=True)
    assert set(out) == set(plain) | {"generated_motifs"}
    for k in ("generated_rowptr", "generated_colidx", "generated_spatial"):
        assert torch.equal(out[k], plain[k]), k
    census, _ = layers.graph_motifs(out["generated_rowptr"], out["generated_colidx"], B, N)
    gm = out["generated_motifs"]
    assert torch.equal(gm.tensors, census)
    assert np.array_equal(gm.census, _ref_census("model_generated", out["generated_rowptr"].cpu().numpy(),
                                                 out["generated_colidx"].cpu().numpy()))
    with pytest.raises(ValueError, match="motifs"):
        model.generate(db, mode="mean", motifs=True)


def test_trainer_evaluate_generation_motifs(tmp_path):
    from snd_vae_amd.config import tscale
    from snd_vae_amd.input_data import load_data_syn, write_synthetic_dataset
    from snd_vae_amd.metrics import MotifStats
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
    res = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False, motifs=True)
    assert set(res) == set(base) | {"motifs"} and "motifs" not in base
    for k in base:                                                            # unchanged key for key
        assert _same(res[k], base[k]), k
    data = MotifStats.concat([t.model.graph_motifs(b) for b in t.batches])
    gen = MotifStats.concat([t.model.generate(b, mode="mean", step=i, adj_format="csr", threshold=0.0,
                                              motifs=True)["generated_motifs"] for i, b in enumerate(t.batches)])
    m = res["motifs"]
    assert m["dataset"] == data and m["generated"] == gen and data.n_graphs == 4
    want = data.compare(gen)
    assert set(m) == {"mmd_orbits", "self", "other", "dataset", "generated"}
    for k, v in want.items():
        assert _same(m[k], v), k
    for x, y in zip(state, (t.model.params, o.m, o.v, o.step_counter)):
        assert torch.equal(x, y)
    t.train_epoch()                                                           # the captured graphs still replay
    assert o.global_step == 4


def test_disent_trainer_evaluate_generation_motifs(tmp_path):
    from test_gpu_disent_trainer import data_cfg, same_state, state, trainer
    from snd_vae_amd import layers
    from snd_vae_amd.input_data import load_data_syn, write_synthetic_dataset
    from snd_vae_amd.metrics import MotifStats
    write_synthetic_dataset(str(tmp_path), data_cfg(), 4, seed=3, with_rel=True)
    ds = load_data_syn("train", str(tmp_path), sampling_num=3, rng=np.random.RandomState(1))
    t = trainer(ds)
    t.train(1)
    before = state(t.model)
    base = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False)
    res = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False, motifs=True)
    same_state(before, state(t.model), "evaluate_generation(motifs=True)")
    assert set(res) == set(base) | {"motifs"}
    for k in base:
        assert _same(res[k], base[k]), k
    data, gen = [], []
    for i, b in enumerate(t.batches):
        ms = MotifStats(layers.graph_motifs(b.rowptr, b.colidx, B, N)[0], N)
        assert np.array_equal(ms.census, _ref_census(f"disent_batch_{i}", b.rowptr.cpu().numpy(),
                                                     b.colidx.cpu().numpy()))
        data.append(ms)
        rp, ci = res["generated_csr"][i]
        mg = MotifStats(layers.graph_motifs(rp, ci, B, N)[0], N)
        assert np.array_equal(mg.census, _ref_census(f"disent_gen_{i}", rp.cpu().numpy(), ci.cpu().numpy()))
        gen.append(mg)
    data, gen = MotifStats.concat(data), MotifStats.concat(gen)
    m = res["motifs"]
    assert m["dataset"] == data and m["generated"] == gen
    assert set(m) == {"mmd_orbits", "self", "other", "dataset", "generated"}
    for k, v in data.compare(gen).items():
        assert _same(m[k], v), k
    t.train(1)                                                                # the captured graphs still replay
