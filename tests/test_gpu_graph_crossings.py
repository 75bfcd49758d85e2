"""snd_graph_crossings (edge crossings as drawn) on the GPU, through the raw entry point on the
guarded buffers of tests/abi_ops.py: every operand, every output and the workspace of exactly the
queried bytes sit between NaN-pattern guards, outputs and workspace start at the pattern, so a
store outside an output or a missed store shows.  coords is passed with ldc = 3 and the guard
pattern in column 2.  counts, work, cross_out, hist[0] and the sums of hist[1] and hist[2] are
compared for exact equality with tests/graph_crossings_ref.py; the two angle histograms through
cumulative counts within 2^-10 of a bin at every edge (atan2f is not correctly rounded; the
reference's angles are float64).  Then the layers, model and trainer levels at N = 25.
"""
import numpy as np
import pytest
import torch

import abi_ops as A
import graph_crossings_ref as X
import graph_stats_ref as G

pytestmark = pytest.mark.gpu

I64_PAT = np.uint64(A.PATTERN["f64"][2]).astype(np.int64)       # int64 outputs ride in 8-byte "f64" buffers
I32_PAT = np.uint32(A.PATTERN["i32"][2]).astype(np.int32)
F32_PAT = np.uint32(A.PATTERN["f32"][2])
ERR_ARG = -1
NO_CAP = (1 << 62)


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def run_raw(c, work_cap=NO_CAP, expect_rc=0, override=None, per_edge=True):
    """One call on fresh guarded buffers.  Returns counts [B, 7], hist [B, 3, 256], work [B] and
    cross_out [cap] after the call, with every guard and input checked."""
    from snd_vae_amd import _lib
    L = _lib.lib()
    R, cap = c.B * c.n, len(c.ci)
    bufs = {"rowptr": A.guarded(1, R + 1, None, "i32", 0, c.rp, "rowptr"),
            "colidx": A.guarded(1, cap, None, "i32", 0, c.ci, "colidx"),
            "coords": A.guarded(R, 2, 3, "f32", 0, c.xy, "coords"),
            "counts": A.guarded(1, c.B * 7, None, "f64", 0, None, "counts"),
            "hist": A.guarded(1, c.B * 3 * 256, None, "f64", 0, None, "hist"),
            "work": A.guarded(1, c.B, None, "f64", 0, None, "work"),
            "cross_out": A.guarded(1, cap, None, "i32", 0, None, "cross_out")}
    wsb = L.snd_graph_crossings_workspace(c.B, c.n, cap)
    assert wsb % 16 == 0 and wsb >= c.B * 64 + (c.B + 1) * 8 + cap * 28
    bufs["ws"] = A.guarded(1, wsb // 4, None, "f32", 0, None, "workspace")    # exactly the queried bytes
    dev = {k: torch.from_numpy(g.arr).cuda() for k, g in bufs.items()}
    ptr = {k: dev[k].data_ptr() + g.off * g.arr.itemsize for k, g in bufs.items()}
    args = dict(rowptr=ptr["rowptr"], colidx=ptr["colidx"], nnz_cap=cap, n_graphs=c.B, n=c.n, coords=ptr["coords"],
                ldc=3, work_cap=work_cap, counts=ptr["counts"], hist=ptr["hist"], work=ptr["work"],
                cross_out=ptr["cross_out"] if per_edge else None, workspace=ptr["ws"], workspace_bytes=wsb)
    args.update(override or {})
    rc = L.snd_graph_crossings(*args.values(), _lib.stream_ptr())
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
    for k in ("rowptr", "colidx", "coords"):                                  # inputs bitwise intact
        assert np.array_equal(after[k].view(np.uint32), bufs[k].arr.view(np.uint32)), k
    i64 = lambda k: np.ascontiguousarray(bufs[k].block(after[k])).view(np.int64).ravel()
    cross = np.ascontiguousarray(bufs["cross_out"].block(after["cross_out"])).ravel()
    if rc == 0 and per_edge:                                                  # entries past rowptr[B n] are untouched
        assert (cross[int(c.rp[-1]):] == I32_PAT).all(), "cross_out past rowptr[B n]"
    if not per_edge:
        assert (cross == I32_PAT).all()
    return {"counts": i64("counts").reshape(c.B, 7), "hist": i64("hist").reshape(c.B, 3, 256), "work": i64("work"),
            "cross_out": cross if per_edge else None, "err": err,
            "raw": {k: after[k] for k in ("counts", "hist", "work", "cross_out")}}


def check_bands(c, want, name):
    """On the reference alone: at most 2 % of a case's angle values lie within the band of a bin
    edge (about 0.2 % is expected)."""
    dv = np.concatenate(want["dir_vals"])
    # K8 on a circle is left out of the angle share: by the inscribed-angle theorem the chords of a
    # regular octagon meet at multiples of pi / 8, which are bin edges (64 k); its hist[2] still
    # has to lie in the band like every other graph's
    av = np.concatenate(want["ang_vals"][1:] if name == "closed" else want["ang_vals"])
    sd, sa = X.band_share(dv, wrap=True), X.band_share(av[av < 255.5])
    print(f"GCROSS {name} band shares: directions {sd:.5f} of {len(dv)}, angles {sa:.5f} of {len(av)}")
    assert sd <= 0.02 and sa <= 0.02, (name, sd, sa)
    return sd, sa


@pytest.mark.parametrize("name", list(X.CASES))
def test_cases(name):
    c = X.build_case(name)
    cap = X.case_work_cap(name)
    want = X.reference(c, cap)
    check_bands(c, want, name)
    out = run_raw(c, NO_CAP if cap is None else cap)
    print(f"GCROSS {name} B {c.B} n {c.n} work {want['work'].tolist()[:4]} counts[0] {want['counts'][0].tolist()}")
    X.assert_equal(out, want, name)
    if name == "closed":
        forms = X.closed_forms(c.n)
        rows = [0, 2, 4, 5, 6, 7, 8]                                          # an empty and a one-edge graph between
        for g, (nm, pairs, _, x) in zip(rows, forms):
            assert want["counts"][g, 0] == len(pairs) and want["counts"][g, 1] == x, (nm, want["counts"][g])
        assert want["counts"][1].tolist() == [0] * 7 and want["counts"][3, :2].tolist() == [1, 0]
        gd = out["hist"][4]                                                   # the grid with both diagonals
        assert want["counts"][4, 0] == 72 and gd[2, 255] == 16 and gd[2].sum() == 16
        assert sorted(np.nonzero(gd[1])[0].tolist()) == [0, 64, 128, 192]
        assert X.band_share(want["dir_vals"][4], wrap=True) == 0.0
        assert np.array_equal(gd[1], want["hist"][4, 1])
        assert want["counts"][8, 5] == 1                                      # the zero-length edge
    if name == "cap_middle":
        assert (out["counts"][1] == -1).all() and (out["counts"][[0, 2], 0] > 0).all()
        assert not out["hist"][1].any()
        lo, hi = int(c.rp[c.n]), int(c.rp[2 * c.n])
        assert (out["cross_out"][lo:hi] == -1).all() and (out["cross_out"][:lo] >= 0).all()
        full = X.reference(c)
        assert np.array_equal(out["counts"][[0, 2]], full["counts"][[0, 2]])
    if name == "cap0":
        assert out["counts"][:, 0].tolist() == [-1, 0, 1, -1]                 # two edges, none, one, K5
    if name in X.WALK_CASES:
        # the case has its power only while a wave holds several work items: more tile pairs than waves
        E = want["counts"][:, 0]
        items = sum(X.tile_pairs(e) for e in E if e >= 0)
        waves = X.pair_waves(c.B, c.n, len(c.ci), torch.cuda.get_device_properties(0).multi_processor_count)
        print(f"GCROSS {name} tile pairs {items} waves {waves}")
        assert items > waves, (items, waves)                                  # ranges of two items or more
        if name == "walk_batch":
            assert (E == 0).sum() > 100 and (E < 0).sum() > 100 and (E > 256).sum() > 100
    if name == "tile_edges":
        assert want["counts"][:, 0].tolist() == [X.TILE - 1, X.TILE, X.TILE + 1, 2 * X.TILE + 1]


def test_tile_size_is_the_kernels():
    import os
    import re
    from snd_vae_amd import layers
    hpp = open(os.path.join(os.path.dirname(layers.__file__), "csrc", "snd_gcrossings.hpp")).read()
    assert int(re.search(r"kGxTile\s*=\s*(\d+)", hpp).group(1)) == layers.CROSSINGS_TILE == X.TILE


def test_null_cross_out():
    c = X.build_case("r33")
    out = run_raw(c, per_edge=False)
    X.assert_equal(out, X.reference(c), "r33 without cross_out")


def test_no_entries_at_all():
    """nnz_cap = 0 with a NULL colidx and a NULL cross_out: every count is 0."""
    c = X.Case("no_entries", 3, 7, np.zeros(22, np.int32), np.zeros(0, np.int32),
               np.random.default_rng(1).random((21, 2)).astype(np.float32))
    out = run_raw(c, per_edge=False, override=dict(nnz_cap=0, colidx=None))
    assert not out["counts"].any() and not out["hist"].any() and not out["work"].any()


def test_two_runs_and_a_graph_replay_are_bitwise_equal():
    from snd_vae_amd import layers
    c = X.build_case("b70_mixed")
    a, b = run_raw(c), run_raw(c)
    for k in a["raw"]:
        assert np.array_equal(a["raw"][k].view(np.uint8), b["raw"][k].view(np.uint8)), k
    want = X.reference(c)
    rp, ci, xy = (torch.from_numpy(np.array(x)).cuda() for x in (c.rp, c.ci, c.xy))
    eager = layers.graph_crossings(rp, ci, c.B, c.n, xy, work_cap=NO_CAP, per_edge=True)
    got = dict(zip(("counts", "hist", "work", "cross_out"), (t.cpu().numpy() for t in eager)))
    X.assert_equal(got, want, "layers")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        layers.graph_crossings(rp, ci, c.B, c.n, xy, work_cap=NO_CAP, per_edge=True)       # warm-up
        with torch.cuda.graph(g, stream=s):
            outs = layers.graph_crossings(rp, ci, c.B, c.n, xy, work_cap=NO_CAP, per_edge=True)
    torch.cuda.current_stream().wait_stream(s)
    for o in outs[:3]:
        o.fill_(-3)
    outs[3][:int(c.rp[-1])].fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager):
        assert torch.equal(o.view(torch.uint8), e.view(torch.uint8))
    # the default cap counts these graphs; three results without per_edge
    plain = layers.graph_crossings(rp, ci, c.B, c.n, xy)
    assert len(plain) == 3 and all(torch.equal(p, e) for p, e in zip(plain, eager))
    c0 = layers.graph_crossings(rp, ci, c.B, c.n, xy, work_cap=0)[0]
    assert torch.equal(c0.cpu(), torch.from_numpy(np.array(X.reference(c, 0)["counts"])))


def test_rejected_calls_touch_nothing():
    """Every SND_ERR_ARG call returns the code with a message naming the entry point, and all
    buffers (outputs and workspace included: they keep the guard pattern) are bitwise intact."""
    from snd_vae_amd import _lib
    c = X.build_case("r33")
    need = _lib.lib().snd_graph_crossings_workspace(c.B, c.n, len(c.ci))
    bad = [dict(n_graphs=0), dict(n=0), dict(n=X.MAX_N + 1), dict(n=X.MAX_N, n_graphs=1 << 17), dict(nnz_cap=-1),
           dict(work_cap=-1), dict(ldc=1), dict(rowptr=None), dict(coords=None), dict(counts=None), dict(hist=None),
           dict(work=None), dict(colidx=None), dict(workspace_bytes=need - 1), dict(workspace=None)]
    for kw in bad:
        out = run_raw(c, expect_rc=ERR_ARG, override=kw)
        assert "snd_graph_crossings" in out["err"], (kw, out["err"])
        assert (out["counts"] == I64_PAT).all() and (out["work"] == I64_PAT).all(), kw
        assert (out["hist"] == I64_PAT).all() and (out["cross_out"] == I32_PAT).all(), kw
    out = run_raw(c, expect_rc=ERR_ARG, override=dict(workspace=8))           # a misaligned pointer; nothing reads it
    assert "snd_graph_crossings" in out["err"] and "aligned" in out["err"]


def test_identities_against_graph_motifs():
    """counts[0] and counts[4] are snd_graph_motifs' census[0] and census[9]; hist[1] sums to
    E - counts[5]."""
    from snd_vae_amd import layers
    c = X.build_case("r33")
    rp, ci, xy = (torch.from_numpy(np.array(x)).cuda() for x in (c.rp, c.ci, c.xy))
    counts, hist, _ = layers.graph_crossings(rp, ci, c.B, c.n, xy, work_cap=NO_CAP)
    census, _ = layers.graph_motifs(rp, ci, c.B, c.n, work_cap=NO_CAP)
    cnt, cen, h = counts.cpu().numpy(), census.cpu().numpy(), hist.cpu().numpy()
    assert (cnt[:, 4] > 0).all()
    assert np.array_equal(cnt[:, 0], cen[:, 0]) and np.array_equal(cnt[:, 4], cen[:, 9])
    assert np.array_equal(h[:, 1].sum(axis=1), cnt[:, 0] - cnt[:, 5])
    assert np.array_equal(h[:, 0].sum(axis=1), cnt[:, 0]) and np.array_equal(h[:, 2].sum(axis=1), cnt[:, 1])


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


def _ref(name, rp, ci, xy):
    c = X.Case(name, B, N, np.array(rp, np.int32), np.array(ci, np.int32), np.array(xy, np.float32)[:, :2])
    return X.reference(c)


def _assert_stats(cs, name, rp, ci, xy):
    want = _ref(name, rp, ci, xy)
    X.assert_equal({"counts": cs.counts, "hist": cs.hist, "work": want["work"]}, want, name)


def test_model_graph_crossings_and_generate():
    from snd_vae_amd import layers
    from snd_vae_amd.config import tscale
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.metrics import CrossingStats
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    cfg = tscale(N, 16, mean_degree=4.0)
    batch = synthetic_batch(cfg, B, seed=31)
    model = SGCNModelVAE(cfg, B, dtype="f32", seed=4)
    db = DeviceBatch(batch)
    cs = model.graph_crossings(db)
    assert isinstance(cs, CrossingStats) and cs.n == N and cs.n_skipped == 0
    counts, hist, _ = layers.graph_crossings(db.rowptr, db.colidx, B, N, db.spatial_truth)
    assert torch.equal(cs.tensors[0], counts) and torch.equal(cs.tensors[1], hist)
    _assert_stats(cs, "model_batch", batch.rowptr, batch.colidx, db.spatial_truth.cpu().numpy())

    plain = model.generate(db, mode="mean", adj_format="csr")
    out = model.generate(db, mode="mean", adj_format="csr", crossings=True)
    assert set(out) == set(plain) | {"generated_crossings"}
    for k in ("generated_rowptr", "generated_colidx", "generated_spatial"):
        assert torch.equal(out[k], plain[k]), k
    counts, hist, _ = layers.graph_crossings(out["generated_rowptr"], out["generated_colidx"], B, N,
                                             out["generated_spatial"])
    gc = out["generated_crossings"]
    assert torch.equal(gc.tensors[0], counts) and torch.equal(gc.tensors[1], hist)
    _assert_stats(gc, "model_generated", out["generated_rowptr"].cpu().numpy(),
                  out["generated_colidx"].cpu().numpy(), out["generated_spatial"].cpu().numpy())
    with pytest.raises(ValueError, match="crossings"):
        model.generate(db, mode="mean", crossings=True)


def test_spatial_dim_3_is_refused():
    """The Python levels raise before any launch when the plan's spatial_dim is not 2 (the check
    reads the config only, so a 2-D model is shown a 3-D copy of its config)."""
    import dataclasses
    from snd_vae_amd.config import tscale
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    cfg = tscale(N, 16, mean_degree=4.0)
    model = SGCNModelVAE(cfg, B, dtype="f32", seed=4)
    db = DeviceBatch(synthetic_batch(cfg, B, seed=32))
    model.cfg = dataclasses.replace(cfg, spatial_dim=3)
    with pytest.raises(ValueError, match="spatial_dim"):
        model.graph_crossings(db)
    with pytest.raises(ValueError, match="spatial_dim"):
        model.generate(db, mode="mean", adj_format="csr", crossings=True)


def test_trainer_evaluate_generation_crossings(tmp_path):
    from snd_vae_amd.config import tscale
    from snd_vae_amd.input_data import load_data_syn, write_synthetic_dataset
    from snd_vae_amd.metrics import CrossingStats
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
    res = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False, crossings=True)
    assert set(res) == set(base) | {"crossings"} and "crossings" not in base
    for k in base:                                                            # unchanged key for key
        assert _same(res[k], base[k]), k
    data = CrossingStats.concat([t.model.graph_crossings(b) for b in t.batches])
    gen = CrossingStats.concat([t.model.generate(b, mode="mean", step=i, adj_format="csr", threshold=0.0,
                                                 crossings=True)["generated_crossings"]
                                for i, b in enumerate(t.batches)])
    m = res["crossings"]
    assert m["dataset"] == data and m["generated"] == gen and data.n_graphs == 4
    want = data.compare(gen)
    assert set(m) == set(want) | {"dataset", "generated"}
    for k, v in want.items():
        assert _same(m[k], v), k
    for x, y in zip(state, (t.model.params, o.m, o.v, o.step_counter)):
        assert torch.equal(x, y)
    t.train_epoch()                                                           # the captured graphs still replay
    assert o.global_step == 4
    import dataclasses
    t.cfg = dataclasses.replace(t.cfg, spatial_dim=3)
    with pytest.raises(ValueError, match="spatial_dim"):
        t.evaluate_generation(mode="mean", threshold=0.0, crossings=True)


def test_disent_trainer_evaluate_generation_crossings(tmp_path):
    from test_gpu_disent_trainer import data_cfg, same_state, state, trainer
    from snd_vae_amd import layers
    from snd_vae_amd.input_data import load_data_syn, write_synthetic_dataset
    from snd_vae_amd.metrics import CrossingStats
    write_synthetic_dataset(str(tmp_path), data_cfg(), 4, seed=3, with_rel=True)
    ds = load_data_syn("train", str(tmp_path), sampling_num=3, rng=np.random.RandomState(1))
    t = trainer(ds)
    t.train(1)
    before = state(t.model)
    base = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False)
    res = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False, crossings=True)
    same_state(before, state(t.model), "evaluate_generation(crossings=True)")
    assert set(res) == set(base) | {"crossings"}
    for k in base:
        assert _same(res[k], base[k]), k
    data = []
    for i, b in enumerate(t.batches):
        cs = CrossingStats(*layers.graph_crossings(b.rowptr, b.colidx, B, N, b.spatial)[:2], N)
        _assert_stats(cs, f"disent_batch_{i}", b.rowptr.cpu().numpy(), b.colidx.cpu().numpy(),
                      b.spatial.cpu().numpy())
        data.append(cs)
    data = CrossingStats.concat(data)
    m = res["crossings"]
    assert m["dataset"] == data and m["generated"].n_graphs == data.n_graphs
    for i, (rp, ci) in enumerate(res["generated_csr"]):                       # the generated side on the same CSR
        part = m["generated"].counts[i * B:(i + 1) * B]
        assert np.array_equal(part[:, 0], layers.graph_motifs(rp, ci, B, N)[0].cpu().numpy()[:, 0])
    for k, v in data.compare(m["generated"]).items():
        assert _same(m[k], v), k
    t.train(1)                                                                # the captured graphs still replay
    import dataclasses
    t.cfg = dataclasses.replace(t.cfg, spatial_dim=3)
    with pytest.raises(ValueError, match="spatial_dim"):
        t.evaluate_generation(mode="mean", threshold=0.0, crossings=True)
