"""snd_graph_spectrum (Chebyshev moments of the spectral density) on the GPU, through the raw entry
point on the guarded buffers of tests/abi_ops.py: every operand, both outputs and the workspace of
exactly the queried bytes sit between NaN-pattern guards, outputs and workspace start at the
pattern, so a store outside an output or a missed store shows.  info is compared for exact
equality and every moment within 1e-9 N with tests/graph_spectrum_ref.py (|mu_k| <= N; the
float64 routes differ by 1e-10 at most on these cases on the CPU, an fp32 recurrence by 3e-3).
Then the layers, model and trainer levels at N = 25.
"""
import numpy as np
import pytest
import torch

import abi_ops as A
import graph_spectrum_ref as S
import graph_stats_ref as G

pytestmark = pytest.mark.gpu

I64_PAT = np.uint64(A.PATTERN["f64"][2]).astype(np.int64)       # int64 outputs ride in 8-byte "f64" buffers
F32_PAT = np.uint32(A.PATTERN["f32"][2])
ERR_ARG = -1
BAR = 1e-9                                                      # times N, per moment


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def run_raw(c, K, R=0, seed=0, flags=0, expect_rc=0, override=None):
    """One call on fresh guarded buffers.  Returns moments [B, K], info [B, 4] after the call,
    with every guard and input checked."""
    from snd_vae_amd import _lib
    L = _lib.lib()
    rows, cap = c.B * c.n, len(c.ci)
    bufs = {"rowptr": A.guarded(1, rows + 1, None, "i32", 0, c.rp, "rowptr"),
            "colidx": A.guarded(1, cap, None, "i32", 0, c.ci, "colidx"),
            "moments": A.guarded(1, c.B * K, None, "f64", 0, None, "moments"),
            "info": A.guarded(1, c.B * 4, None, "f64", 0, None, "info")}
    wsb = L.snd_graph_spectrum_workspace(c.B, c.n, cap)
    assert wsb % 16 == 0 and wsb >= c.B * 32 + cap * 8 + rows * (512 + 4)
    bufs["ws"] = A.guarded(1, wsb // 4, None, "f32", 0, None, "workspace")    # exactly the queried bytes
    dev = {k: torch.from_numpy(g.arr).cuda() for k, g in bufs.items()}
    ptr = {k: dev[k].data_ptr() + g.off * g.arr.itemsize for k, g in bufs.items()}
    args = dict(rowptr=ptr["rowptr"], colidx=ptr["colidx"], nnz_cap=cap, n_graphs=c.B, n=c.n, n_moments=K,
                n_probes=R, seed=seed, flags=flags, moments=ptr["moments"], info=ptr["info"], workspace=ptr["ws"],
                workspace_bytes=wsb)
    args.update(override or {})
    rc = L.snd_graph_spectrum(*args.values(), _lib.stream_ptr())
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
    flat = lambda k, t: np.ascontiguousarray(bufs[k].block(after[k])).view(t).ravel()
    return {"moments": flat("moments", np.float64).reshape(c.B, K), "info": flat("info", np.int64).reshape(c.B, 4),
            "err": err, "raw": {k: after[k] for k in ("moments", "info")}}


def check(out, want_m, want_i, n, what, exact):
    assert np.array_equal(out["info"], want_i), what
    m = out["moments"]
    assert np.isfinite(m).all(), what
    err = np.abs(m - want_m).max()
    print(f"GSPECTRUM {what}: max |moment error| {err:.3g}, bar {BAR * n:.3g}")
    assert err <= BAR * n, (what, err)
    assert (m[:, 0] == n).all(), what                                         # mu_0 = N exactly
    if exact:
        assert np.array_equal(m[:, 1], -want_i[:, 1].astype(np.float64)), what    # mu_1 = -isolated exactly


@pytest.mark.parametrize("name", list(S.CASES))
def test_exact_moments(name):
    c = S.build_case(name)
    K = S.CASES[name]
    want_m, want_i = S.reference(name)
    for g, lam in S.known_spectra(name).items():                              # the reference's own closed forms
        assert np.abs(want_m[g] - S.moments_of_spectrum(lam, K)).max() <= BAR * c.n, (name, g)
    check(run_raw(c, K), want_m, want_i, c.n, name, True)


@pytest.mark.parametrize("name,K", [("n65", 9), ("b70_mixed", 3), ("n64", 2), ("b70_mixed", 5)])
def test_odd_and_smallest_moment_counts(name, K):
    c = S.build_case(name)
    check(run_raw(c, K), *S.reference(name, K), c.n, f"{name} K={K}", True)


@pytest.mark.parametrize("R", [32, 40])
@pytest.mark.parametrize("name,flags", [("b70_mixed", 0), ("b70_mixed", S.FORCE_GLOBAL), ("n64", 0), ("n65", 0),
                                        ("r257", 0)])
def test_probe_moments(name, flags, R):
    """Hutchinson estimates over the Philox signs: R = 32 is one full probe block, R = 40 leaves a
    partial second one."""
    c = S.build_case(name)
    seed = (0x9E37 << 32) | 0x1234567
    want_m, want_i = S.reference(name, 64, R, seed)
    check(run_raw(c, 64, R, seed, flags), want_m, want_i, c.n, f"{name} R={R} flags={flags}", False)


@pytest.mark.parametrize("name", ["b70_mixed", "n64", "k64"])
def test_the_forced_global_path_agrees_with_the_lds_path(name):
    c = S.build_case(name)
    K = S.CASES[name]
    want_m, want_i = S.reference(name)
    lds, glob = run_raw(c, K), run_raw(c, K, flags=S.FORCE_GLOBAL)
    check(glob, want_m, want_i, c.n, f"{name} forced global", True)
    assert np.array_equal(lds["info"], glob["info"])
    assert np.abs(lds["moments"] - glob["moments"]).max() <= BAR * c.n


@pytest.mark.parametrize("force_global", [False, True])
def test_two_runs_and_a_graph_replay_are_bitwise_equal(force_global):
    from snd_vae_amd import layers
    c = S.build_case("b70_mixed")
    flags = S.FORCE_GLOBAL if force_global else 0
    for R in (0, 40):
        a, b = run_raw(c, 32, R, 5, flags), run_raw(c, 32, R, 5, flags)
        for k in a["raw"]:
            assert np.array_equal(a["raw"][k].view(np.uint8), b["raw"][k].view(np.uint8)), (k, R)
    rp, ci = (torch.from_numpy(np.array(x)).cuda() for x in (c.rp, c.ci))
    kw = dict(n_moments=32, n_probes=40, seed=5, force_global=force_global)
    moments, info = layers.graph_spectrum(rp, ci, c.B, c.n, **kw)
    assert torch.equal(moments.cpu(), torch.from_numpy(a["moments"])) and torch.equal(info.cpu(), torch.from_numpy(a["info"]))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        layers.graph_spectrum(rp, ci, c.B, c.n, **kw)                         # warm-up
        with torch.cuda.graph(g, stream=s):
            outs = layers.graph_spectrum(rp, ci, c.B, c.n, **kw)
    torch.cuda.current_stream().wait_stream(s)
    for o in outs:
        o.fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, (moments, info)):
        assert torch.equal(o.view(torch.uint8), e.view(torch.uint8))


def test_layers_defaults_and_an_empty_colidx():
    from snd_vae_amd import layers
    c = S.build_case("b70_mixed")
    rp, ci = (torch.from_numpy(np.array(x)).cuda() for x in (c.rp, c.ci))
    moments, info = layers.graph_spectrum(rp, ci, c.B, c.n)                   # exact, K = 128
    want_m, want_i = S.reference("b70_mixed")
    assert moments.shape == (70, 128) and moments.dtype == torch.float64 and info.dtype == torch.int64
    assert np.array_equal(info.cpu().numpy(), want_i) and np.abs(moments.cpu().numpy() - want_m).max() <= BAR * c.n
    n = 300                                                                   # above SPECTRUM_EXACT_MAX_N: 32 probes
    rp0 = torch.zeros(2 * n + 1, dtype=torch.int32, device="cuda")
    moments, info = layers.graph_spectrum(rp0, torch.zeros(0, dtype=torch.int32, device="cuda"), 2, n, n_moments=7)
    assert info.cpu().tolist() == [[0, n, 0, layers.SPECTRUM_PROBES]] * 2     # the empty graph: mu_k = N (-1)^k
    assert np.array_equal(moments.cpu().numpy(), np.tile(n * (-1.0) ** np.arange(7), (2, 1)))


def test_rejected_calls_touch_nothing():
    """Every SND_ERR_ARG call returns the code with a message naming the entry point, and all
    buffers (outputs and workspace included: they keep the guard pattern) are bitwise intact."""
    from snd_vae_amd import _lib
    c = S.build_case("n65")
    need = _lib.lib().snd_graph_spectrum_workspace(c.B, c.n, len(c.ci))
    bad = [dict(n_graphs=0), dict(n=0), dict(n=S.MAX_N + 1), dict(n=S.MAX_N, n_graphs=1 << 17), dict(nnz_cap=-1),
           dict(n_moments=1), dict(n_moments=S.MAX_MOMENTS + 1), dict(n_probes=-1), dict(flags=2), dict(rowptr=None),
           dict(moments=None), dict(info=None), dict(colidx=None), dict(workspace_bytes=need - 1), dict(workspace=None)]
    for kw in bad:
        out = run_raw(c, 16, expect_rc=ERR_ARG, override=kw)
        assert "snd_graph_spectrum" in out["err"], (kw, out["err"])
        assert (out["moments"].view(np.int64) == I64_PAT).all() and (out["info"] == I64_PAT).all(), kw


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


def _check_ref(st, name, rp, ci):
    c = G.Case(name, B, N, np.array(rp, np.int32), np.array(ci, np.int32))
    assert st.n == N and st.n_moments == 128
    assert np.array_equal(st.info, S.info(c)), name
    assert np.abs(st.moments - S.exact_moments(c, 128)).max() <= BAR * N, name


SPECTRUM_KEYS = {"mmd_spectrum", "kld_spectrum", "self", "other", "dataset", "generated"}


def test_model_graph_spectrum_and_generate():
    from snd_vae_amd import layers
    from snd_vae_amd.config import tscale
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.metrics import SpectrumStats
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    cfg = tscale(N, 16, mean_degree=4.0)
    batch = synthetic_batch(cfg, B, seed=31)
    model = SGCNModelVAE(cfg, B, dtype="f32", seed=4)
    db = DeviceBatch(batch)
    st = model.graph_spectrum(db)
    assert isinstance(st, SpectrumStats)
    _check_ref(st, "model_batch", batch.rowptr, batch.colidx)
    d = st.density()
    assert d.shape == (B, 200) and (d >= 0).all() and np.abs(d.sum(axis=1) - 1).max() <= 1e-12

    plain = model.generate(db, mode="mean", adj_format="csr")
    out = model.generate(db, mode="mean", adj_format="csr", spectrum=True)
    assert set(out) == set(plain) | {"generated_spectrum"}
    for k in ("generated_rowptr", "generated_colidx", "generated_spatial"):
        assert torch.equal(out[k], plain[k]), k
    moments, info = layers.graph_spectrum(out["generated_rowptr"], out["generated_colidx"], B, N)
    gs = out["generated_spectrum"]
    assert torch.equal(gs.tensors[0], moments) and torch.equal(gs.tensors[1], info)
    _check_ref(gs, "model_generated", out["generated_rowptr"].cpu().numpy(), out["generated_colidx"].cpu().numpy())
    with pytest.raises(ValueError, match="spectrum"):
        model.generate(db, mode="mean", spectrum=True)


def test_trainer_evaluate_generation_spectrum(tmp_path):
    from snd_vae_amd.config import tscale
    from snd_vae_amd.input_data import load_data_syn, write_synthetic_dataset
    from snd_vae_amd.metrics import SpectrumStats
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
    res = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False, spectrum=True)
    assert set(res) == set(base) | {"spectrum"} and "spectrum" not in base
    for k in base:                                                            # unchanged key for key
        assert _same(res[k], base[k]), k
    data = SpectrumStats.concat([t.model.graph_spectrum(b) for b in t.batches])
    gen = SpectrumStats.concat([t.model.generate(b, mode="mean", step=i, adj_format="csr", threshold=0.0,
                                                 spectrum=True)["generated_spectrum"] for i, b in enumerate(t.batches)])
    m = res["spectrum"]
    assert m["dataset"] == data and m["generated"] == gen and data.n_graphs == 4
    want = data.compare(gen)
    assert set(m) == SPECTRUM_KEYS
    for k, v in want.items():
        assert _same(m[k], v), k
    for x, y in zip(state, (t.model.params, o.m, o.v, o.step_counter)):
        assert torch.equal(x, y)
    t.train_epoch()                                                           # the captured graphs still replay
    assert o.global_step == 4


def test_disent_trainer_evaluate_generation_spectrum(tmp_path):
    from test_gpu_disent_trainer import data_cfg, same_state, state, trainer
    from snd_vae_amd import layers
    from snd_vae_amd.input_data import load_data_syn, write_synthetic_dataset
    from snd_vae_amd.metrics import SpectrumStats
    write_synthetic_dataset(str(tmp_path), data_cfg(), 4, seed=3, with_rel=True)
    ds = load_data_syn("train", str(tmp_path), sampling_num=3, rng=np.random.RandomState(1))
    t = trainer(ds)
    t.train(1)
    before = state(t.model)
    base = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False)
    res = t.evaluate_generation(mode="mean", threshold=0.0, inclusive=False, spectrum=True)
    same_state(before, state(t.model), "evaluate_generation(spectrum=True)")
    assert set(res) == set(base) | {"spectrum"}
    for k in base:
        assert _same(res[k], base[k]), k
    data, gen = [], []
    for i, b in enumerate(t.batches):
        st = SpectrumStats(*layers.graph_spectrum(b.rowptr, b.colidx, B, N), N)
        _check_ref(st, f"disent_batch_{i}", b.rowptr.cpu().numpy(), b.colidx.cpu().numpy())
        data.append(st)
        rp, ci = res["generated_csr"][i]
        sg = SpectrumStats(*layers.graph_spectrum(rp, ci, B, N), N)
        _check_ref(sg, f"disent_gen_{i}", rp.cpu().numpy(), ci.cpu().numpy())
        gen.append(sg)
    data, gen = SpectrumStats.concat(data), SpectrumStats.concat(gen)
    m = res["spectrum"]
    assert m["dataset"] == data and m["generated"] == gen
    assert set(m) == SPECTRUM_KEYS
    for k, v in data.compare(gen).items():
        assert _same(m[k], v), k
    t.train(1)                                                                # the captured graphs still replay
