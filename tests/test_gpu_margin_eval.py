"""``snd_margin_eval`` and ``snd_disent_losses`` (ABI 23) at the C ABI on guarded operands
(tests/margin_eval_ref.py): the margin histogram and the confusion counts must equal the
NumPy restatement exactly, the loss tail the float64 formula to 1e-15 relative, every guard
band must stay intact and every SND_ERR_ARG rule must fire before anything is launched.

Shapes: N = 1 (everything TN, an empty histogram), 2 (the small-N diagonal test), 5, 25
(the reference's), 33, and 100 / 101 (more than one 8192-entry chunk per graph; odd N puts
the later graphs and chunks off 16-byte alignment: the scalar path), B = 1, 3, 70.
"""
import numpy as np
import pytest
import torch

import margin_eval_ref as M

pytestmark = pytest.mark.gpu
ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def lib():
    from snd_vae_amd import _lib
    return _lib.lib(), _lib.stream_ptr(), _lib


def run(margin, adj, offset=0, accumulate=0, calls=1, clear=False):
    """The op on guarded copies of margin / adj (pointers ``offset`` floats off alignment) and
    guarded outputs pre-filled with a pattern (cleared first for the accumulate test)."""
    L, S, _lib = lib()
    B, N, _ = margin.shape
    gm, ga = M.Guarded(margin, offset=offset), M.Guarded(adj, offset=offset)
    fill = 0 if clear else 77
    gh = M.Guarded(np.full((B, 2, M.BINS), fill, np.int64))
    gc = M.Guarded(np.full((B, 4), fill, np.int64))
    for _ in range(calls):
        _lib.check(L.snd_margin_eval(gm.t.data_ptr(), ga.t.data_ptr(), B, N, gh.t.data_ptr(), gc.t.data_ptr(),
                                     accumulate, None, 0, S), "snd_margin_eval")
    torch.cuda.synchronize()
    assert gm.intact() and ga.intact() and gh.intact() and gc.intact(), "a guard band was written"
    assert np.array_equal(gm.t.cpu().numpy(), margin, equal_nan=True) and np.array_equal(ga.t.cpu().numpy(), adj)
    return gh.t.cpu().numpy(), gc.t.cpu().numpy()


def check(margin, adj, **kw):
    hist, counts = run(margin, adj, **kw)
    rh, rc = M.margin_eval_ref(margin, adj)
    B, N, _ = margin.shape
    assert np.array_equal(counts, rc), (counts[:2], rc[:2])
    assert np.array_equal(hist, rh)
    assert np.all(hist.sum((1, 2)) == N * N - N) and np.all(counts.sum(1) == N * N)


@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("N", [1, 2, 5, 25, 33])
def test_equals_the_restatement(N, B):
    check(*M.random_case(B, N, seed=1))


@pytest.mark.parametrize("N,B", [(100, 2), (101, 3)])
def test_more_than_one_chunk_per_graph(N, B):
    check(*M.random_case(B, N, seed=2))


@pytest.mark.parametrize("N,B", [(5, 3), (25, 3), (33, 1), (101, 2)])
def test_pointers_offset_by_one_float(N, B):
    check(*M.random_case(B, N, seed=3), offset=1)


def test_workspace_is_empty_and_null_is_accepted():
    L, _, _ = lib()
    assert L.snd_margin_eval_workspace(3, 25) == 0


def test_bin_edges_on_and_off_the_diagonal():
    margin, adj, expect = M.edge_case()
    hist, counts = run(margin, adj)
    N = margin.shape[1]
    off = ~np.eye(N, dtype=bool)
    for label in (0, 1):
        sel = off & ((adj[0] != 0) == bool(label))
        assert np.array_equal(hist[0, label], np.bincount(expect[0][sel], minlength=M.BINS)), label
    rh, rc = M.margin_eval_ref(margin, adj)
    assert np.array_equal(hist, rh) and np.array_equal(counts, rc)


@pytest.mark.parametrize("N,B", [(5, 3), (25, 2)])
def test_a_diagonal_of_1e30_is_ignored(N, B):
    margin, adj = M.random_case(B, N, seed=4)
    base = run(margin, adj)
    m2, a2 = M.random_case(B, N, seed=4, diag=1e30)
    a2[:, np.arange(N), np.arange(N)] = 1.0
    got = run(m2, a2)
    assert np.array_equal(base[0], got[0]) and np.array_equal(base[1], got[1])


def test_accumulate_twice_is_twice_one_call():
    margin, adj = M.random_case(3, 25, seed=5)
    one = run(margin, adj)
    two = run(margin, adj, accumulate=1, calls=2, clear=True)
    assert np.array_equal(two[0], 2 * one[0]) and np.array_equal(two[1], 2 * one[1])
    again = run(margin, adj, accumulate=0, calls=2)                     # accumulate = 0 clears first
    assert np.array_equal(again[0], one[0]) and np.array_equal(again[1], one[1])


def test_nan_margins_stay_inside_the_outputs():
    margin, adj = M.random_case(2, 25, seed=6)
    margin[0, 3, 4] = margin[1, 7, 2] = np.nan
    hist, counts = run(margin, adj)                                     # the guards are checked in run()
    assert np.all(counts.sum(1) == 25 * 25)


def test_layers_margin_eval_and_edge_counts():
    from snd_vae_amd import layers
    from snd_vae_amd.metrics import EdgeCounts
    margin, adj = M.random_case(3, 25, seed=7)
    m, a = torch.from_numpy(margin).cuda(), torch.from_numpy(adj).cuda()
    rh, rc = M.margin_eval_ref(margin, adj)
    assert EdgeCounts(*layers.margin_eval(m, a)) == EdgeCounts(rh, rc)
    buf = EdgeCounts.zeros(3, device="cuda")
    for _ in range(2):
        layers.margin_eval(m, a, *buf.tensors, accumulate=True)
    assert buf == EdgeCounts(2 * rh, 2 * rc)
    with pytest.raises(ValueError):
        layers.margin_eval(m, a[:, :, :24].contiguous())
    with pytest.raises(ValueError):
        layers.margin_eval(m, a, accumulate=True)


def test_margin_eval_rejects_bad_arguments_before_launching():
    L, S, _lib = lib()
    margin, adj = M.random_case(2, 5, seed=8)
    gm, ga = M.Guarded(margin), M.Guarded(adj)
    gh, gc = M.Guarded(np.full((2, 2, M.BINS), 77, np.int64)), M.Guarded(np.full((2, 4), 77, np.int64))
    m, a, h, c = (g.t.data_ptr() for g in (gm, ga, gh, gc))
    bad = [(None, a, 2, 5, h, c), (m, None, 2, 5, h, c), (m, a, 2, 5, None, c), (m, a, 2, 5, h, None),
           (m, a, 0, 5, h, c), (m, a, -1, 5, h, c), (m, a, 2, 0, h, c), (m, a, 2, -3, h, c)]
    for args in bad:
        assert L.snd_margin_eval(*args, 0, None, 0, S) == ERR_ARG, args
        assert "snd_margin_eval" in _lib.last_error()
    torch.cuda.synchronize()
    # accumulate = 0 would have cleared the outputs: nothing ran
    assert np.all(gh.t.cpu().numpy() == 77) and np.all(gc.t.cpu().numpy() == 77)
    assert all(g.intact() for g in (gm, ga, gh, gc))


# ---------------------------------------------------------------- snd_disent_losses
def losses_case(blocks, seed, base=False):
    rng = np.random.default_rng(seed)
    c = {"sse_node": rng.random(blocks) * 3.0, "sse_spatial": rng.random(blocks) * 5.0,
         "ce_out": np.array([rng.random() * 900.0, float(rng.integers(0, 1250))]),
         "reg_s": None if base else rng.random(4), "reg_g": None if base else rng.random(4), "reg_sg": rng.random(4),
         "node_count": 50.0, "spatial_count": 100.0, "pair_count": 1250.0}
    return c


def run_losses(c, **over):
    L, S, _lib = lib()
    g = {k: M.Guarded(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    out = M.Guarded(np.full(8, np.nan))
    p = {k: v.t.data_ptr() for k, v in g.items()}
    p["losses"] = out.t.data_ptr()
    a = dict(c, **{k: p.get(k) for k in ("sse_node", "sse_spatial", "ce_out", "reg_s", "reg_g", "reg_sg", "losses")},
             node_blocks=c["sse_node"].size, spatial_blocks=c["sse_spatial"].size)
    a.update(over)
    rc = L.snd_disent_losses(a["sse_node"], a["node_blocks"], a["node_count"], a["sse_spatial"], a["spatial_blocks"],
                             a["spatial_count"], a["ce_out"], a["pair_count"], a["reg_s"], a["reg_g"], a["reg_sg"],
                             a["losses"], S)
    torch.cuda.synchronize()
    assert out.intact() and all(v.intact() for v in g.values())
    return rc, out.t.cpu().numpy(), _lib


@pytest.mark.parametrize("base", [False, True], ids=["three_groups", "base"])
@pytest.mark.parametrize("blocks", [1, 37])
def test_disent_losses_match_the_formula(blocks, base):
    c = losses_case(blocks, seed=blocks, base=base)
    rc, got, _lib = run_losses(c)
    _lib.check(rc, "snd_disent_losses")
    ref = M.disent_losses_ref(c["sse_node"], c["node_count"], c["sse_spatial"], c["spatial_count"], c["ce_out"],
                              c["pair_count"], c["reg_s"], c["reg_g"], c["reg_sg"])
    assert np.all(np.abs(got - ref) <= 1e-15 * np.abs(ref)), (got, ref)
    assert got[7] == c["ce_out"][1]
    if base:
        assert got[4] == 0.0 and got[5] == 0.0


def test_disent_losses_reject_bad_arguments_before_launching():
    c = losses_case(3, seed=9)
    bad = [{"sse_node": None}, {"sse_spatial": None}, {"ce_out": None}, {"reg_sg": None}, {"losses": None},
           {"node_blocks": 0}, {"spatial_blocks": 0}, {"node_blocks": -2}, {"node_count": 0.0},
           {"spatial_count": -1.0}, {"pair_count": 0.0}, {"pair_count": float("nan")}]
    for over in bad:
        rc, got, _lib = run_losses(c, **over)
        assert rc == ERR_ARG, over
        assert "snd_disent_losses" in _lib.last_error()
        assert np.all(np.isnan(got)), over                              # nothing was written
