"""snd_zzt_edges (fused zz^T edge extraction: the predicted graph as a CSR) on the GPU.

The reference is float64 NumPy on the same fp32 z.

* Exact: z on small dyadic grids (integers / 8, a few rows x 4, one zero row), so every fp32
  product and partial sum is exact and rowptr / colidx / nnz must equal np.nonzero(L > tau).
* Real-valued z: the op's edge set may differ from the float64 one only on pairs whose logit
  lies within the fmaf-chain bound of the threshold; the output is exactly symmetric.
* The raw entry point on guarded, strided operands; capacity one short; the sizing call.
* Rejected arguments, the model-level identities against generate() / evaluate(), capture.
"""
import functools
import math

import numpy as np
import pytest
import torch

import abi_ops as A

pytestmark = pytest.mark.gpu

INF = float("inf")
T = 128                                                   # the kernel's tile


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


# ------------------------------------------------------------------ reference
def logits64(z):
    """Per graph the float64 logits of fp32 z [B, n, d]."""
    return [zb @ zb.T for zb in z.astype(np.float64)]


def ref_edges(z, tau, inclusive, logits=None):
    """(rowptr, colidx) of fp32 z [B, n, d]: float64 logits (``logits64(z)``, computed here
    when not given), edge iff i != j and L > tau (>= when inclusive), global ascending column
    ids."""
    B, n, _ = z.shape
    counts, cols = [], []
    for b, L in enumerate(logits64(z) if logits is None else logits):
        m = (L >= tau) if inclusive else (L > tau)
        np.fill_diagonal(m, False)
        counts.append(m.sum(axis=1))
        cols.append(np.nonzero(m)[1] + b * n)
    rp = np.zeros(B * n + 1, np.int64)
    np.cumsum(np.concatenate(counts), out=rp[1:])
    return rp, np.concatenate(cols).astype(np.int64)


EXACT_SHAPES = [(3, 200, 16), (2, 129, 64), (1, 25, 20), (2, 384, 128), (1, 1, 16), (1, 128, 64),
                (2, 257, 50), (260, 200, 16), (20, 1100, 16)]
# (tau, inclusive)
EXACT_RULES = [(0.0, 0), (0.0, 1), (0.5, 0), (-1.0, 0), (-INF, 0), (INF, 0)]


@functools.lru_cache(maxsize=None)
def exact_z(B, n, d):
    """The dyadic grid of test_gpu_eval.exact_case, with row 3 of every graph zero: its
    logits are all exactly 0, so the row is empty at L > 0 and full at L >= 0."""
    rng = np.random.default_rng(1000 * B + n + d)
    m = 16 if d <= 20 else (8 if d <= 64 else 4)       # multiples of 1/8; narrower for wide d
    z = rng.integers(-m, m + 1, size=(B, n, d)).astype(np.float32) / 8.0
    z[:, [r for r in (0, 1, 11) if r < n]] *= 4.0      # a few rows reach past +-16
    if n > 3:
        z[:, 3] = 0.0
    z.setflags(write=False)
    return z


def run_op(z, tau=0.0, inclusive=False, capacity=None):
    from snd_vae_amd import layers
    B, n, d = z.shape
    zt = torch.from_numpy(z.reshape(B * n, d).copy()).cuda()
    rp, ci, nnz = layers.zzt_edges(zt, B, n, tau, inclusive, capacity)
    torch.cuda.synchronize()
    if capacity is not None:
        nnz = int(nnz.item())
    return rp.cpu().numpy(), ci.cpu().numpy(), nnz


def test_exact_cases_hold_the_edge_cases():
    """On the CPU: the exact cases hold off-diagonal pairs with L == 0 (the inclusive flag
    changes the answer), an empty row, a full row and a row whose hits span >= 3 tiles, at a
    finite threshold."""
    z = exact_z(2, 384, 128)
    n = 384
    L = z[0].astype(np.float64) @ z[0].astype(np.float64).T
    off = ~np.eye(n, dtype=bool)
    assert ((L == 0) & off).sum() >= n - 1
    rp0, ci0 = ref_edges(z, 0.0, False)
    rp1, ci1 = ref_edges(z, 0.0, True)
    assert rp1[-1] > rp0[-1]
    deg0, deg1 = np.diff(rp0), np.diff(rp1)
    assert deg0[3] == 0 and deg1[3] == n - 1                    # empty at >, full at >=
    row = ci0[rp0[5]:rp0[6]]
    assert len(np.unique(row // T)) >= 3                        # one row, three tiles
    rp, ci = ref_edges(exact_z(20, 1100, 16)[:1], 0.0, False)
    assert len(np.unique(ci[rp[5]:rp[6]] // T)) == math.ceil(1100 / T)     # and one over all nine


@pytest.mark.parametrize("B,n,d", EXACT_SHAPES)
def test_exact_csr(B, n, d):
    z = exact_z(B, n, d)
    logits = logits64(z)                                  # once per case
    for tau, inclusive in EXACT_RULES:
        want_rp, want_ci = ref_edges(z, tau, bool(inclusive), logits)
        rp, ci, nnz = run_op(z, tau, bool(inclusive))
        what = (B, n, d, tau, inclusive)
        assert nnz == want_rp[-1], (what, nnz, int(want_rp[-1]))
        assert rp.dtype == np.int32 and ci.dtype == np.int32 and ci.shape == (nnz,)
        assert np.array_equal(rp, want_rp), what
        assert np.array_equal(ci, want_ci), what
        if tau == -INF:
            assert nnz == B * n * (n - 1)
        if tau == INF:
            assert nnz == 0


# ------------------------------------------------------------------ real-valued
@pytest.mark.parametrize("B,n,d,seed", [(2, 200, 64, 77), (1, 384, 128, 80)])
def test_real_valued_within_fmaf_bound(B, n, d, seed):
    """z = 0.5 randn against float64 logits of the same fp32 z.  An fp32 fmaf chain of d
    terms is within gamma_d sum_k |z_ik z_jk| of the exact logit (gamma_d = d u / (1 - d u),
    u = 2^-24), so the op's edge set and the float64 one may differ only on the near pairs,
    those with |L - tau| <= that bound; the near set is at most 0.1 % of the pairs, so the
    subset test means something.  The products commute and k runs in one order, so the
    output is exactly symmetric."""
    rng = np.random.default_rng(seed)
    z = (0.5 * rng.standard_normal((B, n, d))).astype(np.float32)
    u = 2.0 ** -24
    gamma = d * u / (1.0 - d * u)
    off = ~np.eye(n, dtype=bool)
    pairs = B * (n * n - n)
    for tau in (0.0, 0.5, -0.75, 1.0):
        rp, ci, nnz = run_op(z, tau)
        got = np.zeros((B * n, n), bool)
        got[np.repeat(np.arange(B * n), np.diff(rp)), ci % n] = True
        assert np.array_equal(ci // n, np.repeat(np.arange(B * n), np.diff(rp)) // n)   # own block
        near_total = diff_total = 0
        for b in range(B):
            zb = z[b].astype(np.float64)
            L = zb @ zb.T
            near = (np.abs(L - tau) <= gamma * (np.abs(zb) @ np.abs(zb).T)) & off
            g = got[b * n:(b + 1) * n]
            diff = g != ((L > tau) & off)
            assert not (diff & ~near).any(), (tau, b, int((diff & ~near).sum()))
            assert np.array_equal(g, g.T), (tau, b)
            near_total += int(near.sum())
            diff_total += int(diff.sum())
        print(f"EDGES_REAL {(B, n, d)} tau {tau} nnz {nnz} near {near_total} of {pairs} differ {diff_total}")
        assert near_total <= 0.001 * pairs, (tau, near_total, pairs)
        assert 0 < nnz < pairs


# ------------------------------------------------------------------ raw ABI
I32_PAT = np.int32(A.PATTERN["i32"][2])


def _raw_call(L, _lib, ptr, ld, B, n, d, tau, inclusive, colidx_ptr, cap, ws):
    return L.snd_zzt_edges(ptr["z"], ld, B, n, d, tau, inclusive, ptr["rowptr"], colidx_ptr, cap, ptr["nnz"],
                           _lib.ptr(ws), ws.numel(), _lib.stream_ptr())


@pytest.mark.parametrize("ld,offset", [(72, 0), (67, 1)], ids=["ld72_aligned", "ld67_unaligned"])
def test_raw_abi_guarded(ld, offset):
    """ldz > d through the raw entry point with guard bands around z, rowptr, colidx and
    *nnz_out (the int64 rides in the helpers' 8-byte "f64" buffer): capacity exactly nnz,
    one short of it, the sizing call, and two runs bitwise equal."""
    from snd_vae_amd import _lib
    B, n, d = 2, 129, 64
    z = exact_z(B, n, d)
    want_rp, want_ci = ref_edges(z, 0.0, False)
    total = int(want_rp[-1])
    L = _lib.lib()
    wsb = L.snd_zzt_edges_workspace(B, n, d)
    assert wsb >= B * n * 4
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")

    def fresh(cap):
        bufs = {"z": A.guarded(B * n, d, ld, "f32", offset, z.reshape(B * n, d), "z"),
                "rowptr": A.guarded(1, B * n + 1, None, "i32", 0, None, "rowptr"),
                "colidx": A.guarded(1, cap, None, "i32", 0, None, "colidx"),
                "nnz": A.guarded(1, 1, None, "f64", 0, None, "nnz")}
        dev = {k: torch.from_numpy(g.arr).cuda() for k, g in bufs.items()}
        ptr = {k: dev[k].data_ptr() + g.off * g.arr.itemsize for k, g in bufs.items()}
        return bufs, dev, ptr

    def after_of(bufs, dev):
        torch.cuda.synchronize()
        after = {k: t.cpu().numpy() for k, t in dev.items()}
        for k, g in bufs.items():
            g.check_untouched(after[k])
        assert np.array_equal(after["z"].view(np.uint32), bufs["z"].arr.view(np.uint32))
        return after

    def outputs(bufs, after):
        return (bufs["rowptr"].block(after["rowptr"]).ravel(), bufs["colidx"].block(after["colidx"]).ravel(),
                int(np.ascontiguousarray(bufs["nnz"].block(after["nnz"])).view(np.int64)[0, 0]))

    # capacity exactly nnz, twice
    runs = []
    for _ in range(2):
        bufs, dev, ptr = fresh(total)
        _lib.check(_raw_call(L, _lib, ptr, ld, B, n, d, 0.0, 0, ptr["colidx"], total, ws), "snd_zzt_edges")
        after = after_of(bufs, dev)
        rp, ci, nnz = outputs(bufs, after)
        assert nnz == total and np.array_equal(rp, want_rp) and np.array_equal(ci, want_ci)
        runs.append(after)
    for k in ("rowptr", "colidx", "nnz"):
        assert np.array_equal(runs[0][k].view(np.uint8), runs[1][k].view(np.uint8)), k

    # capacity one short: colidx wholly untouched, rowptr and the total still right, rc 0
    bufs, dev, ptr = fresh(total - 1)
    assert _raw_call(L, _lib, ptr, ld, B, n, d, 0.0, 0, ptr["colidx"], total - 1, ws) == 0
    after = after_of(bufs, dev)
    rp, ci, nnz = outputs(bufs, after)
    assert nnz == total and np.array_equal(rp, want_rp)
    assert (ci == I32_PAT).all()

    # colidx = NULL: the count pass only
    bufs, dev, ptr = fresh(total)
    assert _raw_call(L, _lib, ptr, ld, B, n, d, 0.0, 0, None, 0, ws) == 0
    after = after_of(bufs, dev)
    rp, ci, nnz = outputs(bufs, after)
    assert nnz == total and np.array_equal(rp, want_rp)
    assert (ci == I32_PAT).all()


# ------------------------------------------------------------------ argument errors
def test_rejected_arguments():
    from snd_vae_amd import _lib, layers
    n, d = 8, 16
    with pytest.raises(_lib.SNDError, match="d=129"):
        layers.zzt_edges(torch.zeros(n, 129, device="cuda"), 1, n)
    L = _lib.lib()
    P = _lib.ptr
    z = torch.ones(n, d, device="cuda")
    rowptr = torch.full((n + 1,), 5, dtype=torch.int32, device="cuda")
    colidx = torch.full((n * n,), 5, dtype=torch.int32, device="cuda")
    nnz = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    wsb = L.snd_zzt_edges_workspace(1, n, d)
    assert wsb > 0 and L.snd_zzt_edges_workspace(1, n, 129) == 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")

    def call(zp=None, ldz=d, dd=d, thr=0.0, rp=None, nz=None, wbytes=wsb):
        return L.snd_zzt_edges(P(z) if zp is None else zp, ldz, 1, n, dd, thr, 0, P(rowptr) if rp is None else rp,
                               P(colidx), n * n, P(nnz) if nz is None else nz, P(ws), wbytes, _lib.stream_ptr())

    for kw, msg in ((dict(dd=129, ldz=129), "d=129"), (dict(ldz=15), "ldz"), (dict(zp=0), "null"),
                    (dict(rp=0), "null"), (dict(nz=0), "null"), (dict(thr=float("nan")), "NaN"),
                    (dict(wbytes=wsb - 1), "workspace")):
        assert call(**kw) == -1, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert int(rowptr.min()) == 5 == int(rowptr.max()) and int(colidx.min()) == 5 == int(colidx.max())
    assert int(nnz.item()) == 5                               # nothing was launched
    assert call() == 0                                        # and the same operands are accepted
    torch.cuda.synchronize()
    assert int(nnz.item()) == n * (n - 1)                     # z = 1: every logit is d > 0


# ------------------------------------------------------------------ model level
def _csr_pairs(rp, ci, n):
    """Per global row the local column ids, as a dense bool [B*n, n]."""
    rows = rp.shape[0] - 1
    m = np.zeros((rows, n), bool)
    owner = np.repeat(np.arange(rows), np.diff(rp))
    assert np.array_equal(ci // n, owner // n)
    m[owner, ci % n] = True
    return m


@pytest.mark.parametrize("preset,dtype", [("C1s", "f32"), ("C1s", "bf16"), ("C1", "f32"), ("C1", "bf16"),
                                          ("SG25", "f32")])
def test_model_generate_csr(preset, dtype):
    """Node latent (C1s), graph latent (C1) and the spatial-graph encoder (SG25)."""
    from snd_vae_amd.config import PRESETS
    from snd_vae_amd.data import generated_batch, sgjoint_batch, synthetic_batch
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    cfg = PRESETS[preset]
    B, n = 2, cfg.n_nodes
    batch = sgjoint_batch(cfg, B, seed=31) if preset == "SG25" else synthetic_batch(cfg, B, seed=31)
    model = SGCNModelVAE(cfg, B, dtype=dtype, seed=4)
    db = DeviceBatch(batch)

    # the CSR is the dense generated_adj, and the default output is what it was
    dense = model.generate(db, mode="mean")
    assert set(dense) == {"generated_adj", "generated_spatial", "generated_node_feat", "z", "z_mean", "z_std"}
    g = dense["generated_adj"]
    assert g.dtype == torch.uint8 and tuple(g.shape) == (B, n, n)
    g = g.cpu().numpy()
    out = model.generate(db, mode="mean", adj_format="csr")
    assert out["generated_adj"] is None
    rp, ci = out["generated_rowptr"].cpu().numpy(), out["generated_colidx"].cpu().numpy()
    rows, cols = np.nonzero(g.reshape(B * n, n))
    assert out["generated_nnz"] == len(rows) == rp[-1] and 0 < len(rows) < g.size
    assert np.array_equal(rp, np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=B * n))]))
    assert np.array_equal(ci, cols + rows // n * n)
    for k in ("generated_spatial", "generated_node_feat", "z", "z_mean", "z_std"):
        assert torch.equal(out[k], dense[k]), k
    again = model.generate(db, mode="mean")
    assert torch.equal(again["generated_adj"], dense["generated_adj"])

    # the threshold best_f1 reports, applied: exactly that F1
    thr, f1 = model.evaluate(db, mode="mean").total().best_f1()
    best = model.generate(db, mode="mean", adj_format="csr", threshold=thr, inclusive=True)
    pred = _csr_pairs(best["generated_rowptr"].cpu().numpy(), best["generated_colidx"].cpu().numpy(), n)
    truth = np.concatenate([batch.dense_adj(b) != 0 for b in range(B)])
    tp, fp = float((pred & truth).sum()), float((pred & ~truth).sum())
    assert 2.0 * tp / (tp + fp + float(truth.sum())) == f1, (thr, f1, tp, fp)

    # a generated graph goes back in as a batch and scores itself perfectly
    gb = generated_batch(cfg, rp, ci, out["generated_node_feat"].cpu().numpy(),
                         out["generated_spatial"].cpu().numpy(), B)
    assert gb.nnz == out["generated_nnz"] and gb.features.shape[0] == B * n
    ec = model.evaluate(DeviceBatch(gb), mode="given", z=out["z"])
    c = ec.counts.sum(axis=0)
    assert c[0] == out["generated_nnz"] and c[1] == 0 and c[2] == 0, c


# ------------------------------------------------------------------ capture
def test_graph_capture_replays_the_eager_bytes():
    from snd_vae_amd import layers
    B, n, d = 2, 200, 64
    rng = np.random.default_rng(5)
    zs = [torch.from_numpy((0.5 * rng.standard_normal((B * n, d))).astype(np.float32)).cuda() for _ in range(2)]
    cap = B * n * n
    eager = []
    for zt in zs:
        rp, ci, nnz = layers.zzt_edges(zt, B, n, 0.25, False, capacity=cap)
        torch.cuda.synchronize()
        eager.append((rp.cpu().numpy(), ci.cpu().numpy()[:int(nnz.item())], int(nnz.item())))
    assert eager[0][2] != eager[1][2] and 0 < eager[0][2] < cap
    zin = zs[0].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        layers.zzt_edges(zin, B, n, 0.25, False, capacity=cap)       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rp, ci, nnz = layers.zzt_edges(zin, B, n, 0.25, False, capacity=cap)
    for zt, want in zip(zs[::-1], eager[::-1]):                      # the other operand first
        zin.copy_(zt)
        graph.replay()
        torch.cuda.synchronize()
        total = int(nnz.item())
        assert total == want[2]
        assert np.array_equal(rp.cpu().numpy(), want[0])
        assert np.array_equal(ci.cpu().numpy()[:total], want[1])
