"""Per-op parity of the HIP kernels (libsndvae.so) against the CPU oracle.

fp32 operands: the oracle's float64 result within fp32 accumulation error.
bf16 operands (fp32 accumulation): documented looser tolerance.
Integer/index work (CSR ingest, accuracy counts): bit-exact.
"""
import numpy as np
import pytest
import torch

from oracle import ref_numpy as R
from snd_vae_amd.config import tscale
from snd_vae_amd.data import csr_from_dense, rgg_edges, csr_from_pairs, stack_csr, synthetic_batch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from snd_vae_amd import layers
    return layers


def cu(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def rand_batch_csr(n, B, kbar, seed):
    parts = []
    for b in range(B):
        _, pairs = rgg_edges(n, kbar, np.random.default_rng(seed + b))
        parts.append(csr_from_pairs(n, pairs))
    rp, ci = stack_csr(parts, n)
    return rp, ci, None


def rand_batch(n, B, kbar, seed):
    parts = []
    for b in range(B):
        _, pairs = rgg_edges(n, kbar, np.random.default_rng(seed + b))
        parts.append(csr_from_pairs(n, pairs))
    rp, ci = stack_csr(parts, n)
    dense = []
    for b in range(B):
        a = np.zeros((n, n))
        for i in range(n):
            s, e = rp[b * n + i], rp[b * n + i + 1]
            a[i, ci[s:e] - b * n] = 1
        dense.append(a)
    return rp, ci, dense


@pytest.mark.parametrize("width", [64, 48, 128])
def test_spmm_plain(width):
    from snd_vae_amd import layers
    n, B = 300, 3
    rp, ci, dense = rand_batch(n, B, 10.0, 1)
    h = np.random.default_rng(0).standard_normal((n * B, width)).astype(np.float32)
    out = layers.spmm(cu(rp, torch.int32), cu(ci, torch.int32), cu(h)).cpu().numpy()
    ref = R.spmm(dense, h.astype(np.float64), n)
    assert rel(out, ref) < 1e-6


@pytest.mark.parametrize("n,B,kbar,width", [(256, 8, 12.0, 64), (300, 3, 10.0, 128),
                                             (96, 2, 2.0, 48), (64, 8, 0.0, 64)])
def test_spmm_bf16(n, B, kbar, width):
    """bf16 rows, fp32 accumulation, bf16 out; XCD row-block order when n % 32 == 0 and
    B % 8 == 0.  Isolated nodes (kbar 2, 0) give all-zero rows."""
    from snd_vae_amd import layers
    rp, ci, dense = rand_batch(n, B, kbar, 5)
    h = torch.from_numpy(np.random.default_rng(1).standard_normal((n * B, width)).astype(np.float32))
    hb = h.to(torch.bfloat16)
    out = layers.spmm_bf16(cu(rp, torch.int32), cu(ci if len(ci) else np.zeros(1, np.int32), torch.int32),
                           hb.cuda(), n, B).float().cpu().numpy()
    ref = R.spmm(dense, hb.float().numpy().astype(np.float64), n)
    assert np.abs(out - ref).max() <= 2 ** -7 * max(np.abs(ref).max(), 1.0)
    iso = np.diff(rp) == 0
    assert np.all(out[iso] == 0.0)
    # the locality schedule changes the processing order only: bitwise-equal rows
    from snd_vae_amd.data import GraphBatch, locality_order
    gb = GraphBatch(B, n, rp, ci, np.zeros((n * B, 1), np.float32), np.zeros((n * B, 1), np.float32),
                    np.zeros((n * B, 2), np.float32))
    order = locality_order(gb)
    assert np.array_equal(np.sort(order), np.arange(n * B))
    assert all(set(order[b * n:(b + 1) * n]) == set(range(b * n, (b + 1) * n)) for b in range(B))
    out2 = layers.spmm_bf16(cu(rp, torch.int32), cu(ci if len(ci) else np.zeros(1, np.int32), torch.int32),
                            hb.cuda(), n, B, cu(order, torch.int32)).float().cpu().numpy()
    assert np.array_equal(out, out2)


@pytest.mark.parametrize("n,B,kbar,width,tile_rows,locality",
                         [(4096, 8, 16.0, 64, 64, True), (4096, 64, 16.0, 64, 64, True),
                          (4096, 8, 16.0, 64, 128, True), (4096, 2, 16.0, 64, 64, False),
                          (2048, 1, 16.0, 128, 64, True), (300, 3, 10.0, 48, 64, True),
                          (96, 2, 0.0, 64, 32, True), (200, 1, 8.0, 64, 7, True),
                          (256, 4, 40.0, 64, 64, True), (1000, 3, 16.0, 128, 100, True)])
def test_spmm_bf16_tiled_bitwise(n, B, kbar, width, tile_rows, locality):
    """The LDS-staged, pipelined SpMM over row tiles sums every row's neighbours in
    colidx order: bitwise equal to spmm_bf16.  64 graphs give every workgroup a run
    of several tiles (the pipeline); natural order at N = 4096 makes the sets exceed
    the 319-row LDS image, so the launch takes the register-gather kernel; degree
    ~40 rows take the lcol-reading rounds past the 32 prefetched ids; 100-row tiles
    put two rows on an 8-lane group."""
    from snd_vae_amd import layers
    from snd_vae_amd.data import GraphBatch, locality_order, row_tiles
    from snd_vae_amd.model import DeviceTiles
    rp, ci, dense = rand_batch(n, B, kbar, 9) if B <= 8 else rand_batch_csr(n, B, kbar, 9)
    gb = GraphBatch(B, n, rp, ci, np.zeros((n * B, 1), np.float32), np.zeros((n * B, 1), np.float32),
                    np.zeros((n * B, 2), np.float32))
    order = locality_order(gb) if locality else None
    rt = row_tiles(gb, order, tile_rows)
    if not locality and n >= 2048:
        assert rt.ustride > 319                          # the register-gather fallback
    tiles = DeviceTiles(rt)
    hb = torch.from_numpy(np.random.default_rng(2).standard_normal((n * B, width)).astype(np.float32)).to(torch.bfloat16)
    d_rp, d_ci = cu(rp, torch.int32), cu(ci if len(ci) else np.zeros(1, np.int32), torch.int32)
    d_o = cu(order, torch.int32) if order is not None else None
    ref = layers.spmm_bf16(d_rp, d_ci, hb.cuda(), n, B, d_o)
    out = layers.spmm_bf16_tiled(d_rp, d_ci, tiles, hb.cuda(), n, B, d_o)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    if dense is not None:
        r64 = R.spmm(dense, hb.float().numpy().astype(np.float64), n)
        assert np.abs(out.float().cpu().numpy() - r64).max() <= 2 ** -7 * max(np.abs(r64).max(), 1.0)


@pytest.mark.parametrize("n,B,kbar,seed", [(4096, 8, 16.0, 9), (4096, 64, 16.0, 9), (4096, 1, 16.0, 3),
                                             (1000, 3, 16.0, 4), (300, 3, 10.0, 5), (96, 2, 0.0, 6),
                                             (256, 4, 40.0, 7), (200, 1, 50.0, 8), (130, 5, 3.0, 2)])
def test_spmm_bf16_window_bitwise(n, B, kbar, seed):
    """The sliding-window SpMM (h rows DMA'd once into a 1096-row LDS ring, two
    128-row steps ahead) sums every row's neighbours in colidx order: bitwise equal
    to spmm_bf16.  64 graphs: one workgroup per graph, 32 steps; 8 graphs: 32
    one-step segments per graph; n = 1000 / 130: partial last steps; kbar 40 / 50:
    rows past 32 neighbours; kbar 0: empty rows.  N = 4096 (beta ~ 260): one
    barrier per step, and (forced) the two-barrier step of wider windows."""
    from snd_vae_amd import layers
    from snd_vae_amd.data import GraphBatch, locality_order, window_plan
    rp, ci, dense = rand_batch(n, B, kbar, seed) if B <= 8 else rand_batch_csr(n, B, kbar, seed)
    gb = GraphBatch(B, n, rp, ci, np.zeros((n * B, 1), np.float32), np.zeros((n * B, 1), np.float32),
                    np.zeros((n * B, 2), np.float32))
    order = locality_order(gb)
    wp = window_plan(gb, order)
    assert (wp.beta + 7) // 8 * 8 <= 352
    if kbar >= 40:
        assert wp.max_degree > 32
    hb = torch.from_numpy(np.random.default_rng(seed).standard_normal((n * B, 64)).astype(np.float32)).to(torch.bfloat16)
    d_rp, d_ci = cu(rp, torch.int32), cu(ci if len(ci) else np.zeros(1, np.int32), torch.int32)
    ref = layers.spmm_bf16(d_rp, d_ci, hb.cuda(), n, B, cu(order, torch.int32))
    out = layers.spmm_bf16_window(layers.DeviceWindowPlan(wp), hb.cuda(), n, B)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    if n == 4096:
        # the two-barrier step (the schedule for beta > 288), forced by debug bit 32 << 24,
        # and the unbalanced group order (wave w sums group w, bit 64 << 24): same sums
        from snd_vae_amd import _lib
        for flag in (32 << 24, 64 << 24):
            _lib.check(_lib.lib().snd_debug_set(flag))
            try:
                out2 = layers.spmm_bf16_window(layers.DeviceWindowPlan(wp), hb.cuda(), n, B)
                torch.cuda.synchronize()
            finally:
                _lib.check(_lib.lib().snd_debug_set(0))
            assert torch.equal(out2.view(torch.int16), ref.view(torch.int16)), flag
    if dense is not None:
        r64 = R.spmm(dense, hb.float().numpy().astype(np.float64), n)
        assert np.abs(out.float().cpu().numpy() - r64).max() <= 2 ** -7 * max(np.abs(r64).max(), 1.0)


def test_gather_sums_nonfinite_column_pairing():
    """Pins how a non-finite bf16 value spreads in the dot2 gather sums: every
    gather kernel adds the low / high bf16 of a 32-bit word through v_dot2_f32_bf16 with
    (1, 0) / (0, 1), so the other half of the word is multiplied by 0 -- an inf in column
    2c turns column 2c + 1 of every neighbouring output row into NaN (inf * 0), and the
    other columns stay finite.  Finite inputs are unaffected (bitwise the widening adds)."""
    from snd_vae_amd import layers
    from snd_vae_amd.data import GraphBatch, locality_order, window_plan
    n, B = 512, 1
    rp, ci, _ = rand_batch(n, B, 8, 5)
    gb = GraphBatch(B, n, rp, ci, np.zeros((n, 1), np.float32), np.zeros((n, 1), np.float32),
                    np.zeros((n, 2), np.float32))
    order = locality_order(gb)
    h = np.random.default_rng(1).standard_normal((n, 64)).astype(np.float32)
    bad = int(np.argmax(np.diff(rp)))              # a row with neighbours
    h[bad, 6] = np.inf                             # word 3 = (column 6, column 7)
    hb = torch.from_numpy(h).to(torch.bfloat16)
    d_rp, d_ci = cu(rp, torch.int32), cu(ci, torch.int32)
    outs = [layers.spmm_bf16(d_rp, d_ci, hb.cuda(), n, B, cu(order, torch.int32)),
            layers.spmm_bf16_window(layers.DeviceWindowPlan(window_plan(gb, order)), hb.cuda(), n, B)]
    torch.cuda.synchronize()
    touched = np.array([bad in ci[rp[r]:rp[r + 1]] for r in range(n)])
    for o in outs:
        o = o.float().cpu().numpy()
        assert np.isinf(o[touched, 6]).all() and np.isnan(o[touched, 7]).all()
        assert np.isfinite(np.delete(o[touched], [6, 7], axis=1)).all()
        assert np.isfinite(o[~touched]).all()


def test_spmm_bf16_window_rejects_wide_window():
    """Natural (generator) order puts neighbours ~N apart: the window plan's beta
    exceeds the ring and the launch refuses (the caller keeps the tiled kernel)."""
    from snd_vae_amd import _lib, layers
    from snd_vae_amd.data import GraphBatch, window_plan
    n, B = 4096, 1
    rp, ci = rand_batch_csr(n, B, 16.0, 1)[:2]
    gb = GraphBatch(B, n, rp, ci, np.zeros((n, 1), np.float32), np.zeros((n, 1), np.float32),
                    np.zeros((n, 2), np.float32))
    wp = window_plan(gb, np.arange(n, dtype=np.int32))
    assert wp.beta > 352
    with pytest.raises(_lib.SNDError):
        layers.spmm_bf16_window(layers.DeviceWindowPlan(wp), torch.zeros(n, 64, dtype=torch.bfloat16, device="cuda"), n, B)


def test_graph_convolution_epilogue():
    from snd_vae_amd import layers
    n, B, f, w = 150, 2, 3, 64
    rp, ci, dense = rand_batch(n, B, 8.0, 4)
    rng = np.random.default_rng(1)
    X = rng.random((n * B, f)).astype(np.float32)
    H = rng.standard_normal((n * B, 67)).astype(np.float32)
    W = (0.3 * rng.standard_normal((67, w))).astype(np.float32)
    g, b = (1 + 0.1 * rng.standard_normal(w)).astype(np.float32), (0.1 * rng.standard_normal(w)).astype(np.float32)
    ge, be = (1 + 0.1 * rng.standard_normal(w + f)).astype(np.float32), (0.1 * rng.standard_normal(w + f)).astype(np.float32)
    out, pre, out2 = layers.graph_convolution(cu(rp, torch.int32), cu(ci, torch.int32), cu(H), cu(W),
                                              cu(g), cu(b), cu(X), cu(ge), cu(be))
    P = R.spmm(dense, H.astype(np.float64) @ W, n)
    Bo = R.lrelu(P) * g * R.BN_C + b
    H2 = np.concatenate([Bo, X], 1)
    G = H2 * ge * R.BN_C + be
    assert rel(pre.cpu().numpy(), P) < 1e-5
    assert rel(out.cpu().numpy(), H2) < 1e-5
    assert rel(out2.cpu().numpy(), G) < 1e-5


@pytest.mark.parametrize("dtype,tol", [("f32", 2e-6), ("bf16", 1.5e-2)])
@pytest.mark.parametrize("m,n,k,tw", [(1000, 64, 3, False), (777, 67, 130, False),
                                      (4096, 128, 64, False), (513, 64, 128, True)])
def test_gemm(dtype, tol, m, n, k, tw):
    from snd_vae_amd import layers
    rng = np.random.default_rng(m + n + k)
    x = rng.standard_normal((m, k)).astype(np.float32)
    w = rng.standard_normal((n, k) if tw else (k, n)).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    out = layers.linear(cu(x), cu(w), cu(b), dtype, trans_w=tw).cpu().numpy()
    ref = x.astype(np.float64) @ (w.T if tw else w).astype(np.float64) + b
    assert rel(out, ref) < tol


@pytest.mark.parametrize("dtype,tol", [("f32", 2e-6), ("bf16", 1.5e-2)])
@pytest.mark.parametrize("n,B,cin,cout", [(37, 3, 20, 10), (64, 2, 64, 100), (5, 4, 50, 20)])
def test_conv1d_fwd_bwd(dtype, tol, n, B, cin, cout):
    from snd_vae_amd import layers
    rng = np.random.default_rng(n * cin)
    x = rng.standard_normal((n * B, cin)).astype(np.float32)
    w = (0.2 * rng.standard_normal((5, cin, cout))).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(cout)).astype(np.float32)
    be = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    out, pre = layers.conv1d_same(cu(x), cu(w), cu(b), n, cu(g), cu(be), dtype)
    ref_pre = R.per_graph_conv(x.astype(np.float64), w.astype(np.float64), b, n)
    assert rel(pre.cpu().numpy(), ref_pre) < tol
    assert rel(out.cpu().numpy(), R.lrelu(ref_pre * g * R.BN_C + be)) < tol
    dy = rng.standard_normal((n * B, cout)).astype(np.float32)
    dx, dw = layers.conv1d_same_bwd(cu(x), cu(w), cu(dy), n, dtype)
    rdx, rdw, _ = R.per_graph_conv_bwd(x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64), n)
    assert rel(dx.cpu().numpy(), rdx) < tol
    assert rel(dw.cpu().numpy(), rdw) < tol


def _zzt_case(n, d, B, kbar, seed, scale):
    rp, ci, dense = rand_batch(n, B, kbar, seed)
    z = (scale * np.random.default_rng(seed).standard_normal((n * B, d))).astype(np.float32)
    return rp, ci, dense, z


@pytest.mark.parametrize("n,d,B,kbar", [(200, 16, 2, 8.0), (257, 64, 2, 12.0), (130, 32, 3, 6.0),
                                        (64, 128, 1, 10.0), (1, 16, 2, 0.0), (90, 64, 2, 0.0)])
def test_zzt_ce_f32(n, d, B, kbar):
    from snd_vae_amd import layers
    rp, ci, dense, z = _zzt_case(n, d, B, kbar, n + d, 0.4)
    ce, correct, dz = layers.inner_product_ce(cu(z), B, cu(rp, torch.int32), cu(ci, torch.int32),
                                              dtype="f32")
    rce, rdz, rcorrect = R.adj_ce(z.astype(np.float64), dense, n)
    assert ce == pytest.approx(rce, rel=2e-6)
    # accuracy: exact up to pairs whose logit sign is within fp32 rounding of 0
    L = [z[b * n:(b + 1) * n].astype(np.float64) @ z[b * n:(b + 1) * n].T.astype(np.float64) for b in range(B)]
    ambiguous = sum(int((np.abs(l) < 1e-5).sum()) for l in L)
    assert abs(correct - rcorrect) <= ambiguous
    assert rel(dz.cpu().numpy(), rdz) < 1e-5


@pytest.mark.parametrize("n,d,B,scale", [(300, 64, 2, 0.25), (128, 128, 2, 0.25), (300, 32, 3, 0.3),
                                         (700, 64, 1, 0.25), (257, 64, 2, 1.0), (130, 16, 2, 0.5),
                                         (700, 128, 1, 0.25), (257, 128, 2, 0.7), (1100, 128, 3, 0.2)])
def test_zzt_ce_bf16(n, d, B, scale):
    """bf16 zz^T + CE (v4 for d <= 64: 32x32x16 MFMA, select-free epilogue; v7 for d = 128:
    one dual-use LDS image per tile, transposed reads for the backward operand).
    (700, d, 1): column splits; scale 1.0: logits up to |L| ~ 40."""
    from snd_vae_amd import layers
    rp, ci, dense, z = _zzt_case(n, d, B, 10.0, 7, scale)
    ce, correct, dz = layers.inner_product_ce(cu(z), B, cu(rp, torch.int32), cu(ci, torch.int32),
                                              dtype="bf16")
    rce, rdz, rcorrect = R.adj_ce(z.astype(np.float64), dense, n)
    assert ce == pytest.approx(rce, rel=2e-3)
    assert abs(correct - rcorrect) <= 0.01 * B * n * n
    assert rel(dz.cpu().numpy(), rdz) < 2e-2


@pytest.mark.parametrize("d", [64, 128])
def test_zzt_ce_bf16_extreme_logits(d):
    """Planted blocks of logits far beyond the v4/v7 quad-product range (L = -100 between
    rows 0-3 and 4-7, +100 inside each block): the overflow fallback keeps the CE exact."""
    from snd_vae_amd import layers
    n, B = 200, 2
    rp, ci, dense, z = _zzt_case(n, d, B, 8.0, 11, 0.25)
    a = np.zeros(d, np.float32)
    a[:4] = 5.0                                   # |a|^2 = 100
    for b in range(B):
        z[b * n:b * n + 4] = a
        z[b * n + 4:b * n + 8] = -a
    ce, correct, dz = layers.inner_product_ce(cu(z), B, cu(rp, torch.int32), cu(ci, torch.int32),
                                              dtype="bf16")
    rce, rdz, rcorrect = R.adj_ce(z.astype(np.float64), dense, n)
    assert np.isfinite(ce)
    assert ce == pytest.approx(rce, rel=2e-3)
    assert abs(correct - rcorrect) <= 0.01 * B * n * n
    assert rel(dz.cpu().numpy(), rdz) < 2e-2


@pytest.mark.parametrize("n,d,B", [(4096, 64, 8), (300, 32, 3), (4096, 64, 1), (200, 16, 2)])
def test_zzt_variants_match_in_step(n, d, B):
    """The step's zz^T launch in both shipped bf16 kernels on the same staged z: v4 (the
    default: 32x32x16 MFMAs, signed epilogue, 4 waves per SIMD) against v1 (round 1's
    kernel: 8 waves x 16 rows, 16x16x32 MFMAs, the |x| epilogue with masks; bench.py's
    previous_variant): loss and count agree to bf16 rounding, dJ within bf16 operand
    rounding.  B = 1 at N = 4096 runs v4's column splits (C3 per rank)."""
    from snd_vae_amd import _lib
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    from snd_vae_amd.optimizer import OptimizerVAE
    cfg = tscale(n, d)
    db = DeviceBatch(synthetic_batch(cfg, B, seed=1000))
    model = SGCNModelVAE(cfg, B, dtype="bf16")
    opt = OptimizerVAE(model)
    opt.step(db)
    torch.cuda.synchronize()
    L = _lib.lib()
    bc = db.c_struct()
    pz = model.buffer("PZZT", torch.float64)
    djd = model.buffer("DJD")
    out = {}
    for name in ("zzt_dense_v1", "zzt_dense"):
        pz.zero_()
        _lib.check(L.snd_plan_launch(model.plan, bc, model.workspace.data_ptr(), name.encode(),
                                     _lib.stream_ptr()))
        torch.cuda.synchronize()
        out[name] = (pz.view(-1, 2).sum(0).cpu().numpy(), djd.clone().cpu().numpy())
    (s1, d1), (s4, d4) = out["zzt_dense_v1"], out["zzt_dense"]
    assert s4[0] == pytest.approx(s1[0], rel=1e-4)
    assert abs(s4[1] - s1[1]) <= 1e-4 * B * n * n
    assert rel(d4, d1) < 1e-2


def test_zzt_ce_weighted_bce():
    from snd_vae_amd import layers
    n, d, B = 140, 32, 2
    rp, ci, dense, z = _zzt_case(n, d, B, 9.0, 3, 0.5)
    pw, nm = 3.5, 0.7
    ce, _, dz = layers.inner_product_ce(cu(z), B, cu(rp, torch.int32), cu(ci, torch.int32),
                                        pos_weight=pw, norm=nm, dtype="f32")
    rce, rdz, _ = R.adj_ce(z.astype(np.float64), dense, n, pos_weight=pw, norm=nm)
    assert ce == pytest.approx(rce, rel=2e-6)
    assert rel(dz.cpu().numpy(), rdz) < 1e-5


def test_zzt_ce_full_size_f32_and_bf16():
    """C2 size (N=4096, d=64): full oracle comparison for one graph."""
    from snd_vae_amd import layers
    n, d, B = 4096, 64, 1
    rp, ci, dense, z = _zzt_case(n, d, B, 16.0, 0, 0.2)
    rce, rdz, rcorrect = R.adj_ce(z.astype(np.float64), dense, n)
    ce, correct, dz = layers.inner_product_ce(cu(z), B, cu(rp, torch.int32), cu(ci, torch.int32), dtype="f32")
    assert ce == pytest.approx(rce, rel=2e-6)
    assert rel(dz.cpu().numpy(), rdz) < 1e-5
    ce16, c16, dz16 = layers.inner_product_ce(cu(z), B, cu(rp, torch.int32), cu(ci, torch.int32), dtype="bf16")
    assert ce16 == pytest.approx(rce, rel=2e-3)
    assert rel(dz16.cpu().numpy(), rdz) < 2e-2


def test_dense_to_csr_bit_exact():
    from snd_vae_amd import layers
    n, B = 333, 3
    rp, ci, dense = rand_batch(n, B, 9.0, 5)
    adj = np.stack(dense).astype(np.float32)
    adj[0, 5, 5] = 1.0                                   # diagonal is dropped (input_data.py:65)
    rpd, cid = layers.dense_to_csr(cu(adj))
    assert np.array_equal(rpd.cpu().numpy(), rp) and np.array_equal(cid.cpu().numpy(), ci)
    ref = [csr_from_dense(a) for a in dense]
    assert int(rpd[-1]) == sum(int(r[-1]) for r, _ in ref)


def test_adam_tf1_matches_oracle():
    from snd_vae_amd import _lib
    rng = np.random.default_rng(0)
    n = 1000
    p, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    tp, tg = cu(p), cu(g)
    tm, tv = torch.zeros_like(tp), torch.zeros_like(tp)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    po, mo, vo = {"w": p.astype(np.float64)}, {"w": np.zeros(n)}, {"w": np.zeros(n)}
    for t in range(1, 4):
        step.fill_(t)
        _lib.check(_lib.lib().snd_adam_tf1(tp.data_ptr(), tg.data_ptr(), tm.data_ptr(), tv.data_ptr(),
                                           n, 0.0008, 0.9, 0.999, 1e-8, 1.0, step.data_ptr(),
                                           _lib.stream_ptr()))
        R.adam_tf1(po, {"w": g.astype(np.float64)}, mo, vo, t, 0.0008)
    assert np.abs(tp.cpu().numpy() - po["w"]).max() < 1e-6


@pytest.mark.parametrize("ranges", [[(0, 1000), (2000, 400), (4096, 3000)],   # float4 launch
                                    [(3, 997), (2001, 398)]])                  # per-range fallback
def test_adam_tf1_ranges_equals_per_range_updates(ranges):
    """snd_adam_tf1_ranges (one launch over the blocks a fused update leaves) equals one
    snd_adam_tf1 per range, and leaves everything outside the ranges untouched."""
    import ctypes
    from snd_vae_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(3)
    n = 8192
    p, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    m0, v0 = 0.1 * rng.standard_normal(n).astype(np.float32), rng.random(n).astype(np.float32)
    step = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    out = []
    for multi in (False, True):
        tp, tg, tm, tv = cu(p), cu(g), cu(m0), cu(v0)
        if multi:
            off = (ctypes.c_longlong * len(ranges))(*[o for o, _ in ranges])
            cnt = (ctypes.c_longlong * len(ranges))(*[c for _, c in ranges])
            _lib.check(L.snd_adam_tf1_ranges(tp.data_ptr(), tg.data_ptr(), tm.data_ptr(), tv.data_ptr(),
                                             off, cnt, len(ranges), 0.0008, 0.9, 0.999, 1e-8, 0.5,
                                             step.data_ptr(), _lib.stream_ptr()))
        else:
            for o, c in ranges:
                _lib.check(L.snd_adam_tf1(tp.data_ptr() + 4 * o, tg.data_ptr() + 4 * o, tm.data_ptr() + 4 * o,
                                          tv.data_ptr() + 4 * o, c, 0.0008, 0.9, 0.999, 1e-8, 0.5,
                                          step.data_ptr(), _lib.stream_ptr()))
        torch.cuda.synchronize()
        out.append([t.cpu().numpy() for t in (tp, tm, tv)])
    inside = np.zeros(n, bool)
    for o, c in ranges:
        inside[o:o + c] = True
    for a, b, init in zip(out[0], out[1], (p, m0, v0)):
        assert np.array_equal(a, b)
        assert np.array_equal(b[~inside], init[~inside])


def test_reparam_injected_and_philox():
    from snd_vae_amd import _lib
    rows, L = 2000, 64
    rng = np.random.default_rng(2)
    ms = (0.3 * rng.standard_normal((rows, 2 * L))).astype(np.float32)
    eps = rng.standard_normal((rows, L)).astype(np.float32)
    nb = _lib.lib().snd_reparam_kl_blocks(rows, L)
    kl = torch.zeros(nb, dtype=torch.float64, device=DEV)
    z = torch.empty(rows, L, device=DEV)
    tms, teps = cu(ms), cu(eps)
    _lib.check(_lib.lib().snd_reparam_kl(tms.data_ptr(), 2 * L, rows, L, teps.data_ptr(), 0, 0, 0,
                                         z.data_ptr(), kl.data_ptr(), _lib.stream_ptr()))
    mu, s = ms[:, :L].astype(np.float64), ms[:, L:].astype(np.float64)
    assert rel(z.cpu().numpy(), mu + eps * np.exp(s)) < 1e-6
    assert float(kl.sum()) == pytest.approx(np.sum(1 + 2 * s - mu ** 2 - np.exp(s) ** 2), rel=1e-6)
    # device Philox stream: standard-normal moments, and (seed, step) changes the draw
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    zero = torch.zeros(rows, 2 * L, device=DEV)
    e1 = torch.empty(rows, L, device=DEV)
    e2 = torch.empty(rows, L, device=DEV)
    for out in (e1, e2):
        _lib.check(_lib.lib().snd_reparam_kl(zero.data_ptr(), 2 * L, rows, L, 0, 42, step.data_ptr(),
                                             out.data_ptr(), z.data_ptr(), kl.data_ptr(),
                                             _lib.stream_ptr()))
        step += 1
    a = e1.cpu().numpy().ravel()
    assert abs(a.mean()) < 0.02 and abs(a.std() - 1) < 0.02
    assert not torch.equal(e1, e2)


def test_sigmoid_mse_head():
    from snd_vae_amd import _lib
    rows, cin, cout = 1000, 10, 2
    rng = np.random.default_rng(3)
    u = rng.standard_normal((rows, cin)).astype(np.float32)
    w = rng.standard_normal((cin, cout)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    y = rng.random((rows, cout)).astype(np.float32)
    nb = _lib.lib().snd_sigmoid_mse_blocks(rows)
    sse = torch.zeros(nb, dtype=torch.float64, device=DEV)
    du = torch.empty(rows, cin, device=DEV)
    dw = torch.zeros(cin, cout, device=DEV)
    db = torch.zeros(cout, device=DEV)
    ws = torch.empty(nb * (cin * cout + cout) * 4, dtype=torch.uint8, device=DEV)
    yh = torch.empty(rows, cout, device=DEV)
    tu, tw, tb, ty = cu(u), cu(w), cu(b), cu(y)   # keep alive across the raw-pointer call
    _lib.check(_lib.lib().snd_sigmoid_mse(tu.data_ptr(), cin, rows, cin, tw.data_ptr(),
                                          tb.data_ptr(), cout, ty.data_ptr(), cout,
                                          sse.data_ptr(), yh.data_ptr(), du.data_ptr(), cin,
                                          dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _lib.stream_ptr()))
    U = u.astype(np.float64)
    yhat = R.sigmoid(U @ w + b)
    dpre = 2 * (yhat - y) / y.size * yhat * (1 - yhat)
    assert float(sse.sum()) == pytest.approx(((yhat - y) ** 2).sum(), rel=1e-6)
    assert rel(du.cpu().numpy(), dpre @ w.T) < 1e-5
    assert rel(dw.cpu().numpy(), U.T @ dpre) < 1e-5
    assert rel(db.cpu().numpy(), dpre.sum(0)) < 1e-5
