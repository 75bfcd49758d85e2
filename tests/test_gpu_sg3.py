"""SpatialGraphConvolution_3D HIP layer (csrc/snd_sg3.hip) vs the float64 references of
tests/sg3_ref.py (`layers.py:200-277`, `model.py:139-140`).

Layer bar: fp32 kernels against float64, every output and gradient block within 1e-5 of the
block's max-abs with tests/test_gpu_sg.py's floor of 1 (that test's bar for the same
arithmetic: fp32 FMA chains against float64).  Every case is off the lrelu kinks
(tests/test_sg3_cpu.py), so lrelu' on the device is the reference's factor.  Each block prints
its error and the bar before asserting.

Cases (tests/sg3_ref.py CASES): spanning trees at the protein layer-1 shape; graphs with
triangles (k = i, p in {i, j}); a hub of degree 69; R = 4105 rows (many split-K parts over rows and edges, short last parts); widths
past one GEMM tile; no edges / an isolated node; strided x / dx at pointers 4 bytes past
16-byte alignment with NaN-patterned guard bands around every output and the workspace.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_ops as A
import sg3_ref as S

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def close(tag, got, ref, tol=TOL):
    got = got.double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    err, bar = np.abs(got - ref).max() if ref.size else 0.0, tol * max(1.0, np.abs(ref).max() if ref.size else 0.0)
    print(f"{tag}: err {err:.3e} bar {bar:.3e} max-abs {np.abs(ref).max() if ref.size else 0.0:.3e}")
    assert np.isfinite(got).all(), tag
    assert err <= bar, (tag, err, bar)


def dev(a, dt=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def graph_of(c):
    from snd_vae_amd.sg import SGGraph
    return SGGraph(c.rp, c.ci, c.N, dev(c.rel))


def flat_params(c, p=None, F=None, hid=None):
    from snd_vae_amd.sg import sg3_pack
    p = c.p if p is None else p
    return dev(sg3_pack(F or c.F, hid or c.hid, {S.NAMES[k]: v for k, v in p.items()}))


def run_layer(c, bn_act):
    from snd_vae_amd.sg import SpatialGraphConvolution3D
    layer = SpatialGraphConvolution3D(c.F, c.hid, flat_params(c), bn_act=bn_act)
    out, y = layer.forward(graph_of(c), dev(c.x.reshape(c.B * c.N, c.F)))
    grads, dx = layer.backward(dev(c.dout.reshape(c.B * c.N, -1)))
    torch.cuda.synchronize()
    return y, out, grads, dx


def check_layer(c, y, out, grads, dx, bn_act):
    ry, rout, rg = S.reference(c.name, bn_act)
    R = c.B * c.N
    close(f"{c.name} y", y, ry.reshape(R, -1))
    if bn_act:
        close(f"{c.name} out", out, rout.reshape(R, -1))
    gb = S.unpack_layer(np.asarray(grads, np.float64) if not torch.is_tensor(grads) else grads.double().cpu().numpy(),
                        c.F, c.hid)
    for k in S.BLOCKS:
        close(f"{c.name} d{k}", gb[k], rg[k])
    if dx is not None:
        close(f"{c.name} dx", dx, rg["x"].reshape(R, c.F))


@pytest.mark.parametrize("name", ["tree", "graph", "hub", "split", "tails", "empty", "isolated"])
def test_layer_fwd_bwd(name):
    c = S.make_case(name)
    check_layer(c, *run_layer(c, False), False)


def test_layer_bn_act():
    c = S.make_case("graph")
    check_layer(c, *run_layer(c, True), True)


def test_two_runs_are_bitwise_equal():
    c = S.make_case("split")
    a, b = run_layer(c, True), run_layer(c, True)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_encoder_stack_bn():
    """Two layers at the protein widths [[10]*4, [20]*4] (main.py:223), BN + lrelu between;
    gradients through both layers."""
    from snd_vae_amd.sg import SGEncoder, SGGraph, SpatialGraphConvolution3D
    c = S.make_stack()
    ref, rg = S.encoder_grads(S.sgconv3_torch, c.adj, c.x, c.rel, c.layers, c.dout)
    enc = SGEncoder(c.F, c.hids, blocks=[{S.NAMES[k]: v for k, v in p.items()} for p in c.layers])
    assert all(isinstance(l, SpatialGraphConvolution3D) for l in enc.layers) and enc.out_width == 20
    g = SGGraph(c.rp, c.ci, c.N, dev(c.rel))
    R = c.B * c.N
    out = enc.forward(g, dev(c.x.reshape(R, c.F)))
    close("stack out", out, ref.reshape(R, -1))
    grads, _ = enc.backward(dev(c.dout.reshape(R, -1)))
    f = c.F
    for li, hid in enumerate(c.hids):
        gb = S.unpack_layer(grads[li].double().cpu().numpy(), f, hid)
        for k in S.BLOCKS:
            close(f"stack layer {li} d{k}", gb[k], rg[li][k])
        f = hid[3]


def test_sgencoder_mixes_two_and_three_hop():
    from snd_vae_amd.sg import SGEncoder, SpatialGraphConvolution, SpatialGraphConvolution3D
    enc = SGEncoder(1, ((4, 5, 6), (3, 4, 5, 7)))
    assert isinstance(enc.layers[0], SpatialGraphConvolution) and enc.layers[0].f == 1
    assert isinstance(enc.layers[1], SpatialGraphConvolution3D) and enc.layers[1].f == 6
    assert enc.out_width == 7
    with pytest.raises(ValueError):
        SGEncoder(1, ((4, 5),))


# ------------------------------------------------------------------ the C ABI on guarded operands
class AbiRun:
    """One case at the C ABI: every operand, output and the workspace (exactly
    snd_sg3_workspace bytes) in a NaN-patterned guarded buffer on the device."""

    def __init__(self, c, ldx_pad=0, lddx_pad=0, offset=0, bn_act=1, want_dx=True):
        from snd_vae_amd import _lib
        from snd_vae_amd.sg import path_count
        self.c, self.L, self._lib = c, _lib.lib(), _lib
        self.bn_act, self.want_dx = bn_act, want_dx
        R, F, h3 = c.B * c.N, c.F, c.hid[3]
        self.R, self.ldx, self.lddx = R, F + ldx_pad, F + lddx_pad
        self.g = graph_of(c)
        self.nnz, self.n_paths = int(c.rp[-1]), path_count(c.rp, c.ci)
        n_par = self.L.snd_sg3_param_count(F, *c.hid)
        self.ws_bytes = self.L.snd_sg3_workspace(R, self.nnz, self.n_paths, F, *c.hid)
        assert self.ws_bytes % 4 == 0
        o = offset
        self.host = {
            "x": A.guarded(R, F, self.ldx, offset=o, data=c.x.reshape(R, F), name="x"),
            "params": A.vec(n_par, offset=o, data=S.pack_layer(c.p, F, c.hid), name="params"),
            "dout": A.guarded(R, h3, offset=o, data=c.dout.reshape(R, h3), name="dout"),
            "y": A.guarded(R, h3, offset=o, name="y"),
            "out": A.guarded(R, h3, offset=o, name="out"),
            "dx": A.guarded(R, F, self.lddx, offset=o, name="dx"),
            "grads": A.vec(n_par, offset=o, name="grads"),
            "ws": A.vec(self.ws_bytes // 4, name="workspace"),           # aligned, as tests/abi_ops_sg.py keeps it
        }
        self.dev = {k: torch.from_numpy(v.arr.copy()).cuda() for k, v in self.host.items()}

    def ptr(self, k):
        return self.dev[k].data_ptr() + 4 * self.host[k].off

    def fwd(self, **kw):
        c = self.c
        a = dict(g=C.byref(self.g.c), rel=self.g.rel.data_ptr(), nnz=self.nnz, n_paths=self.n_paths, x=self.ptr("x"),
                 ldx=self.ldx, f=c.F, h0=c.hid[0], h1=c.hid[1], h2=c.hid[2], h3=c.hid[3], params=self.ptr("params"),
                 bn_act=self.bn_act, y=self.ptr("y"), out=self.ptr("out"), ws=self.ptr("ws"), ws_bytes=self.ws_bytes)
        a.update(kw)
        return self.L.snd_sg3_layer_fwd(a["g"], a["rel"], a["nnz"], a["n_paths"], a["x"], a["ldx"], a["f"], a["h0"],
                                        a["h1"], a["h2"], a["h3"], a["params"], a["bn_act"], a["y"], a["out"], a["ws"],
                                        a["ws_bytes"], self._lib.stream_ptr())

    def bwd(self, **kw):
        c = self.c
        a = dict(g=C.byref(self.g.c), rel=self.g.rel.data_ptr(), nnz=self.nnz, n_paths=self.n_paths, x=self.ptr("x"),
                 ldx=self.ldx, f=c.F, h0=c.hid[0], h1=c.hid[1], h2=c.hid[2], h3=c.hid[3], params=self.ptr("params"),
                 bn_act=self.bn_act, y=self.ptr("y"), dout=self.ptr("dout"),
                 dx=self.ptr("dx") if self.want_dx else None, lddx=self.lddx, grads=self.ptr("grads"),
                 ws=self.ptr("ws"), ws_bytes=self.ws_bytes)
        a.update(kw)
        return self.L.snd_sg3_layer_bwd(a["g"], a["rel"], a["nnz"], a["n_paths"], a["x"], a["ldx"], a["f"], a["h0"],
                                        a["h1"], a["h2"], a["h3"], a["params"], a["bn_act"], a["y"], a["dout"], a["dx"],
                                        a["lddx"], a["grads"], a["ws"], a["ws_bytes"], self._lib.stream_ptr())

    def after(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.dev.items()}

    def unchanged(self):
        for k, v in self.after().items():
            assert np.array_equal(v.view(np.uint32), self.host[k].arr.view(np.uint32)), f"{k} changed"


@pytest.mark.parametrize("want_dx", [True, False])
def test_strided_guarded_operands(want_dx):
    """ldx = F + 3, lddx = F + 5, base pointers 4 bytes past 16-byte alignment, BN + lrelu; every
    guard and padding element intact; dx = NULL leaves the dx buffer alone."""
    c = S.make_case("strided")
    r = AbiRun(c, ldx_pad=3, lddx_pad=5, offset=1, bn_act=1, want_dx=want_dx)
    assert all(r.ptr(k) % 16 == 4 for k in r.host if k != "ws")
    assert r.fwd() == 0, r._lib.last_error()
    assert r.bwd() == 0, r._lib.last_error()
    after = r.after()
    for k, gb in r.host.items():
        gb.check_untouched(after[k])
    val = lambda k: r.host[k].values(after[k])
    check_layer(c, val("y"), val("out"), val("grads")[0], val("dx") if want_dx else None, True)
    if not want_dx:
        assert np.array_equal(after["dx"].view(np.uint32), r.host["dx"].arr.view(np.uint32))
    for k in ("x", "params", "dout"):
        assert np.array_equal(after[k].view(np.uint32), r.host[k].arr.view(np.uint32)), k


ERR_FWD = [("ldx", dict(ldx=1)), ("width", dict(h0=0)), ("width", dict(h3=-1)), ("width", dict(f=0)),
           ("bn_act needs out", dict(out=None)), ("null", dict(x=None)), ("null", dict(params=None)),
           ("null", dict(y=None)), ("null", dict(ws=None)), ("null", dict(rel=None)), ("graph", dict(g=None)),
           ("workspace", "short_ws"), ("n_paths", dict(n_paths=-1)), ("nnz", dict(nnz=-1))]
ERR_BWD = [("lddx", dict(lddx=1)), ("ldx", dict(ldx=1)), ("width", dict(h2=0)), ("null", dict(dout=None)),
           ("null", dict(grads=None)), ("null", dict(y=None)), ("workspace", "short_ws")]


def test_argument_errors_touch_nothing():
    """Every SND_ERR_ARG rule: returned before anything is launched, the message names the entry
    point, no buffer changes."""
    c = S.make_case("strided")
    r = AbiRun(c, offset=1)
    clone = lambda: type(r.g.c).from_buffer_copy(r.g.c)
    for fn, name, rules in ((r.fwd, "snd_sg3_layer_fwd", ERR_FWD), (r.bwd, "snd_sg3_layer_bwd", ERR_BWD)):
        for what, kw in rules:
            kw = dict(ws_bytes=r.ws_bytes - 1) if kw == "short_ws" else kw
            assert fn(**kw) == -1, (name, what, kw)
            msg = r._lib.last_error()
            assert name in msg, (what, msg)
    gc = clone()
    gc.n_rows = r.R - 1                                              # not a multiple of n_per_graph
    assert r.fwd(g=C.byref(gc)) == -1 and "n_per_graph" in r._lib.last_error()
    assert r.bwd(g=C.byref(gc)) == -1 and "snd_sg3_layer_bwd" in r._lib.last_error()
    gc = clone()
    gc.edge_rev = None
    assert r.fwd(g=C.byref(gc)) == -1
    r.unchanged()
    assert r.fwd() == 0 and r.bwd() == 0                             # and the operands were good


def test_asymmetric_rejected():
    from snd_vae_amd.sg import SGGraph
    rp = np.array([0, 1, 1], np.int32)
    ci = np.array([1], np.int32)
    with pytest.raises(ValueError, match="symmetric"):
        SGGraph(rp, ci, 2, torch.zeros(1, 2, 2, device="cuda"))
    g = SGGraph(np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), 2, torch.zeros(1, 2, 2, device="cuda"))
    assert (g.nnz, g.n_paths) == (2, 2)                              # what the three-hop entry points are handed


# ------------------------------------------------------------------ the disentangled model, 3-D
def test_disentangled_model_step_three_hop(monkeypatch):
    """One step of DisentangledSGCNModelVAE with spatial_dim = 3 and the protein widths
    [[10]*4, [20]*4] against oracle/ref_disent_model.py, whose spatial-graph layer is replaced
    by dispatchers on the number of widths (the oracle's F = hid[2] holds: equal widths)."""
    from oracle import ref_disent_model as RM
    from oracle import ref_sg as RS
    from snd_vae_amd.config import sgjoint
    from snd_vae_amd.data import sgjoint_batch
    from snd_vae_amd.disent_model import DeviceDisentBatch, DisentangledConfig, DisentangledSGCNModelVAE, init_blocks
    from test_gpu_disent_model import compare, dense_trees, draw_eps
    two_unpack, two_conv = RS.unpack_layer, RS.sgconv_torch
    monkeypatch.setattr(RS, "unpack_layer",
                        lambda flat, F, hid: (S.unpack_layer if len(hid) == 4 else two_unpack)(flat, F, hid))
    monkeypatch.setattr(RS, "sgconv_torch",
                        lambda adj, x, rel, p: (S.sgconv3_torch if "M0" in p else two_conv)(adj, x, rel, p))
    B, n, Sn = 2, 12, 2
    cfg = DisentangledConfig(n_nodes=n, sampling_num=Sn, spatial_dim=3, sg_conv_hidden=((10,) * 4, (20,) * 4))
    b = sgjoint_batch(sgjoint(n, 16, mean_degree=4.0, sampling_num=Sn), B, seed=3, spatial_dim=3)
    ins = {"x": b.feature_truth.reshape(B, n, -1), "spatial": b.spatial_truth.reshape(B, n, 3),
           "adj": np.stack([b.dense_adj(g) for g in range(B)]), "x_sg": b.features.reshape(B * Sn, n, -1),
           "trees": dense_trees(b), "rel": b.rel}
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in init_blocks(cfg, 0).items()}
    model = DisentangledSGCNModelVAE(cfg, B, blocks=p)
    eps = draw_eps(np.random.default_rng(5), cfg, B)
    got = model.step(DeviceDisentBatch(b), {k: torch.from_numpy(e).cuda() for k, e in eps.items()})
    e64 = {k: e.astype(np.float64) for k, e in eps.items()}
    ref, rg = RM.disent_forward_backward(p, ins, e64, cfg)
    assert np.abs(rg["g_sg0_conv"]).max() > 0 and np.abs(rg["g_sg1_conv"]).max() > 0
    compare(got, ref, model.grad_blocks(), rg, "three-hop", p, ins, e64, cfg)
    blocks = model.blocks()                                          # Adam moved every SG parameter block
    for k in ("g_sg0_conv", "g_sg1_conv"):
        assert 0 < np.abs(blocks[k] - p[k]).max() <= 1.01 * cfg.learning_rate
