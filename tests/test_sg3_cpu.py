"""SpatialGraphConvolution_3D (`layers.py:200-277`) without a GPU: the float64 references of
tests/sg3_ref.py against each other and against finite differences, the Python layout
helpers, the C ABI's exports and host-side argument rules, and the kink condition of every
committed GPU case (so tests/test_gpu_sg3.py compares lrelu' off its kink).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sg3_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("snd_sg3_param_count", "snd_sg3_workspace", "snd_sg3_layer_fwd", "snd_sg3_layer_bwd")
DENSE = [k for k, v in S.CASES.items() if v[5] == "dense"] + ["split"]       # B N^4 fits


def small(seed=0, B=2, N=6, F=2, hid=(3, 4, 3, 2)):
    """The shapes of the factorisation's first check: random symmetric graphs with triangles,
    rel shifted to both signs."""
    rng = np.random.default_rng(seed)
    adj = S._random_graphs(B, N, rng, 0.5)
    rel = rng.random((B, N, N)) - 0.4
    return adj, rng.normal(size=(B, N, F)), rel, S.init_params(F, hid, rng), rng.normal(size=(B, N, hid[3]))


def rel_err(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def test_numpy_equals_torch_dense():
    adj, x, rel, p, _ = small()
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    y = S.sgconv3_torch(t(adj), t(x), t(rel), {k: t(v) for k, v in p.items()}).numpy()
    assert rel_err(S.sgconv3(adj, x, rel, p), y) < 1e-12
    assert np.abs(y).max() > 0.1


def test_dense_uses_every_index_coincidence():
    """k = i and p in {i, j} are on A-masked paths (as in the reference): dropping them changes y."""
    adj, x, rel, p, _ = small()
    assert (np.einsum("bij,bji->b", adj, adj) > 0).all()             # i-j-i paths exist
    y = S.sgconv3(adj, x, rel, p)
    q = dict(p)
    q["M0"] = p["M0"].copy()
    q["M0"][4 * 2 + 4] += 1.0                                        # the dis_ip row
    assert np.abs(S.sgconv3(adj, x, rel, q) - y).max() > 1e-3


def test_autograd_against_central_differences():
    adj, x, rel, p, dout = small(1, B=1, N=5)
    _, _, g = S.layer_grads(S.sgconv3_torch, adj, x, rel, p, dout, bn_act=True)
    rng = np.random.default_rng(2)

    def loss(xx, pp):
        y = S.sgconv3(adj, xx, rel, pp)
        return (S.lrelu(y * (pp["gamma"] * S.BN_C) + pp["beta"]) * dout).sum()
    h = 1e-6
    for k in list(p) + ["x"]:
        base = x if k == "x" else p[k]
        for _ in range(4):
            idx = tuple(rng.integers(s) for s in base.shape)
            vals = []
            for sgn in (1.0, -1.0):
                v = base.copy()
                v[idx] += sgn * h
                vals.append(loss(v, p) if k == "x" else loss(x, {**p, k: v}))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert fd == pytest.approx(g[k][idx], rel=1e-5, abs=1e-7), (k, idx)


@pytest.mark.parametrize("name", ["first"] + DENSE)
def test_factorised_equals_dense(name):
    """Outputs and all gradients to 1e-12 (of max(1, max-abs)), with and without BN + lrelu."""
    if name == "first":
        adj, x, rel, p, dout = small()
    else:
        c = S.make_case(name)
        adj, x, rel, p, dout = c.adj, c.x, c.rel, c.p, c.dout
    for bn_act in (False, True):
        if name == "tree" and bn_act:
            continue                                                 # the literal N = 24 graph once
        yd, od, gd = (S.reference(name, bn_act) if name != "first" and S.make_case(name).ref == "dense"
                      else S.layer_grads(S.sgconv3_torch, adj, x, rel, p, dout, bn_act=bn_act))
        yf, of, gf = S.layer_grads(S.sgconv3_fact, adj, x, rel, p, dout, bn_act=bn_act)
        assert rel_err(yf, yd) < 1e-12 and rel_err(of, od) < 1e-12
        for k in gd:
            assert rel_err(gf[k], gd[k]) < 1e-12, (name, bn_act, k)
        if not bn_act:
            assert not gd["gamma"].any() and not gd["beta"].any()


def test_stack_factorised_equals_dense():
    c = S.make_stack()
    od, gd = S.encoder_grads(S.sgconv3_torch, c.adj, c.x, c.rel, c.layers, c.dout)
    of, gf = S.encoder_grads(S.sgconv3_fact, c.adj, c.x, c.rel, c.layers, c.dout)
    assert rel_err(of, od) < 1e-12
    for a, b in zip(gf, gd):
        for k in b:
            assert rel_err(a[k], b[k]) < 1e-12, k


def test_shapes_pack_unpack():
    from snd_vae_amd import sg
    F, hid = 2, (7, 5, 3, 4)
    shp = dict(sg.sg3_param_shapes(F, hid))
    assert shp == {S.NAMES[k]: v for k, v in S.shapes(F, hid)}
    assert list(shp) == ["Matrix0", "bias0", "Matrix1", "bias1", "Matrix2", "bias2", "Matrix3", "bias3",
                         "gamma", "beta"]
    assert shp["Matrix0"] == (13, 7) and shp["Matrix1"] == (16, 5) and shp["Matrix2"] == (10, 3)
    assert shp["Matrix3"] == (5, 4)
    rng = np.random.default_rng(0)
    p = S.init_params(F, hid, rng)
    flat = sg.sg3_pack(F, hid, {S.NAMES[k]: v for k, v in p.items()})
    assert np.array_equal(flat, S.pack_layer(p, F, hid))
    back = sg.sg3_unpack(F, hid, flat)
    for k, v in p.items():
        assert np.array_equal(back[S.NAMES[k]], v)
    nobn = sg.sg3_unpack(F, hid, sg.sg3_pack(F, hid, {S.NAMES[k]: v for k, v in p.items() if k[0] != "g" and k != "beta"}))
    assert (nobn["gamma"] == 1).all() and not nobn["beta"].any()
    with pytest.raises(ValueError):
        sg.sg3_pack(F, hid, {"Matrix0": np.zeros((3, 3))})
    with pytest.raises(ValueError):
        sg.sg3_unpack(F, hid, flat[:-1])
    init = sg.init_sg3_layer(F, hid, rng)
    assert all(init[k].shape == s for k, s in shp.items())
    assert not init["bias0"].any() and (init["gamma"] == 1).all()
    assert 0.01 < init["Matrix1"].std() < 0.03                       # layers.py:214: N(0, 0.02)
    assert dict(sg.layer_param_shapes(F, hid)) == shp
    assert dict(sg.layer_param_shapes(F, hid[:3])) == dict(sg.sg_param_shapes(F, hid[:3]))
    with pytest.raises(ValueError):
        sg.layer_param_shapes(F, (1, 2))


@pytest.mark.parametrize("name", ["graph", "hub", "empty", "isolated", "tree"])
def test_path_count_brute_force(name):
    from snd_vae_amd.sg import path_count
    c = S.make_case(name)
    a = c.adj.astype(np.int64)
    brute = sum(int(a[b, i, j] * a[b, j, k]) for b in range(c.B) for i in range(c.N) for j in range(c.N)
                for k in range(c.N)) if c.N <= 24 else int(np.einsum("bij,bjk->", a, a))
    assert path_count(c.rp, c.ci) == brute
    assert brute == int((a.sum(-1) ** 2).sum())                      # P2 = sum_j d_j^2


def test_model_block_shapes_follow_the_widths():
    """Four-width entries size the three-hop layer in the disentangled model; three-width
    configurations keep their shapes; the fused plan refuses four widths."""
    from snd_vae_amd import sg
    from snd_vae_amd.config import sgjoint
    from snd_vae_amd.disent_model import DisentangledConfig, block_shapes, init_blocks
    from snd_vae_amd.params import block_shapes as plan_shapes
    n3 = lambda f, h: sum(int(np.prod(s)) for _, s in sg.sg3_param_shapes(f, h))
    cfg = DisentangledConfig(n_nodes=12, spatial_dim=3, sg_conv_hidden=((10,) * 4, (20,) * 4))
    s = block_shapes(cfg)
    assert s["g_sg0_conv"] == (n3(1, (10,) * 4),) and s["g_sg1_conv"] == (n3(10, (20,) * 4),)
    assert s["g_sg1_lin/Matrix"] == (12 * 20, cfg.sg_hidden)
    assert s["g_s1_conv/kernel"][1] == 3 and s["d_s_lin2/Matrix"][1] == 3
    b = init_blocks(cfg, 0)
    l0 = sg.sg3_unpack(1, (10,) * 4, b["g_sg0_conv"])
    assert not l0["bias0"].any() and (l0["gamma"] == 1).all() and l0["Matrix0"].std() > 0.005
    old = block_shapes(DisentangledConfig())
    assert old["g_sg0_conv"] == (sum(int(np.prod(v)) for _, v in sg.sg_param_shapes(1, (20, 20, 20))),)
    with pytest.raises(ValueError, match="two-hop"):
        plan_shapes(sgjoint(12, 16, sampling_num=2, sg_conv_hidden=((10,) * 4, (20,) * 4)))


def test_sgjoint_batch_3d_is_additive():
    from snd_vae_amd.config import sgjoint
    from snd_vae_amd.data import sgjoint_batch
    cfg = sgjoint(12, 16, mean_degree=4.0, sampling_num=2)
    b2, b3 = sgjoint_batch(cfg, 2, seed=3), sgjoint_batch(cfg, 2, seed=3, spatial_dim=3)
    assert b2.spatial_truth.shape == (24, 2) and b3.spatial_truth.shape == (24, 3)
    assert np.array_equal(b3.spatial_truth[:, :2], b2.spatial_truth)
    assert (b3.spatial_truth >= 0).all() and (b3.spatial_truth < 1).all()
    for k in ("rowptr", "colidx", "tree_rowptr", "tree_colidx", "features", "feature_truth"):
        assert np.array_equal(getattr(b2, k), getattr(b3, k)), k
    pos = b3.spatial_truth[:12].astype(np.float64)
    want = np.linalg.norm(pos[:, None] - pos[None], axis=-1)
    assert np.allclose(b3.rel[0], want, atol=1e-6) and np.abs(b3.rel - b2.rel).max() > 1e-3
    assert np.array_equal(sgjoint_batch(cfg, 2, seed=3, spatial_dim=2).rel, b2.rel)


def test_header_lib_and_binding_export_the_entry_points(lib_built):
    from snd_vae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snd_vae.h")).read()
    so = ctypes.CDLL(lib_built)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert hasattr(so, name), name
    assert "layers.py:200-277" in hdr and "model.py:139-140" in hdr
    assert int(re.search(r"#define\s+SND_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 21


def test_host_functions(lib_built):
    """Parameter count against the layout; the workspace grows with rows, edges and widths and
    refuses bad arguments (both are host functions: no device needed)."""
    from snd_vae_amd import _lib
    L = _lib.lib()
    for F, hid in ((1, (10,) * 4), (2, (7, 5, 3, 4)), (2, (65, 7, 66, 9))):
        want = sum(int(np.prod(s)) for _, s in S.shapes(F, hid))
        assert L.snd_sg3_param_count(F, *hid) == want
    assert L.snd_sg3_param_count(0, 1, 1, 1, 1) == -1 and L.snd_sg3_param_count(1, 1, 1, 0, 1) == -1
    w = L.snd_sg3_workspace(60, 100, 400, 2, 7, 5, 3, 4)
    assert w > 0 and w % 256 == 0
    assert L.snd_sg3_workspace(120, 100, 400, 2, 7, 5, 3, 4) > w
    assert L.snd_sg3_workspace(60, 200, 900, 2, 7, 5, 3, 4) > w
    assert L.snd_sg3_workspace(60, 100, 400, 2, 65, 5, 3, 4) > w
    assert L.snd_sg3_workspace(60, 0, 0, 2, 7, 5, 3, 4) > 0
    for bad in ((-1, 0, 0, 2, 7, 5, 3, 4), (60, -1, 0, 2, 7, 5, 3, 4), (60, 0, -1, 2, 7, 5, 3, 4),
                (60, 0, 0, 0, 7, 5, 3, 4), (60, 0, 0, 2, 7, 5, 3, 0)):
        assert L.snd_sg3_workspace(*bad) == 0, bad


@pytest.mark.parametrize("name", list(S.CASES))
def test_committed_cases_are_off_the_kinks(name):
    """Every lrelu argument on an A-masked path of every committed GPU case lies outside its own
    propagated fp32 forward bound of 0 (S4 per path and channel, S3 per edge and channel, m2s of
    nodes with edges, the BN pre-activation): the device's lrelu' is the reference's factor."""
    c = S.make_case(name)
    assert S.kink_violations(c.adj, c.x, c.rel, c.p, bn_act=True) == 0


def test_committed_stack_is_off_the_kinks():
    c = S.make_stack()
    x = c.x
    for p in c.layers:
        assert S.kink_violations(c.adj, x, c.rel, p, bn_act=True) == 0
        t = lambda a: torch.tensor(np.asarray(a, np.float64))
        y = S.sgconv3_fact(t(c.adj), t(x), t(c.rel), {k: t(v) for k, v in p.items()}).numpy()
        x = S.lrelu(y * (p["gamma"] * S.BN_C) + p["beta"])


def test_committed_cases_cover_what_they_claim():
    deg = lambda n: S.make_case(n).adj.sum(-1)
    assert deg("hub").max() == 69 and S.make_case("hub").adj[0, 1:, 1:].sum() > 0      # chords: triangles
    assert deg("split").size == 4105 and (deg("split") == 0).any()
    assert not deg("empty").any() and (deg("isolated") == 0).sum() == 1
    assert (deg("tree").sum(-1) == 2 * 23).all()                                        # spanning trees
    g = S.make_case("graph").adj
    assert np.einsum("bij,bjk,bki->", g, g, g) > 0                                      # triangles
    for n in S.CASES:
        r = S.make_case(n).rel
        assert (r > 0).any() and (r < 0).any()
