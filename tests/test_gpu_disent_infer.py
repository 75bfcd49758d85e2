"""Inference of the disentangled SND-VAE (encode, decode, generate, traverse;
snd_vae_amd/disent_model.py) against the literal float64 references of
tests/disent_infer_ref.py, at the shapes of tests/test_gpu_disent_model.py: N = 25 with
B = 2, S = 10 and B = 4, S = 3, the init_blocks weights with the big matrices x 4 rounded to
fp32.

With init weights the generated adjacency is almost all zeros, which would make the test
vacuous, so the setup first sets d_e_lin2/bias to centre the float64 off-diagonal margin
of the sampled reconstruction on its median: half ones (each class >= 25 % asserted).

Bars: a tensor within max(1e-5, 10 e32) of its max-abs, e32 the same reference's own error
in torch.float32 (the conditioning idiom of tests/test_gpu_disent_model.py); generated_adj
equal to the reference wherever the float64 |margin| exceeds the margin's bar, at most 1 %
of the off-diagonal entries excluded that way; the sigmoid outputs within 1e-5 relative.
On the CPU, with these inputs: the float64 reference has no entry under 1e-5 max|margin|,
e32 of the margin is 1.07e-6 in both configurations (the bar 1.07e-5 max|margin|), 0.08 % of
the entries at B = 4, S = 3 and none at B = 2, S = 10 are under the looser 1e-4 max|margin|, and
the fp32 reference flips no entry.
"""
import numpy as np
import pytest
import torch

import disent_infer_ref as IR
from test_gpu_disent_model import case, draw_eps

pytestmark = pytest.mark.gpu

CONFIGS = {"b2_s10": dict(B=2, S=10, seed=3, init=0, eps=5), "b4_s3": dict(B=4, S=3, seed=11, init=1, eps=9)}


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def big_blocks(cfg, seed):
    from snd_vae_amd.disent_model import init_blocks
    big = lambda k: k.endswith(("/Matrix", "/w", "/w1"))
    return {k: (v * 4.0 if big(k) else v).astype(np.float32).astype(np.float64) for k, v in init_blocks(cfg, seed).items()}


def offdiag(a):
    N = a.shape[-1]
    return a[:, ~np.eye(N, dtype=bool)]


def reference(p, ins, eps, cfg, dtype):
    enc = IR.encode_ref(p, ins, eps, cfg, dtype)
    dec = IR.decode_literal(p, cfg, enc["s"]["z"], enc["sg"]["z"], enc["g"]["z"], dtype)
    return enc, dec


@pytest.fixture(scope="module", params=list(CONFIGS), ids=list(CONFIGS))
def setup(request):
    from types import SimpleNamespace as NS
    from snd_vae_amd.disent_model import DeviceDisentBatch, DisentangledSGCNModelVAE
    k = CONFIGS[request.param]
    cfg, b, ins = case(k["B"], S=k["S"], seed=k["seed"])
    p = big_blocks(cfg, k["init"])
    eps = draw_eps(np.random.default_rng(k["eps"]), cfg, k["B"])
    e64 = {n: e.astype(np.float64) for n, e in eps.items()}
    m = reference(p, ins, e64, cfg, torch.float64)[1]["margin"]
    bias = p["d_e_lin2/bias"].copy()
    bias[1] -= np.median(offdiag(m))                              # margin = l1 - l0: centre it
    p["d_e_lin2/bias"] = bias.astype(np.float32).astype(np.float64)
    s = NS(cfg=cfg, B=k["B"], ins=ins, p=p, eps=eps)
    s.enc, s.dec = reference(p, ins, e64, cfg, torch.float64)
    s.enc32, s.dec32 = reference(p, ins, e64, cfg, torch.float32)
    s.model = DisentangledSGCNModelVAE(cfg, k["B"], blocks=p)
    s.batch = DeviceDisentBatch(b)
    s.deps = {n: torch.from_numpy(e).cuda() for n, e in eps.items()}
    return s


def close(name, got, ref, ref32, strict=False):
    """max-abs error relative to the tensor's max-abs: under max(1e-5, 10 e32), or under
    1e-5 itself (strict: the sigmoid outputs)."""
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    scale = max(np.abs(ref).max(), 1e-30)
    err, e32 = np.abs(got - ref).max() / scale, np.abs(ref32 - ref).max() / scale
    print(f"INFER_ERR {name} err {err:.3e} e32 {e32:.3e}")
    assert err < (1e-5 if strict else max(1e-5, 10 * e32)), (name, err, e32)


def check_adjacency(name, out, ref, ref32):
    """The margin within its bar, the adjacency exact wherever the reference decides it."""
    m, m32 = ref["margin"], ref32["margin"]
    top = np.abs(m).max()
    e32 = np.abs(m32 - m).max() / top
    bar = max(1e-5, 10 * e32) * top
    got = out["margin"].double().cpu().numpy()
    err = np.abs(got - m).max()
    print(f"INFER_ERR {name} margin err {err / top:.3e} e32 {e32:.3e}")
    assert err < bar, (name, err / top, e32)
    N = m.shape[-1]
    assert (got[:, np.arange(N), np.arange(N)] == -1).all()
    adj = out["generated_adj"]
    assert adj.dtype == torch.uint8
    adj = adj.cpu().numpy()
    assert (adj[:, np.arange(N), np.arange(N)] == 0).all()
    decided = np.abs(m) > bar
    excluded = (~offdiag(decided)).mean()
    print(f"INFER_ADJ {name} excluded {excluded:.5f} ones {offdiag(adj).mean():.3f}")
    assert excluded <= 0.01, (name, excluded)
    assert np.array_equal(adj[decided], ref["adj"][decided].astype(np.uint8)), name
    return offdiag(adj).mean()


def test_encode_matches_the_float64_encoders(setup):
    s = setup
    enc = s.model.encode(s.batch, s.deps)
    for g in ("s", "g", "sg"):
        for k in ("mu", "logstd", "z"):
            assert enc[g][k].is_contiguous()
            close(f"encode {g} {k}", enc[g][k], s.enc[g][k], s.enc32[g][k])
    plain = s.model.encode(s.batch)
    assert all("z" not in plain[g] for g in plain)
    assert all(torch.equal(plain[g]["mu"], enc[g]["mu"]) for g in plain)
    from snd_vae_amd.disent_model import mean_over_copies
    zbar = mean_over_copies(enc["sg"]["mu"], s.cfg.sampling_num)
    assert tuple(zbar.shape) == (s.B, s.cfg.sg_latent)


def test_generate_sample_reconstructs_the_reference(setup):
    s = setup
    out = s.model.generate(s.batch, z="sample", eps=s.deps, want_margin=True)
    ones = check_adjacency("sample", out, s.dec, s.dec32)
    assert 0.25 <= ones <= 0.75, ones                               # both classes: the test is not vacuous
    ref_ones = offdiag(s.dec["adj"]).mean()
    assert 0.25 <= ref_ones <= 0.75
    close("sample spatial", out["generated_spatial"], s.dec["spatial"], s.dec32["spatial"], strict=True)
    close("sample node", out["generated_node_feat"], s.dec["node"], s.dec32["node"], strict=True)
    for g in ("s", "g", "sg"):
        close(f"sample z_mean_{g}", out[f"z_mean_{g}"], s.enc[g]["mu"], s.enc32[g]["mu"])
    plain = s.model.generate(s.batch, z="sample", eps=s.deps)
    assert "margin" not in plain and torch.equal(plain["generated_adj"], out["generated_adj"])


def test_generate_mean_is_decode_of_the_means(setup):
    s = setup
    enc = s.model.encode(s.batch)
    out = s.model.generate(s.batch, z="mean", want_margin=True)
    dec = s.model.decode(enc["s"]["mu"], enc["sg"]["mu"], enc["g"]["mu"], want_margin=True)
    for k in ("generated_adj", "generated_spatial", "generated_node_feat", "margin"):
        assert torch.equal(out[k], dec[k]), k


def test_generate_prior_is_reproducible_per_seed(setup):
    s = setup
    a = s.model.generate(s.batch, z="prior", seed=7, want_margin=True)
    b = s.model.generate(s.batch, z="prior", seed=7, want_margin=True)
    c = s.model.generate(s.batch, z="prior", seed=8, want_margin=True)
    for k in ("generated_adj", "generated_spatial", "generated_node_feat", "margin"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["margin"], c["margin"])
    assert tuple(a["generated_spatial"].shape) == (s.B, s.cfg.n_nodes, s.cfg.spatial_dim)
    assert tuple(a["generated_node_feat"].shape) == (s.B, s.cfg.n_nodes, s.cfg.num_feature)
    # the caller's normals are the latents
    given = s.model.generate(s.batch, z="prior", eps=s.deps, want_margin=True)
    dec = s.model.decode(s.deps["s"], s.deps["sg"], s.deps["g"], want_margin=True)
    assert torch.equal(given["margin"], dec["margin"])


def test_decode_is_not_tied_to_the_constructor_batch(setup):
    """B = 7 graphs with S' = 2 copies on a model built for another n_graphs."""
    s = setup
    cfg, B, Sp = s.cfg, 7, 2
    rng = np.random.default_rng(21)
    z = {"s": rng.standard_normal((B, cfg.s_latent)), "sg": rng.standard_normal((B * Sp, cfg.sg_latent)),
         "g": rng.standard_normal((B, cfg.g_latent))}
    z = {k: v.astype(np.float32) for k, v in z.items()}
    ref = IR.decode_literal(s.p, cfg, z["s"], z["sg"], z["g"], torch.float64)
    ref32 = IR.decode_literal(s.p, cfg, z["s"], z["sg"], z["g"], torch.float32)
    d = {k: torch.from_numpy(v).cuda() for k, v in z.items()}
    out = s.model.decode(d["s"], d["sg"], d["g"], want_margin=True)
    check_adjacency("decode_b7", out, ref, ref32)
    close("decode_b7 spatial", out["generated_spatial"], ref["spatial"], ref32["spatial"], strict=True)
    close("decode_b7 node", out["generated_node_feat"], ref["node"], ref32["node"], strict=True)
    with pytest.raises(ValueError):
        s.model.decode(d["s"], d["sg"][:13], d["g"])                # 13 copies do not divide over 7 graphs
    with pytest.raises(ValueError):
        s.model.decode(d["s"][:6], d["sg"], d["g"])


def test_traverse_all_in_chunks_is_one_decode():
    """Latents 3 / 2 / 4, V = 2: 18 graphs in chunks of 3 equal one unchunked decode bitwise,
    and traverse() is a block of it."""
    from snd_vae_amd.disent_model import DisentangledConfig, DisentangledSGCNModelVAE, traverse_all_rows
    cfg = DisentangledConfig(n_nodes=7, s_latent=3, g_latent=2, sg_latent=4, sampling_num=2)
    model = DisentangledSGCNModelVAE(cfg, 2, blocks=big_blocks(cfg, 2))
    rng = np.random.default_rng(4)
    zs, zg, zsg = (rng.standard_normal((1, n)).astype(np.float32) for n in (3, 2, 4))
    values = np.array([-2.0, 2.0], np.float32)
    chunked = model.traverse_all(zs, zg, zsg, values, chunk=3, want_margin=True)
    rows = [torch.from_numpy(r).cuda() for r in traverse_all_rows(zs, zg, zsg, values)]
    whole = model.decode(rows[0], rows[2], rows[1], want_margin=True)
    assert tuple(chunked["generated_adj"].shape) == (18, 7, 7)
    for k in whole:
        assert torch.equal(chunked[k], whole[k]), k
    one = model.traverse("g", 1, zs, zg, zsg, values, want_margin=True)   # block Ls + 1 = 4: rows 8, 9
    for k in whole:
        assert torch.equal(one[k], whole[k][8:10]), k
