"""The disentangled-model references, bounds and guards of tests/abi_ops_disent.py, without a GPU:

(a) on contiguous inputs every float64 reference equals oracle/ref_disent.py to 1e-12: the e2e
    filter and its gradients, the regularisers and their gradients, and pair -> e2e -> head
    composed against the oracle's structure decoder;
(b) the float32 emulation passes every committed case;
(c) each planted fault fails its case, and the failure names the element.
"""
import numpy as np
import pytest

import abi_ops as A
import abi_ops_disent as D
from oracle import ref_disent as O
from test_abi_ops_cpu import ELEMENT, close, fails, ids, passes


# ---------------------------------------------------------------- (a) the oracle
@pytest.mark.parametrize("case", D.E2E_CASES[:6], ids=ids(D.E2E_CASES[:6]))
def test_e2e_references_are_the_oracle(case):
    _, B, N, C, K, Oc, _ = case
    rng = np.random.default_rng(1)
    x, w, b = rng.standard_normal((B, N, N, C)), rng.standard_normal((K, C, Oc)), rng.standard_normal(Oc)
    dout = rng.standard_normal((B, N, N, Oc))
    close(D.ref_e2e_fwd(x, w, b).ref, O.e2e(x, w, b))
    dx, dw, db = O.e2e_grads(x, w, b, dout)
    L = D.ref_e2e_bwd(x, w, dout)
    close(L["dx"].ref, dx), close(L["dw1"].ref, dw), close(L["db1"].ref, db)
    # K counts the products an element really has: taps that fall outside the graph add none
    full = D.ref_e2e_fwd(np.ones((1, N, N, 1)), np.ones((K, 1, 1)), np.zeros(1))
    assert np.array_equal(D.ref_e2e_fwd(x, w, b).K[0], C * full.ref[0] + 1)


def decoder_inputs(rng, B, N, Dz, widths):
    z = rng.standard_normal((B, N, Dz))
    up = np.triu(rng.random((B, N, N)) < 0.4, 1)
    adj = (up | up.transpose(0, 2, 1)).astype(np.float64)
    adj[:, 0, 0] = 1.0
    layers, cin = [], 2 * Dz
    for o in widths:
        layers.append({"gamma": 1 + 0.3 * rng.standard_normal(cin), "beta": 0.3 * rng.standard_normal(cin),
                       "w": rng.standard_normal((N, cin, o)) / np.sqrt(2 * N * cin), "b": rng.standard_normal(o)})
        cin = o
    head = {"gamma": 1 + 0.3 * rng.standard_normal(cin), "beta": 0.3 * rng.standard_normal(cin),
            "w": rng.standard_normal((cin, 2)), "b": rng.standard_normal(2)}
    return z, adj, layers, head


def test_head_reference_is_the_oracle_decoder_without_layers():
    rng = np.random.default_rng(2)
    B, N, Dz = 2, 6, 3
    z, adj, _, head = decoder_inputs(rng, B, N, Dz, ())
    ce, correct, dz, _, hg = O.structure_decoder_grads(z, adj, [], head)
    y = D.pair_concat(z)
    r = D.ref_head_ce(y, adj, head["gamma"], head["beta"], head["w"], head["b"])
    close(float(r.links["ce"].ref) / (B * N * N), ce)
    assert r.correct == correct
    for mine, theirs in (("dw", "w"), ("db", "b"), ("dgamma", "gamma"), ("dbeta", "beta")):
        close(r.links[mine].ref, hg[theirs])
    dy = r.links["dy"].ref.reshape(B, N, N, 2 * Dz)
    close(dy[..., :Dz].sum(2) + dy[..., Dz:].sum(1), dz)


def test_pair_e2e_bn_relu_head_compose_to_the_oracle_decoder():
    rng = np.random.default_rng(3)
    B, N, Dz = 2, 5, 2
    z, adj, layers, head = decoder_inputs(rng, B, N, Dz, (4, 3))
    ce, correct, dz, lg, hg = O.structure_decoder_grads(z, adj, layers, head)
    l0, l1 = layers
    x0 = D.ref_pair_fwd(z, l0["gamma"], l0["beta"]).ref.reshape(B, N, N, 2 * Dz)
    y1 = D.ref_e2e_fwd(x0, l0["w"], l0["b"]).ref
    x1 = A.ref_bn_act_fwd(y1.reshape(-1, 4), l1["gamma"], l1["beta"], 1, 0).ref.reshape(B, N, N, 4)
    y2 = D.ref_e2e_fwd(x1, l1["w"], l1["b"]).ref
    r = D.ref_head_ce(y2, adj, head["gamma"], head["beta"], head["w"], head["b"])
    close(float(r.links["ce"].ref) / (B * N * N), ce)
    assert r.correct == correct
    for mine, theirs in (("dw", "w"), ("db", "b"), ("dgamma", "gamma"), ("dbeta", "beta")):
        close(r.links[mine].ref, hg[theirs])
    b2 = D.ref_e2e_bwd(x1, l1["w"], r.links["dy"].ref.reshape(y2.shape))
    close(b2["dw1"].ref, lg[1]["w"]), close(b2["db1"].ref, lg[1]["b"])
    bn = A.ref_bn_act_bwd(b2["dx"].ref.reshape(-1, 4), y1.reshape(-1, 4), l1["gamma"], l1["beta"], 1, 0)
    close(bn["dgamma"].ref, lg[1]["gamma"]), close(bn["dbeta"].ref, lg[1]["beta"])
    b1 = D.ref_e2e_bwd(x0, l0["w"], bn["dy"].ref.reshape(y1.shape))
    close(b1["dw1"].ref, lg[0]["w"]), close(b1["db1"].ref, lg[0]["b"])
    pb = D.ref_pair_bwd(b1["dx"].ref, z, l0["gamma"], l0["beta"])
    close(pb["dz"].ref, dz), close(pb["dgamma"].ref, lg[0]["gamma"]), close(pb["dbeta"].ref, lg[0]["beta"])


@pytest.mark.parametrize("name,kw,_z,_ws", D.LATENT_WEIGHTS, ids=ids(D.LATENT_WEIGHTS))
@pytest.mark.parametrize("B,L", D.LATENT_SHAPES[1:3])
def test_latent_reference_is_the_oracle(B, L, name, kw, _z, _ws):
    rng = np.random.default_rng(4)
    mu, s, eps = 0.8 * rng.standard_normal((B, L)), 0.3 * rng.standard_normal((B, L)), rng.standard_normal((B, L))
    z = mu + eps * np.exp(s)
    kw = {k: float(np.float32(v)) for k, v in kw.items()}         # snd_latent_reg_t holds floats
    r = D.ref_latent(mu, s, z, kw)
    ref = O.group_reg(mu, s, z, **kw)
    for k in ("kl", "term", "dip", "tc"):
        assert abs(getattr(r, k) - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), k
    val, dmu, ds = O.group_reg_torch(mu, s, eps, **kw)
    assert abs(r.term - val) <= 1e-12 * max(1.0, abs(val))
    if np.abs(dmu).max() == 0:
        assert not r.dmu.ref.any() and not r.ds.ref.any()           # capacity off
    else:
        close(r.dmu.ref, dmu), close(r.ds.ref, ds)


def test_workspace_sizes_are_the_documented_layouts():
    assert D.pair_workspace_floats(3, 5, 4) == 3 * 8 * 2 + 3 * 5 * 4
    assert D.latent_workspace_floats(50, 100) == 2500 + 250000 + 10000 + 50        # TC's regions
    assert D.latent_workspace_floats(1, 16) == 16 * 16 + 16                         # DIP's


# ---------------------------------------------------------------- (b) a correct implementation passes
@pytest.mark.parametrize("case", D.E2E_CASES, ids=ids(D.E2E_CASES))
def test_emulated_e2e_passes(case):
    c = D.e2e_setup(case)
    passes(D.e2e_verify(c, D.e2e_emulate(c)))


@pytest.mark.parametrize("case", D.BN_RELU_CASES, ids=ids(D.BN_RELU_CASES))
def test_emulated_bn_relu_passes(case):
    c = D.bn_relu_setup(case)
    passes(D.bn_relu_verify(c, D.bn_relu_emulate(c)))


@pytest.mark.parametrize("case", D.PAIR_CASES, ids=ids(D.PAIR_CASES))
def test_emulated_pair_passes(case):
    c = D.pair_setup(case)
    passes(D.pair_verify(c, D.pair_emulate(c)))


@pytest.mark.parametrize("case", D.HEAD_CE_CASES, ids=ids(D.HEAD_CE_CASES))
def test_emulated_head_ce_passes(case):
    c = D.head_ce_setup(case)
    passes(D.head_ce_verify(c, D.head_ce_emulate(c)))


def test_head_ce_cases_reach_what_they_claim():
    c = D.head_ce_setup(D.HEAD_CE_CASES[0])
    assert c.B * c.N * c.N < 256 and c.C == 1
    assert D.HEAD_CE_CASES[1][3] == 32
    c = D.head_ce_setup(D.HEAD_CE_CASES[3])
    diag = c.adj[0][np.arange(c.N), np.arange(c.N)]
    assert diag.any() and not diag.all()
    r = D.ref_head_ce(c.y, c.adj, c.gamma, c.beta, c.w, c.b)
    assert r.correct <= c.N * c.N - diag.sum()                   # the (1, 0) diagonal never matches A_ii = 1


@pytest.mark.parametrize("case", D.LATENT_CASES, ids=ids(D.LATENT_CASES))
def test_emulated_latent_reg_passes(case):
    c = D.latent_setup(case)
    passes(D.latent_verify(c, D.latent_emulate(c)))


def test_latent_cases_reach_what_they_claim():
    by = {k[0]: k for k in D.LATENT_CASES}
    on, off = D.latent_setup(by["b10_l16_cap_on"]), D.latent_setup(by["b10_l16_cap_off"])
    assert D.ref_latent(on.mu, on.s, on.z, on.kw).kterm > 0 and D.ref_latent(off.mu, off.s, off.z, off.kw).kterm == 0
    c = D.latent_setup(by["b50_l100_dip_tc"])
    assert c.bufs["ws"].width == 2500 + 250000 + 10000 + 50 > 100 * 100 + 100     # S / Q cover cov / mean
    assert "z" not in D.latent_setup(by["b3_l5_kl_no_z_no_ws"]).bufs
    assert "ws" not in D.latent_setup(by["b3_l5_kl_no_z_no_ws"]).bufs


# ---------------------------------------------------------------- (c) planted faults
def case_of(cases, name):
    return next(k for k in cases if k[0] == name)


@pytest.mark.parametrize("fault,case,pattern", [
    ("pb_k_half", "b1_n6_c2_k4_o3", "snd_e2e_fwd out: " + ELEMENT),
    ("column_slides_over_j", "b2_n7_c3_k7_o5", "snd_e2e_fwd out: " + ELEMENT),
    ("db1_without_2", "b2_n7_c3_k7_o5", "snd_e2e_bwd db1: " + ELEMENT),
    ("taps_clipped_to_n", "b1_n4_c2_k11_o3", "snd_e2e_fwd out: " + ELEMENT),
], ids=["pb_k_half", "column_slides_over_j", "db1_without_2", "taps_clipped_to_n"])
def test_fault_e2e(fault, case, pattern):
    c = D.e2e_setup(case_of(D.E2E_CASES, case))
    fails(lambda: D.e2e_verify(c, D.e2e_emulate(c, fault)), pattern)


def test_fault_e2e_pb_is_unseen_at_odd_k():
    c = D.e2e_setup(D.E2E_CASES[0])                              # K = 7: K / 2 == (K - 1) / 2
    D.e2e_verify(c, D.e2e_emulate(c, "pb_k_half"))


@pytest.mark.parametrize("fault,pattern", [
    ("no_column_half", "snd_e2e_pair_bwd dz: " + ELEMENT),
    ("dgamma_graph_0", "snd_e2e_pair_bwd dgamma: " + ELEMENT),
], ids=["no_column_half", "dgamma_graph_0"])
def test_fault_pair(fault, pattern):
    c = D.pair_setup(D.PAIR_CASES[0])
    fails(lambda: D.pair_verify(c, D.pair_emulate(c, fault)), pattern)


@pytest.mark.parametrize("fault,case,pattern", [
    ("diagonal_kept", "b3_n11_c20", "snd_e2e_head_ce dy: " + ELEMENT),
    ("sum_not_mean", "b3_n11_c20", "snd_e2e_head_ce dy: " + ELEMENT),
    ("drop_channel_31", "b2_n7_c32", "snd_e2e_head_ce dy: " + ELEMENT),
], ids=["diagonal_kept", "sum_not_mean", "drop_channel_31"])
def test_fault_head_ce(fault, case, pattern):
    c = D.head_ce_setup(case_of(D.HEAD_CE_CASES, case))
    msg = fails(lambda: D.head_ce_verify(c, D.head_ce_emulate(c, fault)), pattern)
    if fault == "diagonal_kept":                                 # the first bad row is on a diagonal
        row = int(msg.split("element (")[1].split(",")[0])
        assert row // c.N % c.N == row % c.N


def test_fault_head_ce_count_off_by_one():
    c = D.head_ce_setup(D.HEAD_CE_CASES[2])
    after = D.head_ce_emulate(c)
    c.bufs["out"].block(after["out"])[0, 1] += 1.0
    fails(lambda: D.head_ce_verify(c, after), r"out\[1\]: element \(1,\).*the count is exact")


@pytest.mark.parametrize("fault,case,pattern", [
    ("ws_reused_before_dip_grad", "b10_l16_dip_tc", "snd_latent_reg dmu: " + ELEMENT),
    ("no_ds_through_z", "b10_l16_tc", "snd_latent_reg dlogstd: " + ELEMENT),
], ids=["ws_reused_before_dip_grad", "no_ds_through_z"])
def test_fault_latent_reg(fault, case, pattern):
    c = D.latent_setup(case_of(D.LATENT_CASES, case))
    fails(lambda: D.latent_verify(c, D.latent_emulate(c, fault)), pattern)


def test_fault_latent_workspace_reuse_is_unseen_without_tc():
    c = D.latent_setup(case_of(D.LATENT_CASES, "b10_l16_dip"))
    D.latent_verify(c, D.latent_emulate(c, "ws_reused_before_dip_grad"))


def test_fault_unwritten_output_is_an_infinite_ratio():
    c = D.pair_setup(D.PAIR_CASES[3])
    after = D.pair_emulate(c)
    after["dz"][A.G + 7] = c.bufs["dz"].arr[A.G + 7]             # never written: the pattern stays
    fails(lambda: D.pair_verify(c, after), r"snd_e2e_pair_bwd dz: element \(0, 1, 3\).*ratio inf")
