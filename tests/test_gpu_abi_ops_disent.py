"""The disentangled-model entry points at the C ABI on the guarded operands of
tests/abi_ops_disent.py: snd_e2e_fwd / _bwd at K != N, snd_e2e_pair_fwd / _bwd past 256
nodes, snd_bn_relu_fwd / _bwd, snd_e2e_head_ce at 1, 20 and 32 channels with an exact count,
snd_latent_reg with DIP and TC sharing the workspace; workspaces of exactly the queried size.
One library call per op and case, then the op's ``verify``: every output against the float64
reference within its derived bound, every guard intact.  Ratios are printed as
"ABI_RATIO <op> <case> <output> <ratio>" (DESIGN.md §3).
"""
import ctypes

import pytest
import torch

import abi_ops_disent as D
from test_gpu_abi_ops import Device, ids, lib, ok, report
from test_gpu_abi_ops_sg import rejected

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


@pytest.mark.parametrize("case", D.E2E_CASES, ids=ids(D.E2E_CASES))
def test_e2e_fwd_bwd(case):
    L, S, _ = lib()
    c = D.e2e_setup(case)
    d = Device(c)
    ok(L.snd_e2e_fwd(d.p("x"), c.B, c.N, c.C, d.p("w1"), d.p("b1"), c.K, c.O, d.p("out"), S), "snd_e2e_fwd")
    ok(L.snd_e2e_bwd(d.p("x"), c.B, c.N, c.C, d.p("w1"), c.K, c.O, d.p("dout"), d.p("dx"), d.p("dw1"), d.p("db1"), S),
       "snd_e2e_bwd")
    report("e2e", case[0], D.e2e_verify(c, d.back()))


@pytest.mark.parametrize("case", D.PAIR_CASES, ids=ids(D.PAIR_CASES))
def test_e2e_pair_fwd_bwd(case):
    L, S, _ = lib()
    c = D.pair_setup(case)
    assert L.snd_e2e_pair_bwd_workspace(c.B, c.N, c.D) == 4 * c.bufs["ws"].width
    d = Device(c)
    ok(L.snd_e2e_pair_fwd(d.p("z"), c.B, c.N, c.D, d.p("gamma"), d.p("beta"), d.p("x0"), S), "snd_e2e_pair_fwd")
    ok(L.snd_e2e_pair_bwd(d.p("dx0"), d.p("z"), c.B, c.N, c.D, d.p("gamma"), d.p("beta"), d.p("dz"), d.p("dgamma"),
                          d.p("dbeta"), d.p("ws"), S), "snd_e2e_pair_bwd")
    report("e2e_pair", case[0], D.pair_verify(c, d.back()))


@pytest.mark.parametrize("case", D.BN_RELU_CASES, ids=ids(D.BN_RELU_CASES))
def test_bn_relu_fwd_bwd(case):
    L, S, _ = lib()
    c = D.bn_relu_setup(case)
    d = Device(c)
    ok(L.snd_bn_relu_fwd(d.p("y"), c.rows, c.c, d.p("gamma"), d.p("beta"), d.p("x"), S), "snd_bn_relu_fwd")
    ok(L.snd_bn_relu_bwd(d.p("dx"), d.p("y"), c.rows, c.c, d.p("gamma"), d.p("beta"), d.p("dy"), d.p("dgamma"),
                         d.p("dbeta"), S), "snd_bn_relu_bwd")
    report("bn_relu", case[0], D.bn_relu_verify(c, d.back()))


def head_ce(L, S, d, c, channels=None):
    return L.snd_e2e_head_ce(d.p("y"), d.p("adj"), c.B, c.N, c.C if channels is None else channels, d.p("gamma"),
                             d.p("beta"), d.p("w"), d.p("b"), d.p("dy"), d.p("dw"), d.p("db"), d.p("dgamma"),
                             d.p("dbeta"), d.p("out"), S)


@pytest.mark.parametrize("case", D.HEAD_CE_CASES, ids=ids(D.HEAD_CE_CASES))
def test_e2e_head_ce(case):
    L, S, _ = lib()
    c = D.head_ce_setup(case)                                    # asserts every argmax decidable
    d = Device(c)
    ok(head_ce(L, S, d, c), "snd_e2e_head_ce")
    report("e2e_head_ce", case[0], D.head_ce_verify(c, d.back()))


def latent_reg(L, S, _lib, d, c, kw=None):
    kw = c.kw if kw is None else kw
    w = _lib.LatentReg(*[float(kw.get(k, 0.0)) for k in D.LATENT_FIELDS])
    return L.snd_latent_reg(d.p("mu"), d.p("logstd"), d.p("z"), c.B, c.L, ctypes.byref(w), d.p("dmu"), d.p("dlogstd"),
                            d.p("out"), d.p("ws"), S)


@pytest.mark.parametrize("case", D.LATENT_CASES, ids=ids(D.LATENT_CASES))
def test_latent_reg(case):
    L, S, _lib = lib()
    c = D.latent_setup(case)
    if "ws" in c.bufs:
        assert L.snd_latent_reg_workspace(c.B, c.L) == 4 * c.bufs["ws"].width
    d = Device(c)
    ok(latent_reg(L, S, _lib, d, c), "snd_latent_reg")
    report("latent_reg", case[0], D.latent_verify(c, d.back()))


# ---------------------------------------------------------------- error returns
def test_e2e_head_ce_rejects_33_channels():
    L, S, _ = lib()
    c = D.head_ce_setup(D.HEAD_CE_CASES[1])                      # 32 channels
    d = Device(c)
    rejected(head_ce(L, S, d, c, channels=33), d, "snd_e2e_head_ce")


def test_latent_reg_rejects_tc_without_z_and_dip_without_workspace():
    L, S, _lib = lib()
    by = {k[0]: k for k in D.LATENT_CASES}
    c = D.latent_setup(by["b3_l5_dip_no_z"])                     # no z: TC cannot run
    d = Device(c)
    rejected(latent_reg(L, S, _lib, d, c, dict(w_kl=1.0, w_tc=10.0)), d, "snd_latent_reg")
    c = D.latent_setup(by["b3_l5_kl_no_z_no_ws"])                # no workspace: DIP cannot run
    d = Device(c)
    rejected(latent_reg(L, S, _lib, d, c, dict(w_kl=1.0, w_dip=0.5, lambda_od=10.0, lambda_d=100.0)), d, "snd_latent_reg")
