"""The stand-alone C ABI ops (include/snd_vae.h) on guarded, strided, tail-shaped operands.

Every case runs the entry point once on the guarded operands of tests/abi_ops.py (raw
pointers = data_ptr() + the helper's offset, leading dimensions wider than the rows),
synchronises, and hands the buffers to the op's ``verify``: worst err / bound < 1 for every
output against the float64 reference (derived bounds, no exclusions), and every guard and
padding element of every input and output bitwise intact.  The ratios are printed
("ABI_RATIO <op> <case> <output> <ratio>"; run with -s to collect them): DESIGN.md §3
records them, the bars stay the derived bounds.
"""
import ctypes

import numpy as np
import pytest
import torch

import abi_ops as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
ERR_ARG = -1
_ITEM = {"f32": 4, "bf16": 2, "f64": 8, "i32": 4}


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def ids(cases):
    return [c[0] for c in cases]


class Device:
    """The guarded buffers of a context on the device."""

    def __init__(self, c):
        self.c = c
        self.t = {k: torch.from_numpy(g.arr.view(np.int16) if g.dtype == "bf16" else g.arr).to(DEV)
                  for k, g in c.bufs.items()}

    def p(self, name):
        """Device pointer of the operand's [0, 0] (0 = NULL for an operand the case leaves out)."""
        g = self.c.bufs.get(name)
        return 0 if g is None else self.t[name].data_ptr() + g.off * _ITEM[g.dtype]

    def ld(self, name, default=0):
        g = self.c.bufs.get(name)
        return default if g is None else g.ld

    def back(self):
        torch.cuda.synchronize()
        return {k: (t.cpu().numpy().view(np.uint16) if self.c.bufs[k].dtype == "bf16" else t.cpu().numpy())
                for k, t in self.t.items()}


def lib():
    from snd_vae_amd import _lib
    return _lib.lib(), _lib.stream_ptr(), _lib


def ok(rc, what):
    from snd_vae_amd import _lib
    _lib.check(rc, what)


def report(op, case, res):
    for k, r in res.items():
        print(f"ABI_RATIO {op} {case} {k} {r:.4f}")
    assert all(r < 1.0 for r in res.values()), res


# ---------------------------------------------------------------- snd_gemm
@pytest.mark.parametrize("dtype", [A.F32, A.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", A.GEMM_CASES, ids=ids(A.GEMM_CASES))
def test_gemm(case, dtype):
    L, S, _ = lib()
    c = A.gemm_setup(case, dtype)
    d = Device(c)
    ok(L.snd_gemm(c.ta, c.tb, c.m, c.n, c.k, d.p("a"), d.ld("a"), d.p("b"), d.ld("b"), d.p("c"), d.ld("c"),
                  d.p("bias"), dtype, S), "snd_gemm")
    report("gemm_" + ("bf16" if dtype else "f32"), case[0], A.gemm_verify(c, d.back()))


# ---------------------------------------------------------------- conv1d k=5 SAME
def run_conv(c):
    L, S, _ = lib()
    d = Device(c)
    if c.op == "fwd":
        ok(L.snd_conv1d_same_fwd(d.p("x"), d.ld("x"), c.rows, c.npg, c.cin, d.p("w"), c.cout, d.p("bias"),
                                 d.p("gamma"), d.p("beta"), d.p("y_pre"), d.ld("y_pre", c.cout + 1), d.p("out"),
                                 d.ld("out"), c.dtype, S), "snd_conv1d_same_fwd")
    elif c.op == "bwd_data":
        ok(L.snd_conv1d_same_bwd_data(d.p("dy"), d.ld("dy"), c.rows, c.npg, c.cout, d.p("w"), c.cin, d.p("dx"),
                                      d.ld("dx"), c.dtype, S), "snd_conv1d_same_bwd_data")
    else:
        need = L.snd_conv1d_bwd_weight_workspace(c.rows, c.cin, c.cout)
        assert need == c.splits * 5 * c.cin * c.cout * 4, (need, c.splits)       # the expected split count
        ok(L.snd_conv1d_same_bwd_weight(d.p("x"), d.ld("x"), d.p("dy"), d.ld("dy"), c.rows, c.npg, c.cin, c.cout,
                                        d.p("dw"), d.p("ws"), need, c.dtype, S), "snd_conv1d_same_bwd_weight")
    return A.conv_verify(c, d.back())


@pytest.mark.parametrize("dtype", [A.F32, A.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("op", ["fwd", "bwd_data"])
@pytest.mark.parametrize("case", A.CONV_CASES, ids=ids(A.CONV_CASES))
def test_conv1d(case, op, dtype):
    report(f"conv1d_{op}_" + ("bf16" if dtype else "f32"), case[0], run_conv(A.conv_setup(case, dtype, op)))


@pytest.mark.parametrize("dtype", [A.F32, A.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", A.CONV_WGRAD_CASES, ids=ids(A.CONV_WGRAD_CASES))
def test_conv1d_bwd_weight(case, dtype):
    c = A.conv_setup(case, dtype, "bwd_weight")
    assert c.splits == (2 if c.rows == 1066 else 1)
    report("conv1d_bwd_weight_" + ("bf16" if dtype else "f32"), case[0], run_conv(c))


# ---------------------------------------------------------------- CSR SpMM
@pytest.mark.parametrize("case", A.SPMM_PLAIN_CASES, ids=ids(A.SPMM_PLAIN_CASES))
def test_csr_spmm_plain(case):
    L, S, _ = lib()
    c = A.spmm_setup(case, False)
    d = Device(c)
    vec = c.width % 64 == 0 and d.ld("h") % 4 == 0 and d.p("h") % 16 == 0 and d.ld("out") % 4 == 0 and d.p("out") % 16 == 0
    assert vec == (case[0] in ("w64_vec", "w128_vec")), "the dispatch condition this case is named for"
    ok(L.snd_csr_spmm(d.p("rowptr"), d.p("colidx"), c.rows, d.p("h"), d.ld("h"), c.width, d.p("out"), d.ld("out"),
                      0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, S), "snd_csr_spmm")
    report("csr_spmm_plain", case[0], A.spmm_verify(c, d.back()))


@pytest.mark.parametrize("case", A.SPMM_GCN_CASES, ids=ids(A.SPMM_GCN_CASES))
def test_csr_spmm_gcn(case):
    L, S, _ = lib()
    c = A.spmm_setup(case, True)
    d = Device(c)
    assert (d.ld("preact") % 4 == 0 and d.p("preact") % 16 == 0 and d.p("h") % 16 == 0) == (case[1] == 64)
    ok(L.snd_csr_spmm(d.p("rowptr"), d.p("colidx"), c.rows, d.p("h"), d.ld("h"), c.width, d.p("out"), d.ld("out"),
                      1, d.p("gamma"), d.p("beta"), d.p("preact"), d.ld("preact"), d.p("x"), d.ld("x", c.fx + 2), c.fx,
                      d.p("gamma2"), d.p("beta2"), d.p("out2"), d.ld("out2", c.width + c.fx + 3), S), "snd_csr_spmm")
    report("csr_spmm_gcn", case[0], A.spmm_verify(c, d.back()))


@pytest.mark.parametrize("case", A.SPMM_BF16_CASES, ids=ids(A.SPMM_BF16_CASES))
def test_csr_spmm_bf16(case):
    L, S, _ = lib()
    outs = []
    for ordered in (False, True):
        c = A.spmm_bf16_setup(case, ordered)
        d = Device(c)
        ok(L.snd_csr_spmm_bf16(d.p("rowptr"), d.p("colidx"), c.rows, d.p("h"), d.ld("h"), c.width, d.p("out"),
                               d.ld("out"), c.n, c.B, d.p("row_order"), S), "snd_csr_spmm_bf16")
        after = d.back()
        report("csr_spmm_bf16", case[0] + ("_row_order" if ordered else ""), A.spmm_bf16_verify(c, after))
        outs.append(c.bufs["out"].block(after["out"]).copy())
    assert np.array_equal(outs[0], outs[1]), "the result does not depend on row_order"


# ---------------------------------------------------------------- reparameterisation
@pytest.mark.parametrize("case", A.REPARAM_CASES, ids=ids(A.REPARAM_CASES))
def test_reparam_kl(case):
    L, S, _ = lib()
    c = A.reparam_setup(case)
    assert L.snd_reparam_kl_blocks(c.rows, c.L) == c.nb
    d = Device(c)
    ok(L.snd_reparam_kl(d.p("ms"), d.ld("ms"), c.rows, c.L, d.p("eps"), 0, 0, d.p("eps_out"), d.p("z"),
                        d.p("kl_part"), S), "snd_reparam_kl")
    report("reparam_kl", case[0], A.reparam_verify(c, d.back()))


@pytest.mark.parametrize("mode", A.REPARAM_BWD_MODES)
@pytest.mark.parametrize("case", A.REPARAM_BWD_CASES, ids=ids(A.REPARAM_BWD_CASES))
def test_reparam_bwd(case, mode):
    L, S, _ = lib()
    c = A.reparam_bwd_setup(case, mode)
    d = Device(c)
    ok(L.snd_reparam_bwd(d.p("ms"), d.ld("ms"), c.rows, c.L, d.p("eps"), d.p("dz"), d.p("add_mu"), d.p("add_ls"),
                         d.p("dms"), d.ld("dms"), S), "snd_reparam_bwd")
    report("reparam_bwd", f"{case[0]}_{mode}", A.reparam_bwd_verify(c, d.back()))


# ---------------------------------------------------------------- sigmoid head + MSE
@pytest.mark.parametrize("case", A.HEAD_CASES, ids=ids(A.HEAD_CASES))
def test_sigmoid_mse(case):
    L, S, _ = lib()
    c = A.head_setup(case)
    assert L.snd_sigmoid_mse_blocks(c.rows) == c.nb
    d = Device(c)
    ok(L.snd_sigmoid_mse(d.p("u"), d.ld("u"), c.rows, c.cin, d.p("w"), d.p("b"), c.cout, d.p("target"),
                         d.ld("target"), d.p("sse"), d.p("yhat"), d.p("du"), d.ld("du"), d.p("dw"), d.p("db"),
                         d.p("ws"), 4 * c.bufs["ws"].width, S), "snd_sigmoid_mse")
    report("sigmoid_mse", case[0], A.head_verify(c, d.back()))


# ---------------------------------------------------------------- frozen BN + activation
@pytest.mark.parametrize("case", A.BN_ACT_CASES, ids=ids(A.BN_ACT_CASES))
def test_bn_act_fwd(case):
    L, S, _ = lib()
    c = A.bn_act_setup(case, False)
    A.assert_off_kink(c.y, c.gamma, c.beta, c.act, c.first)        # on the CPU, before the launch
    d = Device(c)
    ok(L.snd_bn_act_fwd(d.p("y"), d.ld("y"), c.rows, c.c, d.p("gamma"), d.p("beta"), c.act, c.first, d.p("x"),
                        d.ld("x"), S), "snd_bn_act_fwd")
    report("bn_act_fwd", case[0], A.bn_act_verify(c, d.back()))


@pytest.mark.parametrize("case", A.BN_ACT_BWD_CASES, ids=ids(A.BN_ACT_BWD_CASES))
def test_bn_act_bwd(case):
    L, S, _ = lib()
    c = A.bn_act_setup(case, True)
    A.assert_off_kink(c.y, c.gamma, c.beta, c.act, c.first)
    d = Device(c)
    ok(L.snd_bn_act_bwd(d.p("dx"), d.ld("dx"), d.p("y"), d.ld("y"), c.rows, c.c, d.p("gamma"), d.p("beta"), c.act,
                        c.first, d.p("dy"), d.ld("dy"), d.p("dgamma"), d.p("dbeta"), S), "snd_bn_act_bwd")
    after = d.back()
    res = A.bn_act_verify(c, after)
    if c.rows == 0:                                                 # dgamma = dbeta = 0, dy untouched
        assert not c.bufs["dgamma"].values(after["dgamma"]).any() and not c.bufs["dbeta"].values(after["dbeta"]).any()
        assert np.array_equal(after["dy"].view(np.uint32), c.bufs["dy"].arr.view(np.uint32))
    report("bn_act_bwd", case[0], res)


@pytest.mark.parametrize("case", A.ADD_CASES, ids=ids(A.ADD_CASES))
def test_add_strided(case):
    L, S, _ = lib()
    c = A.add_setup(case)
    d = Device(c)
    ok(L.snd_add_strided(c.rows, c.cols, A.ADD_ALPHA, d.p("x"), d.ld("x"), d.p("y"), d.ld("y"), S), "snd_add_strided")
    report("add_strided", case[0], A.add_verify(c, d.back()))


# ---------------------------------------------------------------- TF1 Adam
def hp():
    return tuple(A.ADAM_HP[k] for k in ("lr", "beta1", "beta2", "eps", "grad_scale"))


@pytest.mark.parametrize("case", A.ADAM_CASES, ids=ids(A.ADAM_CASES))
def test_adam_tf1(case):
    L, S, _ = lib()
    c = A.adam_setup(case)
    d = Device(c)
    vec = c.n % 4 == 0 and all(d.p(k) % 16 == 0 for k in "pgmv")
    assert vec == ("vec" in case[0] or c.n == 0), "the kernel this case is named for"
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    state, worst = A.initial(c), {}
    for t in range(1, A.ADAM_STEPS + 1):
        step.fill_(t)
        ok(L.snd_adam_tf1(d.p("p"), d.p("g"), d.p("m"), d.p("v"), c.n, *hp(), step.data_ptr(), S), "snd_adam_tf1")
        after = d.back()
        for k, r in A.adam_verify_step(c, state, after, t).items():     # from the state the GPU left
            worst[k] = max(worst.get(k, 0.0), r)
        state = after
    report("adam_tf1", case[0], worst)


@pytest.mark.parametrize("case", A.ADAM_RANGE_CASES, ids=ids(A.ADAM_RANGE_CASES))
def test_adam_tf1_ranges(case):
    L, S, _ = lib()
    c = A.adam_ranges_setup(case)
    d = Device(c)
    off = (ctypes.c_longlong * len(c.ranges))(*[o for o, _ in c.ranges])
    cnt = (ctypes.c_longlong * len(c.ranges))(*[k for _, k in c.ranges])
    step = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    ok(L.snd_adam_tf1_ranges(d.p("p"), d.p("g"), d.p("m"), d.p("v"), off, cnt, len(c.ranges), *hp(), step.data_ptr(), S),
       "snd_adam_tf1_ranges")
    report("adam_tf1_ranges", case[0], A.adam_verify_step(c, A.initial(c), d.back(), 5))


# ---------------------------------------------------------------- dense -> CSR
@pytest.mark.parametrize("short", [0, 5], ids=["cap_nnz", "cap_nnz_minus_5"])
def test_dense_to_csr(short):
    L, S, _ = lib()
    c = A.csr_setup(short)
    assert L.snd_dense_to_csr_workspace(c.B, c.n) == 4 * c.bufs["ws"].width
    d = Device(c)
    ok(L.snd_dense_to_csr(d.p("adj"), c.B, c.n, d.p("rowptr"), d.p("colidx"), c.cap, d.p("nnz_out"), d.p("ws"),
                          4 * c.bufs["ws"].width, S), "snd_dense_to_csr")
    A.csr_verify(c, d.back())


# ---------------------------------------------------------------- error returns
def rejected(rc, d):
    """SND_ERR_ARG with a message, returned before any launch: every buffer as it was."""
    _, _, _lib = lib()
    assert rc == ERR_ARG, rc
    assert _lib.last_error()
    after = d.back()
    for k, g in d.c.bufs.items():
        assert np.array_equal(after[k].view(np.uint8), g.arr.view(np.uint8)), f"{k} changed by a rejected call"


@pytest.mark.parametrize("width,fx", [(0, 0), (129, 0), (64, 17)])
def test_csr_spmm_rejects(width, fx):
    L, S, _ = lib()
    c = A.spmm_setup(A.SPMM_GCN_CASES[-1], True)
    d = Device(c)
    rejected(L.snd_csr_spmm(d.p("rowptr"), d.p("colidx"), c.rows, d.p("h"), d.ld("h"), width, d.p("out"), d.ld("out"),
                            1, d.p("gamma"), d.p("beta"), d.p("preact"), d.ld("preact"), d.p("x"), d.ld("x"), fx,
                            d.p("gamma2"), d.p("beta2"), d.p("out2"), d.ld("out2"), S), d)


@pytest.mark.parametrize("width,ldh,ldo", [(12, 72, 80), (136, 144, 152), (0, 72, 80), (-8, 72, 80), (64, 68, 80),
                                           (64, 72, 84)])
def test_csr_spmm_bf16_rejects(width, ldh, ldo):
    L, S, _ = lib()
    c = A.spmm_bf16_setup(A.SPMM_BF16_CASES[2], False)
    d = Device(c)
    rejected(L.snd_csr_spmm_bf16(d.p("rowptr"), d.p("colidx"), c.rows, d.p("h"), ldh, width, d.p("out"), ldo, c.n,
                                 c.B, 0, S), d)


@pytest.mark.parametrize("latent", [257, 0])
def test_reparam_kl_rejects(latent):
    L, S, _ = lib()
    c = A.reparam_setup(A.REPARAM_CASES[1])
    d = Device(c)
    rejected(L.snd_reparam_kl(d.p("ms"), d.ld("ms"), c.rows, latent, d.p("eps"), 0, 0, d.p("eps_out"), d.p("z"),
                              d.p("kl_part"), S), d)


@pytest.mark.parametrize("cin,cout", [(65, 4), (64, 5)])
def test_sigmoid_mse_rejects(cin, cout):
    L, S, _ = lib()
    c = A.head_setup(A.HEAD_CASES[2])                                # 1 row, 64 x 4: one block
    d = Device(c)
    ws = torch.zeros(cin * cout + cout, device=DEV)                  # large enough for the claimed shape
    rejected(L.snd_sigmoid_mse(d.p("u"), d.ld("u"), c.rows, cin, d.p("w"), d.p("b"), cout, d.p("target"),
                               d.ld("target"), d.p("sse"), d.p("yhat"), d.p("du"), d.ld("du"), d.p("dw"), d.p("db"),
                               ws.data_ptr(), 4 * ws.numel(), S), d)
    assert not ws.any()


@pytest.mark.parametrize("op", ["fwd", "bwd_data", "bwd_weight"])
def test_conv1d_rejects_rows_not_a_multiple_of_the_graph(op):
    L, S, _ = lib()
    c = A.conv_setup(A.CONV_CASES[3], A.F32, op)                     # 20 rows; claim 6 per graph
    d = Device(c)
    if op == "fwd":
        rc = L.snd_conv1d_same_fwd(d.p("x"), d.ld("x"), c.rows, 6, c.cin, d.p("w"), c.cout, d.p("bias"), d.p("gamma"),
                                   d.p("beta"), d.p("y_pre"), d.ld("y_pre"), d.p("out"), d.ld("out"), A.F32, S)
    elif op == "bwd_data":
        rc = L.snd_conv1d_same_bwd_data(d.p("dy"), d.ld("dy"), c.rows, 6, c.cout, d.p("w"), c.cin, d.p("dx"),
                                        d.ld("dx"), A.F32, S)
    else:
        rc = L.snd_conv1d_same_bwd_weight(d.p("x"), d.ld("x"), d.p("dy"), d.ld("dy"), c.rows, 6, c.cin, c.cout,
                                          d.p("dw"), d.p("ws"), 4 * c.bufs["ws"].width, A.F32, S)
    rejected(rc, d)


def test_strided_elementwise_ops_reject_a_short_ld():
    L, S, _ = lib()
    c = A.bn_act_setup(A.BN_ACT_CASES[4], False)                     # 300 x 5
    d = Device(c)
    for ldy, ldx in ((4, 8), (8, 4)):
        rejected(L.snd_bn_act_fwd(d.p("y"), ldy, c.rows, c.c, d.p("gamma"), d.p("beta"), c.act, c.first, d.p("x"),
                                  ldx, S), d)
    rejected(L.snd_bn_act_fwd(d.p("y"), 8, c.rows, c.c, d.p("gamma"), d.p("beta"), 3, c.first, d.p("x"), 8, S), d)
    c = A.bn_act_setup(A.BN_ACT_BWD_CASES[4], True)
    d = Device(c)
    for lds in ((4, 8, 8), (8, 4, 8), (8, 8, 4)):
        rejected(L.snd_bn_act_bwd(d.p("dx"), lds[0], d.p("y"), lds[1], c.rows, c.c, d.p("gamma"), d.p("beta"), c.act,
                                  c.first, d.p("dy"), lds[2], d.p("dgamma"), d.p("dbeta"), S), d)
    c = A.reparam_bwd_setup(A.REPARAM_BWD_CASES[1], "all")           # L = 100
    d = Device(c)
    for ldms, lddms in ((199, 205), (203, 199)):
        rejected(L.snd_reparam_bwd(d.p("ms"), ldms, c.rows, c.L, d.p("eps"), d.p("dz"), d.p("add_mu"), d.p("add_ls"),
                                   d.p("dms"), lddms, S), d)
    c = A.add_setup(A.ADD_CASES[1])                                  # 7 columns
    d = Device(c)
    for ldx, ldy in ((6, 9), (10, 6)):
        rejected(L.snd_add_strided(c.rows, c.cols, A.ADD_ALPHA, d.p("x"), ldx, d.p("y"), ldy, S), d)
