"""The references, bounds and guards of tests/abi_ops.py, checked without a GPU:

(a) on contiguous inputs every float64 reference equals its counterpart in oracle/ to 1e-12;
(b) a correct float32 implementation (abi_ops' emulation) passes every committed case;
(c) each planted fault fails its case, and the failure names the element;
(d) the guard helper sees a changed NaN payload, not only a changed value.
"""
import math
import re

import numpy as np
import pytest

import abi_ops as A
from oracle import ref_numpy as R


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max(initial=0.0) <= tol * max(np.abs(b).max(initial=0.0), 1e-300)


def ids(cases):
    return [c[0] for c in cases]


# ---------------------------------------------------------------- (a) the oracle
def test_spmm_reference_is_the_oracle():
    n, B = 37, 3
    rp, ci = A.random_batch_csr(n, B, 3)
    h = np.random.default_rng(0).standard_normal((n * B, 24))
    dense = []
    for b in range(B):
        a = np.zeros((n, n))
        for i in range(n):
            a[i, ci[rp[b * n + i]:rp[b * n + i + 1]] - b * n] = 1
        dense.append(a)
    close(A.ref_spmm(rp, ci, h).ref, R.spmm(dense, h, n))


@pytest.mark.parametrize("case", A.CONV_WGRAD_CASES, ids=ids(A.CONV_WGRAD_CASES))
def test_conv_references_are_the_oracle(case):
    _, npg, B, cin, cout, _ = case
    rng = np.random.default_rng(1)
    x, dy = rng.standard_normal((npg * B, cin)), rng.standard_normal((npg * B, cout))
    w, b = rng.standard_normal((5, cin, cout)), rng.standard_normal(cout)
    close(A.ref_conv_pre(x, w, b, npg, A.F32).ref, R.per_graph_conv(x, w, b, npg))
    dx, dw, _ = R.per_graph_conv_bwd(x, w, dy, npg)
    close(A.ref_conv_bwd_data(dy, w, npg, A.F32).ref, dx)
    close(A.ref_conv_bwd_weight(x, dy, npg, A.F32).ref, dw)


def test_adam_reference_is_the_oracle():
    rng = np.random.default_rng(2)
    n = 500
    hp = A.ADAM_HP
    lr, b1, b2, eps, gs = (float(np.float32(hp[k])) for k in ("lr", "beta1", "beta2", "eps", "grad_scale"))
    p, g = rng.standard_normal(n), rng.standard_normal(n)
    m, v = 0.1 * rng.standard_normal(n), rng.random(n)
    po, mo, vo = {"w": p.copy()}, {"w": m.copy()}, {"w": v.copy()}
    for t in (1, 2, 3):
        lm, lv = A.ref_adam_moments(g, m, v)
        m, v = lm.ref, lv.ref
        p = A.ref_adam_param(p, m, v, t, lrt=lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)).ref
        R.adam_tf1(po, {"w": g * gs}, mo, vo, t, lr, b1, b2, eps)
        close(m, mo["w"]), close(v, vo["w"]), close(p, po["w"])
        # the float32 lr_t the kernels use is the same number rounded once
        assert abs(float(A.adam_lrt(t)) / (lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)) - 1) <= 2.0 ** -24


def test_head_reference_is_the_oracle():
    rng = np.random.default_rng(3)
    rows, cin, cout = 40, 7, 3
    u, w, b = rng.standard_normal((rows, cin)), rng.standard_normal((cin, cout)), rng.standard_normal(cout)
    t, dw0, db0 = rng.random((rows, cout)), rng.standard_normal((cin, cout)), rng.standard_normal(cout)
    L = A.ref_head(u, w, b, t, dw0, db0)
    y = R.sigmoid(u @ w + b)
    dp = 2 * (y - t) / y.size * y * (1 - y)
    close(L["yhat"].ref, y), close(L["sse"].ref, ((y - t) ** 2).sum())
    close(L["du"].ref, dp @ w.T), close(L["dw"].ref, dw0 + u.T @ dp), close(L["db"].ref, db0 + dp.sum(0))


@pytest.mark.parametrize("act,first", A.BN_ACT_PAIRS)
def test_bn_act_references_are_the_disent_oracle_formulas(act, first):
    """oracle/ref_disent_model.py: bn = ref_torch.bn, lrelu = ref_torch.lrelu, torch.relu, and
    autograd for the backward."""
    import torch
    from oracle import ref_torch as T
    rng = np.random.default_rng(4)
    y, dx = rng.standard_normal((30, 5)), rng.standard_normal((30, 5))
    gam, bet = 1 + 0.3 * rng.standard_normal(5), 0.3 * rng.standard_normal(5)
    f = {0: lambda v: v, 1: torch.relu, 2: T.lrelu}[act]
    ty, tg, tb = (torch.tensor(a, requires_grad=True) for a in (y, gam, bet))
    x = T.bn(f(ty), tg, tb) if first else f(T.bn(ty, tg, tb))
    close(A.ref_bn_act_fwd(y, gam, bet, act, first).ref, x.detach().numpy())
    (x * torch.tensor(dx)).sum().backward()
    L = A.ref_bn_act_bwd(dx, y, gam, bet, act, first)
    close(L["dy"].ref, ty.grad.numpy()), close(L["dgamma"].ref, tg.grad.numpy()), close(L["dbeta"].ref, tb.grad.numpy())


def test_reparam_references_are_the_disent_oracle_formulas():
    """z = mu + eps e^logstd (ref_disent_model.py groups), its autograd backward, and the KL
    sum of optimizer.py:193 as the oracle writes it."""
    import torch
    rng = np.random.default_rng(5)
    rows, L = 20, 3
    ms, eps = 0.5 * rng.standard_normal((rows, 2 * L)), rng.standard_normal((rows, L))
    dz, am, al = (rng.standard_normal((rows, L)) for _ in range(3))
    tms = torch.tensor(ms, requires_grad=True)
    mu, ls = tms[:, :L], tms[:, L:]
    z = mu + torch.tensor(eps) * torch.exp(ls)
    close(A.ref_reparam_z(ms, eps, L).ref, z.detach().numpy())
    close(A.ref_reparam_kl(ms, L).ref, float(torch.sum(1 + 2 * ls - mu ** 2 - torch.exp(ls) ** 2).detach()), 1e-11)
    ((z * torch.tensor(dz)).sum() + (mu * torch.tensor(am)).sum() + (ls * torch.tensor(al)).sum()).backward()
    close(A.ref_reparam_bwd(ms, eps, L, dz, am, al).ref, tms.grad.numpy())
    close(A.ref_reparam_bwd(ms, eps, L, None, am, None).ref[:, L:], 0 * am)
    close(A.ref_add(ms, ms, -0.5).ref, 0.5 * ms)


def test_gemm_reference():
    rng = np.random.default_rng(6)
    a, b, bias = rng.standard_normal((9, 4)), rng.standard_normal((7, 9)), rng.standard_normal(7)
    close(A.ref_gemm(1, 1, a, b, bias, A.F32).ref, a.T @ b.T + bias)
    close(A.ref_gemm(0, 0, a.T, b.T, None, A.BF16).ref, A.bf16(a.T) @ A.bf16(b.T))


# ---------------------------------------------------------------- (b) a correct implementation passes
def passes(res):
    assert all(r < 1.0 for r in res.values()), res


@pytest.mark.parametrize("dtype", [A.F32, A.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", A.GEMM_CASES, ids=ids(A.GEMM_CASES))
def test_emulated_gemm_passes(case, dtype):
    c = A.gemm_setup(case, dtype)
    passes(A.gemm_verify(c, A.gemm_emulate(c)))


@pytest.mark.parametrize("dtype", [A.F32, A.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("op,case", [(op, k) for op in ("fwd", "bwd_data") for k in A.CONV_CASES]
                         + [("bwd_weight", k) for k in A.CONV_WGRAD_CASES],
                         ids=lambda v: v if isinstance(v, str) else v[0])
def test_emulated_conv_passes(op, case, dtype):
    c = A.conv_setup(case, dtype, op)
    passes(A.conv_verify(c, A.conv_emulate(c)))


def test_conv_split_cases_reach_what_they_claim():
    assert A.conv_splits(41 * 26) == 2 and A.conv_splits(1024) == 1 and A.conv_splits(1025) == 2
    kchunk = -(-(-(-1066 // 2)) // 64) * 64
    assert kchunk == 576 and 14 * 41 <= kchunk < 15 * 41         # the boundary falls inside graph 14


@pytest.mark.parametrize("gcn,case", [(False, k) for k in A.SPMM_PLAIN_CASES] + [(True, k) for k in A.SPMM_GCN_CASES],
                         ids=lambda v: v[0] if isinstance(v, tuple) else ("gcn" if v else "plain"))
def test_emulated_spmm_passes(gcn, case):
    c = A.spmm_setup(case, gcn)
    passes(A.spmm_verify(c, A.spmm_emulate(c)))


@pytest.mark.parametrize("ordered", [False, True], ids=["natural", "row_order"])
@pytest.mark.parametrize("case", A.SPMM_BF16_CASES, ids=ids(A.SPMM_BF16_CASES))
def test_emulated_spmm_bf16_passes(case, ordered):
    c = A.spmm_bf16_setup(case, ordered)
    assert np.array_equal(np.sort(c.order), np.arange(c.rows))
    passes(A.spmm_bf16_verify(c, A.spmm_bf16_emulate(c)))


@pytest.mark.parametrize("case", A.REPARAM_CASES, ids=ids(A.REPARAM_CASES))
def test_emulated_reparam_passes(case):
    c = A.reparam_setup(case)
    passes(A.reparam_verify(c, A.reparam_emulate(c)))


def test_reparam_cases_reach_the_grid_stride_loop():
    for _, rows, L in A.REPARAM_CASES[2:]:
        assert A.reparam_blocks(rows, L) * (256 // L) < rows
    assert [256 // L for _, _, L in A.REPARAM_CASES[2:]] == [2, 1]


@pytest.mark.parametrize("mode", A.REPARAM_BWD_MODES)
@pytest.mark.parametrize("case", A.REPARAM_BWD_CASES, ids=ids(A.REPARAM_BWD_CASES))
def test_emulated_reparam_bwd_passes(case, mode):
    c = A.reparam_bwd_setup(case, mode)
    passes(A.reparam_bwd_verify(c, A.reparam_bwd_emulate(c)))


@pytest.mark.parametrize("case", A.HEAD_CASES, ids=ids(A.HEAD_CASES))
def test_emulated_head_passes(case):
    c = A.head_setup(case)
    passes(A.head_verify(c, A.head_emulate(c)))


@pytest.mark.parametrize("case", A.BN_ACT_CASES, ids=ids(A.BN_ACT_CASES))
def test_emulated_bn_act_fwd_passes(case):
    c = A.bn_act_setup(case, False)
    passes(A.bn_act_verify(c, A.bn_act_emulate(c)))


@pytest.mark.parametrize("case", A.BN_ACT_BWD_CASES, ids=ids(A.BN_ACT_BWD_CASES))
def test_emulated_bn_act_bwd_passes(case):
    c = A.bn_act_setup(case, True)
    passes(A.bn_act_verify(c, A.bn_act_emulate(c)))


def test_bn_act_kink_assertion_fires():
    y, g, b = np.array([[1.0]], np.float32), np.array([1.0], np.float32), np.array([-A.BN_C], np.float32)
    with pytest.raises(AssertionError, match="kink"):
        A.assert_off_kink(y, g, b, 2, 0)
    A.assert_off_kink(y, g, b, 0, 0)
    A.assert_off_kink(y, g, b, 2, 1)


@pytest.mark.parametrize("case", A.ADD_CASES, ids=ids(A.ADD_CASES))
def test_emulated_add_passes(case):
    c = A.add_setup(case)
    passes(A.add_verify(c, A.add_emulate(c)))


@pytest.mark.parametrize("case", A.ADAM_CASES, ids=ids(A.ADAM_CASES))
def test_emulated_adam_passes(case):
    c = A.adam_setup(case)
    state = A.initial(c)
    for t in range(1, (A.ADAM_STEPS if c.n < 1 << 20 else 1) + 1):   # the 8.4 M case: one step here
        nxt = A.adam_emulate_step(c, state, t)
        passes(A.adam_verify_step(c, state, nxt, t))
        state = nxt


@pytest.mark.parametrize("case", A.ADAM_RANGE_CASES, ids=ids(A.ADAM_RANGE_CASES))
def test_emulated_adam_ranges_passes(case):
    c = A.adam_ranges_setup(case)
    state = A.initial(c)
    nxt = A.adam_emulate_step(c, state, 5)
    passes(A.adam_verify_step(c, state, nxt, 5))
    nxt["m"][A.G + 1500] += 1.0                                 # an element outside every range
    with pytest.raises(AssertionError, match=r"m\[1500\] outside the ranges changed"):
        A.adam_verify_step(c, state, nxt, 5)


@pytest.mark.parametrize("short", [0, 5])
def test_emulated_dense_to_csr_passes(short):
    c = A.csr_setup(short)
    A.csr_verify(c, A.csr_emulate(c))


# ---------------------------------------------------------------- (c) planted faults
ELEMENT = r"element \(\d+(, \d+)*,?\)"


def fails(fn, pattern):
    with pytest.raises(AssertionError, match=pattern) as e:
        fn()
    return str(e.value)


@pytest.mark.parametrize("dtype", [A.F32, A.BF16], ids=["f32", "bf16"])
def test_fault_conv_tap_crosses_a_graph_boundary(dtype):
    for op in ("fwd", "bwd_data", "bwd_weight"):
        c = A.conv_setup(A.CONV_CASES[1], dtype, op)              # 30 graphs of 3 nodes
        fails(lambda: A.conv_verify(c, A.conv_emulate(c, "cross_graph")), "conv1d_same_" + op + r".*" + ELEMENT)
    # the halo rows alone are wrong: in the 37-node case the first bad row is the last of graph 0
    c = A.conv_setup(A.CONV_CASES[2], dtype, "fwd")
    msg = fails(lambda: A.conv_verify(c, A.conv_emulate(c, "cross_graph")), "y_pre.*" + ELEMENT)
    row = int(re.search(r"element \((\d+),", msg).group(1))
    assert row % 37 in (0, 1, 35, 36)
    # one graph: there is no boundary to cross, the same fault changes nothing
    one = A.conv_setup(("one_graph", 37, 1, 5, 4, True), dtype, "fwd")
    A.conv_verify(one, A.conv_emulate(one, "cross_graph"))


@pytest.mark.parametrize("dtype", [A.F32, A.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [k for k in A.GEMM_CASES if k[5] > 0], ids=[k[0] for k in A.GEMM_CASES if k[5] > 0])
def test_fault_dropped_last_k_column(case, dtype):
    c = A.gemm_setup(case, dtype)
    fails(lambda: A.gemm_verify(c, A.gemm_emulate(c, "drop_last_k")), "snd_gemm c.*" + ELEMENT)


def test_fault_width_used_where_ld_belongs():
    c = A.gemm_setup(A.GEMM_CASES[0], A.F32)
    fails(lambda: A.gemm_verify(c, A.gemm_emulate(c, "width_for_ld")), "snd_gemm c.*" + ELEMENT + ".*nan")
    # with ld == width the same code is right: only the strided case can see it
    c = A.gemm_setup(A.GEMM_CASES[0], A.F32)
    c.bufs["c"] = A.guarded(c.m, c.n, name="c")
    A.gemm_verify(c, A.gemm_emulate(c, "width_for_ld"))


def test_fault_dw_overwritten_instead_of_accumulated():
    c = A.head_setup(A.HEAD_CASES[4])
    fails(lambda: A.head_verify(c, A.head_emulate(c, "dw_overwrite")), "sigmoid_mse dw.*" + ELEMENT)
    c.dw0[...] = 0                                               # zeroed first, as the old test did: unseen
    c.bufs["dw"] = A.guarded(c.cin, c.cout, data=c.dw0, name="dw")
    A.head_verify(c, A.head_emulate(c, "dw_overwrite"))


def test_fault_store_into_a_padding_column():
    c = A.spmm_setup(A.SPMM_PLAIN_CASES[4], False)               # ldo = 65
    fails(lambda: A.spmm_verify(c, A.spmm_emulate(c, "pad_store")), r"out: padding, \(row 3, column 64\) changed")


def test_fault_store_into_the_trailing_guard():
    c = A.spmm_setup(A.SPMM_PLAIN_CASES[0], False)
    fails(lambda: A.spmm_verify(c, A.spmm_emulate(c, "tail_guard_store")),
          r"out: trailing guard, \(row 53, column 0\) changed")


def test_fault_adam_m_from_the_unscaled_gradient():
    c = A.adam_setup(A.ADAM_CASES[1])
    state = A.initial(c)
    fails(lambda: A.adam_verify_step(c, state, A.adam_emulate_step(c, state, 1, "m_unscaled_grad"), 1),
          r"adam_tf1 m \(step 1\).*" + ELEMENT)


def test_fault_unwritten_output_and_padding_read():
    c = A.add_setup(A.ADD_CASES[1])
    after = A.add_emulate(c)
    c.bufs["y"].block(after["y"])[999, 6] = c.bufs["y"].block()[999, 6] * 0 + np.float32(np.nan)
    fails(lambda: A.add_verify(c, after), r"add_strided y: element \(999, 6\).*ratio inf")


# ---------------------------------------------------------------- (d) the guard helper
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f64", "i32"])
def test_guard_detects_a_changed_nan_payload(dtype):
    data = np.arange(12).reshape(3, 4)
    g = A.guarded(3, 4, 6, dtype, offset=1, data=data, name="buf")
    arr, off, check = g
    assert off == A.G + 1 and arr.size == off + 3 * 6 + A.G
    adt, idt, pat = A.PATTERN[dtype]
    assert np.array_equal(g.values(), data)
    if dtype != "i32":
        assert np.isnan(arr[0].astype(np.float32) if dtype != "bf16" else A.bf16_values(arr[:1])[0])
    check(arr.copy())
    inside = arr.copy()
    g.block(inside)[...] = 0                                     # the block itself is free to change
    check(inside)
    for pos, where in ((off + 4, r"padding, \(row 0, column 4\)"), (off + 17, r"padding, \(row 2, column 5\)"),
                       (off - 1, r"leading guard, \(row -1, column -1\)"), (0, r"leading guard"),
                       (off + 18, r"trailing guard, \(row 3, column 0\)"), (arr.size - 1, r"trailing guard")):
        bad = arr.copy()
        bad.view(idt)[pos] ^= idt(1)                             # still a quiet NaN: only the payload differs
        if dtype in ("f32", "f64"):
            assert np.isnan(bad[pos])
        with pytest.raises(AssertionError, match="buf: " + where):
            check(bad)


def test_guard_patterns_are_quiet_nans():
    assert np.isnan(np.array([A.PATTERN["f32"][2]], np.uint32).view(np.float32)[0])
    assert np.isnan(A.bf16_values(np.array([A.PATTERN["bf16"][2]], np.uint16))[0])
    assert np.isnan(np.array([A.PATTERN["f64"][2]], np.uint64).view(np.float64)[0])
    assert A.PATTERN["f32"][2] & 0x00400000 and A.PATTERN["bf16"][2] & 0x0040
