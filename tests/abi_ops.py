"""Guarded, strided operands and float64 references for the stand-alone C ABI ops
(include/snd_vae.h), plain NumPy: importable without a GPU.

Outside callers (ops.py, through which layers.py, autograd.py, rowshard.py and disent_model.py
call, and any FFI binding) hand the entry points raw pointers and leading dimensions.  This
module gives every op

* its operands in *guarded* buffers: G guard elements, ``rows`` rows of ``ld`` elements,
  G guard elements, with the guards and the padding columns ``width..ld-1`` holding one
  fixed quiet-NaN bit pattern.  A store outside the logical block changes a guard (compared
  through integer views, so a changed NaN payload counts); a load outside it puts a NaN
  into the result, which ``Link.ratio`` reports as an infinite ratio; an output element
  that is never written keeps the pattern and fails the same way;
* one float64 reference returning ``own_operands.Link`` objects, bounded by that module's
  derived rules only: (K + 4) 2^-23 mag for fp32 accumulation of K terms, + 2^-8 |ref| for
  a bf16 store, + 1e-6 relative for a value through a hardware exp / rcp / sqrt.  Where an
  output feeds another one inside the kernel (y_pre -> out, preact -> out -> out2, Adam's
  m', v' -> p') the second link is taken on the first one's STORED values;
* a float32 emulation (the same formulas at dt = float32, bf16 round-to-nearest-even where
  the kernel rounds): a correct implementation the bounds must admit, and the vehicle of
  the planted faults of tests/test_abi_ops_cpu.py.

An op is three functions over a context ``c`` (SimpleNamespace): ``<op>_setup(case)`` builds
the guarded operands (``c.bufs``: name -> Guarded), ``<op>_emulate(c)`` returns the buffers a
correct float32 implementation leaves (name -> flat array), ``<op>_verify(c, after)``
asserts every link (ratio < 1, the failure names the element) and every guard, and returns
{output: ratio}.  tests/test_gpu_abi_ops.py replaces the emulation with the library call.
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

from own_operands import (BN_C, KINK, TRANS, U23, Link, bf16, conv_bwd_data, conv_fwd, conv_wgrad,
                          ident, lrelu, lrelu_grad)

F32, BF16 = 0, 1                      # SND_F32 / SND_BF16
G = 64                                # guard elements (a multiple of 8: 16-byte aligned blocks)
# dtype -> (array dtype, integer view, guard pattern); the float patterns are quiet NaNs
PATTERN = {"f32": (np.float32, np.uint32, 0x7FC5A5A5), "bf16": (np.uint16, np.uint16, 0x7FC5),
           "f64": (np.float64, np.uint64, 0x7FF8A5A5A5A5A5A5), "i32": (np.int32, np.uint32, 0x7FC5A5A5),
           "u16": (np.uint16, np.uint16, 0xA5C5)}     # raw uint16 operands ("bf16" converts its data)


def bf16_bits(a):
    """float array -> bf16 bit patterns (round to nearest even) as uint16."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def bf16_values(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


class Guarded:
    """A logical [rows, width] operand inside a flat guarded array (see the module text)."""

    def __init__(self, name, rows, width, ld, dtype, offset, data):
        adt, idt, pat = PATTERN[dtype]
        self.name, self.rows, self.width, self.ld, self.dtype = name, rows, width, ld, dtype
        self.off = G + offset
        self.arr = np.full(self.off + rows * ld + G, pat, idt).view(adt)
        if data is not None:
            d = bf16_bits(data) if dtype == "bf16" else np.asarray(data, adt)
            self.block()[...] = d.reshape(rows, width)

    def __iter__(self):               # (array, element offset of [0, 0], check_untouched)
        return iter((self.arr, self.off, self.check_untouched))

    def block(self, a=None):
        """The logical block of ``a`` (default: the initial array) as a [rows, width] view."""
        a = self.arr if a is None else a
        return a[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.width]

    def values(self, a=None):
        """The logical block as float64 (bf16 decoded)."""
        b = self.block(a)
        return bf16_values(b) if self.dtype == "bf16" else np.asarray(b, np.float64)

    def check_untouched(self, after):
        """Every guard and padding element of ``after`` is bitwise the pattern."""
        adt, idt, pat = PATTERN[self.dtype]
        after = np.asarray(after)
        assert after.dtype == adt and after.shape == self.arr.shape, (self.name, after.dtype, after.shape)
        bits = after.view(idt)
        end = self.off + self.rows * self.ld
        bad = bits != idt(pat)
        bad[self.off:end].reshape(self.rows, self.ld)[:, :self.width] = False
        if bad.any():
            i = int(np.argmax(bad))
            if i < self.off:
                where = f"leading guard, (row -1, column {i - self.off})"
            elif i >= end:
                where = f"trailing guard, (row {self.rows}, column {i - end})"
            else:
                where = f"padding, (row {(i - self.off) // self.ld}, column {(i - self.off) % self.ld})"
            raise AssertionError(f"{self.name}: {where} changed: {pat:#x} -> {int(bits[i]):#x} "
                                 f"({int(bad.sum())} elements in all)")


def guarded(rows, width, ld=None, dtype="f32", offset=0, data=None, name="buffer"):
    """Guarded buffer of a [rows, width] operand with leading dimension ld (default width);
    ``offset`` extra leading guard elements make the base pointer not 16-byte aligned;
    ``data`` None leaves the block itself at the pattern (an output)."""
    ld = width if ld is None else ld
    assert ld >= width and rows >= 0 and offset >= 0
    return Guarded(name, rows, width, ld, dtype, offset, data)


def vec(n, dtype="f32", offset=0, data=None, name="buffer"):
    return guarded(1, n, n, dtype, offset, data, name)


def ratios(link, got):
    ref = np.asarray(link.ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / link.bound())
    return np.where(np.isfinite(got), r, np.inf), got, ref


def assert_link(name, link, got):
    """worst err / bound of one output; fails naming the worst element.  No exclusions."""
    assert link.excl is None, f"{name}: no element may be excluded"
    r, got, ref = ratios(link, got)
    if r.size == 0:
        return 0.0
    i = np.unravel_index(int(np.argmax(r)), r.shape) if r.ndim else ()
    worst = float(r[i])
    if not worst < 1.0:
        raise AssertionError(f"{name}: element {tuple(int(k) for k in i)} got {got[i]!r} ref {ref[i]!r} "
                             f"err {abs(got[i] - ref[i]):.3e} bound {float(link.bound()[i]):.3e} "
                             f"ratio {worst:.3f} ({int((r >= 1).sum())} of {r.size} over the bound)")
    return worst


def emulate_store(link):
    """What a correct implementation stores: the float32 result, bf16-rounded if so stored."""
    v = np.asarray(link.ref, np.float32).astype(np.float64)
    return bf16(v) if link.stored == "bf16" else v


def check_guards(c, after):
    for k, g in c.bufs.items():
        g.check_untouched(after[k])


def initial(c):
    return {k: g.arr.copy() for k, g in c.bufs.items()}


def put(c, after, name, value):
    g = c.bufs[name]
    v = np.asarray(value)
    g.block(after[name])[...] = (bf16_bits(v) if g.dtype == "bf16" else v).reshape(g.rows, g.width)


def _seed(case):
    # a stable seed from the case's numbers (str hashes are salted per process)
    return [int(v) for v in case if isinstance(v, (int, np.integer))] + [len(case)]


def _normal(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def _rd(dtype):
    return bf16 if dtype == BF16 else ident


def _t(dt):
    return lambda a: np.asarray(a, dt)


# ================================================================= snd_gemm
# (id, trans_a, trans_b, m, n, k, bias)
GEMM_CASES = (
    ("nn_65x67x129", 0, 0, 65, 67, 129, True),      # 3 K tiles, M and N tails
    ("tn_130x1x65", 1, 0, 130, 1, 65, False),       # A_COL, one column
    ("nt_1x130x64", 0, 1, 1, 130, 64, True),        # one row, exactly one K tile
    ("tt_63x65x200", 1, 1, 63, 65, 200, False),     # 4 K tiles: the t + 3 prefetch
    ("nn_7x5x0", 0, 0, 7, 5, 0, True),              # K = 0: C equals bias
    ("tt_64x64x1", 1, 1, 64, 64, 1, True),          # a single term
)


def ref_gemm(ta, tb, a, b, bias, dtype, dt=np.float64):
    rd, T = _rd(dtype), _t(dt)
    A, B = T(rd(a)), T(rd(b))
    A = A.T if ta else A
    B = B.T if tb else B
    ref, mag = A @ B, np.abs(A) @ np.abs(B)
    if bias is not None:
        ref, mag = ref + T(bias), mag + np.abs(T(bias))
    return Link(ref, mag, A.shape[1] + 1)


def gemm_setup(case, dtype):
    _, ta, tb, m, n, k, has_bias = case
    rng = np.random.default_rng(_seed(case))
    c = NS(case=case, dtype=dtype, ta=ta, tb=tb, m=m, n=n, k=k)
    ash, bsh = ((k, m) if ta else (m, k)), ((n, k) if tb else (k, n))
    c.a, c.b = _normal(rng, *ash), _normal(rng, *bsh)
    c.bias = _normal(rng, n) if has_bias else None
    c.bufs = {"a": guarded(*ash, ash[1] + 3, data=c.a, name="a"),
              "b": guarded(*bsh, bsh[1] + 3, data=c.b, name="b"),
              "c": guarded(m, n, n + 3, name="c")}
    if has_bias:
        c.bufs["bias"] = vec(n, data=c.bias, name="bias")
    return c


def gemm_emulate(c, fault=None):
    after = initial(c)
    a, b = c.a, c.b
    if fault == "drop_last_k" and c.k > 0:            # the last K column never reaches the sum
        a = a.copy()
        (a[-1:, :] if c.ta else a[:, -1:])[...] = 0
    out = emulate_store(ref_gemm(c.ta, c.tb, a, b, c.bias, c.dtype, np.float32))
    if fault == "width_for_ld":                       # rows stored at stride width, not ld
        g = c.bufs["c"]
        flat = after["c"][g.off:g.off + g.rows * g.width]
        flat[...] = out.astype(np.float32).ravel()
    else:
        put(c, after, "c", out)
    return after


def gemm_verify(c, after):
    res = {"c": assert_link("snd_gemm c", ref_gemm(c.ta, c.tb, c.a, c.b, c.bias, c.dtype),
                            c.bufs["c"].values(after["c"]))}
    check_guards(c, after)
    return res


# ================================================================= conv1d k=5 SAME
# (id, n_per_graph, B, cin, cout, bn)
CONV_CASES = (
    ("n1_b70_13_13", 1, 70, 13, 13, True),      # every tap but the centre is padding; step4 wraps
    ("n3_b30_3_70", 3, 30, 3, 70, True),        # several graph boundaries inside one 64-row tile
    ("n37_b3_70_3", 37, 3, 70, 3, True),        # K = 350
    ("n5_b4_50_20", 5, 4, 50, 20, True),        # the existing shape, strided
    ("n5_b4_50_20_plain", 5, 4, 50, 20, False), # gamma = NULL, y_pre = NULL
)
# the weight gradient also runs split-K: 1066 rows = 2 splits of kchunk 576, the boundary
# inside graph 14 (rows 574..614); and exactly 1024 rows (the last single-split size)
CONV_WGRAD_CASES = CONV_CASES[:4] + (
    ("n41_b26_6_10_split2", 41, 26, 6, 10, True),
    ("n32_b32_6_10_rows1024", 32, 32, 6, 10, True),
)


def conv_splits(rows):
    """snd_conv1d_bwd_weight_workspace's split count (gemm_splits(rows, 64))."""
    return max(1, min(64, -(-rows // 1024)))


def ref_conv_pre(x, w, bias, npg, dtype, dt=np.float64):
    rd, T = _rd(dtype), _t(dt)
    X, W = T(rd(x)), T(rd(w))
    ref, mag = conv_fwd(X, W, npg), conv_fwd(np.abs(X), np.abs(W), npg)
    if bias is not None:
        ref, mag = ref + T(bias), mag + np.abs(T(bias))
    return Link(ref, mag, 5 * x.shape[1] + 1)


def ref_conv_act(y_pre, gamma, beta, dt=np.float64):
    """out = lrelu(y_pre gamma c + beta) on the STORED y_pre (the epilogue's register value)."""
    T = _t(dt)
    y, gc, be = T(y_pre), T(gamma) * dt(BN_C), T(beta)
    return Link(lrelu(y * gc + be), np.abs(y * gc) + np.abs(be), 2)


def ref_conv_bwd_data(dy, w, npg, dtype, dt=np.float64):
    rd, T = _rd(dtype), _t(dt)
    D, W = T(rd(dy)), T(rd(w))
    return Link(conv_bwd_data(D, W, npg), conv_bwd_data(np.abs(D), np.abs(W), npg), 5 * dy.shape[1])


def ref_conv_bwd_weight(x, dy, npg, dtype, dt=np.float64):
    rd, T = _rd(dtype), _t(dt)
    X, D = T(rd(x)), T(rd(dy))
    return Link(conv_wgrad(X, D, npg), conv_wgrad(np.abs(X), np.abs(D), npg), x.shape[0])


def conv_setup(case, dtype, op):
    """op: "fwd", "bwd_data" or "bwd_weight"."""
    _, npg, B, cin, cout, bn = case
    rows = npg * B
    rng = np.random.default_rng(_seed(case))
    c = NS(case=case, dtype=dtype, op=op, npg=npg, rows=rows, cin=cin, cout=cout, bn=bn)
    c.x, c.dy = _normal(rng, rows, cin), _normal(rng, rows, cout)
    c.w = (_normal(rng, 5, cin, cout) / np.float32(math.sqrt(5 * cin)))
    c.bias, c.gamma, c.beta = _normal(rng, cout), 1 + 0.3 * _normal(rng, cout), 0.3 * _normal(rng, cout)
    ldx, ldy, ldo = cin + 5, cout + 1, cout + 2
    X = lambda: guarded(rows, cin, ldx, data=c.x, name="x")
    W = lambda: vec(5 * cin * cout, data=c.w, name="w")
    DY = lambda: guarded(rows, cout, ldy, data=c.dy, name="dy")
    if op == "fwd":
        c.bufs = {"x": X(), "w": W(), "bias": vec(cout, data=c.bias, name="bias"),
                  "out": guarded(rows, cout, ldo, name="out")}
        if bn:
            c.bufs.update(gamma=vec(cout, data=c.gamma, name="gamma"), beta=vec(cout, data=c.beta, name="beta"),
                          y_pre=guarded(rows, cout, ldy, name="y_pre"))
    elif op == "bwd_data":
        c.bufs = {"dy": DY(), "w": W(), "dx": guarded(rows, cin, ldx, name="dx")}
    else:
        c.splits = conv_splits(rows)
        c.bufs = {"x": X(), "dy": DY(), "dw": vec(5 * cin * cout, name="dw"),
                  "ws": vec(c.splits * 5 * cin * cout, name="ws")}
    return c


def conv_emulate(c, fault=None):
    after = initial(c)
    npg = c.rows if fault == "cross_graph" else c.npg     # taps run on into the next graph
    f32 = np.float32
    if c.op == "fwd":
        pre = emulate_store(ref_conv_pre(c.x, c.w, c.bias, npg, c.dtype, f32))
        if c.bn:
            put(c, after, "y_pre", pre)
            put(c, after, "out", emulate_store(ref_conv_act(pre, c.gamma, c.beta, f32)))
        else:
            put(c, after, "out", pre)
    elif c.op == "bwd_data":
        put(c, after, "dx", emulate_store(ref_conv_bwd_data(c.dy, c.w, npg, c.dtype, f32)))
    else:
        put(c, after, "dw", emulate_store(ref_conv_bwd_weight(c.x, c.dy, npg, c.dtype, f32)))
        after["ws"][G:G + c.bufs["ws"].width] = 0.0       # the slabs are scratch: any finite value
    return after


def conv_verify(c, after):
    res = {}
    if c.op == "fwd":
        pre = ref_conv_pre(c.x, c.w, c.bias, c.npg, c.dtype)
        if c.bn:
            got = c.bufs["y_pre"].values(after["y_pre"])
            res["y_pre"] = assert_link("conv1d_same_fwd y_pre", pre, got)
            res["out"] = assert_link("conv1d_same_fwd out", ref_conv_act(got, c.gamma, c.beta),
                                     c.bufs["out"].values(after["out"]))
        else:
            res["out"] = assert_link("conv1d_same_fwd out", pre, c.bufs["out"].values(after["out"]))
    elif c.op == "bwd_data":
        res["dx"] = assert_link("conv1d_same_bwd_data dx", ref_conv_bwd_data(c.dy, c.w, c.npg, c.dtype),
                                c.bufs["dx"].values(after["dx"]))
    else:
        res["dw"] = assert_link("conv1d_same_bwd_weight dw", ref_conv_bwd_weight(c.x, c.dy, c.npg, c.dtype),
                                c.bufs["dw"].values(after["dw"]).reshape(5, c.cin, c.cout))
        assert np.isfinite(c.bufs["ws"].values(after["ws"])).all(), "conv1d_same_bwd_weight: workspace slabs"
    check_guards(c, after)
    return res


# ================================================================= CSR SpMM (fp32)
SPMM_ROWS = 53                                              # 3 blocks of 16 rows + a tail of 5
SPMM_DEGREES = (0, 1, 3, 4, 5, 8, 9, 44, 2, 7, 12, 16, 6)   # cycled over the rows


def hand_csr(rows=SPMM_ROWS, seed=7):
    """One graph, built by hand: row r has SPMM_DEGREES[r % 13] sorted distinct neighbours."""
    rng = np.random.default_rng(seed)
    rp, ci = [0], []
    for r in range(rows):
        d = SPMM_DEGREES[r % len(SPMM_DEGREES)]
        ci.extend(sorted(rng.choice(rows, size=d, replace=False).tolist()))
        rp.append(len(ci))
    return np.asarray(rp, np.int32), np.asarray(ci, np.int32)


def csr_matrix(rp, ci, dt=np.float64):
    import scipy.sparse as sp
    R = len(rp) - 1
    return sp.csr_matrix((np.ones(len(ci), dt), ci.astype(np.int64), rp.astype(np.int64)), shape=(R, R))


# PLAIN: (id, width, ldh, ldo, h_offset)
SPMM_PLAIN_CASES = (
    ("w64_vec", 64, 64, 64, 0), ("w128_vec", 128, 128, 128, 0), ("w64_ldh66", 64, 66, 64, 0),
    ("w64_h_off1", 64, 64, 64, 1), ("w64_ldo65", 64, 64, 65, 0), ("w1", 1, 4, 2, 0),
    ("w17", 17, 20, 18, 0), ("w100", 100, 103, 101, 0), ("w127", 127, 130, 128, 0),
)
# GCN: (id, ldp, fx, out2) at width 64: ldp 64 takes the float4 kernel, 65 the scalar one
SPMM_GCN_CASES = tuple((f"ldp{ldp}_fx{fx}_{'out2' if o2 else 'no_out2'}", ldp, fx, o2)
                       for ldp in (64, 65) for fx in (0, 1, 16) for o2 in (False, True))


def ref_spmm(rp, ci, h, stored="f32", dt=np.float64):
    A, H = csr_matrix(rp, ci, dt), np.asarray(h, dt)
    return Link(A @ H, A @ np.abs(H), np.diff(rp).astype(np.float64)[:, None], stored)


def ref_gcn_out(preact, gamma, beta, x, dt=np.float64):
    """[lrelu(preact) gamma c + beta || x] on the STORED preact."""
    T = _t(dt)
    a, gc, be = lrelu(T(preact)), T(gamma) * dt(BN_C), T(beta)
    ref, mag = a * gc + be, np.abs(a * gc) + np.abs(be)
    if x is not None and x.shape[1]:
        ref, mag = np.concatenate([ref, T(x)], 1), np.concatenate([mag, np.abs(T(x))], 1)
    return Link(ref, mag, 2)


def ref_gcn_out2(out, gamma2, beta2, dt=np.float64):
    """out2 = out g2 c + b2 on the STORED out (the BN of the concat columns included)."""
    T = _t(dt)
    o, gc, be = T(out), T(gamma2) * dt(BN_C), T(beta2)
    return Link(o * gc + be, np.abs(o * gc) + np.abs(be), 2)


def spmm_setup(case, gcn):
    rp, ci = hand_csr()
    rows = SPMM_ROWS
    rng = np.random.default_rng(_seed(case) + [int(gcn)])
    c = NS(case=case, gcn=gcn, rp=rp, ci=ci, rows=rows)
    if not gcn:
        _, w, ldh, ldo, hoff = case
        c.width, c.fx, c.out2 = w, 0, False
        c.h = _normal(rng, rows, w)
        c.bufs = {"h": guarded(rows, w, ldh, offset=hoff, data=c.h, name="h"), "out": guarded(rows, w, ldo, name="out")}
    else:
        _, ldp, fx, o2 = case
        w = 64
        c.width, c.fx, c.out2 = w, fx, o2
        c.h, c.x = _normal(rng, rows, w), _normal(rng, rows, fx)
        c.gamma, c.beta = 1 + 0.3 * _normal(rng, w), 0.3 * _normal(rng, w)
        c.gamma2, c.beta2 = 1 + 0.3 * _normal(rng, w + fx), 0.3 * _normal(rng, w + fx)
        c.bufs = {"h": guarded(rows, w, 64, data=c.h, name="h"),
                  "out": guarded(rows, w + fx, w + fx + 1, name="out"),
                  "gamma": vec(w, data=c.gamma, name="gamma"), "beta": vec(w, data=c.beta, name="beta"),
                  "preact": guarded(rows, w, ldp, name="preact")}
        if fx:
            c.bufs["x"] = guarded(rows, fx, fx + 2, data=c.x, name="x")
        if o2:
            c.bufs.update(gamma2=vec(w + fx, data=c.gamma2, name="gamma2"), beta2=vec(w + fx, data=c.beta2, name="beta2"),
                          out2=guarded(rows, w + fx, w + fx + 3, name="out2"))
    c.bufs["rowptr"] = vec(rows + 1, "i32", data=rp, name="rowptr")
    c.bufs["colidx"] = vec(len(ci), "i32", data=ci, name="colidx")
    return c


def spmm_emulate(c, fault=None):
    after = initial(c)
    f32 = np.float32
    acc = emulate_store(ref_spmm(c.rp, c.ci, c.h, dt=f32))
    if not c.gcn:
        put(c, after, "out", acc)
        if fault == "pad_store":                     # the tile tail stores one column too far
            g = c.bufs["out"]
            after["out"][g.off + 3 * g.ld + g.width] = 0.0
        if fault == "tail_guard_store":              # ... one row too far
            g = c.bufs["out"]
            after["out"][g.off + g.rows * g.ld] = 0.0
        return after
    put(c, after, "preact", acc)
    out = emulate_store(ref_gcn_out(acc, c.gamma, c.beta, c.x, f32))
    put(c, after, "out", out)
    if c.out2:
        put(c, after, "out2", emulate_store(ref_gcn_out2(out, c.gamma2, c.beta2, f32)))
    return after


def spmm_verify(c, after):
    deg = np.diff(c.rp)
    assert {0, 1, 3, 4, 5, 8, 9} <= set(deg.tolist()) and deg.max() >= 40, "hand CSR: degrees"
    assert all(np.all(np.diff(c.ci[s:e]) > 0) for s, e in zip(c.rp[:-1], c.rp[1:])), "sorted, distinct"
    V = lambda k: c.bufs[k].values(after[k])
    res = {}
    if not c.gcn:
        res["out"] = assert_link("csr_spmm out", ref_spmm(c.rp, c.ci, c.h), V("out"))
    else:
        res["preact"] = assert_link("csr_spmm preact", ref_spmm(c.rp, c.ci, c.h), V("preact"))
        res["out"] = assert_link("csr_spmm out", ref_gcn_out(V("preact"), c.gamma, c.beta, c.x), V("out"))
        if c.fx:
            assert np.array_equal(V("out")[:, c.width:], c.x.astype(np.float64)), "csr_spmm: concat columns"
        if c.out2:
            res["out2"] = assert_link("csr_spmm out2", ref_gcn_out2(V("out"), c.gamma2, c.beta2), V("out2"))
    check_guards(c, after)
    return res


# ================================================================= CSR SpMM (bf16)
# (id, n, B, width): (37, 3) natural order, (32, 8) the XCD row-block order
SPMM_BF16_CASES = tuple((f"n{n}_b{B}_w{w}", n, B, w) for n, B in ((37, 3), (32, 8)) for w in (8, 24, 64, 72, 128))


def random_batch_csr(n, B, seed):
    rng = np.random.default_rng(seed)
    rp, ci = [0], []
    for r in range(n * B):
        d = int(rng.integers(0, min(n, 14)))
        ci.extend((r // n * n + np.sort(rng.choice(n, size=d, replace=False))).tolist())
        rp.append(len(ci))
    return np.asarray(rp, np.int32), np.asarray(ci, np.int32)


def spmm_bf16_setup(case, ordered):
    _, n, B, w = case
    rng = np.random.default_rng(_seed(case))
    c = NS(case=case, n=n, B=B, width=w, rows=n * B, ordered=ordered)
    c.rp, c.ci = random_batch_csr(n, B, 3)
    c.h = bf16(_normal(rng, c.rows, w))
    c.order = np.concatenate([b * n + rng.permutation(n) for b in range(B)]).astype(np.int32)
    c.bufs = {"h": guarded(c.rows, w, w + 8, "bf16", data=c.h, name="h"),
              "out": guarded(c.rows, w, w + 16, "bf16", name="out"),
              "rowptr": vec(c.rows + 1, "i32", data=c.rp, name="rowptr"),
              "colidx": vec(len(c.ci), "i32", data=c.ci, name="colidx")}
    if ordered:
        c.bufs["row_order"] = vec(c.rows, "i32", data=c.order, name="row_order")
    return c


def spmm_bf16_emulate(c, fault=None):
    after = initial(c)
    put(c, after, "out", emulate_store(ref_spmm(c.rp, c.ci, c.h, "bf16", np.float32)))
    return after


def spmm_bf16_verify(c, after):
    res = {"out": assert_link("csr_spmm_bf16 out", ref_spmm(c.rp, c.ci, c.h, "bf16"), c.bufs["out"].values(after["out"]))}
    check_guards(c, after)
    return res


# ================================================================= reparameterisation + KL
# (id, rows, L): the last two reach the grid-stride loop with 2 and 1 rows per block pass
REPARAM_CASES = (("r7_l1", 7, 1), ("r50_l3", 50, 3), ("r4101_l100", 4101, 100), ("r2085_l256", 2085, 256))
REPARAM_BWD_CASES = (("r9_l1", 9, 1), ("r300_l100", 300, 100))
REPARAM_BWD_MODES = ("all", "dz_only", "no_dz")


def reparam_blocks(rows, L):
    """snd_reparam_kl_blocks."""
    return max(1, min(2048, -(-rows * L // 256)))


def ref_reparam_z(ms, eps, L, dt=np.float64):
    T = _t(dt)
    mu, s, e = T(ms)[:, :L], T(ms)[:, L:], T(eps)
    t = e * np.exp(s)
    return Link(mu + t, np.abs(mu) + np.abs(t), 2, extra=TRANS * np.abs(t).astype(np.float64))


def ref_reparam_kl(ms, L, dt=np.float64):
    """sum(1 + 2s - mu^2 - e^2s), fp32 elements (kl_elem) summed in double: K = 4 on the sum
    of the |terms| an element is formed from (own_operands' "l:kl_sum" link)."""
    T, f64 = _t(dt), np.float64
    mu, s = T(ms)[:, :L], T(ms)[:, L:]
    x2 = 2 * s
    if dt is np.float64:
        br = np.expm1(x2) - x2
    else:                               # kl_elem's own branches
        tl = np.zeros_like(x2) + dt(1.0 / 3628800.0)
        for k in (362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0, 2.0):
            tl = tl * x2 + dt(1.0 / k)
        br = np.where(np.abs(x2) < 0.5, x2 * x2 * tl, (np.exp(x2) - 1) - x2)
    klx = np.where(np.abs(x2) >= 0.5, np.exp(x2) + 1.0 + np.abs(x2), 0.0).sum(dtype=f64)
    return Link(np.array((-br - mu * mu).sum(dtype=f64)), np.array((np.abs(br) + mu * mu).sum(dtype=f64) + klx), 4,
                extra=TRANS * float(klx))


def reparam_setup(case):
    _, rows, L = case
    rng = np.random.default_rng(_seed(case))
    c = NS(case=case, rows=rows, L=L, nb=reparam_blocks(rows, L))
    c.ms, c.eps = (0.5 * _normal(rng, rows, 2 * L)), _normal(rng, rows, L)
    c.bufs = {"ms": guarded(rows, 2 * L, 2 * L + 3, data=c.ms, name="ms"),
              "eps": guarded(rows, L, data=c.eps, name="eps"), "eps_out": guarded(rows, L, name="eps_out"),
              "z": guarded(rows, L, name="z"), "kl_part": vec(c.nb, "f64", name="kl_part")}
    return c


def reparam_emulate(c, fault=None):
    after = initial(c)
    put(c, after, "z", emulate_store(ref_reparam_z(c.ms, c.eps, c.L, np.float32)))
    put(c, after, "eps_out", c.eps)
    part = np.zeros(c.nb)
    part[0] = float(ref_reparam_kl(c.ms, c.L, np.float32).ref)
    put(c, after, "kl_part", part)
    return after


def reparam_verify(c, after):
    V = lambda k: c.bufs[k].values(after[k])
    res = {"z": assert_link("reparam_kl z", ref_reparam_z(c.ms, c.eps, c.L), V("z"))}
    assert np.array_equal(c.bufs["eps_out"].block(after["eps_out"]).view(np.uint32), c.eps.view(np.uint32)), \
        "reparam_kl: eps_out is not the injected eps, bit for bit"
    res["kl"] = assert_link("reparam_kl kl sum", ref_reparam_kl(c.ms, c.L), np.array(V("kl_part").sum()))
    check_guards(c, after)
    return res


def ref_reparam_bwd(ms, eps, L, dz, add_mu, add_ls, dt=np.float64):
    """dms = [dz + add_mu || dz eps e^s + add_logstd]; NULL operands are zero."""
    T = _t(dt)
    s, e = T(ms)[:, L:], T(eps)
    z = np.zeros_like(e)
    d, am, al = (z if dz is None else T(dz)), (z if add_mu is None else T(add_mu)), (z if add_ls is None else T(add_ls))
    t = d * e * np.exp(s)
    return Link(np.concatenate([d + am, t + al], 1),
                np.concatenate([np.abs(d) + np.abs(am), np.abs(t) + np.abs(al)], 1), 3,
                extra=np.concatenate([np.zeros(e.shape), TRANS * np.abs(t).astype(np.float64)], 1))


def reparam_bwd_setup(case, mode):
    _, rows, L = case
    rng = np.random.default_rng(_seed(case))
    c = NS(case=case, mode=mode, rows=rows, L=L)
    c.ms, c.eps = 0.5 * _normal(rng, rows, 2 * L), _normal(rng, rows, L)
    dz, am, al = _normal(rng, rows, L), _normal(rng, rows, L), _normal(rng, rows, L)
    c.dz = None if mode == "no_dz" else dz
    c.add_mu, c.add_ls = (am, al) if mode != "dz_only" else (None, None)
    c.bufs = {"ms": guarded(rows, 2 * L, 2 * L + 3, data=c.ms, name="ms"), "eps": guarded(rows, L, data=c.eps, name="eps"),
              "dms": guarded(rows, 2 * L, 2 * L + 5, name="dms")}
    for k in ("dz", "add_mu", "add_ls"):
        if getattr(c, k) is not None:
            c.bufs[k] = guarded(rows, L, data=getattr(c, k), name=k)
    return c


def reparam_bwd_emulate(c, fault=None):
    after = initial(c)
    put(c, after, "dms", emulate_store(ref_reparam_bwd(c.ms, c.eps, c.L, c.dz, c.add_mu, c.add_ls, np.float32)))
    return after


def reparam_bwd_verify(c, after):
    res = {"dms": assert_link("reparam_bwd dms", ref_reparam_bwd(c.ms, c.eps, c.L, c.dz, c.add_mu, c.add_ls),
                              c.bufs["dms"].values(after["dms"]))}
    check_guards(c, after)
    return res


# ================================================================= sigmoid head + MSE
# (id, rows, cin, cout, yhat): 256-row blocks; yhat NULL once
HEAD_CASES = tuple((f"r{r}_{ci}x{co}" + ("_no_yhat" if (r, ci) == (257, 7) else ""), r, ci, co, (r, ci) != (257, 7))
                   for r in (1, 255, 257, 513) for ci, co in ((1, 1), (7, 3), (64, 4)))


def head_blocks(rows):
    return -(-rows // 256)


def ref_head(u, w, b, t, dw0, db0, dt=np.float64):
    """{yhat, sse, du, dw, db}.  z = u w + b in fp32 (cin + 1 terms), yhat = 1 / (1 + e^-z):
    |d yhat| <= z's bound / 4 + 2e-6 yhat (exp, rcp).  Everything downstream is formed from
    the kernel's own yhat, so yhat's bound is carried: through diff = yhat - t into the
    squared error (double sums) and into dpre = 2 diff / count yhat (1 - yhat) (~6 fp32
    roundings), and from dpre into du = dpre w^T, dw += u^T dpre, db += sum dpre."""
    T, f64, ab = _t(dt), np.float64, np.abs
    U, W, Bv, Tg = T(u), T(w), T(b), T(t)
    rows, cin = U.shape
    cout = W.shape[1]
    zo, zm = U @ W + Bv, ab(U) @ ab(W) + ab(Bv)
    y = 1.0 / (1.0 + np.exp(-zo))
    dy = 0.25 * (cin + 5) * U23 * zm.astype(f64) + 2 * TRANS * y.astype(f64)
    diff = y - Tg
    cnt = dt(rows * cout)
    dp = dt(2.0) * diff / cnt * y * (1 - y)
    ddp = (2.0 / (rows * cout)) * (ab(y * (1 - y)) + ab(diff) * ab(1 - 2 * y)).astype(f64) * dy + 8 * U23 * ab(dp).astype(f64)
    e2 = np.asarray(diff, f64) ** 2
    out = {"yhat": Link(y, np.zeros_like(y), 0, extra=dy),
           "sse": Link(np.array(e2.sum()), np.array(e2.sum()), 4, extra=float((2 * ab(diff).astype(f64) * dy + dy * dy).sum())),
           "du": Link(dp @ W.T, ab(dp) @ ab(W.T), cout + 1, extra=ddp @ ab(W.T).astype(f64)),
           "dw": Link(T(dw0) + U.T @ dp, ab(T(dw0)) + ab(U.T) @ ab(dp), rows + 2, extra=ab(U.T).astype(f64) @ ddp),
           "db": Link(T(db0) + dp.sum(0), ab(T(db0)) + ab(dp).sum(0), rows + 2, extra=ddp.sum(0))}
    return out


def head_setup(case):
    _, rows, cin, cout, yh = case
    rng = np.random.default_rng(_seed(case))
    c = NS(case=case, rows=rows, cin=cin, cout=cout, nb=head_blocks(rows), has_yhat=yh)
    c.u, c.w, c.b = _normal(rng, rows, cin), _normal(rng, cin, cout) / np.float32(math.sqrt(cin)), _normal(rng, cout)
    c.t = rng.random((rows, cout)).astype(np.float32)
    c.dw0, c.db0 = _normal(rng, cin, cout), _normal(rng, cout)          # the documented += is observed
    c.bufs = {"u": guarded(rows, cin, cin + 3, data=c.u, name="u"), "w": guarded(cin, cout, data=c.w, name="w"),
              "b": vec(cout, data=c.b, name="b"), "target": guarded(rows, cout, cout + 1, data=c.t, name="target"),
              "sse": vec(c.nb, "f64", name="sse"), "du": guarded(rows, cin, cin + 2, name="du"),
              "dw": guarded(cin, cout, data=c.dw0, name="dw"), "db": vec(cout, data=c.db0, name="db"),
              "ws": vec(c.nb * (cin * cout + cout), name="ws")}
    if yh:
        c.bufs["yhat"] = guarded(rows, cout, name="yhat")
    return c


def head_emulate(c, fault=None):
    after = initial(c)
    dw0 = np.zeros_like(c.dw0) if fault == "dw_overwrite" else c.dw0   # dw = instead of dw +=
    L = ref_head(c.u, c.w, c.b, c.t, dw0, c.db0, np.float32)
    for k in ("du", "dw", "db") + (("yhat",) if c.has_yhat else ()):
        put(c, after, k, emulate_store(L[k]))
    part = np.zeros(c.nb)
    part[0] = float(L["sse"].ref)
    put(c, after, "sse", part)
    after["ws"][G:G + c.bufs["ws"].width] = 0.0
    return after


def head_verify(c, after):
    V = lambda k: c.bufs[k].values(after[k])
    L = ref_head(c.u, c.w, c.b, c.t, c.dw0, c.db0)
    res = {k: assert_link(f"sigmoid_mse {k}", L[k], V(k)) for k in ("du", "dw", "db") + (("yhat",) if c.has_yhat else ())}
    res["sse"] = assert_link("sigmoid_mse sse", L["sse"], np.array(V("sse").sum()))
    assert np.isfinite(V("ws")).all(), "sigmoid_mse: workspace partials"
    check_guards(c, after)
    return res


# ================================================================= frozen BN + activation
BN_ACT_PAIRS = tuple((act, first) for act in (0, 1, 2) for first in (0, 1))
BN_ACT_SHAPES = ((1, 1), (300, 5), (1031, 33))
BN_ACT_CASES = tuple((f"act{a}_first{f}_r{r}_c{cc}", a, f, r, cc) for a, f in BN_ACT_PAIRS for r, cc in BN_ACT_SHAPES)
# backward extras: (id, act, first, rows, c, want dgamma / dbeta)
BN_ACT_BWD_CASES = tuple(k + (True,) for k in BN_ACT_CASES) + (
    ("act2_first0_r300_c5_no_dgamma", 2, 0, 300, 5, False), ("act1_first0_r0_c5", 1, 0, 0, 5, True))


def _act(v, act):
    return np.maximum(v, 0) if act == 1 else (lrelu(v) if act == 2 else v)


def _act_d(v, act):
    one = v.dtype.type(1.0)
    if act == 1:
        return np.where(v > 0, one, v.dtype.type(0.0))
    return lrelu_grad(v) if act == 2 else np.ones_like(v)


def bn_preact(y, gamma, beta, first):
    """(pre-activation, its kink width) in float64: the activation's argument is y itself
    (act_first: exact, the sign of a stored value) or T = y gamma c + beta, which the GPU
    forms in fp32 and may land on the other side of 0 within 2^-22 (|y gamma c| + |beta|)."""
    y, gc, be = np.asarray(y, np.float64), np.asarray(gamma, np.float64) * BN_C, np.asarray(beta, np.float64)
    if first:
        return y, np.zeros_like(y)
    return y * gc + be, KINK * (np.abs(y * gc) + np.abs(be))


def assert_off_kink(y, gamma, beta, act, first):
    if act:
        t, w = bn_preact(y, gamma, beta, first)
        bad = np.abs(t) <= w
        assert not bad.any(), f"bn_act input on the activation kink at {np.argwhere(bad)[0]}"


def ref_bn_act_fwd(y, gamma, beta, act, first, dt=np.float64):
    T = _t(dt)
    Y, gc, be = T(y), T(gamma) * dt(BN_C), T(beta)
    if first:
        a = _act(Y, act)
        return Link(gc * a + be, np.abs(gc * a) + np.abs(be), 2)
    return Link(_act(gc * Y + be, act), np.abs(gc * Y) + np.abs(be), 2)


def ref_bn_act_bwd(dx, y, gamma, beta, act, first, dt=np.float64):
    """{dy, dgamma, dbeta}: dgamma = sum du c t, dbeta = sum du (fp32 sums over the rows)."""
    T, c = _t(dt), dt(BN_C)
    D, Y, g, be = T(dx), T(y), T(gamma), T(beta)
    gc = g * c
    rows = Y.shape[0]
    if first:                           # x = BN(act(y))
        t, du = _act(Y, act), D
        dy = Link(du * gc * _act_d(Y, act), np.abs(du * gc), 2)
    else:                               # x = act(BN(y))
        t, du = Y, D * _act_d(gc * Y + be, act)
        dy = Link(du * gc, np.abs(du * gc), 2)
    return {"dy": dy, "dgamma": Link((du * c * t).sum(0), np.abs(du * c * t).sum(0), rows + 2),
            "dbeta": Link(du.sum(0), np.abs(du).sum(0), rows)}


def bn_act_setup(case, bwd):
    _, act, first, rows, cc = case[:5]
    rng = np.random.default_rng(_seed(case))
    c = NS(case=case, act=act, first=first, rows=rows, c=cc, bwd=bwd, want_dg=(case[5] if bwd else False))
    c.y, c.dx = _normal(rng, rows, cc), _normal(rng, rows, cc)
    c.gamma, c.beta = 1 + 0.3 * _normal(rng, cc), 0.3 * _normal(rng, cc)
    t, w = bn_preact(c.y, c.gamma, c.beta, first)      # move anything on the kink well off it
    c.y = np.where(np.abs(t) <= 4 * w + 1e-30, c.y + np.float32(0.5), c.y).astype(np.float32)
    c.bufs = {"y": guarded(rows, cc, cc + 3, data=c.y, name="y"), "gamma": vec(cc, data=c.gamma, name="gamma"),
              "beta": vec(cc, data=c.beta, name="beta")}
    if not bwd:
        c.bufs["x"] = guarded(rows, cc, cc + 3, name="x")
    else:
        c.bufs.update(dx=guarded(rows, cc, cc + 3, data=c.dx, name="dx"), dy=guarded(rows, cc, cc + 3, name="dy"))
        if c.want_dg:
            c.bufs.update(dgamma=vec(cc, name="dgamma"), dbeta=vec(cc, name="dbeta"))
    return c


def bn_act_emulate(c, fault=None):
    after = initial(c)
    if not c.bwd:
        put(c, after, "x", emulate_store(ref_bn_act_fwd(c.y, c.gamma, c.beta, c.act, c.first, np.float32)))
    else:
        L = ref_bn_act_bwd(c.dx, c.y, c.gamma, c.beta, c.act, c.first, np.float32)
        for k in ("dy",) + (("dgamma", "dbeta") if c.want_dg else ()):
            put(c, after, k, emulate_store(L[k]))
    return after


def bn_act_verify(c, after):
    assert_off_kink(c.y, c.gamma, c.beta, c.act, c.first)
    V = lambda k: c.bufs[k].values(after[k])
    if not c.bwd:
        res = {"x": assert_link("bn_act_fwd x", ref_bn_act_fwd(c.y, c.gamma, c.beta, c.act, c.first), V("x"))}
    else:
        L = ref_bn_act_bwd(c.dx, c.y, c.gamma, c.beta, c.act, c.first)
        res = {k: assert_link(f"bn_act_bwd {k}", L[k], V(k).reshape(np.shape(L[k].ref)))
               for k in ("dy",) + (("dgamma", "dbeta") if c.want_dg else ())}
    check_guards(c, after)
    return res


# ================================================================= y += alpha x
ADD_CASES = (("r1_c1", 1, 1), ("r1000_c7", 1000, 7))
ADD_ALPHA = -0.5


def ref_add(y0, x, alpha, dt=np.float64):
    T = _t(dt)
    t = dt(alpha) * T(x)
    return Link(T(y0) + t, np.abs(T(y0)) + np.abs(t), 2)


def add_setup(case):
    _, rows, cols = case
    rng = np.random.default_rng(_seed(case))
    c = NS(case=case, rows=rows, cols=cols, x=_normal(rng, rows, cols), y0=_normal(rng, rows, cols))
    c.bufs = {"x": guarded(rows, cols, cols + 3, data=c.x, name="x"), "y": guarded(rows, cols, cols + 2, data=c.y0, name="y")}
    return c


def add_emulate(c, fault=None):
    after = initial(c)
    put(c, after, "y", emulate_store(ref_add(c.y0, c.x, ADD_ALPHA, np.float32)))
    return after


def add_verify(c, after):
    res = {"y": assert_link("add_strided y", ref_add(c.y0, c.x, ADD_ALPHA), c.bufs["y"].values(after["y"]))}
    check_guards(c, after)
    return res


# ================================================================= TF1 Adam
ADAM_HP = dict(lr=0.0008, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=0.5)
ADAM_STEPS = 3
# (id, n, pointer offset in floats)
ADAM_CASES = (
    ("n1000_vec", 1000, 0),                                  # float4 kernel
    ("n1003_scalar", 1003, 0),                               # scalar kernel (n % 4)
    ("n1000_off1_scalar", 1000, 1),                          # scalar kernel (unaligned pointers)
    ("n528387_scalar_stride", 2048 * 256 + 4099, 0),         # scalar grid stride
    ("n8389808_vec_stride", 4 * (8192 * 256 + 300), 0),      # float4 grid stride
    ("n0", 0, 0),
)
ADAM_RANGE_N = 8192
ADAM_RANGE_CASES = (("vec", ((0, 1000), (2000, 400), (4096, 3000))), ("fallback", ((3, 997), (2001, 398))))


def adam_lrt(t, hp=ADAM_HP):
    """lr_t: float64 arithmetic on the float32 hyper-parameters, rounded to float32."""
    lr, b1, b2 = (float(np.float32(hp[k])) for k in ("lr", "beta1", "beta2"))
    return np.float32(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def ref_adam_moments(g, m, v, hp=ADAM_HP, dt=np.float64, unscaled=False):
    """adam_elem's m' and v' (K = 2): 1 - beta in float32; g = grad * grad_scale."""
    T = _t(dt)
    b1, b2 = np.float32(hp["beta1"]), np.float32(hp["beta2"])
    ob1, ob2 = dt(np.float32(1) - b1), dt(np.float32(1) - b2)
    gs = T(g) * dt(np.float32(1.0 if unscaled else hp["grad_scale"]))
    if dt is np.float32:
        gs = gs.astype(np.float32)
    m1a, m1b = dt(b1) * T(m), ob1 * gs
    v1a, v1b = dt(b2) * T(v), ob2 * gs * gs
    return Link(m1a + m1b, np.abs(m1a) + np.abs(m1b), 2), Link(v1a + v1b, np.abs(v1a) + np.abs(v1b), 2)


def ref_adam_param(p, m1, v1, t, hp=ADAM_HP, dt=np.float64, lrt=None):
    """p' = p - lr_t m' / (sqrt(v') + eps) on the STORED m', v': one hardware sqrt and one
    hardware rcp (2e-6 of the update covers them and the three roundings around them) and
    the final subtraction's rounding (2^-24 |p'|).  ``lrt`` overrides the float32 lr_t."""
    T = _t(dt)
    upd = dt(adam_lrt(t, hp) if lrt is None else lrt) * T(m1) / (np.sqrt(T(v1)) + dt(np.float32(hp["eps"])))
    ref = T(p) - upd
    return Link(ref, np.zeros_like(ref), 0,
                extra=2.0 ** -24 * np.abs(ref).astype(np.float64) + 2e-6 * np.abs(upd).astype(np.float64))


def adam_setup(case):
    _, n, off = case
    rng = np.random.default_rng(_seed(case))
    c = NS(case=case, n=n, off=off, ranges=None)
    c.p, c.g = _normal(rng, n), _normal(rng, n)
    c.m, c.v = 0.1 * _normal(rng, n), rng.random(n).astype(np.float32)
    c.bufs = {k: vec(n, offset=off, data=getattr(c, k), name=k) for k in ("p", "g", "m", "v")}
    return c


def adam_ranges_setup(case):
    _, ranges = case
    n = ADAM_RANGE_N
    rng = np.random.default_rng(3)
    c = NS(case=case, n=n, off=0, ranges=ranges)
    c.p, c.g = _normal(rng, n), _normal(rng, n)
    c.m, c.v = 0.1 * _normal(rng, n), rng.random(n).astype(np.float32)
    c.inside = np.zeros(n, bool)
    for o, k in ranges:
        c.inside[o:o + k] = True
    c.bufs = {k: vec(n, data=getattr(c, k), name=k) for k in ("p", "g", "m", "v")}
    return c


def adam_state(c, after):
    return tuple(np.asarray(c.bufs[k].block(after[k])[0], np.float32).copy() for k in ("p", "m", "v"))


def adam_emulate_step(c, before, t, fault=None):
    """One step from the buffers ``before`` (name -> flat array): the buffers after it."""
    p, m, v = adam_state(c, before)
    f32 = np.float32
    lm, lv = ref_adam_moments(c.g, m, v, dt=f32, unscaled=(fault == "m_unscaled_grad"))
    if fault == "m_unscaled_grad":
        lv = ref_adam_moments(c.g, m, v, dt=f32)[1]
    m1, v1 = emulate_store(lm).astype(f32), emulate_store(lv).astype(f32)
    p1 = emulate_store(ref_adam_param(p, m1, v1, t, dt=f32)).astype(f32)
    after = {k: a.copy() for k, a in before.items()}
    sel = slice(None) if c.ranges is None else c.inside
    for k, new in (("p", p1), ("m", m1), ("v", v1)):
        c.bufs[k].block(after[k])[0][sel] = new[sel]
    return after


def adam_verify_step(c, before, after, t):
    """One step against the reference started from the state ``before`` (the GPU's own)."""
    p0, m0, v0 = adam_state(c, before)
    p1, m1, v1 = adam_state(c, after)
    sel = slice(None) if c.ranges is None else c.inside
    lm, lv = ref_adam_moments(c.g[sel], m0[sel], v0[sel])
    res = {"m": assert_link(f"adam_tf1 m (step {t})", lm, m1[sel]), "v": assert_link(f"adam_tf1 v (step {t})", lv, v1[sel])}
    res["p"] = assert_link(f"adam_tf1 p (step {t})", ref_adam_param(p0[sel], m1[sel], v1[sel], t), p1[sel])
    if c.ranges is not None:
        for k, a0, a1 in (("p", p0, p1), ("m", m0, m1), ("v", v0, v1)):
            same = a0.view(np.uint32)[~c.inside] == a1.view(np.uint32)[~c.inside]
            assert same.all(), f"adam_tf1_ranges: {k}[{int(np.flatnonzero(~c.inside)[np.argmin(same)])}] outside the ranges changed"
    assert np.array_equal(c.bufs["g"].arr.view(np.uint32), after["g"].view(np.uint32)), "adam_tf1: grad changed"
    check_guards(c, after)
    return res


# ================================================================= dense -> CSR
CSR_N, CSR_B = 300, 2                   # NT = 256 threads: two passes per row


def csr_setup(short=0):
    """``short``: colidx capacity = nnz - short (0: exact)."""
    n, B = CSR_N, CSR_B
    rng = np.random.default_rng(17)
    adj = rng.choice(np.array([0.0, 1.0, 0.5, -0.0], np.float32), size=(B, n, n), p=[0.9, 0.04, 0.03, 0.03])
    c = NS(n=n, B=B, adj=adj, short=short)
    mask = adj != 0                      # -0.0 is not an edge
    mask[:, np.arange(n), np.arange(n)] = False
    assert np.signbit(adj).any() and mask[:, :, 256:].any() and adj[:, np.arange(n), np.arange(n)].any()
    b, i, j = np.nonzero(mask)
    c.colidx = (b * n + j).astype(np.int32)
    c.rowptr = np.concatenate([[0], np.cumsum(mask.reshape(B * n, n).sum(1))]).astype(np.int32)
    c.nnz = len(c.colidx)
    c.cap = c.nnz - short
    c.bufs = {"adj": vec(B * n * n, data=adj, name="adj"), "rowptr": vec(B * n + 1, "i32", name="rowptr"),
              "colidx": vec(c.cap, "i32", name="colidx"), "nnz_out": vec(1, "i32", name="nnz_out"),
              "ws": vec(B * n, "i32", name="ws")}
    return c


def csr_emulate(c, fault=None):
    after = initial(c)
    put(c, after, "rowptr", c.rowptr)
    put(c, after, "colidx", c.colidx[:c.cap])
    put(c, after, "nnz_out", np.array([-1 if c.short else c.nnz], np.int32))
    put(c, after, "ws", np.diff(c.rowptr))
    return after


def csr_verify(c, after):
    B = lambda k: c.bufs[k].block(after[k])[0]
    assert int(B("nnz_out")[0]) == (-1 if c.short else c.nnz), ("dense_to_csr nnz_out", int(B("nnz_out")[0]), c.nnz)
    assert np.array_equal(B("rowptr"), c.rowptr), "dense_to_csr rowptr"
    bad = np.flatnonzero(B("colidx") != c.colidx[:c.cap])
    assert bad.size == 0, f"dense_to_csr colidx[{bad[:1]}]"
    check_guards(c, after)
    return {}
