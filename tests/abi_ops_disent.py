"""Guarded operands, float64 references and float32 emulations for the disentangled-model
entry points of include/snd_vae.h (snd_e2e_fwd / _bwd, snd_e2e_pair_fwd / _bwd with its
workspace, snd_bn_relu_fwd / _bwd, snd_e2e_head_ce, snd_latent_reg with its workspace), on
the harness of tests/abi_ops.py and with its contract: ``<op>_setup(case)``,
``<op>_emulate(c, fault=None)``, ``<op>_verify(c, after)``.

These entry points take contiguous operands, so the guarded buffers have ld = width; the
guards, the NaN-patterned outputs and the exactly-sized workspaces do the work: an element
never written, or accumulated into, keeps or spreads the NaN and shows as an infinite ratio.

Bars, all from own_operands' rules ((K + 4) 2^-23 mag for an fp32 sum of K terms; + 1e-6
relative through a hardware exp / log; an upstream bound carried into what sums it), with K
and mag read off the formula in the header:

* e2e forward / backward, pair forward / backward, bn_relu: single-stage, exactly that rule;
* head: the logits are not stored, so their bound (the BN pre-activation's two roundings
  carried through W) is carried through the softmax into CE, dy and the reductions; the count
  must be exact, which the setup makes decidable (every off-diagonal margin |l1 - l0| larger
  than the two logits' bounds together);
* latent_reg: kl (summed in double), the KL term and the KL gradient on the rule as it stands;
  the DIP and TC values and gradients on the rule propagated stage by stage over the kernel's
  literal formula (``ref_latent``): mean and covariance, G = d DIP / d cov and G (mu - mean);
  Q, S = sum_l Q, the two log-sum-exps, the softmax weights W and the three sums over them,
  then the path through z.  No output of this module is on an inherited bar.
"""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np

import abi_ops as A
from abi_ops import assert_link, check_guards, guarded, initial, put, vec
from own_operands import BN_C, TRANS, U23, Link

LOG_2PI = float(np.log(2.0 * np.pi))


def _base(K, mag):
    return (np.asarray(K, np.float64) + 4.0) * U23 * np.asarray(mag, np.float64)


def _rng(case):
    return np.random.default_rng(A._seed(case))


def _scratch(c, after, name):
    g = c.bufs[name]
    after[name][g.off:g.off + g.width] = 0.0                      # scratch: any value


# ================================================================= e2e filter
# (id, B, N, C, K, O, pointer offset)
E2E_CASES = (
    ("b2_n7_c3_k7_o5", 2, 7, 3, 7, 5, 0),
    ("b1_n6_c2_k4_o3", 1, 6, 2, 4, 3, 0),           # even K != N
    ("b2_n5_c3_k1_o2", 2, 5, 3, 1, 2, 0),
    ("b1_n4_c2_k11_o3", 1, 4, 2, 11, 3, 0),         # K > 2N: taps clipped on both sides
    ("b1_n9_c1_k3_o1", 1, 9, 1, 3, 1, 0),
    ("b3_n18_c2_k18_o2", 3, 18, 2, 18, 2, 0),       # P = 972: the 256-thread tree, 4 trips, a tail
    ("b2_n7_c3_k7_o5_off1", 2, 7, 3, 7, 5, 1),      # every pointer 4 bytes off 16-byte alignment
)


def _shift(a, s, axis):
    """b[.., j, ..] = a[.., j + s, ..] along axis, zero outside."""
    n = a.shape[axis]
    out = np.zeros_like(a)
    if abs(s) >= n:
        return out
    dst, src = [slice(None)] * a.ndim, [slice(None)] * a.ndim
    dst[axis], src[axis] = (slice(0, n - s), slice(s, n)) if s >= 0 else (slice(-s, n), slice(0, n + s))
    out[tuple(dst)] = a[tuple(src)]
    return out


def _e2e_taps(K, N, fault):
    pb = K // 2 if fault == "pb_k_half" else (K - 1) // 2
    return [(t, t - pb) for t in range(min(K, N) if fault == "taps_clipped_to_n" else K)]


def ref_e2e_fwd(x, w, b, dt=np.float64, fault=None):
    """out = 2 b1 + sum_t (x[b, i, j + t - p] + x[b, i + t - p, j]) w1[t]: one term per product."""
    T = A._t(dt)
    X, W, Bv = T(x), T(w), T(b)
    K, C, O = W.shape
    N = X.shape[1]
    ax2 = 2 if fault == "column_slides_over_j" else 1
    ref, mag, cnt = 2 * Bv + np.zeros(X.shape[:3] + (O,), dt), 2 * np.abs(Bv) + np.zeros(X.shape[:3] + (O,), dt), 0.0
    one = np.ones(X.shape[:3] + (1,))
    for t, s in _e2e_taps(K, N, fault):
        ref = ref + (_shift(X, s, 2) + _shift(X, s, ax2)) @ W[t]
        mag = mag + (np.abs(_shift(X, s, 2)) + np.abs(_shift(X, s, ax2))) @ np.abs(W[t])
        cnt = cnt + _shift(one, s, 2) + _shift(one, s, 1)
    return Link(ref, mag, C * cnt + 1)


def ref_e2e_bwd(x, w, dout, dt=np.float64, fault=None):
    """{dx, dw1, db1} of sum(out dout)."""
    T = A._t(dt)
    X, W, D = T(x), T(w), T(dout)
    K, C, O = W.shape
    N, P = X.shape[1], X.shape[0] * X.shape[1] * X.shape[2]
    ax2 = 2 if fault == "column_slides_over_j" else 1
    dx, dxm, cnt = np.zeros_like(X), np.zeros_like(X), 0.0
    dw, dwm = np.zeros_like(W), np.zeros_like(W)
    one = np.ones(X.shape[:3] + (1,))
    for t, s in _e2e_taps(K, N, fault):
        dx = dx + (_shift(D, -s, 2) + _shift(D, -s, ax2)) @ W[t].T
        dxm = dxm + (np.abs(_shift(D, -s, 2)) + np.abs(_shift(D, -s, ax2))) @ np.abs(W[t].T)
        cnt = cnt + _shift(one, -s, 2) + _shift(one, -s, 1)
        xs, xa = _shift(X, s, 2) + _shift(X, s, ax2), np.abs(_shift(X, s, 2)) + np.abs(_shift(X, s, ax2))
        dw[t] = np.einsum("bijc,bijo->co", xs, D)
        dwm[t] = np.einsum("bijc,bijo->co", xa, np.abs(D))
    two = dt(1.0 if fault == "db1_without_2" else 2.0)
    return {"dx": Link(dx, dxm, O * cnt), "dw1": Link(dw, dwm, 2 * P),
            "db1": Link(two * D.sum((0, 1, 2)), 2 * np.abs(D).sum((0, 1, 2)), P + 1)}


def e2e_setup(case):
    _, B, N, C, K, O, off = case
    rng = _rng(case)
    c = NS(case=case, B=B, N=N, C=C, K=K, O=O)
    c.x, c.dout = A._normal(rng, B, N, N, C), A._normal(rng, B, N, N, O)
    c.w, c.b = A._normal(rng, K, C, O) / np.float32(np.sqrt(2 * K * C)), A._normal(rng, O)
    P = B * N * N
    c.bufs = {"x": vec(P * C, offset=off, data=c.x, name="x"), "w1": vec(K * C * O, offset=off, data=c.w, name="w1"),
              "b1": vec(O, offset=off, data=c.b, name="b1"), "out": vec(P * O, offset=off, name="out"),
              "dout": vec(P * O, offset=off, data=c.dout, name="dout"), "dx": vec(P * C, offset=off, name="dx"),
              "dw1": vec(K * C * O, offset=off, name="dw1"), "db1": vec(O, offset=off, name="db1")}
    return c


def e2e_emulate(c, fault=None):
    after = initial(c)
    f32 = np.float32
    put(c, after, "out", A.emulate_store(ref_e2e_fwd(c.x, c.w, c.b, f32, fault)))
    L = ref_e2e_bwd(c.x, c.w, c.dout, f32, fault)
    for k in ("dx", "dw1", "db1"):
        put(c, after, k, A.emulate_store(L[k]))
    return after


def e2e_verify(c, after):
    V = lambda k, ref: c.bufs[k].values(after[k]).reshape(np.shape(ref))
    Lf, Lb = ref_e2e_fwd(c.x, c.w, c.b), ref_e2e_bwd(c.x, c.w, c.dout)
    res = {"out": assert_link("snd_e2e_fwd out", Lf, V("out", Lf.ref))}
    for k in ("dx", "dw1", "db1"):
        res[k] = assert_link(f"snd_e2e_bwd {k}", Lb[k], V(k, Lb[k].ref))
    check_guards(c, after)
    return res


# ================================================================= relu(BN(y)) between e2e layers
BN_RELU_CASES = (("r1_c1", 1, 1), ("r300_c5", 300, 5), ("r1031_c33", 1031, 33))


def _off_kink_inputs(rng, rows, cc):
    """y, gamma, beta with anything on relu's kink moved well off it (as abi_ops.bn_act_setup)."""
    y = A._normal(rng, rows, cc)
    gamma, beta = 1 + 0.3 * A._normal(rng, cc), 0.3 * A._normal(rng, cc)
    t, w = A.bn_preact(y, gamma, beta, 0)
    return np.where(np.abs(t) <= 4 * w + 1e-30, y + np.float32(0.5), y).astype(np.float32), gamma, beta


def bn_relu_setup(case):
    _, rows, cc = case
    rng = _rng(case)
    c = NS(case=case, rows=rows, c=cc)
    c.y, c.gamma, c.beta = _off_kink_inputs(rng, rows, cc)
    c.dx = A._normal(rng, rows, cc)
    A.assert_off_kink(c.y, c.gamma, c.beta, 1, 0)
    c.bufs = {"y": guarded(rows, cc, data=c.y, name="y"), "gamma": vec(cc, data=c.gamma, name="gamma"),
              "beta": vec(cc, data=c.beta, name="beta"), "x": guarded(rows, cc, name="x"),
              "dx": guarded(rows, cc, data=c.dx, name="dx"), "dy": guarded(rows, cc, name="dy"),
              "dgamma": vec(cc, name="dgamma"), "dbeta": vec(cc, name="dbeta")}
    return c


def bn_relu_emulate(c, fault=None):
    after = initial(c)
    f32 = np.float32
    put(c, after, "x", A.emulate_store(A.ref_bn_act_fwd(c.y, c.gamma, c.beta, 1, 0, f32)))
    L = A.ref_bn_act_bwd(c.dx, c.y, c.gamma, c.beta, 1, 0, f32)
    for k in ("dy", "dgamma", "dbeta"):
        put(c, after, k, A.emulate_store(L[k]))
    return after


def bn_relu_verify(c, after):
    V = lambda k: c.bufs[k].values(after[k])
    A.assert_off_kink(c.y, c.gamma, c.beta, 1, 0)
    res = {"x": assert_link("snd_bn_relu_fwd x", A.ref_bn_act_fwd(c.y, c.gamma, c.beta, 1, 0), V("x"))}
    L = A.ref_bn_act_bwd(c.dx, c.y, c.gamma, c.beta, 1, 0)
    for k in ("dy", "dgamma", "dbeta"):
        res[k] = assert_link(f"snd_bn_relu_bwd {k}", L[k], V(k).reshape(np.shape(L[k].ref)))
    check_guards(c, after)
    return res


# ================================================================= pair stage
PAIR_CASES = (("b2_n7_d3", 2, 7, 3), ("b1_n1_d1", 1, 1, 1), ("b1_n257_d1", 1, 257, 1), ("b3_n5_d4", 3, 5, 4))


def pair_workspace_floats(B, N, D):
    """snd_e2e_pair_bwd_workspace / 4: per-graph gamma and beta partials, the column half of dz."""
    return B * 2 * D * 2 + B * N * D


def pair_concat(z):
    """h[b, i, j] = [z_i | z_j] (model.py:193-195)."""
    B, N, D = z.shape
    return np.concatenate([np.broadcast_to(z[:, :, None, :], (B, N, N, D)), np.broadcast_to(z[:, None, :, :], (B, N, N, D))], -1)


def ref_pair_fwd(z, gamma, beta, dt=np.float64):
    h = pair_concat(A._t(dt)(z))
    return A.ref_bn_act_fwd(h.reshape(-1, h.shape[-1]), gamma, beta, 1, 0, dt)


def ref_pair_bwd(dx0, z, gamma, beta, dt=np.float64, fault=None):
    """{dz, dgamma, dbeta}: dz[b, n] = gamma c (sum_m dT[b, n, m, :D] + sum_m dT[b, m, n, D:]) with
    dT = dx0 where the pre-activation is positive: N-term sums, two products, one add."""
    T, cc = A._t(dt), dt(BN_C)
    Z, g, be = T(z), T(gamma), T(beta)
    B, N, D = Z.shape
    h = pair_concat(Z)
    dT = T(dx0).reshape(B, N, N, 2 * D) * (g * cc * h + be > 0)
    aT = np.abs(dT)
    gr, gk = g[:D] * cc, g[D:] * cc
    row, col = dT[..., :D].sum(2) * gr, (0 if fault == "no_column_half" else 1) * dT[..., D:].sum(1) * gk
    mag = aT[..., :D].sum(2) * np.abs(gr) + aT[..., D:].sum(1) * np.abs(gk)
    sel = slice(0, 1) if fault == "dgamma_graph_0" else slice(None)
    return {"dz": Link(row + col, mag, N + 2),
            "dgamma": Link((dT * cc * h)[sel].sum((0, 1, 2)), (aT * cc * np.abs(h)).sum((0, 1, 2)), B * N * N + 2),
            "dbeta": Link(dT.sum((0, 1, 2)), aT.sum((0, 1, 2)), B * N * N)}


def pair_setup(case):
    _, B, N, D = case
    rng = _rng(case)
    c = NS(case=case, B=B, N=N, D=D)
    c.z = A._normal(rng, B, N, D)
    c.gamma, c.beta = 1 + 0.3 * A._normal(rng, 2 * D), 0.3 * A._normal(rng, 2 * D)
    for _ in range(8):                                            # z[b, n, d] feeds channels d and D + d:
        t, w = A.bn_preact(pair_concat(c.z).reshape(-1, 2 * D), c.gamma, c.beta, 0)
        bad = (np.abs(t) <= 4 * w + 1e-30).reshape(B, N, N, 2 * D)
        if not bad.any():                                         # move it until both are off relu's kink
            break
        c.z = (c.z + np.float32(0.5) * (bad[..., :D].any(2) | bad[..., D:].any(1))).astype(np.float32)
    c.dx0 = A._normal(rng, B * N * N, 2 * D)
    A.assert_off_kink(pair_concat(c.z).reshape(-1, 2 * D), c.gamma, c.beta, 1, 0)
    c.bufs = {"z": guarded(B * N, D, data=c.z, name="z"), "gamma": vec(2 * D, data=c.gamma, name="gamma"),
              "beta": vec(2 * D, data=c.beta, name="beta"), "x0": guarded(B * N * N, 2 * D, name="x0"),
              "dx0": guarded(B * N * N, 2 * D, data=c.dx0, name="dx0"), "dz": guarded(B * N, D, name="dz"),
              "dgamma": vec(2 * D, name="dgamma"), "dbeta": vec(2 * D, name="dbeta"),
              "ws": vec(pair_workspace_floats(B, N, D), name="ws")}
    return c


def pair_emulate(c, fault=None):
    after = initial(c)
    f32 = np.float32
    put(c, after, "x0", A.emulate_store(ref_pair_fwd(c.z, c.gamma, c.beta, f32)))
    L = ref_pair_bwd(c.dx0, c.z, c.gamma, c.beta, f32, fault)
    for k in ("dz", "dgamma", "dbeta"):
        put(c, after, k, A.emulate_store(L[k]))
    _scratch(c, after, "ws")
    return after


def pair_verify(c, after):
    V = lambda k: c.bufs[k].values(after[k])
    A.assert_off_kink(pair_concat(c.z).reshape(-1, 2 * c.D), c.gamma, c.beta, 1, 0)
    res = {"x0": assert_link("snd_e2e_pair_fwd x0", ref_pair_fwd(c.z, c.gamma, c.beta), V("x0"))}
    L = ref_pair_bwd(c.dx0, c.z, c.gamma, c.beta)
    for k in ("dz", "dgamma", "dbeta"):
        res[k] = assert_link(f"snd_e2e_pair_bwd {k}", L[k], V(k).reshape(np.shape(L[k].ref)))
    assert np.isfinite(V("ws")).all(), "snd_e2e_pair_bwd: every workspace float is written"
    check_guards(c, after)
    return res


# ================================================================= head + CE
# (id, B, N, c, A_ii = 1 on some diagonal entries)
HEAD_CE_CASES = (("b1_n3_c1", 1, 3, 1, False), ("b2_n7_c32", 2, 7, 32, False), ("b3_n11_c20", 3, 11, 20, False),
                 ("b1_n17_c5_diag", 1, 17, 5, True))


def ref_head_ce(y, adj, gamma, beta, w, b, dt=np.float64, fault=None):
    """Links {ce, dy, dw, db, dgamma, dbeta}, the exact count, and the logits with their bounds
    (the module text: the logits' bound carried through the softmax)."""
    T, f64, ab = A._t(dt), np.float64, np.abs
    B, N = adj.shape[:2]
    C = y.shape[-1]
    rows = B * N * N
    Y, Ad, g, be, W, bl = T(y).reshape(rows, C), T(adj).reshape(rows), T(gamma), T(beta), T(w), T(b)
    if fault == "drop_channel_31" and C == 32:
        W = W.copy()
        W[31] = 0
    gc = g * dt(BN_C)
    t = gc * Y + be
    e_t = _base(2, ab(gc * Y) + ab(be))
    x = np.maximum(t, 0)
    l = x @ W + bl                                              # [rows, 2]
    e_l = e_t @ ab(W).astype(f64) + _base(C + 1, ab(x) @ ab(W) + ab(bl))
    diag = (np.arange(rows) // N % N) == (np.arange(rows) % N)
    if fault == "diagonal_kept":                                # i == j treated like any other pair
        diag = np.zeros(rows, bool)
    l = np.where(diag[:, None], T([1.0, 0.0]), l)
    e_l = np.where(diag[:, None], 0.0, e_l)
    mx = l.max(1)
    lg = np.log(np.exp(l[:, 0] - mx) + np.exp(l[:, 1] - mx))
    lse = mx + lg
    e_lse = e_l.max(1) + 4 * TRANS + _base(1, ab(mx) + ab(lg))
    ce = lse - (1 - Ad) * l[:, 0] - Ad * l[:, 1]
    e_ce = e_lse + (1 - Ad) * e_l[:, 0] + Ad * e_l[:, 1] + _base(3, ab(lse) + (1 - Ad) * ab(l[:, 0]) + Ad * ab(l[:, 1]))
    correct = float(((l[:, 1] > l[:, 0]).astype(dt) == Ad).sum())
    p = np.exp(l - lse[:, None])
    e_a = e_l + e_lse[:, None] + _base(0, ab(l) + ab(lse)[:, None])
    e_p = p.astype(f64) * (np.expm1(e_a) + 2 * TRANS)
    lab = np.stack([1 - Ad, Ad], 1)
    invM = dt(1.0) if fault == "sum_not_mean" else dt(1.0) / dt(rows)
    d = np.where(diag[:, None], dt(0), (p - lab) * invM)
    e_d = np.where(diag[:, None], 0.0, float(invM) * (e_p + _base(2, p + lab)))
    dxv = d @ W.T
    e_dx = e_d @ ab(W.T).astype(f64)
    on = t > 0
    dT = np.where(on, dxv, dt(0))
    e_dT = np.where(on, e_dx + _base(2, ab(d) @ ab(W.T)), 0.0)
    ce_sum, e_sum = ce.sum(dtype=f64), e_ce.sum()
    out = {"ce": Link(np.array(ce_sum), np.zeros(()), 0, extra=float(e_sum)),
           "dy": Link(dT * gc, np.zeros_like(dT), 0, extra=e_dT * ab(gc) + _base(1, ab(dT * gc))),
           "dw": Link(x.T @ d, ab(x.T) @ ab(d), rows, extra=e_t.T @ ab(d).astype(f64) + ab(x.T).astype(f64) @ e_d),
           "db": Link(d.sum(0), ab(d).sum(0), rows, extra=e_d.sum(0)),
           "dgamma": Link((dT * dt(BN_C) * Y).sum(0), ab(dT * dt(BN_C) * Y).sum(0), rows + 2,
                          extra=(e_dT * ab(dt(BN_C) * Y)).sum(0)),
           "dbeta": Link(dT.sum(0), ab(dT).sum(0), rows, extra=e_dT.sum(0))}
    return NS(links=out, correct=correct, l=l, e_l=e_l, diag=diag, t=t)


def head_ce_setup(case):
    _, B, N, C, diag1 = case
    rng = _rng(case)
    c = NS(case=case, B=B, N=N, C=C)
    y, c.gamma, c.beta = _off_kink_inputs(rng, B * N * N, C)
    c.y = y.reshape(B, N, N, C)
    c.w, c.b = A._normal(rng, C, 2) / np.float32(np.sqrt(C)), A._normal(rng, 2)
    up = np.triu(rng.random((B, N, N)) < 0.4, 1)
    c.adj = (up | up.transpose(0, 2, 1)).astype(np.float32)
    if diag1:
        c.adj[:, np.arange(0, N, 3), np.arange(0, N, 3)] = 1.0    # a target the overridden diagonal misses
    A.assert_off_kink(y, c.gamma, c.beta, 1, 0)
    r = ref_head_ce(c.y, c.adj, c.gamma, c.beta, c.w, c.b)
    off = ~r.diag
    margin = np.abs(r.l[:, 1] - r.l[:, 0])[off]
    assert (margin > r.e_l.sum(1)[off]).all(), f"head {case[0]}: an off-diagonal argmax is not decidable"
    c.bufs = {"y": guarded(B * N * N, C, data=c.y, name="y"), "adj": vec(B * N * N, data=c.adj, name="adj"),
              "gamma": vec(C, data=c.gamma, name="gamma"), "beta": vec(C, data=c.beta, name="beta"),
              "w": guarded(C, 2, data=c.w, name="w"), "b": vec(2, data=c.b, name="b"),
              "dy": guarded(B * N * N, C, name="dy"), "dw": guarded(C, 2, name="dw"), "db": vec(2, name="db"),
              "dgamma": vec(C, name="dgamma"), "dbeta": vec(C, name="dbeta"), "out": vec(2, "f64", name="out")}
    return c


def head_ce_emulate(c, fault=None):
    after = initial(c)
    r = ref_head_ce(c.y, c.adj, c.gamma, c.beta, c.w, c.b, np.float32, fault)
    for k in ("dy", "dw", "db", "dgamma", "dbeta"):
        put(c, after, k, A.emulate_store(r.links[k]))
    put(c, after, "out", np.array([float(r.links["ce"].ref), r.correct]))
    return after


def head_ce_verify(c, after):
    V = lambda k: c.bufs[k].values(after[k])
    r = ref_head_ce(c.y, c.adj, c.gamma, c.beta, c.w, c.b)
    res = {k: assert_link(f"snd_e2e_head_ce {k}", r.links[k], V(k).reshape(np.shape(r.links[k].ref)))
           for k in ("dy", "dw", "db", "dgamma", "dbeta")}
    out = V("out")[0]
    res["ce"] = assert_link("snd_e2e_head_ce out[0] (CE sum)", r.links["ce"], np.array(out[0]))
    assert out[1] == r.correct, f"snd_e2e_head_ce out[1]: element (1,) got {out[1]!r} ref {r.correct!r} (the count is exact)"
    check_guards(c, after)
    return res


# ================================================================= latent regularisers
LATENT_SHAPES = ((1, 1), (3, 5), (10, 16), (50, 100))
# (id, weights, z, workspace)
LATENT_WEIGHTS = (
    ("kl", dict(w_kl=0.7), True, True),
    ("cap_on", dict(cap_gamma=2.0, cap_c=0.01), True, True),
    ("cap_off", dict(cap_gamma=2.0, cap_c=50.0), True, True),
    ("dip", dict(w_kl=1.0, w_dip=0.5, lambda_od=10.0, lambda_d=100.0), True, True),
    ("tc", dict(w_kl=0.5, w_tc=10.0), True, True),
    ("dip_tc", dict(w_kl=1.0, w_dip=0.5, lambda_od=10.0, lambda_d=100.0, w_tc=10.0), True, True),
    ("cap_dip_tc", dict(cap_gamma=2.0, cap_c=0.01, w_dip=0.5, lambda_od=10.0, lambda_d=100.0, w_tc=10.0), True, True),
)
LATENT_CASES = tuple((f"b{B}_l{L}_{n}", B, L, kw, z, ws) for B, L in LATENT_SHAPES for n, kw, z, ws in LATENT_WEIGHTS) + (
    ("b3_l5_kl_no_z_no_ws", 3, 5, dict(w_kl=0.7), False, False),            # both legal without DIP and TC
    ("b3_l5_dip_no_z", 3, 5, dict(w_kl=1.0, w_dip=0.5, lambda_od=10.0, lambda_d=100.0), False, True),
)
LATENT_FIELDS = ("w_kl", "cap_gamma", "cap_c", "w_dip", "lambda_od", "lambda_d", "w_tc")


def latent_workspace_floats(B, L):
    """snd_latent_reg_workspace / 4: max(DIP's L L + L, TC's B B + B B L + 2 B L + B)."""
    return max(L * L + L, B * B + B * B * L + 2 * B * L + B)


def _lse(a, axis):
    mx = a.max(axis=axis, keepdims=True)
    return (mx + np.log(np.exp(a - mx).sum(axis=axis, keepdims=True, dtype=a.dtype))).squeeze(axis)


def ref_latent(mu, s, z, kw, dt=np.float64, fault=None):
    """NS(kl, kterm, dip, tc, term, dmu_kl, ds_kl, dmu, ds): the term of the header and its
    gradient, the path through z = mu + eps e^s (d mu += dz, d s += dz (z - mu)) included."""
    T, f64 = A._t(dt), np.float64
    w = {k: np.float32(kw.get(k, 0.0)) for k in LATENT_FIELDS}
    M, S = T(mu), T(s)
    B, L = M.shape
    n = B * L
    r = NS()
    M64, S64 = M.astype(f64), S.astype(f64)
    r.kl = float(-0.5 * (1.0 + 2.0 * S64 - M64 * M64 - np.exp(2.0 * S64)).sum() / n)      # the kernel sums in double
    cap = w["cap_gamma"] > 0
    r.gate_margin = abs(r.kl - float(w["cap_c"])) if cap else np.inf
    wk = dt((w["cap_gamma"] if r.kl > float(w["cap_c"]) else 0.0) if cap else w["w_kl"])
    r.kterm = float(w["cap_gamma"]) * max(r.kl - float(w["cap_c"]), 0.0) if cap else float(w["w_kl"]) * r.kl
    r.wk = abs(float(wk))
    inv = dt(1.0) / dt(n)
    e2 = np.exp(2 * S)
    r.dmu_kl = Link(wk * M * inv, np.abs(wk * M * inv), 0)
    r.ds_kl = Link(wk * (e2 - 1) * inv, np.abs(wk * inv) * (e2 + 1), 2, extra=TRANS * np.abs(wk * inv * e2).astype(f64))
    ab = lambda a: np.abs(a).astype(f64)
    dmu, ds = r.dmu_kl.ref.copy(), r.ds_kl.ref.copy()
    e_dmu, e_ds = r.dmu_kl.bound().copy(), r.ds_kl.bound().copy()
    r.dip = r.tc = r.e_dip = r.e_tc = 0.0
    wd, wt, lod, ld = dt(w["w_dip"]), dt(w["w_tc"]), dt(w["lambda_od"]), dt(w["lambda_d"])
    if w["w_dip"] != 0:
        # mean = sum_b mu / B; cov = sum_b mu_k mu_l / B - mean_k mean_l; G = d DIP / d cov (fp32);
        # DIP itself from cov in double; d mu_b = w_dip (2 / B) G (mu_b - mean)
        mean = M.sum(0, dtype=dt) / dt(B)
        e_mean = _base(B + 1, ab(M).sum(0) / B)
        cov = M.T @ M / dt(B) - np.outer(mean, mean)
        am = ab(mean)
        e_cov = _base(B + 2, ab(M).T @ ab(M) / B + np.outer(am, am)) + np.outer(am, e_mean) + np.outer(e_mean, am)
        eye = np.eye(L)
        lam = np.where(eye > 0, float(ld), float(lod))
        dev = cov.astype(f64) - eye
        r.dip = float((lam * dev * dev).sum())
        r.e_dip = float((lam * (2 * np.abs(dev) * e_cov + e_cov * e_cov)).sum())
        Gm = (2 * T(lam) * (cov - T(eye))).astype(dt)
        e_G = 2 * lam * e_cov + _base(1, 2 * lam * (ab(cov) + eye))
        if fault == "ws_reused_before_dip_grad" and w["w_tc"] != 0:    # TC's S / Q land on cov / mean early
            Gm = np.full_like(Gm, -0.5 * LOG_2PI)
        diff = M - mean
        e_diff = e_mean + _base(0, ab(M) + am)
        part = wd * 2 * (diff @ Gm) / dt(B)
        e_t = ab(diff) @ e_G + e_diff @ ab(Gm) + _base(L, ab(diff) @ ab(Gm))
        e_part = abs(float(wd)) * 2 / B * e_t + _base(2, ab(part))
        e_dmu = e_dmu + e_part + _base(0, ab(dmu) + ab(part))
        dmu = dmu + part
    if w["w_tc"] != 0:
        # Q[j, i, l] = -0.5 ((z_j - mu_i)^2 e^{-2 s_i} + 2 s_i + log 2 pi); S = sum_l Q; SL = LSE_i S;
        # PL = LSE_i Q; TC = (sum SL - sum PL) / B in double; W = (e^{S - SL} - e^{Q - PL}) / B
        Z = T(z)
        iv = np.exp(-2 * S)[None]
        e_iv = TRANS * ab(iv) + _base(0, ab(iv))
        tmp = Z[:, None, :] - M[None, :, :]                         # [j, i, l]
        e_tmp = U23 * (ab(Z)[:, None, :] + ab(M)[None, :, :])
        a2 = tmp * tmp * iv
        e_a2 = 2 * ab(tmp) * e_tmp * ab(iv) + ab(tmp * tmp) * e_iv + _base(0, ab(a2))
        Q = dt(-0.5) * (a2 + 2 * S[None] + dt(LOG_2PI))
        e_Q = 0.5 * e_a2 + _base(2, 0.5 * (ab(a2) + 2 * ab(S)[None] + LOG_2PI))
        Sm = Q.sum(2, dtype=dt)
        e_S = e_Q.sum(2) + _base(L, ab(Q).sum(2))

        def lse_bound(v, e_v, out):
            # out = max + log(sum e^{v - max}): the shifts' bounds average to at most max e_v; the sum of B
            # positive exps is good to 1e-6 + (B + 4) 2^-23 relative, so its log to that much absolutely; the
            # log itself 1e-6 relative; one add
            lg = out - v.max(1)
            return e_v.max(1) + TRANS + (B + 4) * U23 + TRANS * ab(lg) + _base(1, ab(v.max(1)) + ab(lg))
        SL, PL = _lse(Sm, 1), _lse(Q, 1)
        e_SL, e_PL = lse_bound(Sm, e_S, SL), lse_bound(Q, e_Q, PL)
        r.tc = float((SL.astype(f64).sum() - PL.astype(f64).sum()) / B)
        r.e_tc = float((e_SL.sum() + e_PL.sum()) / B)
        p1, p2 = np.exp(Sm - SL[:, None]), np.exp(Q - PL[:, None, :])
        e_p1 = ab(p1) * (np.expm1(e_S + e_SL[:, None] + U23 * (ab(Sm) + ab(SL)[:, None])) + TRANS)
        e_p2 = ab(p2) * (np.expm1(e_Q + e_PL[:, None, :] + U23 * (ab(Q) + ab(PL)[:, None, :])) + TRANS)
        Wt = (p1[:, :, None] - p2) / dt(B)
        e_W = (e_p1[:, :, None] + e_p2) / B + _base(1, (ab(p1)[:, :, None] + ab(p2)) / B)
        tm = Wt * tmp * iv                                          # d z_j = -sum_i, d mu_i = sum_j
        e_tm = e_W * ab(tmp * iv) + ab(Wt) * (e_tmp * ab(iv) + ab(tmp) * e_iv) + _base(0, ab(tm))
        dz, dm = -tm.sum(1, dtype=dt), tm.sum(0, dtype=dt)
        e_dz, e_dm = e_tm.sum(1) + _base(B, ab(tm).sum(1)), e_tm.sum(0) + _base(B, ab(tm).sum(0))
        ts = Wt * (a2 - 1)
        e_ts = e_W * ab(a2 - 1) + ab(Wt) * (e_a2 + _base(0, ab(a2) + 1))
        dsv = ts.sum(0, dtype=dt)
        e_dsv = e_ts.sum(0) + _base(B, (ab(Wt) * (ab(a2) + 1)).sum(0))
        zm = Z - M
        thru = (0 if fault == "no_ds_through_z" else 1) * dz * zm
        pm, ps = wt * (dm + dz), wt * (dsv + thru)
        awt = abs(float(wt))
        e_pm = awt * (e_dm + e_dz) + _base(2, awt * (ab(dm) + ab(dz)))
        e_ps = awt * (e_dsv + e_dz * ab(zm) + ab(dz) * U23 * (ab(Z) + ab(M))) + _base(3, awt * (ab(dsv) + ab(thru)))
        e_dmu, e_ds = e_dmu + e_pm + _base(0, ab(dmu) + ab(pm)), e_ds + e_ps + _base(0, ab(ds) + ab(ps))
        dmu, ds = dmu + pm, ds + ps
    r.term = r.kterm + float(w["w_dip"]) * r.dip + float(w["w_tc"]) * r.tc
    r.e_chain = abs(float(w["w_dip"])) * r.e_dip + abs(float(w["w_tc"])) * r.e_tc
    r.dmu, r.ds = Link(dmu, np.zeros_like(dmu), 0, extra=e_dmu), Link(ds, np.zeros_like(ds), 0, extra=e_ds)
    return r


def latent_setup(case):
    name, B, L, kw, has_z, has_ws = case
    rng = np.random.default_rng([B, L, len(name)])
    c = NS(case=case, B=B, L=L, kw=kw, chain=bool(kw.get("w_dip") or kw.get("w_tc")))
    c.mu, c.s = 0.8 * A._normal(rng, B, L), 0.3 * A._normal(rng, B, L)
    c.z = (c.mu + A._normal(rng, B, L) * np.exp(c.s)).astype(np.float32)
    r = ref_latent(c.mu, c.s, c.z, kw)
    assert r.gate_margin > 1e-3, f"latent {name}: kl {r.kl} on the capacity gate"
    c.bufs = {"mu": guarded(B, L, data=c.mu, name="mu"), "logstd": guarded(B, L, data=c.s, name="logstd"),
              "dmu": guarded(B, L, name="dmu"), "dlogstd": guarded(B, L, name="dlogstd"), "out": vec(4, "f64", name="out")}
    if has_z:
        c.bufs["z"] = guarded(B, L, data=c.z, name="z")
    if has_ws:
        c.bufs["ws"] = vec(latent_workspace_floats(B, L), name="ws")
    return c


def latent_emulate(c, fault=None):
    after = initial(c)
    r = ref_latent(c.mu, c.s, c.z, c.kw, np.float32, fault)
    put(c, after, "dmu", r.dmu.ref)
    put(c, after, "dlogstd", r.ds.ref)
    put(c, after, "out", np.array([r.kl, r.term, r.dip, r.tc]))
    if "ws" in c.bufs and c.chain:
        _scratch(c, after, "ws")
    return after


def latent_verify(c, after):
    V = lambda k: c.bufs[k].values(after[k])
    r = ref_latent(c.mu, c.s, c.z, c.kw)
    out = V("out")[0]
    s64, m64 = c.s.astype(np.float64), c.mu.astype(np.float64)
    klmag = 0.5 * float((1 + 2 * np.abs(s64) + m64 ** 2 + np.exp(2.0 * s64)).sum()) / (c.B * c.L)
    scalar = lambda ref, mag, extra=0.0: Link(np.array(float(ref)), np.array(float(mag)), 0, extra=float(extra))
    res = {"kl": assert_link("snd_latent_reg out[0] (kl)", scalar(r.kl, klmag), np.array(out[0])),
           "term": assert_link("snd_latent_reg out[1] (term)", scalar(r.term, r.wk * klmag + abs(r.term), r.e_chain),
                               np.array(out[1])),
           "dip": assert_link("snd_latent_reg out[2] (DIP)", scalar(r.dip, abs(r.dip), r.e_dip), np.array(out[2])),
           "tc": assert_link("snd_latent_reg out[3] (TC)", scalar(r.tc, abs(r.tc), r.e_tc), np.array(out[3])),
           "dmu": assert_link("snd_latent_reg dmu", r.dmu, V("dmu")),
           "dlogstd": assert_link("snd_latent_reg dlogstd", r.ds, V("dlogstd"))}
    check_guards(c, after)
    return res
