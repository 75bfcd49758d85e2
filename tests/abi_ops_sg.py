"""Guarded operands, float64 references and float32 emulations for the spatial-graph entry
points of include/snd_vae.h: snd_sg_prep, snd_sg_workspace, snd_sg_layer_fwd and
snd_sg_layer_bwd, on the harness of tests/abi_ops.py (same contract: ``sg_setup(case,
bn_act)``, ``sg_emulate(c, fault=None)``, ``sg_verify(c, after)``).

The three calls share one case: the backward needs the forward's workspace, and both need
the edge scalars of snd_sg_prep.  Every operand, output and the workspace (exactly
snd_sg_workspace bytes, mirrored here by ``sg_geo``) sits in a guarded buffer; outputs,
gradients and the workspace start at the NaN pattern.

Reference: the layer in the factorised form the header documents (``sg_chain``), float64.
tests/test_abi_ops_sg_cpu.py pins it to oracle/ref_sg.py's dense B x N x N x N restatement
(sgconv_grads, and sg_encoder's BN + lrelu) to 1e-12 on every committed case.

Bars.
* prep: edge_rev, node_deg and n_unmatched exact; edge_lr one fp32 multiply; node_e and
  edge_q fp32 sums of deg terms on top of edge_lr's bound.
* y (layer_fwd): the base rule (K + 4) 2^-23 mag of own_operands propagated stage by stage
  over the literal formula (``sg_fwd_bounds``): lrelu(x), A lrelu(x), u / v / w, S3 per edge,
  P, m2, y.  A step is |e_in| |W| + (K + 4) 2^-23 (|in| |W| + |b|).
* out: lrelu(BN(y)) on the STORED y, K = 2.
* grads gamma / beta: fp32 sums of R terms formed from dout and the STORED y.
* dx and the gradients of Matrix1..3 / bias1..3: the same propagation through the backward
  (``sg_bwd_bounds``), element by element.  A sum over R = 8225 rows has a worst-case bound
  near 1e-3 of sum |terms|, far above what a fixed-order fp32 sum really loses, so these
  outputs ALSO keep the bar they have in tests/test_gpu_sg.py, 1e-5 of the block's max-abs
  (without that test's floor of 1: never looser); both must hold ("<output>@1e-5" in the
  ratios).  Neither number comes from a GPU or from the emulation.

Kinks (asserted in setup, no exclusions): every S3_ij per channel and every summed m2 of a
node with edges lies outside its own propagated forward bound of 0, and with bn_act the BN
pre-activation lies outside y's bound times |gamma c| plus its own two roundings.  Rows of
degree 0 have m2 = 0 exactly and everything downstream of them is multiplied by the degree.
"""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np

import abi_ops as A
from abi_ops import G, assert_link, check_guards, guarded, initial, put, vec
from own_operands import BN_C, KINK, U23, Link, lrelu, lrelu_grad

# (id, N, B, F, hidden, graphs, ldx - f, lddx - f, pointer offset, want dx, seed)
SG_CASES = (
    ("r4105", 5, 821, 2, (7, 5, 3), "random", 0, 0, 0, True, 4105),     # 2 split-K parts
    ("r8225", 5, 1645, 2, (7, 5, 3), "random", 0, 0, 0, True, 8225),    # 3 parts
    ("strided", 6, 10, 2, (7, 5, 3), "random", 3, 5, 1, True, 60),
    ("no_dx", 4, 3, 2, (7, 5, 3), "random", 0, 0, 0, False, 12),
    ("no_edges", 3, 1, 2, (7, 5, 3), "empty", 0, 0, 0, True, 3),
    ("h0_65", 5, 4, 2, (65, 7, 66), "random", 0, 0, 0, True, 65),       # 2nd N tile, K tails
)
SG_BLOCKS = ("M1", "b1", "M2", "b2", "M3", "b3", "gamma", "beta")
INHERITED = 1e-5                        # tests/test_gpu_sg.py: of the block's max-abs


def sg_case(name):
    return next(k for k in SG_CASES if k[0] == name)


def sg_shapes(F, hidden):
    h0, h1, h2 = hidden
    return (("M1", (3 * F + 3, h0)), ("b1", (h0,)), ("M2", (2 * F + 1 + h0, h1)), ("b2", (h1,)),
            ("M3", (F + h1, h2)), ("b3", (h2,)), ("gamma", (h2,)), ("beta", (h2,)))


def sg_unpack(flat, F, hidden):
    out, o = {}, 0
    for name, shp in sg_shapes(F, hidden):
        n = int(np.prod(shp))
        out[name] = flat[o:o + n].reshape(shp)
        o += n
    assert o == flat.size
    return out


def sg_pack(blocks, F, hidden, dt=np.float64):
    return np.concatenate([np.asarray(blocks[k], dt).reshape(-1) for k, _ in sg_shapes(F, hidden)])


def sg_geo(R, F, hidden):
    """snd_sg.hip geo(): workspace floats, split count, rows per split part, parts."""
    h0, h1, h2 = hidden
    r64 = lambda n: (n + 63) // 64 * 64
    ld2, ld3 = 2 * F + 2 + h0, F + h1 + 1
    sizes = (R * ld2, R * 3 * h0, R * h1, R * ld3, R * h2, R * 2 * h2, R * (F + h1), R * h1,
             R * (2 * F + 1 + h0), R * 3 * h0, R * 4 * h0, R * F, R * F)
    splits = max(1, min(64, -(-R // 4096)))
    mn = max(ld3 * h2, ld2 * h1, F * h0, 2 * h2, 4 * h0)
    kchunk = r64(-(-R // splits))
    return NS(floats=sum(r64(s) for s in sizes) + r64(splits * mn), splits=splits, kchunk=kchunk,
              parts=-(-R // kchunk), ld2=ld2, ld3=ld3)


def sg_graphs(kind, N, B, rng):
    """Random symmetric graphs, edge probability 0.45: isolated nodes and empty graphs included."""
    if kind == "empty":
        return np.zeros((B, N, N), bool)
    up = np.triu(rng.random((B, N, N)) < 0.45, 1)
    return up | up.transpose(0, 2, 1)


def _sp(data, ci, rp, shape, dt):
    import scipy.sparse as sp
    return sp.csr_matrix((np.asarray(data, dt), np.asarray(ci, np.int64), np.asarray(rp, np.int64)), shape=shape)


def _graph_ops(c, dt):
    """(A as a sparse [R, R] matrix, seg: per-edge values [nnz, ...] summed over each row's edges)."""
    R, nnz = c.R, c.nnz
    Asp = _sp(np.ones(nnz), c.ci, c.rp, (R, R), dt)
    Es = _sp(np.ones(nnz), np.arange(nnz), c.rp, (R, max(nnz, 1)), dt)
    return Asp, lambda v: np.asarray(Es[:, :nnz] @ v, dt) if nnz else np.zeros((R,) + v.shape[1:], dt)


# ================================================================= the layer, factorised
def sg_chain(c, x, prm, dt=np.float64, bn_act=0, dout=None, y_for_bn=None, fault=None, wg=None):
    """Forward (and with ``dout`` backward) of one layer in the header's factorised form, at
    dtype dt.  ``wg(Aop, D)``: the weight-gradient product Aop^T D (the emulation splits it);
    ``y_for_bn``: the y the BN backward reads (the stored one; default this forward's)."""
    T = A._t(dt)
    F, (h0, h1, h2), R, n = c.F, c.hidden, c.R, c.N
    p = sg_unpack(T(prm), F, c.hidden)
    M1 = p["M1"]
    M1x, M1y, M1z, m1r, m1s, m1t = M1[:F], M1[F:2 * F], M1[2 * F:3 * F], M1[3 * F], M1[3 * F + 1], M1[3 * F + 2]
    src, dst, nnz = c.src, c.ci, c.nnz
    Asp, seg = _graph_ops(c, dt)
    wg = wg or (lambda a, d: a.T @ d)
    r = NS()
    # ---- snd_sg_prep
    lrel = lrelu(T(c.rel).reshape(R, n))
    r.lrel, r.lr = lrel, lrel[src, dst - src // n * n]
    r.deg = T(np.maximum(c.deg, 1) if fault == "deg0_as_1" else c.deg)
    r.e = seg(r.lr)
    r.Q = (lrel[src] * T(c.aloc)[dst]).sum(1, dtype=dt)
    d = r.deg[:, None]
    # ---- forward
    X = T(x)
    r.LX = lrelu(X)
    r.AX = np.asarray(Asp @ r.LX, dt)
    r.u, r.v, r.w = r.LX @ M1x, r.LX @ M1y, r.AX @ M1z
    r.S3 = (d[dst] * (r.u[src] + r.v[dst] + r.lr[:, None] * m1r + p["b1"]) + r.w[dst] + r.e[dst][:, None] * m1s
            + r.Q[:, None] * m1t)
    r.P = seg(lrelu(r.S3))
    r.Z2e = np.concatenate([d * r.LX, r.AX, r.e[:, None], r.P, d], 1)
    r.M2e = np.concatenate([p["M2"], p["b2"][None]], 0)
    r.m2 = r.Z2e @ r.M2e
    r.Z3e = np.concatenate([r.LX, lrelu(r.m2), np.ones((R, 1), dt)], 1)
    r.M3e = np.concatenate([p["M3"], p["b3"][None]], 0)
    r.y = r.Z3e @ r.M3e
    gc = p["gamma"] * dt(BN_C)
    r.out = lrelu(r.y * gc + p["beta"])
    if dout is None:
        return r
    # ---- backward
    g, D = {}, T(dout)
    if bn_act:
        yb = r.y if y_for_bn is None else T(y_for_bn)
        dT = D * lrelu_grad(yb * gc + p["beta"])
        dy = dT * gc
        ones = np.ones((R, 1), dt)
        g["beta"], g["gamma"] = wg(ones, dT)[0], wg(ones, dT * yb * dt(BN_C))[0]
        r.dT, r.yb = dT, yb
    else:
        dy = D
        g["beta"] = g["gamma"] = None
    gm3 = wg(r.Z3e, dy)
    g["M3"], g["b3"] = gm3[:-1], gm3[-1]
    dZ3 = dy @ p["M3"].T
    dm2 = dZ3[:, F:] * lrelu_grad(r.m2)
    gm2 = wg(r.Z2e, dm2)
    g["M2"], g["b2"] = gm2[:-1], gm2[-1]
    dZ2 = dm2 @ p["M2"].T
    dP = dZ2[:, 2 * F + 1:]
    Gq = dP[src] * lrelu_grad(r.S3)
    if fault == "dw_own_q":             # the reverse edge's S3 formed with edge q's own Q_ij
        s3r = r.S3[c.rev] + (r.Q - r.Q[c.rev])[:, None] * m1t
        Gr = dP[dst] * lrelu_grad(s3r)
    else:
        Gr = Gq[c.rev] if nnz else Gq
    dn, en = r.deg[dst][:, None], r.e[dst][:, None]
    du, dw = seg(Gq * dn), seg(Gr)
    dv = d * dw
    TM = np.concatenate([seg(Gq * dn * r.lr[:, None]), du, seg(Gq * en), seg(Gq * r.Q[:, None])], 1)
    cs = wg(np.ones((R, 1), dt), TM)[0]
    g["M1"] = np.concatenate([wg(r.LX, du), wg(r.LX, dv), wg(r.AX, dw), cs[None, :h0], cs[None, 2 * h0:3 * h0],
                              cs[None, 3 * h0:]], 0)
    g["b1"] = cs[h0:2 * h0]
    dlx = dZ3[:, :F] + d * dZ2[:, :F] + du @ M1x.T + dv @ M1y.T
    dax = dZ2[:, F:2 * F] + dw @ M1z.T
    r.dx = lrelu_grad(X) * (dlx + np.asarray(Asp @ dax, dt))
    r.grads = g
    r.dy, r.dZ3, r.dm2, r.dZ2, r.Gq, r.Gr = dy, dZ3, dm2, dZ2, Gq, Gr
    r.du, r.dw, r.dv, r.TM, r.dlx, r.dax = du, dw, dv, TM, dlx, dax
    return r


def _base(K, mag):
    return (np.asarray(K, np.float64) + 4.0) * U23 * mag


def sg_fwd_bounds(c, r, prm):
    """|fp32 result - float64 reference| of every forward stage, own_operands' base rule
    propagated: {lr, e, Q, S3, m2, y} (arrays shaped like the values)."""
    ab = np.abs
    F, (h0, h1, h2), R, nnz = c.F, c.hidden, c.R, c.nnz
    p = {k: ab(v) for k, v in sg_unpack(np.asarray(prm, np.float64), F, c.hidden).items()}
    M1 = p["M1"]
    M1x, M1y, M1z, m1r, m1s, m1t = M1[:F], M1[F:2 * F], M1[2 * F:3 * F], M1[3 * F], M1[3 * F + 1], M1[3 * F + 2]
    src, dst, n = c.src, c.ci, c.N
    Asp, seg = _graph_ops(c, np.float64)
    deg = c.deg.astype(np.float64)
    d = deg[:, None]
    b = NS()
    e_lrel = _base(0, ab(r.lrel))                                   # one multiply by 0.2
    b.lr = e_lrel[src, dst - src // n * n]
    b.e = seg(b.lr) + _base(deg, seg(ab(r.lr)))
    b.Q = (e_lrel[src] * c.aloc[dst]).sum(1) + _base(deg[dst], (ab(r.lrel)[src] * c.aloc[dst]).sum(1))
    e_LX = _base(0, ab(r.LX))
    e_AX = np.asarray(Asp @ e_LX) + _base(d, np.asarray(Asp @ ab(r.LX)))
    e_u, e_v = e_LX @ M1x + _base(F, ab(r.LX) @ M1x), e_LX @ M1y + _base(F, ab(r.LX) @ M1y)
    e_w = e_AX @ M1z + _base(F, ab(r.AX) @ M1z)
    mag = (d[dst] * (ab(r.u)[src] + ab(r.v)[dst] + ab(r.lr)[:, None] * m1r + p["b1"]) + ab(r.w)[dst]
           + ab(r.e)[dst][:, None] * m1s + ab(r.Q)[:, None] * m1t)
    b.S3 = (d[dst] * (e_u[src] + e_v[dst] + b.lr[:, None] * m1r) + e_w[dst] + b.e[dst][:, None] * m1s
            + b.Q[:, None] * m1t + _base(7, mag))
    e_P = seg(b.S3) + _base(d, seg(ab(lrelu(r.S3))))
    e_Z2 = np.concatenate([d * e_LX + _base(0, d * ab(r.LX)), e_AX, b.e[:, None], e_P, np.zeros((R, 1))], 1)
    M2e = np.concatenate([p["M2"], p["b2"][None]], 0)
    b.m2 = e_Z2 @ M2e + _base(M2e.shape[0], ab(r.Z2e) @ M2e)
    e_Z3 = np.concatenate([e_LX, b.m2 + _base(0, ab(lrelu(r.m2))), np.zeros((R, 1))], 1)
    M3e = np.concatenate([p["M3"], p["b3"][None]], 0)
    b.y = e_Z3 @ M3e + _base(M3e.shape[0], ab(r.Z3e) @ M3e)
    b.LX, b.AX, b.Z2, b.Z3 = e_LX, e_AX, e_Z2, e_Z3
    return b


def sg_bwd_bounds(c, r, b, prm, bn_act):
    """The same propagation through the backward (DESIGN.md §8's derivation, as snd_sg_layer_bwd
    runs it): {block: bound} for Matrix1..3, bias1..3 and dx.  The kernels read the forward's
    STORED Z2e, Z3e, m2 and edge scalars, whose bounds ``b`` come in here; every lrelu' is
    evaluated off its kink (sg_assert_off_kinks), so it is the reference's own factor."""
    ab = np.abs
    F, (h0, h1, h2), R, nnz = c.F, c.hidden, c.R, c.nnz
    p = {k: ab(v) for k, v in sg_unpack(np.asarray(prm, np.float64), F, c.hidden).items()}
    M1x, M1y, M1z = p["M1"][:F], p["M1"][F:2 * F], p["M1"][2 * F:3 * F]
    src, dst = c.src, c.ci
    Asp, seg = _graph_ops(c, np.float64)
    deg = c.deg.astype(np.float64)
    d = deg[:, None]
    wgb = lambda a, ea, g, eg: ea.T @ ab(g) + ab(a).T @ eg + _base(R, ab(a).T @ ab(g))     # a^T g over the R rows
    e_dy = np.zeros_like(r.dy)
    if bn_act:                              # dT = dout lrelu'(t), dy = dT gamma c
        e_dy = _base(0, ab(r.dT)) * (p["gamma"] * BN_C) + _base(1, ab(r.dy))
    out = {}
    e3 = wgb(r.Z3e, b.Z3, r.dy, e_dy)
    out["M3"], out["b3"] = e3[:-1], e3[-1]
    e_dZ3 = e_dy @ p["M3"].T + _base(h2, ab(r.dy) @ p["M3"].T)
    e_dm2 = e_dZ3[:, F:] * lrelu_grad(r.m2) + _base(0, ab(r.dm2))
    e2 = wgb(r.Z2e, b.Z2, r.dm2, e_dm2)
    out["M2"], out["b2"] = e2[:-1], e2[-1]
    e_dZ2 = e_dm2 @ p["M2"].T + _base(h1, ab(r.dm2) @ p["M2"].T)
    e_G = e_dZ2[:, 2 * F + 1:][src] * lrelu_grad(r.S3) + _base(0, ab(r.Gq))
    e_Gr = e_G[c.rev] if nnz else e_G
    dn, en, lq, Qq = deg[dst][:, None], ab(r.e)[dst][:, None], ab(r.lr)[:, None], ab(r.Q)[:, None]
    aG = ab(r.Gq)
    e_du = seg(e_G * dn) + _base(d, seg(aG * dn))
    e_dw = seg(e_Gr) + _base(d, seg(ab(r.Gr)))
    e_dv = d * e_dw + _base(0, ab(r.dv))
    e_TM = np.concatenate([seg(e_G * dn * lq + aG * dn * b.lr[:, None]) + _base(d + 1, seg(aG * dn * lq)), e_du,
                           seg(e_G * en + aG * b.e[dst][:, None]) + _base(d, seg(aG * en)),
                           seg(e_G * Qq + aG * b.Q[:, None]) + _base(d, seg(aG * Qq))], 1)
    e_cs = e_TM.sum(0) + _base(R, ab(r.TM).sum(0))
    out["M1"] = np.concatenate([wgb(r.LX, b.LX, r.du, e_du), wgb(r.LX, b.LX, r.dv, e_dv), wgb(r.AX, b.AX, r.dw, e_dw),
                                e_cs[None, :h0], e_cs[None, 2 * h0:3 * h0], e_cs[None, 3 * h0:]], 0)
    out["b1"] = e_cs[h0:2 * h0]
    e_dlx = (e_dZ3[:, :F] + d * e_dZ2[:, :F] + e_du @ M1x.T + e_dv @ M1y.T
             + _base(2 + 2 * h0, ab(r.dZ3[:, :F]) + d * ab(r.dZ2[:, :F]) + ab(r.du) @ M1x.T + ab(r.dv) @ M1y.T))
    e_dax = e_dZ2[:, F:2 * F] + e_dw @ M1z.T + _base(1 + h0, ab(r.dZ2[:, F:2 * F]) + ab(r.dw) @ M1z.T)
    out["x"] = lrelu_grad(np.asarray(c.x, np.float64)) * (e_dlx + np.asarray(Asp @ e_dax)
                                                          + _base(d + 1, ab(r.dlx) + np.asarray(Asp @ ab(r.dax))))
    return out


def sg_assert_off_kinks(c, r, b, prm, bn_act):
    """No reference pre-activation inside its own forward bound of 0.  No exclusions."""
    bad = np.abs(r.S3) <= b.S3
    assert not bad.any(), f"sg {c.case[0]}: S3 on the lrelu kink at {np.argwhere(bad)[0]} ({int(bad.sum())} in all)"
    has = c.deg > 0
    bad = (np.abs(r.m2) <= b.m2) & has[:, None]
    assert not bad.any(), f"sg {c.case[0]}: summed m2 on the lrelu kink at {np.argwhere(bad)[0]} ({int(bad.sum())} in all)"
    assert not r.m2[~has].any() and not b.m2[~has].any(), "degree-0 rows: m2 is exactly 0"
    if bn_act:
        p = sg_unpack(np.asarray(prm, np.float64), c.F, c.hidden)
        gc = p["gamma"] * BN_C
        t = r.y * gc + p["beta"]
        bad = np.abs(t) <= b.y * np.abs(gc) + KINK * (np.abs(r.y * gc) + np.abs(p["beta"]))
        assert not bad.any(), f"sg {c.case[0]}: BN pre-activation on the lrelu kink at {np.argwhere(bad)[0]}"


# ================================================================= setup / emulate / verify
def sg_setup(case, bn_act):
    name, N, B, F, hidden, kind, xpad, dxpad, off, want_dx, seed = case
    rng = np.random.default_rng(seed)
    h0, h1, h2 = hidden
    R = N * B
    c = NS(case=case, bn_act=bn_act, N=N, B=B, F=F, hidden=hidden, R=R, want_dx=want_dx, geo=sg_geo(R, F, hidden))
    c.adj = sg_graphs(kind, N, B, rng)
    rows, cols = np.nonzero(c.adj.reshape(R, N))
    c.src, c.ci = rows.astype(np.int64), (rows // N * N + cols).astype(np.int32)
    c.deg = c.adj.reshape(R, N).sum(1).astype(np.int64)
    c.rp = np.concatenate([[0], np.cumsum(c.deg)]).astype(np.int32)
    c.nnz = len(c.ci)
    c.aloc = c.adj.reshape(R, N).astype(np.float64)
    key = c.src * R + c.ci                                        # sorted: rows, then columns
    c.rev = np.searchsorted(key, c.ci.astype(np.int64) * R + c.src).astype(np.int32)
    assert c.nnz == 0 or np.array_equal(key[c.rev], c.ci.astype(np.int64) * R + c.src), "symmetric"
    c.rel = (0.5 * rng.standard_normal((B, N, N))).astype(np.float32)
    blocks = {k: (0.3 * rng.standard_normal(s) if k[0] == "M" else 0.1 * rng.standard_normal(s)).astype(np.float32)
              for k, s in sg_shapes(F, hidden)}
    blocks["gamma"] = (1 + 0.3 * rng.standard_normal(h2)).astype(np.float32)
    blocks["beta"] = (0.3 * rng.standard_normal(h2)).astype(np.float32)
    c.prm = sg_pack(blocks, F, hidden, np.float32)
    c.x, c.dout = A._normal(rng, R, F), A._normal(rng, R, h2)
    c.ref = sg_chain(c, c.x, c.prm)                               # forward only: bounds and kinks
    c.fb = sg_fwd_bounds(c, c.ref, c.prm)
    sg_assert_off_kinks(c, c.ref, c.fb, c.prm, bn_act)
    e = max(c.nnz, 1)                                             # the entry points reject NULL
    c.bufs = {"x": guarded(R, F, F + xpad, offset=off, data=c.x, name="x"),
              "params": vec(c.prm.size, offset=off, data=c.prm, name="params"),
              "rel": vec(B * N * N, data=c.rel, name="rel"),
              "rowptr": vec(R + 1, "i32", data=c.rp, name="rowptr"),
              "colidx": vec(e, "i32", data=(c.ci if c.nnz else np.zeros(1, np.int32)), name="colidx"),
              "edge_lr": vec(e, name="edge_lr"), "edge_q": vec(e, name="edge_q"),
              "edge_rev": vec(e, "i32", name="edge_rev"), "node_deg": vec(R, name="node_deg"),
              "node_e": vec(R, name="node_e"), "n_unmatched": vec(1, "i32", name="n_unmatched"),
              "y": guarded(R, h2, name="y"), "dout": guarded(R, h2, data=c.dout, name="dout"),
              "grads": vec(c.prm.size, offset=off, name="grads"), "ws": vec(c.geo.floats, name="ws")}
    if bn_act:
        c.bufs["out"] = guarded(R, h2, name="out")
    if want_dx:
        c.bufs["dx"] = guarded(R, F, F + dxpad, offset=off, name="dx")
    return c


def _split_wg(c, fault):
    """Aop^T D as the split-K slabs form it: parts of kchunk rows, summed in order."""
    def wg(a, d):
        R, k = a.shape[0], c.geo.kchunk
        end = 64 * (R // 64) if fault == "wg_full_tiles_only" else R
        parts = [(s, min(R, s + k)) for s in range(0, R, k)]
        if fault == "wg_drop_last_part":
            parts = parts[:-1]
        acc = np.zeros((a.shape[1], d.shape[1]), a.dtype)
        for s, e in parts:
            e = min(e, end)
            if e > s:
                acc = acc + a[s:e].T @ d[s:e]
        return acc
    return wg


def sg_emulate(c, fault=None):
    after = initial(c)
    f32 = np.float32
    x = c.x
    if fault == "x_ld_f":                                        # rows read at stride f, not ldx
        gx = c.bufs["x"]
        x = gx.arr[gx.off:gx.off + c.R * c.F].reshape(c.R, c.F)
    with np.errstate(invalid="ignore"):
        r = sg_chain(c, x, c.prm, f32, c.bn_act, c.dout, fault=fault, wg=_split_wg(c, fault))
    n = c.nnz
    for k, v in (("edge_lr", r.lr), ("edge_q", r.Q)):
        after[k][G:G + n] = v
    after["edge_rev"][G:G + n] = c.rev
    put(c, after, "node_deg", r.deg)
    put(c, after, "node_e", r.e)
    put(c, after, "n_unmatched", np.zeros(1, np.int32))
    put(c, after, "y", r.y)
    if c.bn_act:
        put(c, after, "out", r.out)
    if c.want_dx:
        put(c, after, "dx", r.dx)
    gg = c.bufs["grads"]
    blk = gg.block(after["grads"])[0]
    o = 0
    for k, shp in sg_shapes(c.F, c.hidden):
        m = int(np.prod(shp))
        if r.grads[k] is not None:                               # bn_act 0 leaves gamma / beta alone
            v = np.asarray(r.grads[k], f32).reshape(-1)
            blk[o:o + m] = blk[o:o + m] + v if fault == "grads_accumulate" else v
        o += m
    gw = c.bufs["ws"]
    after["ws"][gw.off:gw.off + gw.width] = 0.0                  # scratch: any value
    if fault == "ws_overrun":                                    # one float past the workspace end
        after["ws"][gw.off + gw.width] = 0.0
    return after


def _bar(ref):
    """The inherited bar: 1e-5 of the block's max-abs."""
    ref = np.asarray(ref, np.float64)
    return Link(ref, np.zeros_like(ref), 0, extra=INHERITED * float(np.abs(ref).max(initial=0.0)))


def sg_verify_prep(c, after):
    """The edge / node scalars against their definitions in the header."""
    n, r, b = c.nnz, c.ref, c.fb
    B = lambda k: c.bufs[k].block(after[k])[0]
    assert int(B("n_unmatched")[0]) == 0, ("snd_sg_prep n_unmatched", int(B("n_unmatched")[0]))
    bad = np.flatnonzero(B("edge_rev")[:n] != c.rev)
    assert bad.size == 0, (f"snd_sg_prep edge_rev: element ({int(bad[0])},) got {int(B('edge_rev')[bad[0]])} "
                           f"ref {int(c.rev[bad[0]])}")
    bad = np.flatnonzero(B("node_deg").view(np.uint32) != c.deg.astype(np.float32).view(np.uint32))
    assert bad.size == 0, f"snd_sg_prep node_deg: element ({int(bad[0])},) got {B('node_deg')[bad[0]]!r} ref {int(c.deg[bad[0]])}"
    V = lambda k, m: np.asarray(B(k)[:m], np.float64)
    return {"edge_lr": assert_link("snd_sg_prep edge_lr", Link(r.lr, np.zeros(n), 0, extra=b.lr), V("edge_lr", n)),
            "edge_q": assert_link("snd_sg_prep edge_q", Link(r.Q, np.zeros(n), 0, extra=b.Q), V("edge_q", n)),
            "node_e": assert_link("snd_sg_prep node_e", Link(r.e, np.zeros(c.R), 0, extra=b.e), V("node_e", c.R))}


def sg_verify(c, after):
    res = sg_verify_prep(c, after)
    V = lambda k: c.bufs[k].values(after[k])
    F, hidden, R = c.F, c.hidden, c.R
    y = V("y")
    res["y"] = assert_link("snd_sg_layer_fwd y", Link(c.ref.y, np.zeros_like(c.ref.y), 0, extra=c.fb.y), y)
    p = sg_unpack(c.prm.astype(np.float64), F, hidden)
    if c.bn_act:
        A.assert_off_kink(y, p["gamma"], p["beta"], 2, 0)        # the stored y's own BN kink
        res["out"] = assert_link("snd_sg_layer_fwd out", A.ref_conv_act(y, p["gamma"], p["beta"]), V("out"))
    full = sg_chain(c, c.x, c.prm, np.float64, c.bn_act, c.dout, y_for_bn=y if c.bn_act else None)
    bb = sg_bwd_bounds(c, full, c.fb, c.prm, c.bn_act)
    got = sg_unpack(V("grads").reshape(-1), F, hidden)
    both = lambda name, key, ref, e, g: {key: assert_link(name, Link(ref, np.zeros_like(ref), 0, extra=e), g),
                                         key + "@1e-5": assert_link(name + " (1e-5 of the block)", _bar(ref), g)}
    for k in SG_BLOCKS[:6]:
        res.update(both(f"snd_sg_layer_bwd grads {k}", "g:" + k, np.asarray(full.grads[k]), bb[k], got[k]))
    if c.bn_act:
        ab = np.abs
        res["g:gamma"] = assert_link("snd_sg_layer_bwd grads gamma",
                                     Link(full.grads["gamma"], ab(full.dT * full.yb * BN_C).sum(0), R + 2), got["gamma"])
        res["g:beta"] = assert_link("snd_sg_layer_bwd grads beta", Link(full.grads["beta"], ab(full.dT).sum(0), R), got["beta"])
    if c.want_dx:
        res.update(both("snd_sg_layer_bwd dx", "dx", full.dx, bb["x"], V("dx")))
    check_guards(c, after)
    return res
