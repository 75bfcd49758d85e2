"""Float64 references of SpatialGraphConvolution_3D (`layers.py:200-277`), the three-hop
spatial-graph layer, for tests/test_sg3_cpu.py and tests/test_gpu_sg3.py.

* ``sgconv3`` / ``sgconv3_torch``: the literal form with the reference's own dense
  B x N x N x N x N tensors (numpy forward; torch ops for autograd), small N only:
      m4   = lrelu([x_i|x_j|x_k|x_p|rel_ij|rel_jk|rel_kp|rel_ik|rel_ip]) M0 + b0
      m4s  = sum_p A_ij A_jk A_kp m4
      m3   = lrelu([x_i|x_j|x_k|rel_ij|rel_jk|rel_ik|m4s]) M1 + b1 ;  m3s = sum_k A_ij A_jk m3
      m2   = lrelu([x_i|x_j|rel_ij|m3s]) M2 + b2 ;                    m2s = sum_j A_ij m2
      y    = lrelu([x|m2s]) M3 + b3
* ``sgconv3_fact``: the factorised chain include/snd_vae.h documents, in torch ops on dense
  [B, N, N] operands (O(N^3 h0) memory), any dtype: the float64 reference where N^4 does not
  fit, and in float32 the reference's own error e32.  tests/test_sg3_cpu.py pins it to the
  literal form to 1e-12.
* ``fwd_bounds`` / ``assert_off_kinks``: the propagated fp32 forward bound of every lrelu
  argument (the base rule (K + 4) 2^-23 mag of tests/abi_ops_sg.py, stage by stage) and the
  assertion that no argument on an A-masked path lies inside its bound of 0.
* ``CASES`` / ``make_case``: the committed operands of the GPU layer tests.
"""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np

BN_C = 1.0 / np.sqrt(1.0 + 1e-3)
LEAK = 0.2
U23 = 2.0 ** -23
KINK = 2.0 ** -22
BLOCKS = ("M0", "b0", "M1", "b1", "M2", "b2", "M3", "b3", "gamma", "beta")
NAMES = {"M0": "Matrix0", "b0": "bias0", "M1": "Matrix1", "b1": "bias1", "M2": "Matrix2", "b2": "bias2",
         "M3": "Matrix3", "b3": "bias3", "gamma": "gamma", "beta": "beta"}


def lrelu(x):
    return np.maximum(x, LEAK * x)


def shapes(F, hid):
    h0, h1, h2, h3 = hid
    return (("M0", (4 * F + 5, h0)), ("b0", (h0,)), ("M1", (3 * F + 3 + h0, h1)), ("b1", (h1,)),
            ("M2", (2 * F + 1 + h1, h2)), ("b2", (h2,)), ("M3", (F + h2, h3)), ("b3", (h3,)),
            ("gamma", (h3,)), ("beta", (h3,)))


def unpack_layer(flat, F, hid):
    """A layer's flat parameter vector (include/snd_vae.h layout) -> views (numpy or torch)."""
    out, o = {}, 0
    for name, shp in shapes(F, hid):
        n = int(np.prod(shp))
        out[name] = flat[o:o + n].reshape(shp)
        o += n
    assert o == flat.shape[0], (o, flat.shape)
    return out


def pack_layer(p, F, hid):
    return np.concatenate([np.asarray(p[k], np.float64).reshape(-1) for k, _ in shapes(F, hid)])


def init_params(F, hid, rng, stddev=0.3, bias=0.1, bn=0.1):
    """Matrices N(0, stddev), biases N(0, bias) (nonzero), BN gamma 1 + N(0, bn), beta N(0, bn)."""
    p = {}
    for k, shp in shapes(F, hid):
        if k.startswith("M"):
            p[k] = rng.normal(0.0, stddev, shp)
        elif k == "gamma":
            p[k] = 1.0 + bn * rng.normal(size=shp)
        elif k == "beta":
            p[k] = bn * rng.normal(size=shp)
        else:
            p[k] = bias * rng.normal(size=shp)
    return p


# ================================================================= literal dense form
def sgconv3(adj, x, rel, p):
    """adj [B,N,N], x [B,N,F], rel [B,N,N] (rel_dim 1); numpy float64."""
    adj, x, rel = (np.asarray(a, np.float64) for a in (adj, x, rel))
    B, N, F = x.shape
    s5, s4 = (B, N, N, N, N), (B, N, N, N)
    bc = np.broadcast_to
    m4 = np.concatenate([bc(x[:, :, None, None, None, :], s5 + (F,)), bc(x[:, None, :, None, None, :], s5 + (F,)),
                         bc(x[:, None, None, :, None, :], s5 + (F,)), bc(x[:, None, None, None, :, :], s5 + (F,)),
                         bc(rel[:, :, :, None, None, None], s5 + (1,)), bc(rel[:, None, :, :, None, None], s5 + (1,)),
                         bc(rel[:, None, None, :, :, None], s5 + (1,)), bc(rel[:, :, None, :, None, None], s5 + (1,)),
                         bc(rel[:, :, None, None, :, None], s5 + (1,))], -1)
    m4 = lrelu(m4) @ p["M0"] + p["b0"]
    adj4 = adj[:, :, :, None, None] * adj[:, None, :, :, None] * adj[:, None, None, :, :]
    m4s = np.einsum("bijkph,bijkp->bijkh", m4, adj4)
    m3 = np.concatenate([bc(x[:, :, None, None, :], s4 + (F,)), bc(x[:, None, :, None, :], s4 + (F,)),
                         bc(x[:, None, None, :, :], s4 + (F,)), bc(rel[:, :, :, None, None], s4 + (1,)),
                         bc(rel[:, None, :, :, None], s4 + (1,)), bc(rel[:, :, None, :, None], s4 + (1,)), m4s], -1)
    m3 = lrelu(m3) @ p["M1"] + p["b1"]
    adj3 = adj[:, :, :, None] * adj[:, None, :, :]
    m3s = np.einsum("bijkh,bijk->bijh", m3, adj3)
    m2 = np.concatenate([bc(x[:, :, None, :], (B, N, N, F)), bc(x[:, None, :, :], (B, N, N, F)), rel[..., None], m3s], -1)
    m2 = lrelu(m2) @ p["M2"] + p["b2"]
    m2s = np.einsum("bijh,bij->bih", m2, adj)
    return lrelu(np.concatenate([x, m2s], -1)) @ p["M3"] + p["b3"]


def sgconv3_torch(adj, x, rel, p):
    """The same graph in torch ops (autograd stands in for TF autodiff)."""
    import torch
    lr = lambda t: torch.maximum(t, LEAK * t)
    B, N, F = x.shape
    s5, s4 = (B, N, N, N, N), (B, N, N, N)
    m4 = torch.cat([x[:, :, None, None, None, :].expand(*s5, F), x[:, None, :, None, None, :].expand(*s5, F),
                    x[:, None, None, :, None, :].expand(*s5, F), x[:, None, None, None, :, :].expand(*s5, F),
                    rel[:, :, :, None, None, None].expand(*s5, 1), rel[:, None, :, :, None, None].expand(*s5, 1),
                    rel[:, None, None, :, :, None].expand(*s5, 1), rel[:, :, None, :, None, None].expand(*s5, 1),
                    rel[:, :, None, None, :, None].expand(*s5, 1)], -1)
    m4 = lr(m4) @ p["M0"] + p["b0"]
    adj4 = adj[:, :, :, None, None] * adj[:, None, :, :, None] * adj[:, None, None, :, :]
    m4s = torch.einsum("bijkph,bijkp->bijkh", m4, adj4)
    m3 = torch.cat([x[:, :, None, None, :].expand(*s4, F), x[:, None, :, None, :].expand(*s4, F),
                    x[:, None, None, :, :].expand(*s4, F), rel[:, :, :, None, None].expand(*s4, 1),
                    rel[:, None, :, :, None].expand(*s4, 1), rel[:, :, None, :, None].expand(*s4, 1), m4s], -1)
    m3 = lr(m3) @ p["M1"] + p["b1"]
    adj3 = adj[:, :, :, None] * adj[:, None, :, :]
    m3s = torch.einsum("bijkh,bijk->bijh", m3, adj3)
    m2 = torch.cat([x[:, :, None, :].expand(B, N, N, F), x[:, None, :, :].expand(B, N, N, F), rel[..., None], m3s], -1)
    m2 = lr(m2) @ p["M2"] + p["b2"]
    m2s = torch.einsum("bijh,bij->bih", m2, adj)
    return lr(torch.cat([x, m2s], -1)) @ p["M3"] + p["b3"]


# ================================================================= factorised chain
def _terms(adj, x, rel, p, lr, xp):
    """The node / edge / pair terms shared by the factorised forward and its bounds."""
    F = x.shape[-1]
    M0, M1, M2 = p["M0"], p["M1"], p["M2"]
    t = NS()
    t.LX, t.L = lr(x), lr(rel)
    t.d = adj.sum(-1)
    t.e = (adj * t.L).sum(-1)
    t.AX = adj @ t.LX
    t.Q = xp.einsum("bip,bkp->bik", t.L, adj)                        # Q_ik = sum_{p in N(k)} L_ip
    t.a, t.b = t.LX @ M0[:F], t.LX @ M0[F:2 * F]
    t.G = (t.d[..., None] * t.LX) @ M0[2 * F:3 * F] + t.AX @ M0[3 * F:4 * F]
    t.m0 = [M0[4 * F + i] for i in range(5)]                         # ij, jk, kp, ik, ip
    t.u, t.v, t.w = t.LX @ M1[:F], t.LX @ M1[F:2 * F], t.AX @ M1[2 * F:3 * F]
    t.m1 = [M1[3 * F + i] for i in range(3)]                         # ij, jk, ik
    t.M1s = M1[3 * F + 3:]
    return t


def sgconv3_fact(adj, x, rel, p, full=False):
    """The factorised chain in torch ops; full: also the intermediate lrelu arguments."""
    import torch
    lr = lambda v: torch.maximum(v, LEAK * v)
    F = x.shape[-1]
    t = _terms(adj, x, rel, p, lr, torch)
    m0ij, m0jk, m0kp, m0ik, m0ip = t.m0
    dk = t.d[:, None, None, :, None]
    L = t.L
    S4 = (dk * (t.a[:, :, None, None, :] + t.b[:, None, :, None, :] + L[:, :, :, None, None] * m0ij
                + L[:, None, :, :, None] * m0jk + L[:, :, None, :, None] * m0ik + p["b0"])
          + (t.G + t.e[..., None] * m0kp)[:, None, None, :, :] + t.Q[:, :, None, :, None] * m0ip)
    T = torch.einsum("bijkh,bjk->bijh", lr(S4), adj)
    dj = t.d[:, None, :, None]
    S3 = (dj * (t.u[:, :, None, :] + t.v[:, None, :, :] + L[..., None] * t.m1[0] + p["b1"]) + t.w[:, None, :, :]
          + t.e[:, None, :, None] * t.m1[1] + t.Q[..., None] * t.m1[2] + T @ t.M1s)
    P = torch.einsum("bijh,bij->bih", lr(S3), adj)
    M2 = p["M2"]
    di = t.d[..., None]
    m2s = di * (t.LX @ M2[:F] + p["b2"]) + t.AX @ M2[F:2 * F] + t.e[..., None] * M2[2 * F] + P @ M2[2 * F + 1:]
    y = torch.cat([t.LX, lr(m2s)], -1) @ p["M3"] + p["b3"]
    return (y, NS(S4=S4, S3=S3, m2s=m2s, T=T, P=P, t=t)) if full else y


def layer_grads(fn, adj, x, rel, p, dout, bn_act=False, dtype=None):
    """(y, out, {block: grad, 'x': dx}) of sum(out * dout) for fn in (sgconv3_torch,
    sgconv3_fact); out = lrelu(BN(y)) when bn_act, else y.  dtype: torch.float64 (default) or
    torch.float32 (the reference's own fp32 error)."""
    import torch
    dtype = dtype or torch.float64
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), dtype=dtype, requires_grad=g)
    tp = {k: t(v, True) for k, v in p.items()}
    tx = t(x, True)
    y = fn(t(adj), tx, t(rel), tp)
    out = y
    if bn_act:
        pre = y * (tp["gamma"] * BN_C) + tp["beta"]
        out = torch.maximum(pre, LEAK * pre)
    (out * t(dout)).sum().backward()
    g = {k: (v.grad.double().numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in tp.items()}
    g["x"] = tx.grad.double().numpy()
    return y.detach().double().numpy(), out.detach().double().numpy(), g


def encoder_grads(fn, adj, x, rel, layers, dout, dtype=None):
    """The encoder stack s = lrelu(BN(SGConv3D(adj, s, rel))) per layer: (out, [grads per layer])."""
    import torch
    dtype = dtype or torch.float64
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), dtype=dtype, requires_grad=g)
    tps = [{k: t(v, True) for k, v in p.items()} for p in layers]
    s, A, R = t(x), t(adj), t(rel)
    for tp in tps:
        pre = fn(A, s, R, tp) * (tp["gamma"] * BN_C) + tp["beta"]
        s = torch.maximum(pre, LEAK * pre)
    (s * t(dout)).sum().backward()
    return s.detach().double().numpy(), [{k: v.grad.double().numpy() for k, v in tp.items()} for tp in tps]


# ================================================================= fp32 forward bounds, kinks
def _base(K, mag):
    return (np.asarray(K, np.float64) + 4.0) * U23 * mag


def fwd_bounds(adj, x, rel, p):
    """(values, bounds) of S4 [B,N,N,N,h0], S3 [B,N,N,h1], m2s [B,N,h2] and y [B,N,h3]: the float64
    factorised values and |fp32 - float64| bounds, the base rule propagated stage by stage
    (a step is |e_in| |W| + (K + 4) 2^-23 (|in| |W| + |b|))."""
    ab = np.abs
    adj, x, rel = (np.asarray(a, np.float64) for a in (adj, x, rel))
    p = {k: np.asarray(v, np.float64) for k, v in p.items()}
    pa = {k: ab(v) for k, v in p.items()}
    F = x.shape[-1]
    h0 = p["b0"].shape[0]
    t = _terms(adj, x, rel, p, lrelu, np)
    m = _terms(adj, ab(x), ab(rel), pa, lambda v: v, np)                # magnitudes: |LX| <= |x| etc.
    m.LX, m.L = ab(t.LX), ab(t.L)
    m.e, m.AX = (adj * m.L).sum(-1), adj @ m.LX
    m.Q = np.einsum("bip,bkp->bik", m.L, adj)
    d = t.d
    e = NS()
    e.L = _base(0, m.L)
    e.e = (adj * e.L).sum(-1) + _base(d, m.e)
    e.Q = np.einsum("bip,bkp->bik", e.L, adj) + _base(d[:, None, :], m.Q)
    e.LX = _base(0, m.LX)
    e.AX = adj @ e.LX + _base(d[..., None], m.AX)
    M0, M1, M2 = pa["M0"], pa["M1"], pa["M2"]
    e.a = e.LX @ M0[:F] + _base(F, m.LX @ M0[:F])
    e.b = e.LX @ M0[F:2 * F] + _base(F, m.LX @ M0[F:2 * F])
    dLX = d[..., None] * m.LX
    magG = dLX @ M0[2 * F:3 * F] + m.AX @ M0[3 * F:4 * F]
    e.G = (d[..., None] * e.LX + _base(0, dLX)) @ M0[2 * F:3 * F] + e.AX @ M0[3 * F:4 * F] + _base(2 * F, magG)
    mij, mjk, mkp, mik, mip = (M0[4 * F + i] for i in range(5))
    dk = d[:, None, None, :, None]
    L, eL = m.L, e.L
    A5 = lambda v: v[:, :, None, None, :]
    B5 = lambda v: v[:, None, :, None, :]
    K5 = lambda v: v[:, None, None, :, :]
    mag4 = (dk * (A5(ab(t.a)) + B5(ab(t.b)) + L[:, :, :, None, None] * mij + L[:, None, :, :, None] * mjk
                  + L[:, :, None, :, None] * mik + pa["b0"])
            + K5(ab(t.G) + m.e[..., None] * mkp) + m.Q[:, :, None, :, None] * mip)
    e.S4 = (dk * (A5(e.a) + B5(e.b) + eL[:, :, :, None, None] * mij + eL[:, None, :, :, None] * mjk
                  + eL[:, :, None, :, None] * mik)
            + K5(e.G + e.e[..., None] * mkp) + e.Q[:, :, None, :, None] * mip + _base(14, mag4))
    m0 = t.m0
    S4 = (dk * (A5(t.a) + B5(t.b) + t.L[:, :, :, None, None] * m0[0] + t.L[:, None, :, :, None] * m0[1]
                + t.L[:, :, None, :, None] * m0[3] + p["b0"])
          + K5(t.G + t.e[..., None] * m0[2]) + t.Q[:, :, None, :, None] * m0[4])
    lS4 = lrelu(S4)
    T = np.einsum("bijkh,bjk->bijh", lS4, adj)
    magT = np.einsum("bijkh,bjk->bijh", ab(lS4), adj)
    e.T = np.einsum("bijkh,bjk->bijh", e.S4, adj) + _base(d[:, None, :, None], magT)
    M1s = M1[3 * F + 3:]
    TS = T @ t.M1s
    e.TS = e.T @ M1s + _base(h0, magT @ M1s)
    dj = d[:, None, :, None]
    m1ij, m1jk, m1ik = (M1[3 * F + i] for i in range(3))
    mag3 = (dj * (ab(t.u)[:, :, None, :] + ab(t.v)[:, None, :, :] + L[..., None] * m1ij + pa["b1"])
            + ab(t.w)[:, None, :, :] + m.e[:, None, :, None] * m1jk + m.Q[..., None] * m1ik + ab(TS))
    e.u = e.LX @ M1[:F] + _base(F, m.LX @ M1[:F])
    e.v = e.LX @ M1[F:2 * F] + _base(F, m.LX @ M1[F:2 * F])
    e.w = e.AX @ M1[2 * F:3 * F] + _base(F, m.AX @ M1[2 * F:3 * F])
    e.S3 = (dj * (e.u[:, :, None, :] + e.v[:, None, :, :] + eL[..., None] * m1ij) + e.w[:, None, :, :]
            + e.e[:, None, :, None] * m1jk + e.Q[..., None] * m1ik + e.TS + _base(8, mag3))
    S3 = (dj * (t.u[:, :, None, :] + t.v[:, None, :, :] + t.L[..., None] * t.m1[0] + p["b1"]) + t.w[:, None, :, :]
          + t.e[:, None, :, None] * t.m1[1] + t.Q[..., None] * t.m1[2] + TS)
    lS3 = lrelu(S3)
    P = np.einsum("bijh,bij->bih", lS3, adj)
    magP = np.einsum("bijh,bij->bih", ab(lS3), adj)
    e.P = np.einsum("bijh,bij->bih", e.S3, adj) + _base(d[..., None], magP)
    di = d[..., None]
    Z2 = np.concatenate([di * t.LX, t.AX, t.e[..., None], P, di], -1)
    e.Z2 = np.concatenate([di * e.LX + _base(0, dLX), e.AX, e.e[..., None], e.P, np.zeros_like(di)], -1)
    M2e = np.concatenate([p["M2"], p["b2"][None]], 0)
    m2s = Z2 @ M2e
    e.m2s = e.Z2 @ ab(M2e) + _base(M2e.shape[0], ab(Z2) @ ab(M2e))
    Z3 = np.concatenate([t.LX, lrelu(m2s), np.ones_like(di)], -1)
    e.Z3 = np.concatenate([e.LX, e.m2s + _base(0, ab(lrelu(m2s))), np.zeros_like(di)], -1)
    M3e = np.concatenate([p["M3"], p["b3"][None]], 0)
    y = Z3 @ M3e
    e.y = e.Z3 @ ab(M3e) + _base(M3e.shape[0], ab(Z3) @ ab(M3e))
    return NS(S4=S4, S3=S3, m2s=m2s, y=y, d=d), e


def kink_violations(adj, x, rel, p, bn_act):
    """Number of lrelu arguments on an A-masked path inside their own fp32 forward bound of 0:
    S4 per 2-path and channel, S3 per edge and channel, m2s of nodes with edges, and with
    bn_act the BN pre-activation of every row.  No element is excluded."""
    adj = np.asarray(adj, np.float64)
    v, e = fwd_bounds(adj, x, rel, p)
    path = (adj[:, :, :, None] * adj[:, None, :, :]) > 0
    bad = int(((np.abs(v.S4) <= e.S4) & path[..., None]).sum())
    bad += int(((np.abs(v.S3) <= e.S3) & (adj > 0)[..., None]).sum())
    has = v.d > 0
    bad += int(((np.abs(v.m2s) <= e.m2s) & has[..., None]).sum())
    assert not v.m2s[~has].any() and not e.m2s[~has].any(), "degree-0 rows: m2s is exactly 0"
    if bn_act:
        gc = np.asarray(p["gamma"], np.float64) * BN_C
        beta = np.asarray(p["beta"], np.float64)
        t = v.y * gc + beta
        bad += int((np.abs(t) <= e.y * np.abs(gc) + KINK * (np.abs(v.y * gc) + np.abs(beta))).sum())
    return bad


# ================================================================= committed cases
def csr_of(adj):
    """Block-diagonal CSR (rowptr, global sorted colidx) of dense adj [B, N, N]."""
    B, N, _ = adj.shape
    rows = adj.reshape(B * N, N) > 0
    rp = np.concatenate([[0], np.cumsum(rows.sum(1))]).astype(np.int32)
    r, c = np.nonzero(rows)
    return rp, (c + r // N * N).astype(np.int32)


def _random_graphs(B, N, rng, prob=0.45):
    up = np.triu(rng.random((B, N, N)) < prob, 1)
    return (up | up.transpose(0, 2, 1)).astype(np.float64)


def _trees(B, N, rng):
    """Uniform random recursive trees: node v > 0 attaches to a random earlier node."""
    a = np.zeros((B, N, N))
    for b in range(B):
        order = rng.permutation(N)
        for t in range(1, N):
            u, v = order[t], order[rng.integers(t)]
            a[b, u, v] = a[b, v, u] = 1.0
    return a


def _hub(N, rng, chords=5):
    a = np.zeros((1, N, N))
    a[0, 0, 1:] = a[0, 1:, 0] = 1.0                                 # a star: degree N - 1 at node 0
    for _ in range(chords):
        u, v = rng.choice(np.arange(1, N), 2, replace=False)
        a[0, u, v] = a[0, v, u] = 1.0                                # triangles through the hub
    return a


# id: (B, N, F, widths, graphs, reference, seed).  "fact": N^4 (or B N^4) too large for the literal
# form; the factorised float64 chain is the reference (pinned to the literal one on the others).
CASES = {
    "tree": (3, 24, 1, (10, 10, 10, 10), "tree", "dense", 1),
    "graph": (3, 12, 2, (7, 5, 3, 4), "random", "dense", 2),
    "hub": (1, 70, 2, (7, 5, 3, 4), "hub", "fact", 3),
    "split": (821, 5, 2, (7, 5, 3, 4), "random", "fact", 63),
    "tails": (4, 5, 2, (65, 7, 66, 9), "random", "dense", 5),
    "empty": (1, 3, 2, (7, 5, 3, 4), "empty", "dense", 6),
    "isolated": (1, 4, 2, (7, 5, 3, 4), "isolated", "dense", 7),
    "strided": (10, 6, 2, (7, 5, 3, 4), "random", "dense", 8),
}
# the two-layer encoder stack at the protein widths (main.py:223), BN + lrelu
STACK = (2, 10, 1, ((10,) * 4, (20,) * 4), 9)

_cache = {}


def make_case(name):
    """The committed operands of a case (cached, read-only): adj, CSR, rel = 3-D distances -
    0.15 (both signs), x ~ N(0, 1), weights N(0, 0.3), nonzero biases, dout ~ N(0, 1)."""
    if name in _cache:
        return _cache[name]
    B, N, F, hid, kind, ref, seed = CASES[name]
    rng = np.random.default_rng(seed)
    if kind == "tree":
        adj = _trees(B, N, rng)
    elif kind == "random":
        adj = _random_graphs(B, N, rng)
    elif kind == "hub":
        adj = _hub(N, rng)
    elif kind == "empty":
        adj = np.zeros((B, N, N))
    else:                                                            # a triangle and one isolated node
        adj = np.zeros((B, N, N))
        for u, v in ((0, 1), (1, 2), (0, 2)):
            adj[0, u, v] = adj[0, v, u] = 1.0
    pos = rng.random((B, N, 3))
    rel = np.linalg.norm(pos[:, :, None] - pos[:, None], axis=-1) - 0.15
    c = NS(name=name, B=B, N=N, F=F, hid=hid, ref=ref, adj=adj, rel=rel.astype(np.float32).astype(np.float64))
    c.rp, c.ci = csr_of(adj)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)     # exactly what the device reads
    c.x = f32(rng.normal(size=(B, N, F)))
    c.p = {k: f32(v) for k, v in init_params(F, hid, rng).items()}
    c.dout = f32(rng.normal(size=(B, N, hid[3])))
    for v in (c.adj, c.rel, c.x, c.dout, *c.p.values()):
        v.setflags(write=False)
    _cache[name] = c
    return c


def make_stack():
    if "stack" in _cache:
        return _cache["stack"]
    B, N, F, hids, seed = STACK
    rng = np.random.default_rng(seed)
    adj = _trees(B, N, rng)
    pos = rng.random((B, N, 3))
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    c = NS(B=B, N=N, F=F, hids=hids, adj=adj, rel=f32(np.linalg.norm(pos[:, :, None] - pos[:, None], axis=-1) - 0.15))
    c.rp, c.ci = csr_of(adj)
    c.x = f32(rng.random((B, N, F)))
    c.layers, f = [], F
    for hid in hids:
        c.layers.append({k: f32(v) for k, v in init_params(f, hid, rng, stddev=0.2).items()})
        f = hid[3]
    c.dout = f32(rng.normal(size=(B, N, f)))
    _cache["stack"] = c
    return c


_refs = {}


def reference(name, bn_act=False):
    """(y, out, grads) of a committed case in float64, computed once and shared."""
    key = (name, bn_act)
    if key not in _refs:
        c = make_case(name)
        fn = sgconv3_torch if c.ref == "dense" else sgconv3_fact
        _refs[key] = layer_grads(fn, c.adj, c.x, c.rel, c.p, c.dout, bn_act=bn_act)
    return _refs[key]
