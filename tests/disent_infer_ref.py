"""References for the disentangled model's inference (encode, decode, generate, traverse)
and for the forward-only e2e structure decoder ``snd_e2e_decode``; importable without a GPU.

* ``decode_literal``: model.py:172-222 from the oracle's pieces (``oracle.ref_disent.e2e_torch``
  and ``BN_C``, ``oracle.ref_torch``) in any torch dtype: margin, adj, spatial, node;
  ``structure_literal`` is its adjacency part alone (model.py:193-208);
* ``structure_factorised``: the float64 restatement of the factorised layer 0 the kernel
  computes (the header of snd_vae_amd/csrc/snd_e2e_dec.hip), later layers literal;
* ``encode_ref``: the three encoders, the forward part of
  ``oracle.ref_disent_model.disent_loss_torch`` (its ``groups``);
* ``traverse_all_rows_literal`` / ``traverse_rows_literal``: the row construction of
  model.py:232-265,326-358 transcribed (tile, then overwrite slices), without the file I/O;
* ``margin_bound``: own_operands' rule ((K + 4) 2^-23 mag per fp32 sum of K terms) carried
  stage by stage through pair BN, every e2e layer, every BN and the head, as
  tests/abi_ops_disent.py does for the head; ``margin_bar`` is the bar of the C ABI test:
  that bound, capped by the conditioning idiom of tests/test_gpu_disent_model.py.  The rule
  is a worst case (every rounding aligned, carried through sum |w|): at the reference widths
  (N = 25, D = 40, hidden (50, 20); K = 4001 products in layer 0) it comes to 2.7 where the
  largest margin is 1.1, so on its own it could neither decide one argmax there nor notice
  a wrong margin.  The cap max(1e-5, 10 e32) max|margin| -- e32 the literal decoder's own
  error in torch.float32, 4e-8 to 1.4e-6 over this file's cases -- is the tighter of the two in every
  case of this file, so every case asks more of the kernel than the rule alone;
* ``decode_setup``: guarded operands for tests/test_gpu_e2e_decode.py.
"""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np

import abi_ops as A
import abi_ops_disent as D
from abi_ops import guarded, vec
from oracle import ref_disent as RD
from oracle import ref_disent_model as RM
from oracle import ref_torch as T
from own_operands import BN_C, U23, Link


# ---------------------------------------------------------------- literal decode (torch)
def _tt(a, dtype):
    import torch
    return a.to(dtype) if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a, np.float64), dtype=dtype)


def structure_literal(z, layers, head, dtype=None):
    """(margin [B, N, N], adj bool) of model.py:193-208: the logits of
    ``structure_decoder_torch`` (pair concat, e2e(relu(BN(h))) per layer, relu(BN) W + b, the
    diagonal (1, 0)), margin = l1 - l0, adj = argmax (a tie is class 0)."""
    import torch
    dtype = dtype or torch.float64
    z = _tt(z, dtype)
    lay = [{k: _tt(v, dtype) for k, v in l.items()} for l in layers]
    hd = {k: _tt(v, dtype) for k, v in head.items()}
    B, N, Dz = z.shape
    h = torch.cat([z[:, :, None, :].expand(B, N, N, Dz), z[:, None, :, :].expand(B, N, N, Dz)], -1)
    for l in lay:
        h = RD.e2e_torch(torch.relu(l["gamma"] * h * RD.BN_C + l["beta"]), l["w"], l["b"])
    logits = torch.relu(hd["gamma"] * h * RD.BN_C + hd["beta"]) @ hd["w"] + hd["b"]
    diag = 1.0 - torch.eye(N, dtype=dtype)[None]
    p1 = diag * logits[..., 1]
    p0 = diag * logits[..., 0] + (1.0 - diag)
    return p1 - p0, p1 > p0


def structure_factorised(z, layers, head):
    """The same margin with layer 0 factorised (float64 numpy):
    y0[b,i,j] = a_i Wsum_j[:D] + a'_j Wsum_i[D:] + P[b,i] + Q[b,j] + 2 b with
    a = relu(BN0[:D](z)), a' = relu(BN0[D:](z)), Wsum_n = the sum of the taps SAME padding
    keeps at n, P = conv1d_SAME(a, w[:, :D]), Q = conv1d_SAME(a', w[:, D:])."""
    f = lambda a: np.asarray(a, np.float64)
    z = f(z)
    B, N, Dz = z.shape
    l0 = layers[0]
    g, be, w, b = f(l0["gamma"]), f(l0["beta"]), f(l0["w"]), f(l0["b"])
    a = np.maximum(g[:Dz] * BN_C * z + be[:Dz], 0)
    ap = np.maximum(g[Dz:] * BN_C * z + be[Dz:], 0)
    pb = (N - 1) // 2
    wsum = np.zeros((N,) + w.shape[1:])
    P, Q = np.zeros((B, N, w.shape[2])), np.zeros((B, N, w.shape[2]))
    for n in range(N):
        for t in range(N):
            m = n + t - pb
            if 0 <= m < N:
                wsum[n] += w[t]
                P[:, n] += a[:, m] @ w[t, :Dz]
                Q[:, n] += ap[:, m] @ w[t, Dz:]
    y = (np.einsum("bic,jco->bijo", a, wsum[:, :Dz]) + np.einsum("bjc,ico->bijo", ap, wsum[:, Dz:])
         + P[:, :, None, :] + Q[:, None, :, :] + 2 * b)
    for l in layers[1:]:
        x = np.maximum(f(l["gamma"]) * BN_C * y + f(l["beta"]), 0)
        y = RD.e2e(x, f(l["w"]), f(l["b"]))
    logits = np.maximum(f(head["gamma"]) * BN_C * y + f(head["beta"]), 0) @ f(head["w"]) + f(head["b"])
    margin = logits[..., 1] - logits[..., 0]
    margin[:, np.arange(N), np.arange(N)] = -1.0
    return margin


def e2e_params(p, cfg):
    layers = [{"gamma": p[f"d_bn_e{i}/gamma"], "beta": p[f"d_bn_e{i}/beta"], "w": p[f"e{i}_deconv/w1"],
               "b": p[f"e{i}_deconv/biases1"]} for i in range(len(cfg.e_d_hidden))]
    head = {"gamma": p["decoder_adj/gamma"], "beta": p["decoder_adj/beta"], "w": p["d_e_lin2/Matrix"],
            "b": p["d_e_lin2/bias"]}
    return layers, head


def decode_literal(p, cfg, z_s, z_sg, z_g, dtype=None):
    """decoder(z_s, z_sg, z_g) of model.py:172-222 for B = rows(z_s) graphs and S' =
    rows(z_sg) / B copies; p: blocks by name.  Returns numpy float64 {margin, adj (bool),
    spatial [B, N, sd], node [B, N, F]}."""
    import torch
    dtype = dtype or torch.float64
    p = {k: _tt(v, dtype) for k, v in p.items()}
    z_s, z_sg, z_g = (_tt(a, dtype) for a in (z_s, z_sg, z_g))
    bn = lambda t, k: T.bn(t, p[k + "/gamma"], p[k + "/beta"])
    B, N, nh = z_s.shape[0], cfg.n_nodes, cfg.node_h
    S = z_sg.shape[0] // B
    J_sg = torch.reshape(z_sg @ p["d_sg_lin1/Matrix"] + p["d_sg_lin1/bias"], [B, S, N, nh]).mean(1)
    J_s = torch.reshape(z_s @ p["d_s_lin1/Matrix"] + p["d_s_lin1/bias"], [B, N, nh])
    J_g = torch.reshape(z_g @ p["d_g_lin1/Matrix"] + p["d_g_lin1/bias"], [B, N, nh])
    z_sg_g = torch.cat([J_sg, J_g], -1)
    u = z_sg_g
    for i in range(len(cfg.n_d_channel)):
        u = bn(T.conv1d_same(u, p[f"n{i}_deconv/kernel"], p[f"n{i}_deconv/bias"]), f"d_bn_n{i}")
    node = torch.sigmoid(bn(u, "decoder_node") @ p["d_n_lin2/Matrix"] + p["d_n_lin2/bias"])
    layers, head = e2e_params(p, cfg)
    margin, adj = structure_literal(z_sg_g, layers, head, dtype)
    v = torch.cat([J_sg, J_s], -1)
    for i in range(len(cfg.s_d_channel)):
        v = bn(T.conv1d_same(v, p[f"s{i + 1}_deconv/kernel"], p[f"s{i + 1}_deconv/bias"]), f"d_bn_s{i}")
    spatial = torch.sigmoid(v @ p["d_s_lin2/Matrix"] + p["d_s_lin2/bias"])
    n64 = lambda t: t.double().numpy()
    return {"margin": n64(margin), "adj": adj.numpy(), "spatial": n64(spatial), "node": n64(node)}


def encode_ref(p, inputs, eps, cfg, dtype=None):
    """{'s' | 'g' | 'sg': {mu, logstd, z}} (numpy float64): the ``groups`` of
    ``disent_loss_torch``, its forward part up to get_z."""
    import torch
    dtype = dtype or torch.float64
    pt = {k: _tt(v, dtype) for k, v in p.items()}
    it = {k: _tt(v, dtype) for k, v in inputs.items()}
    et = {k: _tt(v, dtype) for k, v in eps.items()}
    with torch.no_grad():
        groups = RM.disent_loss_torch(pt, it, et, cfg)[2]
    return {k: {"mu": g[0].double().numpy(), "logstd": g[1].double().numpy(), "z": g[2].double().numpy()}
            for k, g in groups.items()}


# ---------------------------------------------------------------- traverse rows, literally
def traverse_all_rows_literal(z_s, z_g, z_sg, rang, V):
    """model.py:326-349: z_* [length, 1, L] bases tiled V times, then block k's dimension
    overwritten by rang (visualize_length = V); returns (z_s, z_g, z_sg)."""
    Ls, Lg, Lsg = z_s.shape[-1], z_g.shape[-1], z_sg.shape[-1]
    z_s = np.tile(z_s.reshape(-1, 1, Ls), [1, V, 1]).reshape(-1, Ls)
    z_g = np.tile(z_g.reshape(-1, 1, Lg), [1, V, 1]).reshape(-1, Lg)
    z_sg = np.tile(z_sg.reshape(-1, 1, Lsg), [1, V, 1]).reshape(-1, Lsg)
    for dim in range(Ls):
        base = 0
        z_s[dim * V + base:dim * V + V + base, dim] = rang
    for dim in range(Lg):
        base = Ls * V
        z_g[dim * V + base:dim * V + V + base, dim] = rang
    for dim in range(Lsg):
        base = Ls * V + Lg * V
        z_sg[dim * V + base:dim * V + V + base, dim] = rang
    return z_s, z_g, z_sg


def traverse_rows_literal(group_type, fix_dim, z_s, z_g, z_sg, rang, V):
    """model.py:232-260: the V rows of one (group_type, fix_dim) block."""
    Ls, Lg, Lsg = z_s.shape[-1], z_g.shape[-1], z_sg.shape[-1]
    z_s = np.tile(z_s.reshape(-1, 1, Ls), [1, V, 1]).reshape(-1, Ls)
    z_g = np.tile(z_g.reshape(-1, 1, Lg), [1, V, 1]).reshape(-1, Lg)
    z_sg = np.tile(z_sg.reshape(-1, 1, Lsg), [1, V, 1]).reshape(-1, Lsg)
    if group_type == "s":
        base = 0
        z_s[fix_dim * V + base:fix_dim * V + V + base, fix_dim] = rang
    elif group_type == "g":
        base = Ls * V
        z_g[fix_dim * V + base:fix_dim * V + V + base, fix_dim] = rang
    elif group_type == "sg":
        base = Ls * V + Lg * V
        z_sg[fix_dim * V + base:fix_dim * V + V + base, fix_dim] = rang
    sl = slice(fix_dim * V + base, fix_dim * V + V + base)
    return z_s[sl], z_g[sl], z_sg[sl]


# ---------------------------------------------------------------- derived bound of the margin
def _base(K, mag):
    return (np.asarray(K, np.float64) + 4.0) * U23 * np.asarray(mag, np.float64)


def margin_bound(z, layers, head):
    """NS(margin, bound): the float64 margin and its fp32 bar by own_operands' rule, stage by
    stage.  BN: two roundings, (2 + 4) 2^-23 (|g c y| + |beta|), on top of |g c| times the
    input's bound; relu passes a bound unchanged; an e2e layer: its input's bound through
    |w| plus (K + 4) 2^-23 mag with K = C * taps + 1 products and mag = sum |x| |w| + 2 |b|
    (``abi_ops_disent.ref_e2e_fwd``); the head: the bound through |W| plus (C + 1 + 4) 2^-23
    (|x| |W| + |b|); the margin: both logits' bounds and one subtraction.  The factorised
    layer 0 rounds fewer than K times per product chain (the tap sums, D products, four
    adds), so the literal rule covers it."""
    f, ab = (lambda a: np.asarray(a, np.float64)), np.abs
    h = D.pair_concat(f(z))
    e_y = np.zeros_like(h)
    y = h
    for l in layers:
        gc, be = f(l["gamma"]) * BN_C, f(l["beta"])
        t = gc * y + be
        e_x = ab(gc) * e_y + _base(2, ab(gc * y) + ab(be))
        x = np.maximum(t, 0)
        w, b = f(l["w"]), f(l["b"])
        link = D.ref_e2e_fwd(x, w, b)
        e_y = D.ref_e2e_fwd(e_x, ab(w), np.zeros_like(b)).ref + link.bound()
        y = link.ref
    gc, be = f(head["gamma"]) * BN_C, f(head["beta"])
    e_x = ab(gc) * e_y + _base(2, ab(gc * y) + ab(be))
    x = np.maximum(gc * y + be, 0)
    W, bl = f(head["w"]), f(head["b"])
    lg = x @ W + bl
    e_l = e_x @ ab(W) + _base(x.shape[-1] + 1, ab(x) @ ab(W) + ab(bl))
    margin = lg[..., 1] - lg[..., 0]
    bound = e_l.sum(-1) + _base(0, ab(lg).sum(-1))
    N = margin.shape[1]
    margin[:, np.arange(N), np.arange(N)] = -1.0
    bound[:, np.arange(N), np.arange(N)] = 0.0
    return NS(margin=margin, bound=bound)


def margin_bar(z, layers, head):
    """NS(margin, bound, rule, e32): min(the derived rule, max(1e-5, 10 e32) max|margin|)
    per element (0 on the diagonal, which must be exactly -1); see the module text."""
    import torch
    r = margin_bound(z, layers, head)
    m32 = structure_literal(z, layers, head, torch.float32)[0].double().numpy()
    top = max(np.abs(r.margin).max(), 1e-30)
    e32 = np.abs(m32 - r.margin).max() / top
    return NS(margin=r.margin, rule=r.bound, e32=e32, bound=np.minimum(r.bound, max(1e-5, 10 * e32) * top))


# ---------------------------------------------------------------- operands of the C ABI test
# (id, B, N, D, hidden, pointer offset in floats, extra ldz)
DECODE_CASES = (
    ("n7", 2, 7, 3, (5, 4), 0, 0),
    ("n8_wide", 1, 8, 5, (33, 32), 0, 0),          # even N (asymmetric padding), a width over 32, the head at 32
    ("ref", 3, 25, 40, (50, 20), 0, 0),            # the synthetic2 widths
    ("one_layer", 2, 6, 4, (6,), 0, 0),            # layer 0 feeds the head
    ("three", 2, 5, 2, (9, 7, 5), 0, 0),           # both activations in use
    ("n1", 2, 1, 3, (4, 3), 0, 0),                 # only a diagonal
    ("n2", 1, 2, 3, (4, 3), 0, 0),
    ("many", 70, 5, 3, (5, 4), 0, 0),              # a graph-group tail (70 = 17 * 4 + 2)
    ("off1", 2, 7, 3, (5, 4), 1, 3),               # every pointer 4 bytes off 16-byte alignment, ldz = d + 3
)
ADJ_GUARD, ADJ_PATTERN = 64, 0xA5


def workspace_limit(B, N, Dz, hidden):
    """The workspace cap in bytes (include/snd_vae.h): two activations of the widest layer plus the weight image
    (padded to float4 lanes) and the 16 bytes of alignment slack."""
    up4 = lambda v: (v + 3) // 4 * 4
    return 2 * B * N * N * max(hidden) * 4 + N * 2 * up4(Dz) * up4(hidden[0]) * 4 + 16 + 32


def decode_operands(case, attempt):
    _, B, N, Dz, hidden, off, ldx = case
    rng = np.random.default_rng(A._seed(case[:4]) + list(hidden) + [attempt])
    c = NS(case=case, B=B, N=N, D=Dz, hidden=hidden, off=off, ldz=Dz + ldx)
    c.z = A._normal(rng, B, N, Dz)
    c.layers, cin = [], 2 * Dz
    for co in hidden:
        gamma, beta = 1 + 0.3 * A._normal(rng, cin), 0.3 * A._normal(rng, cin)
        gamma[::3] *= -1                            # negative gammas: relu kills where y is large
        c.layers.append({"gamma": gamma.astype(np.float32), "beta": beta,
                         "w": A._normal(rng, N, cin, co) / np.float32(np.sqrt(2 * N * cin)),
                         "b": 0.3 * A._normal(rng, co)})
        cin = co
    gamma, beta = 1 + 0.3 * A._normal(rng, cin), 0.3 * A._normal(rng, cin)
    gamma[::3] *= -1
    c.head = {"gamma": gamma.astype(np.float32), "beta": beta,
              "w": A._normal(rng, cin, 2) / np.float32(np.sqrt(cin)), "b": np.zeros(2, np.float32)}
    if N > 1:                                       # centre the off-diagonal margin: both classes occur
        m = margin_bound(c.z, c.layers, c.head).margin
        c.head["b"][1] = np.float32(-np.median(m[:, ~np.eye(N, dtype=bool)]))
    return c


def decode_setup(case):
    """Operands whose every off-diagonal argmax is decidable (|margin| over its bar in
    float64; redrawn otherwise) and, for N > 1, hold both classes."""
    for attempt in range(32):
        c = decode_operands(case, attempt)
        r = margin_bar(c.z, c.layers, c.head)
        offd = np.broadcast_to(~np.eye(c.N, dtype=bool), r.margin.shape)
        if (np.abs(r.margin[offd]) > r.bound[offd]).all():
            break
    else:
        raise AssertionError(f"decode {case[0]}: no decidable operands in 32 draws")
    c.ref, c.offd = r, offd
    if c.N > 1:
        pos = (r.margin[offd] > 0).mean()
        assert 0.0 < pos < 1.0, f"decode {case[0]}: one class only"
    B, N, o = c.B, c.N, c.off
    c.bufs = {"z": guarded(B * N, c.D, ld=c.ldz, offset=o, data=c.z, name="z"),
              "margin": vec(B * N * N, offset=o, name="margin")}
    for i, l in enumerate(c.layers):
        for k, v in l.items():
            c.bufs[f"l{i}_{k}"] = vec(v.size, offset=o, data=v, name=f"l{i}_{k}")
    for k, v in c.head.items():
        c.bufs[f"head_{k}"] = vec(v.size, offset=o, data=v, name=f"head_{k}")
    c.adj0 = np.full(ADJ_GUARD + 4 * o + B * N * N + ADJ_GUARD, ADJ_PATTERN, np.uint8)
    c.adj_off = ADJ_GUARD + 4 * o
    return c


def decode_verify(c, after, adj_after):
    """margin within the bar (an unwritten or NaN-fed element is an infinite ratio), adj
    exact, every guard intact; returns {output: ratio}."""
    m = c.bufs["margin"].values(after["margin"]).reshape(c.ref.margin.shape)
    n = c.B * c.N * c.N
    adj = adj_after[c.adj_off:c.adj_off + n].reshape(c.ref.margin.shape)
    guard = np.concatenate([adj_after[:c.adj_off], adj_after[c.adj_off + n:]])
    assert (guard == ADJ_PATTERN).all(), "adj: a guard byte changed"
    res = {"margin": A.assert_link("snd_e2e_decode margin",
                                   Link(c.ref.margin, np.zeros_like(c.ref.margin), 0, extra=c.ref.bound + 0.0), m)}
    want = (c.ref.margin > 0).astype(np.uint8)
    bad = np.argwhere(adj != want)
    assert bad.size == 0, f"snd_e2e_decode adj: element {tuple(bad[0])} got {adj[tuple(bad[0])]} " \
                          f"ref margin {c.ref.margin[tuple(bad[0])]!r} ({len(bad)} wrong)"
    A.check_guards(c, after)
    return res
