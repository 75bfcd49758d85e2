"""Host wrappers of the stand-alone fp32 C ABI ops (include/snd_vae.h), one per entry point.

The only place Python marshals these entry points: ``layers``, ``autograd``, ``rowshard``
and ``disent_model`` call them through here, so a change at the C ABI is made once.  Every
wrapper takes its shapes from the tensors, allocates its outputs unless the caller passes
them, launches on the current stream (``_lib.stream_ptr()``) and reads nothing back.
Operands are float32 device tensors with unit column stride; a caller that passes a view of
a wider tensor (a column slice) gives its row stride as the matching ``ld*`` argument, which
defaults to the view's own width.  Absent pointers are ``None``, integers ``0``.
"""
from __future__ import annotations

import torch

from . import _lib

_P = _lib.ptr
F32 = 0                                 # SND_F32, the dtype argument's default
IDENT, RELU, LRELU = 0, 1, 2            # snd_bn_act_*'s act


def f32(name, *ts):
    """The operand check of every caller: contiguous float32 device tensors (None is skipped)."""
    for t in ts:
        if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise ValueError(f"{name}: expected a contiguous float32 device tensor")


def _new(like, *shape):
    return torch.empty(*shape, device=like.device)


def gemm(a, b, ta=False, tb=False, bias=None, out=None, lda=None, ldb=None, ldc=None, dtype=F32):
    """out[m, n] = op(a) op(b) (+ bias[n]) on MFMA (snd_gemm); a is [m, k], or [k, m] with ta,
    b [k, n], or [n, k] with tb.  dtype: the operands' MFMA format (fp32 accumulation)."""
    m, k = (a.shape[1], a.shape[0]) if ta else a.shape
    n = b.shape[0] if tb else b.shape[1]
    if out is None:
        out = _new(a, m, n)
    _lib.check(_lib.lib().snd_gemm(int(ta), int(tb), m, n, k, _P(a), a.shape[1] if lda is None else lda,
                                   _P(b), b.shape[1] if ldb is None else ldb, _P(out), n if ldc is None else ldc,
                                   _P(bias), dtype, _lib.stream_ptr()), "snd_gemm")
    return out


def colsum(g, out=None, ones=None, ld=None):
    """out[n] = sum over the rows of g [m, n] (1^T g on the GEMM: bias gradients).  ones: at
    least m ones the caller keeps; without it a fresh vector is filled per call."""
    m, n = g.shape
    if ones is None:
        ones = torch.ones(m, device=g.device)
    if out is None:
        out = _new(g, n)
    gemm(ones[:m].view(m, 1), g, ta=True, out=out.view(1, n), ldb=ld)
    return out


def spmm(rowptr, colidx, h, n_out=None):
    """A @ h over a CSR of n_out rows (default: h's; snd_csr_spmm, plain epilogue)."""
    rows, width = h.shape[0] if n_out is None else n_out, h.shape[1]
    out = _new(h, rows, width)
    _lib.check(_lib.lib().snd_csr_spmm(_P(rowptr), _P(colidx), rows, _P(h), width, width, _P(out), width, 0,
                                       None, None, None, 0, None, 0, 0, None, None, None, 0,
                                       _lib.stream_ptr()), "snd_csr_spmm")
    return out


def spmm_gcn(rowptr, colidx, xw, gamma, beta, concat_x=None, enc_gamma=None, enc_beta=None):
    """snd_csr_spmm with the GraphConvolution epilogue: preact = A @ xw,
    out = [BN(lrelu(preact)) | concat_x], out2 = BN_enc(out) when enc_gamma is given.
    Returns (out, preact, out2 or None)."""
    rows, width = xw.shape
    fx = 0 if concat_x is None else concat_x.shape[1]
    out, pre = _new(xw, rows, width + fx), _new(xw, rows, width)
    out2 = torch.empty_like(out) if enc_gamma is not None else None
    _lib.check(_lib.lib().snd_csr_spmm(_P(rowptr), _P(colidx), rows, _P(xw), width, width, _P(out), width + fx, 1,
                                       _P(gamma), _P(beta), _P(pre), width, _P(concat_x), fx, fx, _P(enc_gamma),
                                       _P(enc_beta), _P(out2), width + fx, _lib.stream_ptr()), "snd_csr_spmm")
    return out, pre, out2


def bn_act(y, gamma, beta, act, act_first, out=None, ldy=None, ldx=None):
    """Frozen BN with an activation: act(BN(y)), or BN(act(y)) with act_first (snd_bn_act_fwd)."""
    rows, c = y.shape
    if out is None:
        out = _new(y, rows, c)
    _lib.check(_lib.lib().snd_bn_act_fwd(_P(y), c if ldy is None else ldy, rows, c, _P(gamma), _P(beta), act,
                                         int(act_first), _P(out), c if ldx is None else ldx, _lib.stream_ptr()),
               "snd_bn_act_fwd")
    return out


def bn_act_bwd(dx, y, gamma, beta, act, act_first, dgamma=None, dbeta=None, lddx=None, ldy=None):
    """(dy, dgamma, dbeta) of bn_act at its input y [rows, c] (snd_bn_act_bwd); dx may be the
    first c columns of a wider tensor (lddx)."""
    rows, c = y.shape
    dy = _new(y, rows, c)
    dgamma = _new(y, c) if dgamma is None else dgamma
    dbeta = _new(y, c) if dbeta is None else dbeta
    _lib.check(_lib.lib().snd_bn_act_bwd(_P(dx), c if lddx is None else lddx, _P(y), c if ldy is None else ldy,
                                         rows, c, _P(gamma), _P(beta), act, int(act_first), _P(dy), c, _P(dgamma),
                                         _P(dbeta), _lib.stream_ptr()), "snd_bn_act_bwd")
    return dy, dgamma, dbeta


def conv1d_same(x, w, b, n_per_graph, gamma=None, beta=None, dtype=F32, ldx=None):
    """conv1d(k=5, SAME) over each graph's node axis, w [5, cin, cout] (snd_conv1d_same_fwd).
    Returns (out, y_pre): with gamma / beta out = lrelu(BN(y_pre)), else y_pre is None."""
    rows, cin = x.shape
    cout = w.shape[2]
    out = _new(x, rows, cout)
    pre = _new(x, rows, cout) if gamma is not None else None
    _lib.check(_lib.lib().snd_conv1d_same_fwd(_P(x), cin if ldx is None else ldx, rows, n_per_graph, cin, _P(w),
                                              cout, _P(b), _P(gamma), _P(beta), _P(pre), cout, _P(out), cout,
                                              dtype, _lib.stream_ptr()), "snd_conv1d_same_fwd")
    return out, pre


def conv1d_same_bwd_data(dy, w, n_per_graph, dtype=F32):
    """dx [rows, cin] of conv1d_same (snd_conv1d_same_bwd_data)."""
    rows, cout = dy.shape
    cin = w.shape[1]
    dx = _new(dy, rows, cin)
    _lib.check(_lib.lib().snd_conv1d_same_bwd_data(_P(dy), cout, rows, n_per_graph, cout, _P(w), cin, _P(dx), cin,
                                                   dtype, _lib.stream_ptr()), "snd_conv1d_same_bwd_data")
    return dx


def conv1d_same_bwd_weight(x, dy, n_per_graph, dtype=F32):
    """dw [5, cin, cout] of conv1d_same (snd_conv1d_same_bwd_weight and its workspace)."""
    rows, cin = x.shape
    cout = dy.shape[1]
    nws = _lib.lib().snd_conv1d_bwd_weight_workspace(rows, cin, cout)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)    # never a null pointer
    dw = _new(x, 5, cin, cout)
    _lib.check(_lib.lib().snd_conv1d_same_bwd_weight(_P(x), cin, _P(dy), cout, rows, n_per_graph, cin, cout,
                                                     _P(dw), _P(ws), nws, dtype, _lib.stream_ptr()),
               "snd_conv1d_same_bwd_weight")
    return dw


def sigmoid_mse(u, w, b, target, dw=None, db=None):
    """yhat = sigmoid(u w + b) against target with the mean over rows * cout (snd_sigmoid_mse).
    Returns (sse partials float64 [snd_sigmoid_mse_blocks], yhat, du, dw, db); the kernel adds
    to dw / db, so given ones accumulate and fresh ones start at zero."""
    rows, cin = u.shape
    cout = w.shape[1]
    nb = _lib.lib().snd_sigmoid_mse_blocks(rows)
    sse = torch.zeros(nb, dtype=torch.float64, device=u.device)
    yhat, du = _new(u, rows, cout), _new(u, rows, cin)
    dw = torch.zeros_like(w) if dw is None else dw
    db = torch.zeros_like(b) if db is None else db
    ws = _new(u, max(1, nb * (cin * cout + cout)))
    _lib.check(_lib.lib().snd_sigmoid_mse(_P(u), cin, rows, cin, _P(w), _P(b), cout, _P(target), cout, _P(sse),
                                          _P(yhat), _P(du), cin, _P(dw), _P(db), _P(ws), ws.numel() * 4,
                                          _lib.stream_ptr()), "snd_sigmoid_mse")
    return sse, yhat, du, dw, db


def sigmoid_linear(u, w, b):
    """sigmoid(u w + b), the forward half of sigmoid_mse (snd_sigmoid_linear_fwd)."""
    rows, cin = u.shape
    cout = w.shape[1]
    y = _new(u, rows, cout)
    _lib.check(_lib.lib().snd_sigmoid_linear_fwd(_P(u), cin, rows, cin, _P(w), _P(b), cout, _P(y), cout,
                                                 _lib.stream_ptr()), "snd_sigmoid_linear_fwd")
    return y


def reparam_kl(ms, eps):
    """z = mu + eps e^logstd over ms = [mu | logstd] rows with injected normals
    (snd_reparam_kl).  Returns (z, float64 partials whose sum is sum(1 + 2s - mu^2 - e^2s))."""
    rows, lat = eps.shape
    z = _new(ms, rows, lat)
    kl = torch.zeros(max(1, _lib.lib().snd_reparam_kl_blocks(rows, lat)), dtype=torch.float64, device=ms.device)
    _lib.check(_lib.lib().snd_reparam_kl(_P(ms), 2 * lat, rows, lat, _P(eps), 0, None, None, _P(z), _P(kl),
                                         _lib.stream_ptr()), "snd_reparam_kl")
    return z, kl


def reparam_bwd(ms, eps, dz, add_mu=None, add_logstd=None):
    """dms = [dz + add_mu | dz eps e^logstd + add_logstd] (snd_reparam_bwd)."""
    rows, lat = eps.shape
    dms = _new(ms, rows, 2 * lat)
    _lib.check(_lib.lib().snd_reparam_bwd(_P(ms), 2 * lat, rows, lat, _P(eps), _P(dz), _P(add_mu), _P(add_logstd),
                                          _P(dms), 2 * lat, _lib.stream_ptr()), "snd_reparam_bwd")
    return dms


def add_strided(x, y, alpha=1.0, ldx=None, ldy=None):
    """y[:, :cols] += alpha x over x's [rows, cols] block (snd_add_strided)."""
    rows, cols = x.shape
    _lib.check(_lib.lib().snd_add_strided(rows, cols, alpha, _P(x), cols if ldx is None else ldx, _P(y),
                                          cols if ldy is None else ldy, _lib.stream_ptr()), "snd_add_strided")
    return y


def e2e_train(z, adj, layers, head, dz, layer_grads, head_grads):
    """Forward, CE and every gradient of the e2e structure decoder in one call (snd_e2e_train,
    the factorised engine).  z [B, N, D], adj [B, N, N] float 0/1; layers / head: dicts of
    gamma, beta, w, b; dz, layer_grads, head_grads: destinations of the same shapes, written
    (not accumulated).  Returns out float64 [2] = {CE summed over B N^2, correct}, on the device."""
    import ctypes as C
    B, N, D = z.shape
    n = len(layers)
    L_ = _lib.lib()
    couts = (C.c_int * n)(*[int(lay["w"].shape[2]) for lay in layers])
    arr = (_lib.E2ELayer * n)(*[_lib.E2ELayer(_P(lay["gamma"]), _P(lay["beta"]), _P(lay["w"]), _P(lay["b"]),
                                              int(lay["w"].shape[2])) for lay in layers])
    garr = (_lib.E2ELayerGrad * n)(*[_lib.E2ELayerGrad(_P(g["gamma"]), _P(g["beta"]), _P(g["w"]), _P(g["b"]))
                                     for g in layer_grads])
    nbytes = int(L_.snd_e2e_train_workspace(B, N, D, couts, n))
    ws = torch.empty(max(nbytes, 16), device=z.device, dtype=torch.uint8)
    out = torch.empty(2, device=z.device, dtype=torch.float64)
    _lib.check(L_.snd_e2e_train(_P(z), D, _P(adj), B, N, D, arr, n, _P(head["gamma"]), _P(head["beta"]),
                                _P(head["w"]), _P(head["b"]), _P(dz), D, garr, _P(head_grads["gamma"]),
                                _P(head_grads["beta"]), _P(head_grads["w"]), _P(head_grads["b"]), _P(out), _P(ws),
                                ws.numel(), _lib.stream_ptr()), "snd_e2e_train")
    return out
