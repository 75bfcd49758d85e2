"""torch.autograd.Function wrappers over the C ABI (SURVEY §8b "Caller").

The reference builds its layers as TF graph ops and lets TF autodiff produce the
backward pass.  These wrappers give the same composability on torch tensors: each
forward and backward is one or a few libsndvae launches on the current stream
(no CPU path; a missing library raises), so a caller can assemble a model from the
reference's layers and call ``loss.backward()``.  The fused training step
(``snd_train_step``) remains the throughput path; these serve models the plan does
not cover and tests that compose the layers with torch code.

    spmm(rowptr, colidx, h)                      A @ h           (layers.py:122)
    linear(x, w, b)                              x @ w + b       (layers.py:566-576)
    graph_convolution(rowptr, colidx, x, w, gamma, beta)
                                                 BN(lrelu(A (x w))) (layers.py:115-125 + model.py:107)
    conv1d_same(x, w, b, gamma, beta, n_per_graph)
                                                 lrelu(BN(conv1d(x) + b)) (model_joint.py:115-116)
    reparameterize(mu, logstd, eps)              mu + eps e^logstd (model.py:153-159)
    inner_product_ce(z, rowptr, colidx, n_graphs) sum of the 2-class CE over all pairs
                                                 (layers.py:407-409, model.py:205-207, optimizer.py:142-144)

The adjacency is symmetric (input_data.py:62-67 asserts it), so A^T dY = A dY.
All tensors are contiguous float32 on the device; the index arrays int32.
"""
from __future__ import annotations

import torch

from . import _lib, ops

_P = _lib.ptr
_BNC = 1.0 / (1.0 + 1e-3) ** 0.5   # frozen Keras BN: gamma / sqrt(1 + eps)


class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rowptr, colidx, h):
        ops.f32("snd_vae_amd.autograd", h)
        ctx.save_for_backward(rowptr, colidx)
        return ops.spmm(rowptr, colidx, h)

    @staticmethod
    def backward(ctx, g):
        rowptr, colidx = ctx.saved_tensors
        return None, None, ops.spmm(rowptr, colidx, g.contiguous())


def spmm(rowptr, colidx, h):
    """A @ h over the block-diagonal CSR (tf.matmul(adj, x), layers.py:122)."""
    return _SpMM.apply(rowptr, colidx, h)


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ops.f32("snd_vae_amd.autograd", x, w, b)
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return ops.gemm(x, w, bias=b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        dx = ops.gemm(g, w, tb=True)                     # dx = g w^T
        dw = ops.gemm(x, g, ta=True)                     # dw = x^T g
        return dx, dw, (ops.colsum(g) if ctx.has_b else None)


def linear(x, w, b=None):
    """x @ w + b (linear, layers.py:566-576) on the MFMA GEMM, fp32."""
    return _Linear.apply(x, w, b)


class _GraphConvolution(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rowptr, colidx, x, w, gamma, beta):
        ops.f32("snd_vae_amd.autograd", x, w, gamma, beta)
        out, pre, _ = ops.spmm_gcn(rowptr, colidx, ops.gemm(x, w), gamma, beta)
        ctx.save_for_backward(rowptr, colidx, x, w, gamma, beta, pre)
        return out

    @staticmethod
    def backward(ctx, g):
        rowptr, colidx, x, w, gamma, beta, pre = ctx.saved_tensors
        dpre, dgamma, dbeta = ops.bn_act_bwd(g.contiguous(), pre, gamma, beta, ops.LRELU, True)   # BN(lrelu(.))
        dxw = ops.spmm(rowptr, colidx, dpre)                                                      # A^T = A
        dx = ops.gemm(dxw, w, tb=True)
        dw = ops.gemm(x, dxw, ta=True)
        return None, None, dx, dw, dgamma, dbeta


def graph_convolution(rowptr, colidx, x, w, gamma, beta):
    """BN(lrelu(A (x w))): GraphConvolution (layers.py:115-125, keep_prob 1) followed by
    the frozen Keras BN of model.py:107 (gamma = 1, beta = 0 for the plain layer)."""
    return _GraphConvolution.apply(rowptr, colidx, x, w, gamma, beta)


class _Conv1dSame(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, n_per_graph):
        ops.f32("snd_vae_amd.autograd", x, w, b, gamma, beta)
        out, pre = ops.conv1d_same(x, w, b, n_per_graph, gamma, beta)
        ctx.save_for_backward(x, w, gamma, beta, pre)
        ctx.npg = n_per_graph
        ctx.has_b = b is not None
        return out

    @staticmethod
    def backward(ctx, g):
        x, w, gamma, beta, pre = ctx.saved_tensors
        dpre, dgamma, dbeta = ops.bn_act_bwd(g.contiguous(), pre, gamma, beta, ops.LRELU, False)  # lrelu(BN(.))
        dx = ops.conv1d_same_bwd_data(dpre, w, ctx.npg)
        dw = ops.conv1d_same_bwd_weight(x, dpre, ctx.npg)
        return dx, dw, (ops.colsum(dpre) if ctx.has_b else None), dgamma, dbeta, None


def conv1d_same(x, w, b, gamma, beta, n_per_graph):
    """lrelu(BN(conv1d(x, k=5, SAME) + b)) over each graph's node axis
    (tf.layers.conv1d + Keras BN + lrelu, model_joint.py:115-116,138-139); w is the
    TF kernel [5][cin][cout]."""
    return _Conv1dSame.apply(x, w, b, gamma, beta, n_per_graph)


class _Reparameterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, logstd, eps):
        ops.f32("snd_vae_amd.autograd", mu, logstd, eps)
        ms = torch.cat([mu, logstd], 1).contiguous()
        ctx.save_for_backward(ms, eps)
        return ops.reparam_kl(ms, eps)[0]

    @staticmethod
    def backward(ctx, g):
        ms, eps = ctx.saved_tensors
        lat = eps.shape[1]
        dms = ops.reparam_bwd(ms, eps, g.contiguous())
        return dms[:, :lat], dms[:, lat:], None


def reparameterize(mu, logstd, eps):
    """z = mu + eps * exp(logstd) (get_z, model.py:153-159) with an injected eps."""
    return _Reparameterize.apply(mu, logstd, eps)


class _InnerProductCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, rowptr, colidx, n_graphs, pos_weight, norm):
        ops.f32("snd_vae_amd.autograd", z)
        rows, d = z.shape
        n = rows // n_graphs
        L = _lib.lib()
        wsb = L.snd_zzt_ce_workspace(n_graphs, n, d, 0)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=z.device)
        stats = torch.zeros(2, dtype=torch.float64, device=z.device)
        dz = torch.empty_like(z)
        _lib.check(L.snd_zzt_ce(_P(z), n_graphs, n, d, _P(rowptr), _P(colidx), pos_weight, norm, _P(stats),
                                _P(dz), _P(ws), wsb, 0, _lib.stream_ptr()), "snd_zzt_ce")
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(stats)
        return stats[0].float(), stats

    @staticmethod
    def backward(ctx, g, _):
        (dz,) = ctx.saved_tensors
        return dz * g, None, None, None, None, None


def inner_product_ce(z, rowptr, colidx, n_graphs, pos_weight=1.0, norm=1.0):
    """Sum over all B*N*N pairs of the 2-class softmax CE of the inner-product decoder
    (InnerProductDecoder, layers.py:407-409; diagonal rule model.py:205-207; CE
    optimizer.py:142-144), fp32, fused with its gradient.  Returns (ce_sum, stats) with
    stats = [ce_sum, #correct] in float64 (the accuracy of main.py:334 is
    stats[1] / (B N^2)); divide ce_sum by B N^2 for the reference's mean."""
    return _InnerProductCE.apply(z, rowptr, colidx, n_graphs, float(pos_weight), float(norm))
