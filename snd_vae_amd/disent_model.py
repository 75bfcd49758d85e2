"""The reference's disentangled SND-VAE, assembled.

``SGCNModelVAE`` of `model.py:19-222` with the `optimizer.py:123-203` costs: three
encoders, three latents, three decoders --

* graph encoder (`model.py:104-115`): two GraphConvolution layers on adj_truth and
  the node features (BN after lrelu, the features concatenated back), BN
  encoder_g, flat heads g_g1_lin -> [g_g2_lin | g_g3_lin];
* spatial encoder (`model.py:119-129`): three conv1d(k=5, SAME) + BN + relu over the
  coordinates, BN encoder_s, flat heads g_s1..3_lin;
* spatial-graph encoder (`model.py:134-151`): two SpatialGraphConvolution layers over
  the B * sampling_num spanning-tree copies (lrelu after BN), BN encoder_sg, flat heads
  per copy g_sg1..3_lin; sg_conv_hidden entries of four widths select the three-hop
  SpatialGraphConvolution_3D of the 3-D datasets (`model.py:139-140`, spatial_dim 3);
* decoder (`model.py:172-222`): J_sg = mean over the copies of d_sg_lin1(z_sg)
  (`model.py:177,180`), J_s = d_s_lin1(z_s), J_g = d_g_lin1(z_g); node features from
  [J_sg | J_g] (conv1d + BN, no activation, x2; BN decoder_node; sigmoid(d_n_lin2)),
  the adjacency from [J_sg | J_g] through the e2e structure decoder
  (`disent.structure_decoder`), coordinates from [J_sg | J_s] (conv1d + BN x3,
  sigmoid(d_s_lin2));
* cost (`optimizer.py:142-203`): adj CE + node MSE + spatial MSE + the model_type's
  latent regularisers (`disent.disentangled_cost`), overall_loss in the reference order.

Every forward and backward operation is a HIP kernel of libsndvae.so reached through
the C ABI, the shared fp32 entry points by way of the host wrappers of ``ops.py`` (GEMM,
CSR SpMM with the GraphConvolution epilogue, conv1d, frozen-BN + activation,
SpatialGraphConvolution, reparameterisation, e2e, regularisers, sigmoid MSE heads, TF1
Adam); torch only allocates, views and copies device memory.  The
reference's scale is small (N = 25, B = 10, S = 10: `main.py:100,173-217`), so the
model is a host-ordered composition of launches, not a fused plan.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from types import SimpleNamespace as NS
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from .config import CONV_K
from .data import SGBatch
from .disent import ENGINES, group_weights, latent_reg, structure_decode, structure_decoder
from .layers import graph_convolution, spmm
from .params import _glorot_uniform, _truncated_normal
from .sg import SGGraph, layer_param_shapes, make_layer

_P = _lib.ptr


@dataclass(frozen=True)
class DisentangledConfig:
    """FLAGS of the synthetic2 dataset (`main.py:173-217`) the model reads."""
    n_nodes: int = 25
    num_feature: int = 1
    spatial_dim: int = 2
    g_conv_hidden: Tuple[int, ...] = (10, 20)                    # main.py:189
    g_hidden: int = 100                                          # g_hidden_size
    g_latent: int = 100
    s_channel: Tuple[int, ...] = (10, 10, 20)                    # main.py:181
    s_hidden: int = 100
    s_latent: int = 100
    # three widths per layer: SpatialGraphConvolution; four: SpatialGraphConvolution_3D, the
    # reference's 3-D datasets ([[10]*4, [20]*4] / [[20]*4, [50]*4], main.py:223,241)
    sg_conv_hidden: Tuple[Tuple[int, ...], ...] = ((20, 20, 20), (50, 50, 50))
    sg_hidden: int = 100
    sg_latent: int = 100
    sampling_num: int = 10                                       # main.py:100
    node_h: int = 20                                             # main.py:209
    n_d_channel: Tuple[int, ...] = (50, 20)                      # [:graph_deconv_layers]
    e_d_hidden: Tuple[int, ...] = (50, 20)                       # [:graph_deconv_layers]
    s_d_channel: Tuple[int, ...] = (50, 20, 10)
    model_type: str = "disentangled"                             # main.py:515
    beta: float = 1.0
    gamma: float = 1.0
    capacity: float = 0.0                                        # disentangled_C: C of the step
    learning_rate: float = 0.0008
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_eps: float = 1e-8

    def replace(self, **kw) -> "DisentangledConfig":
        import dataclasses
        return dataclasses.replace(self, **kw)


def _bn(shapes, name, c):
    shapes[name + "/gamma"] = (c,)
    shapes[name + "/beta"] = (c,)


def block_shapes(cfg: DisentangledConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """Variables by reference name (the mu / log-std heads of a group are one
    [hidden, 2 L] block '<..>23_lin' = [<..>2_lin | <..>3_lin])."""
    N, F, nh = cfg.n_nodes, cfg.num_feature, cfg.node_h
    s = OrderedDict()
    f = F
    for i, h in enumerate(cfg.g_conv_hidden):                    # layers.py:117-119
        s[f"g_g{i}_conv/w"] = (f, h)
        _bn(s, f"g_bn_g{i}", h)
        f = h + F
    _bn(s, "encoder_g", f)
    s["g_g1_lin/Matrix"], s["g_g1_lin/bias"] = (N * f, cfg.g_hidden), (cfg.g_hidden,)
    s["g_g23_lin/Matrix"], s["g_g23_lin/bias"] = (cfg.g_hidden, 2 * cfg.g_latent), (2 * cfg.g_latent,)
    c = cfg.spatial_dim
    for i, co in enumerate(cfg.s_channel):
        s[f"g_s{i + 1}_conv/kernel"], s[f"g_s{i + 1}_conv/bias"] = (CONV_K, c, co), (co,)
        _bn(s, f"g_bn_s{i}", co)
        c = co
    _bn(s, "encoder_s", c)
    s["g_s1_lin/Matrix"], s["g_s1_lin/bias"] = (N * c, cfg.s_hidden), (cfg.s_hidden,)
    s["g_s23_lin/Matrix"], s["g_s23_lin/bias"] = (cfg.s_hidden, 2 * cfg.s_latent), (2 * cfg.s_latent,)
    f = F
    for i, hid in enumerate(cfg.sg_conv_hidden):                 # SG layer + its BN (snd_sg / snd_sg3 layout)
        s[f"g_sg{i}_conv"] = (sum(int(np.prod(sh)) for _, sh in layer_param_shapes(f, hid)),)
        f = hid[-1]
    _bn(s, "encoder_sg", f)
    s["g_sg1_lin/Matrix"], s["g_sg1_lin/bias"] = (N * f, cfg.sg_hidden), (cfg.sg_hidden,)
    s["g_sg23_lin/Matrix"], s["g_sg23_lin/bias"] = (cfg.sg_hidden, 2 * cfg.sg_latent), (2 * cfg.sg_latent,)
    for g, lat in (("sg", cfg.sg_latent), ("s", cfg.s_latent), ("g", cfg.g_latent)):
        s[f"d_{g}_lin1/Matrix"], s[f"d_{g}_lin1/bias"] = (lat, N * nh), (N * nh,)
    c = 2 * nh
    for i, co in enumerate(cfg.n_d_channel):
        s[f"n{i}_deconv/kernel"], s[f"n{i}_deconv/bias"] = (CONV_K, c, co), (co,)
        _bn(s, f"d_bn_n{i}", co)
        c = co
    _bn(s, "decoder_node", c)
    s["d_n_lin2/Matrix"], s["d_n_lin2/bias"] = (c, F), (F,)
    c = 4 * nh                                                   # the pair [z_i | z_j] of [J_sg | J_g]
    for i, co in enumerate(cfg.e_d_hidden):
        _bn(s, f"d_bn_e{i}", c)
        s[f"e{i}_deconv/w1"], s[f"e{i}_deconv/biases1"] = (N, c, co), (co,)
        c = co
    _bn(s, "decoder_adj", c)
    s["d_e_lin2/Matrix"], s["d_e_lin2/bias"] = (c, 2), (2,)
    c = 2 * nh
    for i, co in enumerate(cfg.s_d_channel):
        s[f"s{i + 1}_deconv/kernel"], s[f"s{i + 1}_deconv/bias"] = (CONV_K, c, co), (co,)
        _bn(s, f"d_bn_s{i}", co)
        c = co
    s["d_s_lin2/Matrix"], s["d_s_lin2/bias"] = (c, cfg.spatial_dim), (cfg.spatial_dim,)
    return s


def init_blocks(cfg: DisentangledConfig, seed: int = 0) -> Dict[str, np.ndarray]:
    """The reference initialisers: GraphConvolution w and e2e w1 truncated-normal(0.02)
    (layers.py:119,435), linear Matrix N(0, 0.02) (layers.py:570), SG matrices
    N(0, 0.02) (layers.py:158-169,210-225), conv1d glorot-uniform, biases 0, BN gamma 1 beta 0."""
    rng = np.random.default_rng(seed)
    out = {}
    f = cfg.num_feature
    sg_in = {}
    for i, hid in enumerate(cfg.sg_conv_hidden):
        sg_in[f"g_sg{i}_conv"] = (f, hid)
        f = hid[-1]
    for k, shp in block_shapes(cfg).items():
        if k in sg_in:
            fi, hid = sg_in[k]
            parts = [rng.normal(0.0, 0.02, sh).reshape(-1) if n.startswith("Matrix")
                     else (np.ones(sh) if n == "gamma" else np.zeros(sh)).reshape(-1)
                     for n, sh in layer_param_shapes(fi, hid)]
            v = np.concatenate(parts)
        elif k.endswith("_conv/w") or k.endswith("/w1"):
            v = _truncated_normal(rng, shp, 0.02)
        elif k.endswith("/Matrix"):
            v = rng.normal(0.0, 0.02, shp)
        elif k.endswith("/kernel"):
            v = _glorot_uniform(rng, shp)
        elif k.endswith("/gamma"):
            v = np.ones(shp)
        else:
            v = np.zeros(shp)
        out[k] = v.astype(np.float64)
    return out


RELU, LRELU, IDENT = ops.RELU, ops.LRELU, ops.IDENT

# DisentangledSGCNModelVAE.losses (snd_disent_losses): optimizer.py:201's overall_loss, then
# main.py:334's count of correct adjacency entries
LOSS_NAMES = ("cost", "spatial_cost", "adj_cost", "node_cost", "kl_g", "kl_s", "kl_sg", "correct")


def latent_groups(cfg: DisentangledConfig, n_graphs: int):
    """(name, rows, latent) of the three latent groups, in the order a step walks them: one
    row per graph for s and g, one per spanning-tree copy for sg."""
    return (("s", n_graphs, cfg.s_latent), ("g", n_graphs, cfg.g_latent),
            ("sg", n_graphs * cfg.sampling_num, cfg.sg_latent))


class DisentangledSGCNModelVAE:
    """Parameters (one flat fp32 buffer), TF1 Adam state and the training step of the
    disentangled model for batches of ``n_graphs`` SGBatch graphs on one GPU, and its
    inference: ``encode``, ``decode`` (any number of graphs), ``generate`` (reconstruction,
    means, prior samples) and the latent traversals ``traverse`` / ``traverse_all``."""

    def __init__(self, cfg: DisentangledConfig, n_graphs: int, blocks: Optional[Dict[str, np.ndarray]] = None,
                 seed: int = 0, device="cuda", e2e_engine: str = "direct"):
        if not torch.cuda.is_available():
            raise _lib.SNDError("the disentangled model needs a ROCm GPU (no CPU fallback)")
        if e2e_engine not in ENGINES:
            raise ValueError(f"unknown e2e_engine {e2e_engine!r} (one of {ENGINES})")
        self.cfg, self.B, self.device = cfg, n_graphs, device
        self.e2e_engine = e2e_engine      # the training structure decoder; not part of the config (checkpoints)
        self.shapes = block_shapes(cfg)
        self.offsets, off = {}, 0
        for k, shp in self.shapes.items():
            self.offsets[k] = off
            off += -(-int(np.prod(shp)) // 64) * 64
        self.param_count = off
        self.params = torch.zeros(off, device=device)
        self.grads = torch.zeros(off, device=device)
        self.m = torch.zeros(off, device=device)
        self.v = torch.zeros(off, device=device)
        self.step_counter = torch.zeros(1, dtype=torch.int32, device=device)
        self.losses = torch.zeros(len(LOSS_NAMES), dtype=torch.float64, device=device)   # step_device()
        self.load_blocks(blocks if blocks is not None else init_blocks(cfg, seed))
        self._avgs = {}                                               # (B, S') -> the mean over S' copies
        self._avg = self._avg_matrix(n_graphs, cfg.sampling_num)
        self._ones = torch.ones(max(n_graphs * cfg.sampling_num * cfg.n_nodes, 1), device=device)   # colsum
        # (conv, BN) block names of the three conv1d + BN chains
        self.chains = {"enc_s": [(f"g_s{i + 1}_conv", f"g_bn_s{i}") for i in range(len(cfg.s_channel))],
                       "dec_n": [(f"n{i}_deconv", f"d_bn_n{i}") for i in range(len(cfg.n_d_channel))],
                       "dec_s": [(f"s{i + 1}_deconv", f"d_bn_s{i}") for i in range(len(cfg.s_d_channel))]}
        f = cfg.num_feature
        self.sg_layers = []
        for i, hid in enumerate(cfg.sg_conv_hidden):
            self.sg_layers.append(make_layer(f, hid, self.w(f"g_sg{i}_conv")))
            f = hid[-1]

    # ---- parameters
    def w(self, k):
        o = self.offsets[k]
        return self.params[o:o + int(np.prod(self.shapes[k]))].view(self.shapes[k])

    def g(self, k):
        o = self.offsets[k]
        return self.grads[o:o + int(np.prod(self.shapes[k]))].view(self.shapes[k])

    def load_blocks(self, blocks):
        flat = np.zeros(self.param_count, np.float32)
        for k, shp in self.shapes.items():
            o = self.offsets[k]
            flat[o:o + int(np.prod(shp))] = np.asarray(blocks[k], np.float32).reshape(-1)
        self.params.copy_(torch.from_numpy(flat))

    def blocks(self):
        flat = self.params.double().cpu().numpy()
        return {k: flat[self.offsets[k]:self.offsets[k] + int(np.prod(s))].reshape(s) for k, s in self.shapes.items()}

    def grad_blocks(self):
        flat = self.grads.double().cpu().numpy()
        return {k: flat[self.offsets[k]:self.offsets[k] + int(np.prod(s))].reshape(s) for k, s in self.shapes.items()}

    # ---- pieces shared by the step and the inference
    def _bn(self, name, y, act=IDENT):
        """act(BN_name(y)) (frozen Keras BN)."""
        return ops.bn_act(y, self.w(name + "/gamma"), self.w(name + "/beta"), act, False)

    def _bn_bwd(self, name, dx, y, act=IDENT, act_first=False):
        """dy of BN block ``name`` at its input y; its dgamma / dbeta go to the gradient buffer.
        dx may be wider than y (its first columns are read)."""
        return ops.bn_act_bwd(dx, y, self.w(name + "/gamma"), self.w(name + "/beta"), act, act_first,
                              dgamma=self.g(name + "/gamma"), dbeta=self.g(name + "/beta"), lddx=dx.shape[1])[0]

    def _colsum(self, dy, name):
        """Bias gradient ``name`` = sum over the rows of dy."""
        ops.colsum(dy, out=self.g(name), ones=self._ones)

    def _chain(self, h, names, act, keep=False):
        """conv1d(k=5, SAME) + BN + act per (conv, BN) block of ``names`` (model.py:119-129,
        189-191, 214-216).  Returns the output and, with ``keep``, each layer's (input, conv
        output) for ``_chain_bwd``."""
        kept = []
        for conv, bn in names:
            y = ops.conv1d_same(h, self.w(conv + "/kernel"), self.w(conv + "/bias"), self.cfg.n_nodes)[0]
            if keep:
                kept.append((h, y))
            h = self._bn(bn, y, act)
        return h, kept

    def _chain_bwd(self, d, kept, names, act):
        """Backward of ``_chain``: the blocks' gradients into the gradient buffer; returns the
        gradient at the chain's input."""
        for (conv, bn), (h, y) in zip(reversed(names), reversed(kept)):
            dy = self._bn_bwd(bn, d, y, act)
            d = ops.conv1d_same_bwd_data(dy, self.w(conv + "/kernel"), self.cfg.n_nodes)
            self.g(conv + "/kernel").copy_(ops.conv1d_same_bwd_weight(h, dy, self.cfg.n_nodes))
            self._colsum(dy, conv + "/bias")
        return d

    def _avg_matrix(self, B, S):
        """[B, B * S] with zbar = avg @ z_sg the mean over a graph's S copies (model.py:180)."""
        avg = self._avgs.get((B, S))
        if avg is None:
            a = np.zeros((B, B * S), np.float32)
            for b in range(B):
                a[b, b * S:(b + 1) * S] = 1.0 / S
            avg = self._avgs[(B, S)] = torch.from_numpy(a).to(self.device)
        return avg

    def _e2e_blocks(self, get):
        """(layers, head) dicts of ``disent.structure_decoder`` over the parameters (get =
        self.w) or their gradients (self.g)."""
        layers = [{"gamma": get(f"d_bn_e{i}/gamma"), "beta": get(f"d_bn_e{i}/beta"),
                   "w": get(f"e{i}_deconv/w1"), "b": get(f"e{i}_deconv/biases1")}
                  for i in range(len(self.cfg.e_d_hidden))]
        head = {"gamma": get("decoder_adj/gamma"), "beta": get("decoder_adj/beta"),
                "w": get("d_e_lin2/Matrix"), "b": get("d_e_lin2/bias")}
        return layers, head

    def _decoder_front(self, z, avg):
        """Latents {'s', 'g', 'sg'} to the decoders' inputs (model.py:172-184): J = d_*_lin1 of
        z_s, z_g and the mean of z_sg over the copies (``avg``; None: one copy per graph).
        Returns [J_sg | J_g], [J_sg | J_s] as [B * N, 2 node_h] and the projections' inputs
        {'sg': the mean, 's', 'g'}, which the backward reads."""
        N, nh = self.cfg.n_nodes, self.cfg.node_h
        R = z["s"].shape[0] * N
        zin = dict(z)
        if avg is not None:                                           # the mean commutes with d_sg_lin1
            zin["sg"] = ops.gemm(avg, z["sg"])
        J = {k: ops.gemm(zin[k], self.w(f"d_{k}_lin1/Matrix"), bias=self.w(f"d_{k}_lin1/bias")).view(R, nh)
             for k in ("sg", "s", "g")}
        Jsg_g, Jsg_s = (torch.empty(R, 2 * nh, device=self.device) for _ in range(2))
        Jsg_g[:, :nh].copy_(J["sg"]); Jsg_g[:, nh:].copy_(J["g"])
        Jsg_s[:, :nh].copy_(J["sg"]); Jsg_s[:, nh:].copy_(J["s"])
        return Jsg_g, Jsg_s, zin

    # ---- the three encoders (model.py:104-151), shared by step() and encode()
    def _head(self, name, feat, rows):
        """The flat heads <name>1_lin -> [<name>2_lin | <name>3_lin] over feat viewed as
        [rows, K]: (feat, hidden, ms) with ms = [mu | logstd] per row."""
        feat = feat.view(rows, -1)
        hh = ops.gemm(feat, self.w(f"{name}1_lin/Matrix"), bias=self.w(f"{name}1_lin/bias"))
        return feat, hh, ops.gemm(hh, self.w(f"{name}23_lin/Matrix"), bias=self.w(f"{name}23_lin/bias"))

    def _encoders(self, batch: "DeviceDisentBatch", B: int) -> NS:
        """Forward of the graph, spatial and spatial-graph encoders for a batch of B graphs,
        with everything the backward reads: gl (graph layers: input, preactivation), H (their
        output before BN encoder_g), sl / Us (the spatial chain's layers and output), sg_out,
        heads {'s' | 'g' | 'sg': (feat, hidden, ms)}."""
        cfg, e = self.cfg, NS(gl=[], heads={})
        # graph encoder (model.py:104-115)
        hin, n_g = batch.x, len(cfg.g_conv_hidden)
        for i in range(n_g):
            last = i + 1 == n_g
            res = graph_convolution(batch.rowptr, batch.colidx, hin, self.w(f"g_g{i}_conv/w"),
                                    self.w(f"g_bn_g{i}/gamma"), self.w(f"g_bn_g{i}/beta"), concat_x=batch.x,
                                    enc_gamma=self.w("encoder_g/gamma") if last else None,
                                    enc_beta=self.w("encoder_g/beta") if last else None)
            e.gl.append((hin, res[1]))
            hin = res[0]
        e.H = hin
        e.heads["g"] = self._head("g_g", res[2], B)                   # res[2]: BN encoder_g
        # spatial encoder (model.py:119-129)
        e.Us, e.sl = self._chain(batch.spatial, self.chains["enc_s"], RELU, keep=True)
        e.heads["s"] = self._head("g_s", self._bn("encoder_s", e.Us), B)
        # spatial-graph encoder (model.py:134-151) over the B*S copies
        e.sg_out = batch.x_sg
        for layer in self.sg_layers:
            e.sg_out, _ = layer.forward(batch.sg_graph, e.sg_out)
        e.heads["sg"] = self._head("g_sg", self._bn("encoder_sg", e.sg_out), B * cfg.sampling_num)
        return e

    # ---- one training step
    def step(self, batch: "DeviceDisentBatch", eps: Dict[str, torch.Tensor]) -> Dict[str, float]:
        """Forward, hand-chained backward and the TF1-Adam update of one batch
        (main.py:331); eps: {'s': [B, Ls], 'g': [B, Lg], 'sg': [B*S, Lsg]} normals.
        Returns the loss terms, read back from the device."""
        cfg, B = self.cfg, self.B
        (sse_n, n_count), (sse_s, s_count), ce, regs = self._step(batch, eps, cfg.capacity)
        node_cost = float(sse_n.sum().item()) / n_count
        o = ce.cpu().tolist()
        adj_cost, correct = o[0] / (B * cfg.n_nodes * cfg.n_nodes), o[1]
        spatial_cost = float(sse_s.sum().item()) / s_count
        reg, kls = 0.0, {}                                            # disent.disentangled_cost
        for name, r in regs.items():
            v = r.cpu().tolist()
            reg += v[1]
            kls[name] = v[0]
        cost = adj_cost + node_cost + spatial_cost + reg
        out = {"cost": cost, "spatial_cost": spatial_cost, "adj_cost": adj_cost, "node_cost": node_cost}
        if cfg.model_type != "base":                                  # overall_loss order
            out["kl_g"], out["kl_s"] = kls["g"], kls["s"]
        out["kl_sg"] = kls["sg"]
        out["correct"] = correct
        return out

    def step_device(self, batch: "DeviceDisentBatch", eps: Dict[str, torch.Tensor],
                    capacity: Optional[float] = None) -> None:
        """step() without a host synchronisation: the same launches in the same order, then
        snd_disent_losses writes ``self.losses`` (float64 [8], LOSS_NAMES: kl_g / kl_s are 0
        for 'base').  Nothing is read back, so the call can be captured in a HIP graph (after
        one eager call, which sizes the layers' workspaces).  capacity: C of
        'disentangled_C' for this step (None: cfg.capacity)."""
        cfg, B = self.cfg, self.B
        cap = cfg.capacity if capacity is None else float(capacity)
        (sse_n, n_count), (sse_s, s_count), ce, regs = self._step(batch, eps, cap)
        _lib.check(_lib.lib().snd_disent_losses(
            _P(sse_n), sse_n.numel(), float(n_count), _P(sse_s), sse_s.numel(), float(s_count), _P(ce),
            float(B * cfg.n_nodes * cfg.n_nodes), _P(regs.get("s")), _P(regs.get("g")), _P(regs["sg"]),
            _P(self.losses), _lib.stream_ptr()), "snd_disent_losses")

    def _step(self, batch: "DeviceDisentBatch", eps: Dict[str, torch.Tensor], cap: float):
        """The launches of one step, shared by step() and step_device(), stage by stage.
        Returns what the loss terms are made of, on the device: (sse partials, count) of the
        node and of the spatial head, snd_e2e_head_ce's {CE sum, correct} and snd_latent_reg's
        out[4] per group."""
        self.grads.zero_()
        e = self._encode_z(batch, eps)
        d = self._decode_losses(batch, e, cap)
        self._backward_encoders(batch, eps, e, d, self._backward_decoders(d))
        self._adam()
        return d.node_sse, d.spatial_sse, d.ce, d.regs

    def _encode_z(self, batch, eps) -> NS:
        """Stage 1: the encoders and get_z (model.py:153-161), z = mu + eps e^logstd per group."""
        e = self._encoders(batch, self.B)
        e.z = {k: ops.reparam_kl(e.heads[k][2], eps[k])[0] for k, _, _ in latent_groups(self.cfg, self.B)}
        return e

    def _sigmoid_head(self, u, wname, target):
        """sigmoid(linear) against target with its MSE: ((sse partials, count), du); the head's
        gradients are added into the (zeroed) gradient buffer."""
        sse, _, du, _, _ = ops.sigmoid_mse(u, self.w(wname + "/Matrix"), self.w(wname + "/bias"), target,
                                           dw=self.g(wname + "/Matrix"), db=self.g(wname + "/bias"))
        return (sse, target.numel()), du

    def _decode_losses(self, batch, e: NS, cap: float) -> NS:
        """Stage 2: the three decoders forward with their losses and the gradients the fused
        loss kernels leave (the sigmoid heads', the structure decoder's, the regularisers')."""
        cfg, B = self.cfg, self.B
        Jsg_g, Jsg_s, zin = self._decoder_front(e.z, self._avg)
        d = NS(zin=zin)
        # node decoder (model.py:186-191): conv + BN (no activation) x2, BN decoder_node, sigmoid head
        d.nu, d.nlay = self._chain(Jsg_g, self.chains["dec_n"], IDENT, keep=True)
        d.node_sse, d.dVn = self._sigmoid_head(self._bn("decoder_node", d.nu), "d_n_lin2", batch.x)
        # structure decoder (model.py:193-208) with its CE (optimizer.py:142-144)
        layers, head = self._e2e_blocks(self.w)
        glayers, ghead = self._e2e_blocks(self.g)
        if self.e2e_engine == "factorised":     # one call, written straight into the gradient buffer
            d.ce, d.dz_e, _, _ = structure_decoder(Jsg_g.view(B, cfg.n_nodes, 2 * cfg.node_h), batch.adj_dense,
                                                   layers, head, device_out=True, engine="factorised",
                                                   grads_out=(glayers, ghead))
        else:
            d.ce, d.dz_e, eg, hg = structure_decoder(Jsg_g.view(B, cfg.n_nodes, 2 * cfg.node_h), batch.adj_dense,
                                                     layers, head, device_out=True)
            for dst, src in zip(glayers + [ghead], eg + [hg]):
                for k in ("gamma", "beta", "w", "b"):
                    dst[k].copy_(src[k])
        # spatial decoder (model.py:212-219): conv + BN x3 on [J_sg | J_s], sigmoid head
        su, d.slay = self._chain(Jsg_s, self.chains["dec_s"], IDENT, keep=True)
        d.spatial_sse, d.dsu = self._sigmoid_head(su, "d_s_lin2", batch.spatial)
        # latent regularisers (optimizer.py:159-190), per group in the order their terms are added
        groups = {k: (e.heads[k][2][:, :lat].contiguous(), e.heads[k][2][:, lat:].contiguous(), e.z[k])
                  for k, _, lat in latent_groups(cfg, B)}
        d.regs, d.reg_grads = {}, {}
        for name, w in group_weights(cfg.model_type, cfg.beta, cfg.gamma, cap).items():
            d.regs[name], dmu_r, ds_r = latent_reg(*groups[name], device_out=True, **w)
            d.reg_grads[name] = (dmu_r, ds_r)
        return d

    def _backward_decoders(self, d: NS) -> Dict[str, torch.Tensor]:
        """Stage 3a: from the heads' gradients through the decoder chains, the concatenations
        and the d_*_lin1 projections to dz per group (reconstruction path)."""
        cfg, B = self.cfg, self.B
        N, nh = cfg.n_nodes, cfg.node_h
        R = B * N
        dJsg_g = self._chain_bwd(self._bn_bwd("decoder_node", d.dVn, d.nu), d.nlay, self.chains["dec_n"], IDENT)
        ops.add_strided(d.dz_e.view(R, 2 * nh), dJsg_g)
        dJsg_s = self._chain_bwd(d.dsu, d.slay, self.chains["dec_s"], IDENT)
        dJ = {k: torch.empty(R, nh, device=self.device) for k in ("sg", "g", "s")}
        dJ["sg"].copy_(dJsg_g[:, :nh]); dJ["g"].copy_(dJsg_g[:, nh:]); dJ["s"].copy_(dJsg_s[:, nh:])
        ops.add_strided(dJsg_s[:, :nh], dJ["sg"], ldx=2 * nh)
        # projections (d_*_lin1) and the mean over the copies
        dz = {}
        for k in ("sg", "s", "g"):
            dflat = dJ[k].view(B, N * nh)
            ops.gemm(d.zin[k], dflat, ta=True, out=self.g(f"d_{k}_lin1/Matrix"))
            self._colsum(dflat, f"d_{k}_lin1/bias")
            dz[k] = ops.gemm(dflat, self.w(f"d_{k}_lin1/Matrix"), tb=True)
        dz["sg"] = ops.gemm(self._avg, dz["sg"], ta=True)
        return dz

    def _backward_encoders(self, batch, eps, e: NS, d: NS, dz) -> None:
        """Stage 3b: the reparameterisation (dz plus the regularisers' gradients), the flat
        heads and the three encoders."""
        dfeat = {}
        for k, _, _ in latent_groups(self.cfg, self.B):
            feat, hh, ms = e.heads[k]
            dms = ops.reparam_bwd(ms, eps[k], dz[k], *d.reg_grads.get(k, (None, None)))
            ops.gemm(hh, dms, ta=True, out=self.g(f"g_{k}23_lin/Matrix"))
            self._colsum(dms, f"g_{k}23_lin/bias")
            dh = ops.gemm(dms, self.w(f"g_{k}23_lin/Matrix"), tb=True)
            ops.gemm(feat, dh, ta=True, out=self.g(f"g_{k}1_lin/Matrix"))
            self._colsum(dh, f"g_{k}1_lin/bias")
            dfeat[k] = ops.gemm(dh, self.w(f"g_{k}1_lin/Matrix"), tb=True)
        # spatial-graph encoder
        dsg = self._bn_bwd("encoder_sg", dfeat["sg"].view(e.sg_out.shape), e.sg_out)
        for i in range(len(self.sg_layers) - 1, -1, -1):
            gr, dsg = self.sg_layers[i].backward(dsg, want_dx=i > 0)
            self.g(f"g_sg{i}_conv").copy_(gr)
        # spatial encoder
        self._chain_bwd(self._bn_bwd("encoder_s", dfeat["s"].view(e.Us.shape), e.Us), e.sl, self.chains["enc_s"], RELU)
        # graph encoder (G = BN_enc(H2), H2 = [BN_1(lrelu(P1)) | x], ...)
        dH = self._bn_bwd("encoder_g", dfeat["g"].view(e.H.shape), e.H)
        for i in range(len(e.gl) - 1, -1, -1):
            hin, P = e.gl[i]
            dXW = spmm(batch.rowptr, batch.colidx, self._bn_bwd(f"g_bn_g{i}", dH, P, LRELU, True))   # A^T = A
            ops.gemm(hin, dXW, ta=True, out=self.g(f"g_g{i}_conv/w"))
            if i > 0:
                dH = ops.gemm(dXW, self.w(f"g_g{i}_conv/w"), tb=True)

    def _adam(self) -> None:
        """Stage 4: TF1 Adam (optimizer.py:125,197); the step counter is the TF global step."""
        cfg = self.cfg
        self.step_counter += 1
        _lib.check(_lib.lib().snd_adam_tf1(_P(self.params), _P(self.grads), _P(self.m), _P(self.v),
                                           self.param_count, cfg.learning_rate, cfg.adam_beta1, cfg.adam_beta2,
                                           cfg.adam_eps, 1.0, _P(self.step_counter), _lib.stream_ptr()),
                   "snd_adam_tf1")

    # ---- inference: encode, decode, generate, traverse (model.py:153-358)
    def _n_graphs(self, batch: "DeviceDisentBatch") -> int:
        B, rem = divmod(batch.x.numel(), self.cfg.n_nodes * self.cfg.num_feature)
        if rem or B < 1:
            raise ValueError("the batch's node features are not [B * n_nodes, num_feature]")
        return B

    def encode(self, batch: "DeviceDisentBatch", eps: Optional[Dict[str, torch.Tensor]] = None):
        """The three encoders (the forward half of step()): {'s' | 'g' | 'sg': {'mu', 'logstd'
        [, 'z']}}, rows [B, L] for s and g and per copy [B * S, Lsg] for sg (``mean_over_copies``
        averages them, main.py:407).  With eps = {'s': [B, Ls], 'g': [B, Lg], 'sg': [B*S, Lsg]}
        normals, z = mu + eps e^logstd (get_z, model.py:153-161) is included."""
        B = self._n_graphs(batch)
        heads = self._encoders(batch, B).heads
        out = {}
        for name, rows, lat in latent_groups(self.cfg, B):
            ms = heads[name][2]
            out[name] = {"mu": ms[:, :lat].contiguous(), "logstd": ms[:, lat:].contiguous()}
            if eps is not None:
                e = eps[name]
                if tuple(e.shape) != (rows, lat) or e.dtype != torch.float32 or not e.is_contiguous():
                    raise ValueError(f"encode: eps[{name!r}] must be contiguous float32 [{rows}, {lat}]")
                out[name]["z"] = ops.reparam_kl(ms, e)[0]
        return out

    def latent_groups_columns(self) -> Dict[str, slice]:
        """The column slices of ``latent_means``: {'s', 'g', 'sg'} in that order."""
        cfg = self.cfg
        a, b = cfg.s_latent, cfg.s_latent + cfg.g_latent
        return {"s": slice(0, a), "g": slice(a, b), "sg": slice(b, b + cfg.sg_latent)}

    def latent_means(self, batch: "DeviceDisentBatch", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The means of ``encode(batch)`` as one matrix [B, Ls + Lg + Lsg], columns in the
        order s, g, sg, the sg copies of a graph averaged as ``mean_over_copies`` does
        (main.py:407): what main.py:424 hands to disentangle_evaluation.  Written into
        ``out`` when one is given (float32, [B, Ls + Lg + Lsg], unit column stride: a row
        block of a caller-owned device matrix).  No read-back."""
        cfg = self.cfg
        B = self._n_graphs(batch)
        cols = self.latent_groups_columns()
        width = cols["sg"].stop
        if out is None:
            out = torch.empty(B, width, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, width)
                  and (width == 1 or out.stride(1) == 1)):
            raise ValueError(f"latent_means: out must be a float32 device tensor [{B}, {width}] with unit "
                             "column stride")
        enc = self.encode(batch)
        out[:, cols["s"]] = enc["s"]["mu"]
        out[:, cols["g"]] = enc["g"]["mu"]
        out[:, cols["sg"]] = mean_over_copies(enc["sg"]["mu"], cfg.sampling_num)
        return out

    def decode(self, z_s, z_sg, z_g, want_margin: bool = False) -> Dict[str, torch.Tensor]:
        """decoder(z_s, z_sg, z_g) of model.py:172-222 for any number of graphs B (not tied
        to the constructor's n_graphs): z_s [B, Ls], z_g [B, Lg], z_sg [B * S', Lsg] with J_sg
        averaged over the S' copies of a graph (model.py:177-180; S' = 1 for a traversal).
        Returns generated_adj uint8 [B, N, N] (the forward-only e2e decoder), generated_spatial
        [B, N, spatial_dim], generated_node_feat [B, N, F], and with want_margin the adjacency
        margin logit1 - logit0 [B, N, N]."""
        cfg = self.cfg
        N, F, nh = cfg.n_nodes, cfg.num_feature, cfg.node_h
        for t, lat, name in ((z_s, cfg.s_latent, "z_s"), (z_sg, cfg.sg_latent, "z_sg"), (z_g, cfg.g_latent, "z_g")):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2
                    and t.shape[1] == lat and t.shape[0] >= 1):
                raise ValueError(f"decode: {name} must be a contiguous float32 device tensor [rows, {lat}]")
        B = z_s.shape[0]
        Sp, rem = divmod(z_sg.shape[0], B)
        if z_g.shape[0] != B or rem or Sp < 1:
            raise ValueError(f"decode: z_s [{B}, Ls] needs z_g [{B}, Lg] and z_sg [{B} * S', Lsg], "
                             f"got {z_g.shape[0]} and {z_sg.shape[0]} rows")
        Jsg_g, Jsg_s, _ = self._decoder_front({"s": z_s, "g": z_g, "sg": z_sg},
                                              self._avg_matrix(B, Sp) if Sp > 1 else None)
        # node features (model.py:186-194)
        nu, _ = self._chain(Jsg_g, self.chains["dec_n"], IDENT)
        node = ops.sigmoid_linear(self._bn("decoder_node", nu), self.w("d_n_lin2/Matrix"), self.w("d_n_lin2/bias"))
        # adjacency (model.py:193-208)
        res = structure_decode(Jsg_g.view(B, N, 2 * nh), *self._e2e_blocks(self.w), want_margin=want_margin)
        # coordinates (model.py:212-219)
        su, _ = self._chain(Jsg_s, self.chains["dec_s"], IDENT)
        spatial = ops.sigmoid_linear(su, self.w("d_s_lin2/Matrix"), self.w("d_s_lin2/bias"))
        out = {"generated_adj": res[0] if want_margin else res,
               "generated_spatial": spatial.view(B, N, cfg.spatial_dim),
               "generated_node_feat": node.view(B, N, F)}
        if want_margin:
            out["margin"] = res[1]
        return out

    def generate(self, batch: "DeviceDisentBatch", z: str = "sample", eps: Optional[Dict[str, torch.Tensor]] = None,
                 seed: int = 0, want_margin: bool = False) -> Dict[str, torch.Tensor]:
        """Decode one of three latents of a batch: 'sample' get_z (reconstruction,
        test_reconstruct), 'mean' the encoder means, 'prior' get_random_z (model.py:163-169,
        test_generation).  The normals are the caller's eps ({'s': [B, Ls], 'g': [B, Lg],
        'sg': [B*S, Lsg]}) or drawn from a torch generator seeded with ``seed``.  Returns the
        decode() outputs plus z_mean_s / z_mean_g / z_mean_sg (main.py:361)."""
        if z not in ("sample", "mean", "prior"):
            raise ValueError(f"generate: z must be 'sample', 'mean' or 'prior', got {z!r}")
        cfg, B = self.cfg, self._n_graphs(batch)
        if eps is None and z != "mean":
            gen = torch.Generator(device=self.device)
            gen.manual_seed(int(seed))
            eps = {k: torch.randn(rows, lat, device=self.device, generator=gen)
                   for k, rows, lat in latent_groups(cfg, B)}
        enc = self.encode(batch, eps if z == "sample" else None)
        if z == "prior":
            for k, rows, lat in latent_groups(cfg, B):
                if tuple(eps[k].shape) != (rows, lat):
                    raise ValueError(f"generate: eps[{k!r}] must be [{rows}, {lat}]")
            lat = {k: eps[k] for k in ("s", "g", "sg")}
        else:
            lat = {k: enc[k]["z" if z == "sample" else "mu"] for k in ("s", "g", "sg")}
        out = self.decode(lat["s"], lat["sg"], lat["g"], want_margin=want_margin)
        for k in ("s", "g", "sg"):
            out[f"z_mean_{k}"] = enc[k]["mu"]
        return out

    def evaluate(self, batch: "DeviceDisentBatch", mode: str = "mean", out=None):
        """Edge-score counters (metrics.EdgeCounts) of the decoded batch against its adjacency:
        generate(z=mode, want_margin=True), then snd_margin_eval bins the e2e decoder's margin
        l1 - l0 against ``batch.adj_dense``.  The rule m > 0 is generated_adj's, so TP + FP is
        its number of ones.  mode: 'mean' (the encoder means) or 'sample'.  ``out``: an
        EdgeCounts over device tensors (EdgeCounts.zeros(B, device)) to add to and return, with
        no host synchronisation; None returns fresh counters."""
        from .layers import margin_eval
        from .metrics import EdgeCounts
        if mode not in ("mean", "sample"):
            raise ValueError(f"evaluate: mode must be 'mean' or 'sample', got {mode!r}")
        if out is not None and (not isinstance(out, EdgeCounts) or out.tensors is None):
            raise ValueError("evaluate: out must be an EdgeCounts over device tensors")
        gen = self.generate(batch, z=mode, want_margin=True)
        hist, counts = out.tensors if out is not None else (None, None)
        hist, counts = margin_eval(gen["margin"], batch.adj_dense, hist, counts, accumulate=out is not None)
        if out is not None:
            out.invalidate()
            return out
        return EdgeCounts(hist, counts)

    def _rows_to_device(self, rows):
        return [torch.from_numpy(np.ascontiguousarray(r, np.float32)).to(self.device) for r in rows]

    def traverse(self, group: str, dim: int, z_s, z_g, z_sg, values, want_margin: bool = False):
        """traverse(group_type, fix_dim) of model.py:232-265 without the file I/O: decode the
        V graphs of ``traverse_rows`` (dimension ``dim`` of ``group`` walks ``values``)."""
        zs, zg, zsg = self._rows_to_device(traverse_rows(group, dim, z_s, z_g, z_sg, values))
        return self.decode(zs, zsg, zg, want_margin=want_margin)

    def traverse_all(self, z_s, z_g, z_sg, values, chunk: int = 256, want_margin: bool = False):
        """traverse_latent of model.py:326-358: decode the (Ls + Lg + Lsg) V graphs of
        ``traverse_all_rows`` in chunks of at most ``chunk`` graphs (bounded memory) and
        concatenate them."""
        if chunk < 1:
            raise ValueError("traverse_all: chunk must be at least 1")
        zs, zg, zsg = traverse_all_rows(z_s, z_g, z_sg, values)
        parts = []
        for lo in range(0, zs.shape[0], chunk):
            a, b, c = self._rows_to_device((zs[lo:lo + chunk], zg[lo:lo + chunk], zsg[lo:lo + chunk]))
            parts.append(self.decode(a, c, b, want_margin=want_margin))
        return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


def mean_over_copies(z_sg, sampling_num: int):
    """[B * S, L] per-copy latents -> [B, L], the mean over a graph's S copies (main.py:407);
    numpy or torch."""
    rows = z_sg.shape[0]
    if sampling_num < 1 or rows % sampling_num:
        raise ValueError(f"{rows} rows are not a multiple of sampling_num {sampling_num}")
    return z_sg.reshape(rows // sampling_num, sampling_num, -1).mean(1)


def _traverse_args(z_s, z_g, z_sg, values):
    base = [np.atleast_2d(np.asarray(a, np.float32)) for a in (z_s, z_g, z_sg)]
    length = sum(a.shape[1] for a in base)
    M = base[0].shape[0]
    if any(a.ndim != 2 or a.shape[0] != M for a in base) or M not in (1, length):
        raise ValueError(f"traverse: base latents need 1 or Ls + Lg + Lsg = {length} rows each")
    if isinstance(values, dict):
        vals = [np.asarray(values[k], np.float32).reshape(-1) for k in ("s", "g", "sg")]
    else:
        vals = [np.asarray(values, np.float32).reshape(-1)] * 3
    V = vals[0].size
    if V < 1 or any(v.size != V for v in vals):
        raise ValueError("traverse: values needs at least one entry, the same count for every group")
    return base, vals, length, V


def traverse_all_rows(z_s, z_g, z_sg, values):
    """The latent rows of traverse_latent (model.py:326-358), on the host.

    Base latents z_s [M, Ls], z_g [M, Lg], z_sg [M, Lsg] with M = 1 (one base for every
    block) or M = Ls + Lg + Lsg (base k for block k, as the reference's saved latents);
    ``values``: V entries, or {'s' | 'g' | 'sg': V entries} per group.  Block k is V copies
    of its base with one dimension overwritten by ``values``: blocks 0 .. Ls-1 walk the
    dimensions of z_s, the next Lg those of z_g, the last Lsg those of z_sg
    (model.py:339-349).  Returns float32 (z_s, z_g, z_sg) of (Ls + Lg + Lsg) V rows each;
    one z_sg row per graph (S' = 1)."""
    base, vals, length, V = _traverse_args(z_s, z_g, z_sg, values)
    rows = [np.repeat(np.broadcast_to(a, (length, a.shape[1])), V, axis=0).copy() for a in base]
    k = 0
    for r, v in zip(rows, vals):
        for dim in range(r.shape[1]):
            r[k * V:(k + 1) * V, dim] = v
            k += 1
    return tuple(rows)


def traverse_rows(group: str, dim: int, z_s, z_g, z_sg, values):
    """The V rows of one block of ``traverse_all_rows`` (traverse, model.py:232-265):
    dimension ``dim`` of ``group`` ('s', 'g' or 'sg') walks ``values``, everything else
    stays at the block's base."""
    base, vals, length, V = _traverse_args(z_s, z_g, z_sg, values)
    if group not in ("s", "g", "sg"):
        raise ValueError(f"traverse: group must be 's', 'g' or 'sg', got {group!r}")
    gi = ("s", "g", "sg").index(group)
    if not 0 <= dim < base[gi].shape[1]:
        raise ValueError(f"traverse: dim {dim} outside group {group!r} of {base[gi].shape[1]} dimensions")
    k = sum(a.shape[1] for a in base[:gi]) + dim
    rows = [np.repeat(a[k:k + 1] if a.shape[0] > 1 else a, V, axis=0).copy() for a in base]
    rows[gi][:, dim] = vals[gi]
    return tuple(rows)


class DeviceDisentBatch:
    """An SGBatch on the device for the disentangled model: adj_truth (CSR and dense for
    the e2e CE), node features and coordinates per graph, the copies' features, trees
    and rel (the feeds of main.py:253-264)."""

    def __init__(self, batch: SGBatch, device="cuda"):
        t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)
        B, N = batch.n_graphs, batch.n_nodes
        self.rowptr = t(batch.rowptr, torch.int32)
        self.colidx = t(batch.colidx if batch.nnz else np.zeros(1, np.int32), torch.int32)
        self.x = t(batch.feature_truth)
        self.spatial = t(batch.spatial_truth)
        self.adj_dense = t(np.stack([batch.dense_adj(b) for b in range(B)]))
        self.x_sg = t(batch.features)
        self.rel = t(batch.rel)
        self.sg_graph = SGGraph(batch.tree_rowptr, batch.tree_colidx, N, self.rel)
