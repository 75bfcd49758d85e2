"""Training loop of the disentangled model: the `main.py:296-353` train branch for
``DisentangledSGCNModelVAE`` (`main.py:72,505`), with what `main.py:374-469` reports.

The split is uploaded once (one ``DeviceDisentBatch`` per batch of ``batch_size`` graphs).
A step is ``step_device``: no host synchronisation, the loss terms left in
``model.losses``.  With ``use_graphs`` each batch's step is captured into its own HIP graph
on first use and replayed afterwards; all captures share one memory pool, since they replay
one at a time and only ``model.losses`` and the training state, both allocated outside the
graphs, are read afterwards.  ``use_graphs`` is off by default: at the reference's scale the
step is bound by its kernels, not by its launches (12.7 ms either way on one MI355X,
`tools/disent_step_timing.py`), so a replay buys nothing over the eager ``step_device`` and
costs a capture per batch.  The reparameterisation normals of global step t are a pure
function of (seed, t), drawn into three static buffers outside the graph: an eager, a
replayed and a resumed run see the same numbers.  The loss terms are copied into a device
history that is read back once per epoch.
"""
from __future__ import annotations

import math
import os
import time
from typing import Dict, List, Optional

import numpy as np
import torch

from . import checkpoint as ckpt
from . import layers
from .config import sgjoint
from .disent import capacity
from .disent_model import (LOSS_NAMES, DeviceDisentBatch, DisentangledConfig, DisentangledSGCNModelVAE,
                           latent_groups)
from .input_data import SynDataset, dataset_sg_batch

# storer keys of main.py:335-345 -> LOSS_NAMES ('base' reports sg_kl only; adj_acc is derived)
STORER = (("loss", "cost"), ("spatial_loss", "spatial_cost"), ("adj_loss", "adj_cost"),
          ("node_loss", "node_cost"), ("graph_kl", "kl_g"), ("spatial_kl", "kl_s"), ("sg_kl", "kl_sg"))


def eps_shapes(cfg: DisentangledConfig, n_graphs: int) -> Dict[str, tuple]:
    """The normals one step reads: {'s': [B, Ls], 'g': [B, Lg], 'sg': [B*S, Lsg]}."""
    return {k: (rows, lat) for k, rows, lat in latent_groups(cfg, n_graphs)}


def _step_seed(seed: int, t: int) -> int:
    """(seed, t) mixed into one generator seed (splitmix64's finaliser): every bit depends on
    both, as a generator may keep only the low 32."""
    m64 = (1 << 64) - 1
    x = ((int(seed) & m64) * 0x9E3779B97F4A7C15 + (int(t) & m64) + 1) & m64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m64
    return (x ^ (x >> 31)) & ((1 << 63) - 1)


def draw_step_eps(seed: int, t: int, out: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Fill ``out`` (s, g, sg in that order) with the normals of global step t: a generator
    on the buffers' device seeded with (seed, t), so the draw depends on nothing else."""
    dev = out["s"].device
    gen = torch.Generator(device=dev)
    gen.manual_seed(_step_seed(seed, t))
    for k in ("s", "g", "sg"):
        out[k].normal_(generator=gen)
    return out


def dataset_factors(dataset: SynDataset, n_graphs: Optional[int] = None) -> np.ndarray:
    """``dataset.factor`` as float32 [n_graphs, K] (every graph by default), for
    ``evaluate_disentanglement``.  ValueError when the dataset has no factors, when they are
    not 2-D, or when their row count differs from the dataset's graphs: a test split reads
    the training split's factor file (`input_data.py:101`), and no alignment is guessed."""
    f = dataset.factor
    if f is None:
        raise ValueError("the dataset has no generative factors (2D_prop.npy was absent)")
    f = np.asarray(f)
    if f.ndim != 2 or f.shape[1] < 1:
        raise ValueError(f"dataset.factor must be [n_graphs, K], got shape {f.shape}")
    if f.shape[0] != dataset.n_graphs:
        raise ValueError(f"dataset.factor has {f.shape[0]} rows for {dataset.n_graphs} graphs (a test split "
                         "carries the training split's factors, input_data.py:101); no alignment is guessed")
    n = dataset.n_graphs if n_graphs is None else n_graphs
    return np.ascontiguousarray(f[:n], dtype=np.float32)


class DisentTrainer:
    def __init__(self, cfg: DisentangledConfig, dataset: SynDataset, batch_size: int, seed: int = 1234,
                 use_graphs: bool = False, blocks=None, device="cuda", c_max: Optional[float] = None,
                 c_step: int = 20, c_stop_iter: int = 100, e2e_engine: str = "direct"):
        """e2e_engine: the model's training structure decoder ("direct" or "factorised"; not
        part of the config, so checkpoints restore under either).
        c_max / c_step / c_stop_iter: the capacity schedule of 'disentangled_C'
        (`optimizer.py:167`, global_iter = the epoch, `main.py:329`); c_max None keeps
        cfg.capacity for every epoch."""
        self.cfg, self.batch_size, self.seed = cfg, batch_size, seed
        self.batch_num = dataset.n_graphs // batch_size           # main.py:312
        if self.batch_num < 1:
            raise ValueError(f"{dataset.n_graphs} graphs < batch_size {batch_size}")
        data_cfg = sgjoint(cfg.n_nodes, cfg.node_h, sampling_num=cfg.sampling_num,
                           num_feature=cfg.num_feature, spatial_dim=cfg.spatial_dim)
        self.batches: List[DeviceDisentBatch] = [
            DeviceDisentBatch(dataset_sg_batch(dataset, data_cfg, range(i * batch_size, (i + 1) * batch_size)),
                              device=device)
            for i in range(self.batch_num)]
        self.model = DisentangledSGCNModelVAE(cfg, batch_size, blocks=blocks, seed=seed, device=device,
                                              e2e_engine=e2e_engine)
        self.dataset = dataset                # evaluate_disentanglement reads dataset.factor
        self.eps = {k: torch.empty(*shp, device=device) for k, shp in eps_shapes(cfg, batch_size).items()}
        self.use_graphs = use_graphs
        self.c_max, self.c_step, self.c_stop_iter = c_max, c_step, c_stop_iter
        self._cap = cfg.capacity              # C of the captured graphs
        self._graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self._pool = None
        self._warm = False
        self.epoch = 0
        self.global_step = 0                  # steps taken: the t of the next step's normals
        self.history: List[Dict[str, np.ndarray]] = []

    # --------------------------------------------------------------- one step
    def _tensors(self):
        m = self.model
        return (m.params, m.m, m.v, m.step_counter, m.grads, m.losses)

    def _capture(self, i: int):
        """HIP graph of batch i's step at the current C; the training state is left untouched."""
        saved = [t.clone() for t in self._tensors()]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            if not self._warm:          # kernel attributes, the layers' workspaces: set up eagerly
                # A three-hop layer sizes its workspace by the batch's trees and regrows it on a
                # larger batch; a graph captured before that would keep the freed pointer.  So
                # every batch runs once before the first capture; two-hop layers need one.
                three_hop = any(len(h) == 4 for h in self.cfg.sg_conv_hidden)
                for b in (self.batches if three_hop else [self.batches[i]]):
                    self.model.step_device(b, self.eps, capacity=self._cap)
                self._warm = True
        torch.cuda.current_stream().wait_stream(s)
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self._pool):
            self.model.step_device(self.batches[i], self.eps, capacity=self._cap)
        torch.cuda.synchronize()
        for dst, src in zip(self._tensors(), saved):
            dst.copy_(src)
        self._graphs[i] = g
        return g

    def step(self, i: int):
        """One training step on batch i (its loss terms are in ``model.losses`` afterwards)."""
        draw_step_eps(self.seed, self.global_step, self.eps)
        if self.use_graphs:
            (self._graphs.get(i) or self._capture(i)).replay()
        else:
            self.model.step_device(self.batches[i], self.eps, capacity=self._cap)
        self.global_step += 1

    def _set_capacity(self):
        """C of this epoch; graphs captured under another C are dropped (C is baked into
        snd_latent_reg's arguments), at most c_stop_iter / c_step + 1 times in a run."""
        if self.cfg.model_type != "disentangled_C" or self.c_max is None:
            return
        c = capacity(self.epoch, self.c_max, self.c_step, self.c_stop_iter)
        if c != self._cap:
            self._graphs.clear()
            self._pool = None           # the pool went with its last graph: the recaptures share a new one
            self._cap = c

    # ------------------------------------------------------------------ epochs
    def train_epoch(self, verbose: bool = False) -> Dict[str, np.ndarray]:
        """One pass over the batches.  Returns (and appends to ``history``) the epoch's storer:
        per step loss, spatial_loss, adj_loss, adj_acc, node_loss, graph_kl, spatial_kl, sg_kl
        (`main.py:335-345`; 'base' has sg_kl only), plus epoch_time and the capacity C used."""
        self._set_capacity()
        hist = torch.zeros(self.batch_num, len(LOSS_NAMES), dtype=torch.float64, device=self.model.losses.device)
        t0 = time.time()
        for i in range(self.batch_num):
            self.step(i)
            hist[i].copy_(self.model.losses)
        h = hist.cpu().numpy()
        base = self.cfg.model_type == "base"
        storer = {key: h[:, LOSS_NAMES.index(name)].copy() for key, name in STORER
                  if not (base and key in ("graph_kl", "spatial_kl"))}
        storer["adj_acc"] = h[:, LOSS_NAMES.index("correct")] / (self.batch_size * self.cfg.n_nodes ** 2)
        storer["epoch_time"] = np.array([time.time() - t0])
        storer["capacity"] = np.array([self._cap])
        self.history.append(storer)
        if verbose:
            print("Epoch:", "%04d" % (self.epoch + 1), "loss=", "{:.5f}".format(storer["loss"][-1]),
                  "time=", "{:.5f}".format(storer["epoch_time"][0]))
        self.epoch += 1
        return storer

    def train(self, epochs: int, checkpoint_dir: Optional[str] = None, save_every: int = 100,
              verbose: bool = False) -> List[Dict[str, np.ndarray]]:
        """`main.py:310-353`; checkpoints after epochs 0, save_every, ..."""
        out = []
        for _ in range(epochs):
            e = self.epoch
            out.append(self.train_epoch(verbose))
            if checkpoint_dir and e % save_every == 0:
                os.makedirs(checkpoint_dir, exist_ok=True)
                self.save(os.path.join(checkpoint_dir, f"model_dgt_global_{e}.safetensors"))
        return out

    def save(self, path: str):
        ckpt.save(path, self.model, self.model, epoch=self.epoch)

    def restore(self, path: str):
        """Parameters, Adam state, global step and epoch of ``save``; returns the global step."""
        step = ckpt.restore(path, self.model, self.model)
        epoch = ckpt.read_epoch(path)
        if step is None or epoch is None:
            raise ValueError(f"{path}: holds no training state (Adam moments, global step, epoch)")
        self.global_step, self.epoch = step, epoch
        return step

    # -------------------------------------------------------------- evaluation
    def evaluate(self, mode: str = "mean") -> dict:
        """Link-prediction metrics of the current parameters over every batch
        (metrics.EdgeCounts.summary: accuracy, precision, recall, F1, ROC-AUC, average
        precision, the best-F1 threshold on the e2e decoder's margin) plus the summed counters
        under "edge_counts", and node_mse / spatial_mse of the reconstruction against the
        truths (`main.py:423`).  Forward passes only, outside the captured step graphs; all
        batches add into one device buffer that is read back once.  Parameters, Adam state and
        the step counter are not written."""
        from .metrics import EdgeCounts
        if mode not in ("mean", "sample"):
            raise ValueError(f"evaluate: mode must be 'mean' or 'sample', got {mode!r}")
        dev = self.model.params.device
        buf = EdgeCounts.zeros(self.batch_size, device=dev)
        sse = torch.zeros(2, dtype=torch.float64, device=dev)
        for b in self.batches:
            gen = self.model.generate(b, z=mode, want_margin=True)
            layers.margin_eval(gen["margin"], b.adj_dense, *buf.tensors, accumulate=True)
            sse[0] += (gen["generated_node_feat"].reshape(-1).double() - b.x.reshape(-1).double()).square().sum()
            sse[1] += (gen["generated_spatial"].reshape(-1).double() - b.spatial.reshape(-1).double()).square().sum()
        buf.invalidate()
        tot = buf.total()
        out = tot.summary()
        out["edge_counts"] = tot
        node, spatial = sse.cpu().tolist()
        rows = self.batch_num * self.batch_size * self.cfg.n_nodes
        out["node_mse"] = node / (rows * self.cfg.num_feature)
        out["spatial_mse"] = spatial / (rows * self.cfg.spatial_dim)
        return out

    PATH_DETOUR_SCALE = 64.0     # detour bins per unit of route / straight line - 1: 256 bins over [0, 4)

    def evaluate_generation(self, mode: str = "prior", threshold: Optional[float] = None,
                            inclusive: bool = True, seed: int = 0, paths: bool = False,
                            src_step: int = 1, motifs: bool = False, spectrum: bool = False,
                            crossings: bool = False) -> dict:
        """Do generated graphs look like the data?  For every batch the graph statistics
        (metrics.GraphStats) of the batch itself (its CSR and coordinates) and of a graph
        generated at its shape: mode "prior" decodes z ~ N(0, 1) (test_generation,
        `main.py:467`; batch i draws from a generator seeded with seed + i), "mean" the
        batch's reconstruction (`main.py:423`).  An edge is margin >= ``threshold`` off the
        diagonal (> without ``inclusive``); None takes ``evaluate()["best_f1_threshold"]``
        ("mean" for either mode: a prior sample has no truth to tune on).  The generated
        statistics use the generated coordinates.

        Returns ``dataset.compare(generated)`` plus the two GraphStats under "dataset" and
        "generated", the threshold used and the generated graphs' (rowptr, colidx) per batch
        under "generated_csr".  Forward passes only; parameters, Adam state and the step
        counter are not written.

        paths=True adds "paths": the ``metrics.PathStats.compare`` (components, hop distances,
        detour; every ``src_step``-th node a source, PATH_DETOUR_SCALE detour bins per unit) of
        the same two sets of graphs, with the two PathStats under its "dataset" and "generated".

        motifs=True adds "motifs": the ``metrics.MotifStats.compare`` (orbit MMD, mean 4-node
        graphlet frequencies) of the same two sets (``layers.graph_motifs``; a thresholded margin
        may be asymmetric: its one-way arcs are no edges), with the two MotifStats under its
        "dataset" and "generated".

        spectrum=True adds "spectrum": the ``metrics.SpectrumStats.compare`` (MMD and KL
        divergence of the spectral densities of the normalised Laplacian;
        ``layers.graph_spectrum`` at its defaults) of the same two sets, with the two
        SpectrumStats under its "dataset" and "generated".

        crossings=True (spatial_dim 2) adds "crossings": the ``metrics.CrossingStats.compare``
        (edge crossings as drawn, edge directions, crossing angles; ``layers.graph_crossings``
        at its default work_cap) of the same two sets, each at its own coordinates, with the
        two CrossingStats under its "dataset" and "generated"."""
        from .metrics import CrossingStats, GraphStats, MotifStats, PathStats, SpectrumStats
        if crossings and self.cfg.spatial_dim != 2:
            raise ValueError(f"evaluate_generation: crossings=True needs spatial_dim 2, got {self.cfg.spatial_dim}")
        if mode not in ("prior", "mean"):
            raise ValueError(f"evaluate_generation: mode must be 'prior' or 'mean', got {mode!r}")
        if threshold is None:
            threshold = self.evaluate("mean")["best_f1_threshold"]
            if threshold != threshold:                  # no positive anywhere: nothing to tune on
                raise ValueError("evaluate_generation: the dataset has no edge to choose a threshold by")
        B, N, sd = self.batch_size, self.cfg.n_nodes, self.cfg.spatial_dim
        max_len = math.sqrt(sd)
        scale = self.PATH_DETOUR_SCALE
        data, gen, csr, pdata, pgen, mdata, mgen, sdata, sgen = [], [], [], [], [], [], [], [], []
        xdata, xgen = [], []
        for i, b in enumerate(self.batches):
            data.append(GraphStats(*layers.graph_stats(b.rowptr, b.colidx, B, N, b.spatial, max_len), N, max_len))
            if paths:
                pdata.append(PathStats(*layers.graph_paths(b.rowptr, b.colidx, B, N, b.spatial, scale, src_step),
                                       N, scale, src_step))
            if motifs:
                mdata.append(MotifStats(layers.graph_motifs(b.rowptr, b.colidx, B, N)[0], N))
            if spectrum:
                sdata.append(SpectrumStats(*layers.graph_spectrum(b.rowptr, b.colidx, B, N), N))
            if crossings:
                xdata.append(CrossingStats(*layers.graph_crossings(b.rowptr, b.colidx, B, N, b.spatial)[:2], N))
            out = self.model.generate(b, z=mode, seed=seed + i, want_margin=True)
            m = out["margin"]
            dense = ((m >= threshold) if inclusive else (m > threshold)).float()   # the diagonal is ignored
            rowptr, colidx = layers.dense_to_csr(dense)
            coords = out["generated_spatial"].reshape(B * N, sd)
            gen.append(GraphStats(*layers.graph_stats(rowptr, colidx, B, N, coords, max_len), N, max_len))
            if paths:
                pgen.append(PathStats(*layers.graph_paths(rowptr, colidx, B, N, coords, scale, src_step),
                                      N, scale, src_step))
            if motifs:
                mgen.append(MotifStats(layers.graph_motifs(rowptr, colidx, B, N)[0], N))
            if spectrum:
                sgen.append(SpectrumStats(*layers.graph_spectrum(rowptr, colidx, B, N), N))
            if crossings:
                xgen.append(CrossingStats(*layers.graph_crossings(rowptr, colidx, B, N, coords)[:2], N))
            csr.append((rowptr, colidx))
        data, gen = GraphStats.concat(data), GraphStats.concat(gen)
        out = data.compare(gen)
        out.update(dataset=data, generated=gen, threshold=threshold, generated_csr=csr)
        if paths:
            pdata, pgen = PathStats.concat(pdata), PathStats.concat(pgen)
            out["paths"] = dict(pdata.compare(pgen), dataset=pdata, generated=pgen)
        if motifs:
            mdata, mgen = MotifStats.concat(mdata), MotifStats.concat(mgen)
            out["motifs"] = dict(mdata.compare(mgen), dataset=mdata, generated=mgen)
        if spectrum:
            sdata, sgen = SpectrumStats.concat(sdata), SpectrumStats.concat(sgen)
            out["spectrum"] = dict(sdata.compare(sgen), dataset=sdata, generated=sgen)
        if crossings:
            xdata, xgen = CrossingStats.concat(xdata), CrossingStats.concat(xgen)
            out["crossings"] = dict(xdata.compare(xgen), dataset=xdata, generated=xgen)
        return out

    def evaluate_disentanglement(self, n_bins: int = 20, factor_bins: Optional[int] = None) -> dict:
        """Does each latent group capture its own generative factor?  (disentangle_evaluation,
        `main.py:424`.)  The encoder means of every batch (``model.latent_means``: columns s,
        g, sg, the sg copies averaged) fill one device matrix [batch_num * batch_size, L];
        ``dataset.factor`` of the same graphs (the leftover graphs past the last whole batch
        are excluded, as in training) is uploaded once, and one ``layers.latent_mi`` call
        bins both (``n_bins`` per latent, ``factor_bins`` per factor, default n_bins) and
        leaves the mutual-information matrix on the device.

        Returns ``metrics.LatentMI.summary()`` (mig, avg_mi, modularity, group_share,
        best_latent: this project's definitions, see LatentMI) plus the LatentMI under
        "latent_mi", read back once.  Forward passes only; parameters, Adam state and the step
        counter are not written.  ValueError when the dataset's factors are missing, not 2-D or
        not one row per graph (``dataset_factors``)."""
        from .metrics import LatentMI
        rows = self.batch_num * self.batch_size
        factors = dataset_factors(self.dataset, rows)
        dev = self.model.params.device
        cols = self.model.latent_groups_columns()
        z = torch.empty(rows, cols["sg"].stop, device=dev)
        for i, b in enumerate(self.batches):
            self.model.latent_means(b, out=z[i * self.batch_size:(i + 1) * self.batch_size])
        f = torch.from_numpy(factors).to(dev)
        res = LatentMI(*layers.latent_mi(z, f, n_bins=n_bins, factor_bins=factor_bins), groups=cols)
        out = res.summary()
        out["latent_mi"] = res
        return out
