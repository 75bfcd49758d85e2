"""The fused decoder chains on the tile shapes where a phase's row blocks leave a nearly
empty last pass (the halo: 9 row blocks over 4 or 8 waves per column group), on partial
tiles, and on the runtime-chunk instantiations.  The shapes are the smallest that reach
each path (128-row tiles need at least 128 of them):

  tscale(200, 64), B = 64   128 tiles: a full tile (9 row blocks) and a 72-row partial tile
                            (5 row blocks), both at graph edges
  tscale(384, 64), B = 43   129 tiles, an interior tile with both halos inside the graph
  tscale(130, 64), B = 64   a 2-row partial tile (one row block)
  tscale(256, 16), B = 64   the runtime-chunk instantiations of the phases
  tref(1964, 32, ...), B = 8  the same, graph latent: 128 tiles, the last of a graph 44 rows
                            (the graph latent takes at most 8 graphs, so tref(300, 32) cannot
                            reach 128 tiles with B = 43 -- snd_plan_create refuses it; N = 1964
                            is the smallest multiple of 4 with 16 tiles per graph and a partial one)
  tscale(200, 64), B = 32   64-row tiles (conv1: 5 row blocks over 4 waves per column group)

Each shape is one forward_backward on the bf16 fast path per run.  The staging and epilogue
operand loads of both kernels go through selected addresses (`zero` for a row outside the
graph, a column outside the layout): these shapes put such rows and columns in every phase.
(Folding the tail row block into the last full pass was measured and not kept -- DESIGN 5 --
so there is no fold-on / fold-off comparison here.)
"""
import numpy as np
import pytest
import torch

from snd_vae_amd.config import tref, tscale
from snd_vae_amd.data import synthetic_batch
from test_gpu_step import DEC_BUFS, make

pytestmark = pytest.mark.gpu

ROW_ENGINE = 32768      # the unfused decoder (seven launches)
POISON_LDS = 1 << 23    # NaN in every activation byte of the forward kernel's LDS first


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def run(cfg, batch, p0, flags):
    from snd_vae_amd import _lib
    _lib.check(_lib.lib().snd_debug_set(flags))
    try:
        m, o, b = make(cfg, batch, p0, "bf16")
    finally:
        _lib.check(_lib.lib().snd_debug_set(0))
    o.forward_backward(b)
    torch.cuda.synchronize()
    return m, o, b


@pytest.mark.parametrize("topology,n,d,B", [("tscale", 200, 64, 64), ("tscale", 384, 64, 43),
                                            ("tscale", 130, 64, 64), ("tscale", 256, 16, 64),
                                            ("tref", 1964, 32, 8), ("tscale", 200, 64, 32)])
def test_tail_shapes(topology, n, d, B):
    from snd_vae_amd import _lib
    from snd_vae_amd.params import init_blocks
    cfg = tscale(n, d) if topology == "tscale" else tref(n, d, g_hidden=16, latent=8)
    batch = synthetic_batch(cfg, B, seed=11)
    p0 = init_blocks(cfg, 2)
    m0, o0, _ = run(cfg, batch, p0, ROW_ENGINE)
    m1, o1, b1 = run(cfg, batch, p0, 0)
    # fused against the row engine, at test_fused_decoder_matches_row_engine's bars
    for name, dt in DEC_BUFS:
        assert torch.equal(m0.buffer(name, dt), m1.buffer(name, dt)), name
    g0, g1 = o0.grad_blocks(), o1.grad_blocks()
    for k in g0:
        if not k.startswith("dec."):
            continue
        if k.startswith("dec.K"):
            assert np.array_equal(g0[k], g1[k]), k
        else:
            np.testing.assert_allclose(g1[k], g0[k], rtol=1e-4, atol=1e-7 * max(1.0, np.abs(g0[k]).max()),
                                       err_msg=k)
    # the rerun with NaN-poisoned LDS (the device Philox stream is keyed by the step)
    ctr = o1.step_counter.clone()
    o1.forward_backward(b1)
    torch.cuda.synchronize()
    snap = {name: m1.buffer(name, dt).clone() for name, dt in DEC_BUFS}
    o1.step_counter.copy_(ctr)
    _lib.check(_lib.lib().snd_debug_set(POISON_LDS))
    try:
        o1.forward_backward(b1)
        torch.cuda.synchronize()
    finally:
        _lib.check(_lib.lib().snd_debug_set(0))
    for name, dt in DEC_BUFS:
        assert torch.equal(m1.buffer(name, dt), snap[name]), f"{name} with NaN-poisoned LDS"
