"""The Adam step size inside the final reduction against the separate Adam kernel.

reduce_kernel computes the bias-corrected step size
    (float)((double)lr * sqrt(1 - b2^t) / (1 - b1^t))
in every block, between the issue of its slab loads and their wait, from the step counter
it fetches with its descriptor.  snd_adam_tf1 computes the same expression in its own
launch.  With the plan option "reduce_adam" 1 the reduction applies the update, with 0 it
is left to snd_adam_tf1: parameters, both moments and the gradient must agree byte for
byte after every one of three steps, from step counters 0 and 999 (at t = 1000 both
powers differ from 1 in many bits, at t = 1..3 in few).

  tscale(128, 64), B = 2   node latent: every block takes its update in the reduction
  tref_c1_n200_d16         the golden fixture's shape: its head slabs have about 1000
                           parts, the 64-part-lane branch of the reduction
"""
import pytest
import torch

import golden_io
from snd_vae_amd.config import tscale
from snd_vae_amd.data import synthetic_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def shape(name):
    from snd_vae_amd.params import init_blocks
    if name == "tscale_n128":
        cfg = tscale(128, 64)
        return cfg, synthetic_batch(cfg, 2, seed=9), init_blocks(cfg, 1)
    _, cfg, batch, p0 = golden_io.load(name)
    return cfg, batch, p0


def three_steps(cfg, batch, p0, dtype, reduce_adam, start):
    from snd_vae_amd import _lib
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    from snd_vae_amd.optimizer import OptimizerVAE
    model = SGCNModelVAE(cfg, batch.n_graphs, dtype=dtype, blocks=p0)
    model.set_option("reduce_adam", reduce_adam)
    opt = OptimizerVAE(model, fuse_adam=True)
    kinds = [_lib.lib().snd_plan_block_fused(model.plan, i) for i in range(len(model.layout.shapes))]
    opt.step_counter.fill_(start)
    db = DeviceBatch(batch)
    snaps = []
    for _ in range(3):
        opt.step(db)            # device Philox eps, keyed by (seed, step): the same in both runs
        torch.cuda.synchronize()
        snaps.append([t.clone() for t in (model.params, opt.m, opt.v, opt.grads)])
    assert int(opt.step_counter.item()) == start + 3
    return kinds, snaps


@pytest.mark.parametrize("start", [0, 999])
@pytest.mark.parametrize("name,dtype", [("tscale_n128", "bf16"), ("tref_c1_n200_d16", "f32"),
                                        ("tref_c1_n200_d16", "bf16")])
def test_reduction_adam_matches_separate_kernel(name, dtype, start):
    cfg, batch, p0 = shape(name)
    k_sep, sep = three_steps(cfg, batch, p0, dtype, 0, start)
    k_red, red = three_steps(cfg, batch, p0, dtype, 1, start)
    # the comparison is of the two kernels: the reduction must own blocks in one run only
    assert 2 in k_red and 2 not in k_sep, (k_red, k_sep)
    if name == "tscale_n128":
        assert set(k_red) == {2}
    for s, (a, b) in enumerate(zip(sep, red)):
        for what, x, y in zip(("params", "m", "v", "grads"), a, b):
            assert torch.isfinite(x).all(), (what, s)
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, "step", start + s + 1)
    # the update really ran: the parameters moved at every step
    assert not torch.equal(red[0][0], red[1][0]) and not torch.equal(red[1][0], red[2][0])
