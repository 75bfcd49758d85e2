"""The multi-segment weight-gradient launch on both of its grids, against the per-weight
launches: every slab and the flat gradient, byte for byte.

wgrad_multi_kernel takes its segment from the block indices (row chunk, pair group,
segment) when every segment has the same grid, and from a flattened 1-D grid otherwise.
Both read the same 16-dword header of the segment's arguments and run the same body, so
one step on the same inputs and injected eps must leave the same bytes in

  1. the default run (the block-index grid where the segments are uniform),
  2. the run that forces the flattened grid (host debug bit 1 << 31),
  3. the run with one wgrad_kernel launch per weight (host debug bit 4096, set for the
     step only: the plan keeps the multi-segment row chunks, so the slabs are comparable).

Shapes, the smallest that reach each path:

  tscale(200, 64), B = 3   the C2 widths; 200 is no multiple of the 128-row unit, so graph
                           boundaries fall inside units and the last chunk is short; the
                           64-column window split cuts the wide weights into segments
  tscale(256, 128), B = 1  the C5 widths: dy in two column windows and x split in K
"""
import ctypes as C

import pytest
import torch

from snd_vae_amd.config import tscale
from snd_vae_amd.data import synthetic_batch
from test_gpu_step import make

pytestmark = pytest.mark.gpu

FLAT_GRID = 1 << 31     # the flattened 1-D grid even when the segments are uniform
PER_WEIGHT = 4096       # one wgrad_kernel launch per weight
SLABS = ("FSK1", "FSK2S", "FSK2N", "FSK3S", "FSW0", "FSW1", "FSW1T", "FSWMS", "FSWH", "FSWHT")
PLANS = {"c2_widths": (200, 64, 3), "c5_widths": (256, 128, 1)}


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def step(cfg, batch, p0, eps, flags):
    """One train step under `flags` (set for the step, not for the plan): the slabs, the
    flat gradient, and the number of block indices the multi-segment launch carries."""
    from snd_vae_amd import _lib
    L = _lib.lib()
    m, o, b = make(cfg, batch, p0, "bf16")
    _lib.check(L.snd_debug_set(C.c_int(flags).value))
    try:
        o.forward_backward(b, eps)
        torch.cuda.synchronize()
        bc = b.c_struct()
        dims = None
        if not flags & PER_WEIGHT:
            dims = L.snd_plan_launch(m.plan, C.byref(bc), _lib.ptr(m.workspace), b"wgrad_multi:dims",
                                     _lib.stream_ptr())
            assert dims in (1, 3), _lib.check(dims, "snd_plan_launch")
    finally:
        _lib.check(L.snd_debug_set(0))
    slabs = {}
    for name in SLABS:
        try:
            slabs[name] = m.buffer(name).clone()
        except Exception:       # not a buffer of this plan
            continue
    assert len(slabs) >= 6, sorted(slabs)
    return slabs, o.grads.clone(), dims


@pytest.fixture(scope="module")
def runs():
    from snd_vae_amd.params import init_blocks
    out = {}
    for name, (n, d, B) in PLANS.items():
        cfg = tscale(n, d)
        batch = synthetic_batch(cfg, B, seed=7)
        p0 = init_blocks(cfg, 3)
        eps = torch.randn(B * n, d, generator=torch.Generator().manual_seed(5)).cuda()
        out[name] = {f: step(cfg, batch, p0, eps, f) for f in (0, FLAT_GRID, PER_WEIGHT)}
    return out


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("other", [FLAT_GRID, PER_WEIGHT])
def test_slabs_and_gradient_byte_equal(runs, plan, other):
    s0, g0, _ = runs[plan][0]
    s1, g1, dims = runs[plan][other]
    if other == FLAT_GRID:
        assert dims == 1
    assert sorted(s0) == sorted(s1)
    # slabs the step really wrote
    assert sum(s0[k].abs().max().item() > 0 for k in s0) >= 6
    for k in s0:
        assert torch.equal(s0[k].view(torch.int32), s1[k].view(torch.int32)), (plan, k)
    assert torch.isfinite(g0).all() and g0.abs().max().item() > 0
    assert torch.equal(g0.view(torch.int32), g1.view(torch.int32)), plan


def test_default_takes_the_block_index_grid(runs):
    """Otherwise the comparison above is one path against itself."""
    dims = {p: runs[p][0][2] for p in PLANS}
    assert 3 in dims.values(), dims
