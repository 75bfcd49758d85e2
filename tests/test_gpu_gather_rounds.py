"""The bf16 step on hub graphs whose rows hit every boundary of the row gathers.

tests/gather_rounds.py builds symmetric graphs with hub rows of exactly 1, 15, 16, 17, 31,
32, 33, 48, 49 and 65 neighbours, the hubs on the first and last
rows of the kernels' tiles and the largest as the batch's last row, where the gathers'
id prefetch meets the end of colidx.  N = 328, d = 64, B = 2 takes the fused front, both
fused heads and the gathered RC_ENC0; N = 200, d = 128 the two-chunk gathers of the bf16
edge kernels.

Every buffer of the step is checked per element against float64 on its own operands
(tests/own_operands.py: derived bounds, none measured), the dispatch path is asserted as in
test_gpu_own_operands.py, and the step is run a second time on the unfused chain
(snd_debug_set): the buffers both paths write are bitwise equal.  Rows of 0 neighbours
(GraphBatch accepts them) are checked in a case of their own, fused against chain and for
their exact zeros: their dP0 sits on the lrelu kink, which the reference excludes.
"""
import numpy as np
import pytest
import torch

import gather_rounds as G
import own_operands as O

pytestmark = pytest.mark.gpu
CHAIN_BITS = 32768 | 65536 | 262144 | 1048576


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def has_buffer(model, name):
    try:
        model.buffer(name)
        return True
    except Exception:
        return False


def run(cfg, batch, p, eps, B, chain):
    from snd_vae_amd import _lib
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    from snd_vae_amd.optimizer import OptimizerVAE
    _lib.check(_lib.lib().snd_debug_set(CHAIN_BITS if chain else 0))
    try:
        model = SGCNModelVAE(cfg, B, dtype="bf16", blocks=p)
    finally:
        _lib.check(_lib.lib().snd_debug_set(0))
    opt = OptimizerVAE(model, fuse_adam=False)
    opt.forward_backward(DeviceBatch(batch), torch.from_numpy(eps).cuda())
    torch.cuda.synchronize()
    dec_fused, head_bwd = has_buffer(model, "PDHS"), has_buffer(model, "PHBMS")
    return model, opt, dec_fused, head_bwd


def shared_buffers_differ(b, b1):
    shared = [k for k in b if k in b1 and not k.startswith(("g:", "l:"))]
    assert len(shared) >= 25
    return [("fused != chain", k, float(np.abs(b[k] - b1[k]).max())) for k in shared
            if not np.array_equal(b[k], b1[k])]


def test_isolated_rows_fused_equals_chain():
    name, n, d, B = G.CASES[0]
    cfg, batch, p, eps = G.make_case(n, d, B, isolated=G.N_ISOLATED)
    model, opt, dec_fused, head_bwd = run(cfg, batch, p, eps, B, chain=False)
    assert dec_fused and head_bwd
    m1, o1, dec1, head1 = run(cfg, batch, p, eps, B, chain=True)
    assert not dec1 and not head1
    b = O.read_plan(model, opt, batch, cfg, fy3=False)
    b1 = O.read_plan(m1, o1, batch, cfg, fy3=True)
    fails = shared_buffers_differ(b, b1)
    iso = np.flatnonzero(np.diff(batch.rowptr) == 0)
    assert len(iso) == B * G.N_ISOLATED
    for k in ("AX", "AXB", "FP1"):                   # sums over no neighbour
        if np.abs(b[k][iso]).max() != 0.0:
            fails.append((k, "an isolated row's sum is not zero"))
    assert not fails, fails


@pytest.mark.parametrize("name,n,d,B", G.CASES, ids=[c[0] for c in G.CASES])
def test_hub_rows_on_every_gather_boundary(name, n, d, B):
    cfg, batch, p, eps = G.make_case(n, d, B)
    model, opt, dec_fused, head_bwd = run(cfg, batch, p, eps, B, chain=False)
    fails = []
    if not dec_fused or head_bwd != (d <= 64):
        fails.append(("path", dict(dec_fused=dec_fused, head_bwd=head_bwd)))

    plan = O.Plan(cfg, fy3=not dec_fused)
    b = O.read_plan(model, opt, batch, cfg, fy3=not dec_fused)
    if b.pop("JROW_pad") != 0.0:
        fails.append(("ZSTAGE", "padding rows / columns of the staging image are not zero"))
    res = O.check_all(b, p, batch, cfg, plan)
    for k in sorted(res):
        print(f"{name} {k:16s} ratio {res[k][0]:.3f} excluded {res[k][1]}")
    fails += [(k, res[k]) for k in O.failures(res)]

    # ---- the unfused chain on the same inputs: shared buffers bit for bit
    m1, o1, dec1, head1 = run(cfg, batch, p, eps, B, chain=True)
    if dec1 or head1:
        fails.append(("path", "the chain run took a fused kernel"))
    b1 = O.read_plan(m1, o1, batch, cfg, fy3=True)
    fails += shared_buffers_differ(b, b1)
    assert not fails, fails
