"""Every buffer of the bf16 step against float64 on its OWN operands, per element.

The fused kernels are held bitwise to the row-engine chain (test_gpu_step.py) and the whole
step to the float64 oracle at bars measured on the kernels themselves (parity_bars.json);
neither sees a small systematic error in code both sides share.  Here every link of the
step -- tests/own_operands.py, one reference per link, read from the kernels' epilogues --
is evaluated in float64 from the operands exactly as the step left them in HBM, and the
GPU's output must lie within a bound derived from the arithmetic: fp32 accumulation of K
terms, one bf16 ulp where the output is stored in bf16, 1e-6 for a hardware transcendental.
No bound is measured; parity_bars.json is not consulted.

One forward_backward per case; all links are checked and every failure is collected before
the assertion.  Each case asserts the dispatch path it is there for: the fused decoder
(buffer PDHS) and the fused backward head (PHBMS) are present or absent as claimed.  (With
the update not fused -- every gradient block is read back -- snd_plan_block_fused is 0 for
every block, which is asserted.)  The worst |gpu - ref| / bound of every link goes to
own_operand_errors.jsonl beside the parity error log (parity_bars.LOG), one line per case.

Covered: all 30 forward / backward buffers the step materialises for the node latent (AX,
AXB, FH1, FXW1, FP1, FG, FHH, MS, Z, ZB, the zz^T staging rows, DJD, FY1-3, FU1-3, SHAT,
XHAT, FDY3-1, DZDEC, FDMS, FDH, FDP1, FDXW1, FDP0), the graph latent's (Hh, MS, ZL, Z, DZL,
DMS, DH, FDG and the encoder / decoder links above), all 32 (34) gradient blocks, and the
KL / SSE sums; the CE sum and the accuracy count through parity_bars.own_structure.
Not checkable as a link of their own:
* FY3 / FU3 on the fused decoder: conv3's output lives in LDS only.  SHAT and FDY3 are then
  referred to FU2, with conv3's derived bound carried through; the row-engine cases check
  FY3 / FU3 themselves.
* EJ, the per-edge terms: never materialised on the fused paths; they enter FDMS's reference
  from ZB and the CSR: e_i = sum_j ((pw - 1) sigmoid(z_i . z_j) - pw) z_j.  Every case runs
  twice: at the default weights (pos_weight 1: the coefficient is -1, no sigmoid) and, "_w",
  at its batch's own class balance with beta = 4 -- the per-edge sigmoid of each of the
  kernels that evaluate it, norm in adj_scale / the CE sum and beta in kl_scale.
* The transposed staging image and the per-64-row column sums of ZSTAGE, and the per-block
  partial slabs: read only through what is built from them (the CE sum, the gradients).
* The packed weight images: bitwise against pack_kernel in test_gpu_step.py; every link
  here multiplies by the bf16-rounded weight, so a wrong image fails its link.
"""
import json
import os

import numpy as np
import pytest
import torch

import own_operands as O
import parity_bars as PB

pytestmark = pytest.mark.gpu
LOG = os.path.join(os.path.dirname(PB.LOG), "own_operand_errors.jsonl")
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


@pytest.mark.parametrize("name,topology,n,d,B,kbar,chain,weighted", O.CASES, ids=[c[0] for c in O.CASES])
def test_step_buffers_on_their_own_operands(name, topology, n, d, B, kbar, chain, weighted):
    from snd_vae_amd import _lib
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    from snd_vae_amd.optimizer import OptimizerVAE
    cfg, batch, p, eps = O.make_case(topology, n, d, B, kbar, weighted)
    assert (cfg.pos_weight > 1.0 and cfg.norm != 1.0 and cfg.beta == O.WEIGHTED_BETA) == weighted
    if kbar:
        assert np.diff(batch.rowptr).max() > 32        # rounds past the prefetched neighbours
    _lib.check(_lib.lib().snd_debug_set(CHAIN_BITS if chain else 0))
    try:
        model = SGCNModelVAE(cfg, B, dtype="bf16", blocks=p)
    finally:
        _lib.check(_lib.lib().snd_debug_set(0))
    opt = OptimizerVAE(model, fuse_adam=False)
    db = DeviceBatch(batch)
    opt.forward_backward(db, torch.from_numpy(eps).cuda())
    torch.cuda.synchronize()

    # ---- the path this case is there for
    dec_fused, head_bwd = has_buffer(model, "PDHS"), has_buffer(model, "PHBMS")
    want_dec = not chain
    want_head = not chain and topology == "tscale" and d <= 64
    fails = []
    if dec_fused != want_dec or head_bwd != want_head:
        fails.append(("path", dict(dec_fused=dec_fused, head_bwd=head_bwd)))
    nb = _lib.lib().snd_plan_num_blocks(model.plan)
    if any(_lib.lib().snd_plan_block_fused(model.plan, i) for i in range(nb)):
        fails.append(("path", "a block's update is fused: its gradient is not stored"))

    # ---- every link
    plan = O.Plan(cfg, fy3=not dec_fused)
    b = O.read_plan(model, opt, batch, cfg, fy3=not dec_fused)
    if b.pop("JROW_pad") != 0.0:
        fails.append(("ZSTAGE", "padding rows / columns of the staging image are not zero"))
    res = O.check_all(b, p, batch, cfg, plan)
    rec = {"case": name, "pos_weight": cfg.pos_weight, "norm": cfg.norm, "beta": cfg.beta,
           "dec_fused": dec_fused, "head_bwd": head_bwd,
           "links": {k: [r, nx] for k, (r, nx) in res.items()}}
    fails += [(k, res[k]) for k in O.failures(res)]

    # ---- the structure term's CE sum and accuracy count (d = 16: the image padded to 32 columns)
    got = opt.loss_dict()
    try:
        ce, absum, correct, amb = PB.own_structure(model, batch, cfg)
    except AssertionError as ex:                        # its pad check: collected like the rest
        fails.append(("own_structure", str(ex)))
    else:
        e = abs(got["adj_sum"] - ce) / absum
        rec["own_structure"] = {"ce_rel_abs": e, "correct_diff": got["correct"] - correct, "ambiguous": amb}
        if e > 1e-6 or abs(got["correct"] - correct) > amb:
            fails.append(("own_structure", got["adj_sum"], ce, e, got["correct"], correct, amb))

    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(json.dumps(rec) + "\n")
    assert not fails, fails
