"""The d = 64 zz^T + CE kernel's tile loops against each other, bitwise.

The shipped loop (`zzt_dense`) and round 5's loop kept beside it (`zzt_dense_v9`: one
barrier and one full DMA drain per 128-column tile, the -z_i rows read from LDS every
tile) run the same MFMAs, the same epilogue and the same accumulation order, so the
loss/count partials (PZZT), dJ (DJD) and the column splits' partial dJ (DJDX) must be
equal bit for bit: a wrong wait count, a missing barrier or a fill into a slot still
being read shows as a mismatch, not as a tolerance question.  Every named loop of the
ladder (v10 registers, v11 DMA two tiles ahead, v12 two-tile stages) is held to the same.

Column splits: with fewer row blocks than CUs the launcher splits the tile range of a
row block over up to 8 workgroups, so at small n every workgroup of the default launch
sees one tile.  Each case therefore runs twice: as the step launches it, and unsplit
(`s1`: every workgroup walks all the tiles -- 3 tiles = a stage and a half stage, 5 tiles
= two stages and a half).  (2560, 64, 1) splits 20 tiles into ranges of 2 and 3.
"""
import numpy as np
import pytest
import torch

from snd_vae_amd.config import tscale
from snd_vae_amd.data import synthetic_batch

pytestmark = pytest.mark.gpu

PARENT = "zzt_dense_v9"
LADDER = ("zzt_dense_v10", "zzt_dense_v11", "zzt_dense_v12")
DP = 64


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


class Step:
    """One bf16 step at (n, d, B); relaunches of its zz^T on the staged z."""

    def __init__(self, n, d, B):
        from snd_vae_amd import _lib
        from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
        from snd_vae_amd.optimizer import OptimizerVAE
        self.n, self.d, self.B = n, d, B
        cfg = tscale(n, d)
        self.db = DeviceBatch(synthetic_batch(cfg, B, seed=1000))
        self.model = SGCNModelVAE(cfg, B, dtype="bf16")
        OptimizerVAE(self.model).step(self.db)
        torch.cuda.synchronize()
        self.L, self._lib = _lib.lib(), _lib
        self.bc = self.db.c_struct()
        self.bufs = (self.model.buffer("PZZT", torch.float64), self.model.buffer("DJD"),
                     self.model.buffer("DJDX"))

    def staged_rows(self):
        """The staged row image [B][npad][64] of z * sqrt(log2 e) (bf16), in place."""
        npad = -(-self.n // 128) * 128
        raw = self.model.buffer("ZSTAGE", torch.uint8)
        return raw[:self.B * npad * DP * 2].view(torch.bfloat16).view(self.B, npad, DP)

    def launch(self, name):
        for b in self.bufs:
            b.zero_()
        self._lib.check(self.L.snd_plan_launch(self.model.plan, self.bc, self.model.workspace.data_ptr(),
                                               name.encode(), self._lib.stream_ptr()))
        torch.cuda.synchronize()
        return tuple(b.clone() for b in self.bufs)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def check_loops(st, suffix, shipped):
    """shipped launch == the parent's loop == every rung, each launched twice."""
    ref = st.launch(PARENT + suffix)
    assert torch.isfinite(ref[0]).all() and torch.isfinite(ref[1]).all()
    assert ref[1].abs().max().item() > 0
    assert same(st.launch(PARENT + suffix), ref), "the parent's loop does not repeat itself"
    for name in (shipped,) + tuple(v + suffix for v in LADDER):
        for rep in range(2):
            out = st.launch(name)
            for what, x, y in zip(("PZZT", "DJD", "DJDX"), out, ref):
                assert torch.equal(x, y), f"{name} launch {rep}: {what} differs from {PARENT + suffix}"
    return ref


CASES = [(128, 64, 2),    # one tile, nothing to prefetch
         (300, 64, 3),    # npad 384: three tiles, the half stage at the end, partial rows, zero columns
         (512, 64, 2),    # four tiles: two full stages
         (640, 64, 1)]    # five tiles: two stages and a half.  d = 64, not a d < dp: the plan and
                          # the op entry take d in {16, 32, 64, 128} only, so dp = 64 means d = 64


@pytest.mark.parametrize("n,d,B", CASES)
def test_zzt_loops_bitwise_in_step(n, d, B):
    st = Step(n, d, B)
    check_loops(st, "", "zzt_dense")           # as the step launches it
    check_loops(st, "s1", "zzt_dense_v0s1")    # unsplit: every workgroup walks all the tiles


@pytest.mark.parametrize("n", [200, 2560])
def test_zzt_loops_bitwise_column_splits(n):
    """B = 1, fewer row blocks than CUs: n = 200 is the smallest padded size that splits
    (2 tiles, 2 ranges of one tile); n = 2560 has 20 tiles in 8 ranges of 2 and 3 tiles
    (a full stage, and a stage and a half).  DJDX must hold a partial: the launch cannot
    silently run unsplit."""
    st = Step(n, 64, 1)
    ref = check_loops(st, "", "zzt_dense")
    assert ref[2].abs().max().item() > 0, "no column-split partial in DJDX"
    un = check_loops(st, "s1", "zzt_dense_v0s1")
    assert un[2].abs().max().item() == 0


def test_zzt_loops_bitwise_extreme_logits():
    """Planted logits of +-100 (as test_zzt_ce_bf16_extreme_logits): exp2 overflows, the
    wave's sticky overflow path takes over; still bit for bit, split and unsplit."""
    n, B = 300, 2
    st = Step(n, 64, B)
    J = st.staged_rows()
    a = torch.zeros(DP, dtype=torch.float32, device=J.device)
    a[:4] = 5.0 * float(np.sqrt(np.log2(np.e)))   # |z|^2 = 100 before the sqrt(log2 e) scale
    J[:, 0:4] = a.to(torch.bfloat16)
    J[:, 4:8] = (-a).to(torch.bfloat16)
    J[:, 200:204] = a.to(torch.bfloat16)          # a second tile's columns
    for suffix, shipped in (("", "zzt_dense"), ("s1", "zzt_dense_v0s1")):
        check_loops(st, suffix, shipped)   # finite partials: the fallback, not inf - inf
