"""The d = 64 zz^T + CE kernel's tile walk: finite, repeatable bit for bit, split and unsplit.

The kernel (`zzt_dense`, zzt_dense_bf16_v9) walks 128-column tiles through a 3-slot LDS
ring: tile t + 1's DMA is issued in tile t, a full drain and a barrier end each tile.  A
wrong wait count, a missing barrier or a fill into a slot still being read makes the result
depend on timing, so three launches on the same staged z must give the same loss/count
partials (PZZT), dJ (DJD) and column splits' partial dJ (DJDX) bit for bit: a mismatch,
not a tolerance question.  (The four-loop ladder this file used to compare was measured,
lost and is gone: profiles/zzt_stage_ab.txt.)

Column splits: with fewer row blocks than CUs the launcher splits the tile range of a
row block over up to 8 workgroups, so at small n every workgroup of the default launch
sees one tile.  Each case therefore runs twice: as the step launches it (`zzt_dense`), and
unsplit (`zzt_dense_v0s1`: every workgroup walks all the tiles).  These are the smallest
shapes at which the walk can go wrong -- 1, 3, 4 and 5 tiles (one slot, the ring exactly
full, the first slot reused, a trip and two thirds of the unrolled loop); (200, 64, 1) and
(2560, 64, 1) split 2 and 20 tiles into ranges of 1, and of 2 and 3 -- and each runs in
well under a second.

Unknown variants: `launch_zzt_dense` takes 0, 1 and 256 * measurement bits; anything else
(the retired loops' 9 .. 12 among them) is SND_ERR_ARG before any launch.
"""
import numpy as np
import pytest
import torch

from snd_vae_amd.config import tscale
from snd_vae_amd.data import synthetic_batch

pytestmark = pytest.mark.gpu

DP = 64
SND_ERR_ARG = -1
WHAT = ("PZZT", "DJD", "DJDX")


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

    def rc(self, name):
        """snd_plan_launch's return code, synchronised."""
        rc = self.L.snd_plan_launch(self.model.plan, self.bc, self.model.workspace.data_ptr(),
                                    name.encode(), self._lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def launch(self, name):
        for b in self.bufs:
            b.zero_()
        self._lib.check(self.rc(name))
        return tuple(b.clone() for b in self.bufs)


def check_repeats(st, name):
    """Finite, dJ non-zero, and three launches bitwise equal in PZZT, DJD and DJDX."""
    ref = st.launch(name)
    assert torch.isfinite(ref[0]).all() and torch.isfinite(ref[1]).all()
    assert ref[1].abs().max().item() > 0
    for rep in (1, 2):
        out = st.launch(name)
        for what, x, y in zip(WHAT, out, ref):
            assert torch.equal(x, y), f"{name} launch {rep}: {what} differs from launch 0"
    return ref


def check_both(st):
    """As the step launches it, and unsplit: DJDX is exactly zero in the unsplit launch."""
    ref = check_repeats(st, "zzt_dense")
    un = check_repeats(st, "zzt_dense_v0s1")
    assert un[2].abs().max().item() == 0, "the unsplit launch wrote a column-split partial"
    return ref, un


CASES = [(128, 64, 2),    # one tile, nothing to prefetch
         (300, 64, 3),    # npad 384: three tiles, the ring exactly full, partial rows, zero columns
         (512, 64, 2),    # four tiles: the first slot filled a second time
         (640, 64, 1)]    # five tiles.  d = 64, not a d < dp: the plan and the op entry take
                          # d in {16, 32, 64, 128} only, so dp = 64 means d = 64


@pytest.mark.parametrize("n,d,B", CASES)
def test_zzt_loops_bitwise_in_step(n, d, B):
    check_both(Step(n, d, B))


@pytest.mark.parametrize("n", [200, 2560])
def test_zzt_loops_bitwise_column_splits(n):
    """B = 1, fewer row blocks than CUs: n = 200 is the smallest padded size that splits
    (2 tiles, 2 ranges of one tile); n = 2560 has 20 tiles in 8 ranges of 2 and 3 tiles.
    DJDX must hold a partial: the launch cannot silently run unsplit."""
    ref, _ = check_both(Step(n, 64, 1))
    assert ref[2].abs().max().item() > 0, "no column-split partial in DJDX"


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
    check_both(st)   # finite partials: the fallback, not inf - inf


def test_zzt_unknown_variant_is_an_argument_error():
    """A retired loop's number (10) and a number that never named a kernel (5): SND_ERR_ARG
    with a message naming the variant, and PZZT, DJD and DJDX left as they were."""
    st = Step(128, 64, 2)
    for k, b in enumerate(st.bufs):   # a pattern no launch would leave behind
        b.copy_((torch.arange(b.numel(), device=b.device) % 251 + 1 + k).to(b.dtype).view_as(b))
    before = tuple(b.clone() for b in st.bufs)
    for variant in (10, 5):
        name = f"zzt_dense_v{variant}"
        assert st.rc(name) == SND_ERR_ARG
        msg = st._lib.last_error()
        assert f"variant {variant} " in msg, msg
        for what, x, y in zip(WHAT, st.bufs, before):
            assert torch.equal(x, y), f"{name}: {what} was written"
