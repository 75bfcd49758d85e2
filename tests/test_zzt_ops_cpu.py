"""The zz^T + CE link references (tests/zzt_ops.py) on the CPU.

* composed in float64 without any rounding they ARE the oracle: dz, CE sum and count of
  oracle/ref_numpy.adj_ce / adj_ce_rows to 1e-12 at every case (pos_weight, norm included);
* their bounds admit a correct implementation: the float32 emulation with the kernels'
  summation structure passes every link at every case, and stays under a quarter of the
  stats[0] bar (the condition that bar stands on);
* and reject planted faults, each at every case where it is expressible;
* the seeds leave no ambiguous pair up to n = 129 and at most 2e-4 of the pairs beyond.

Worst ratios of the emulation over all cases (err / bound; stats0 against the full bar):
  jrow, jt 0 (bitwise);  colpart 0.020 (n200_d128_f32);  ej 0.164 (n1000_d128_bf16);
  dJd 0.131 (rows1000_d64_bf16, rows 384-896);  dz 0.866 (pw129_d32_bf16: an s that sits on a
  bf16 rounding boundary, the allowance the link derives for it);  stats0 0.206 (n2_d128_bf16;
  the condition is 0.25);  stats1 0 (no ambiguous pair up to n = 129; the largest count beyond
  is 96 of 1.69 M pairs, n1300 at d = 64).
One case is rescaled to meet the quarter-bar condition: n1, d = 128, bf16 runs at z scale
0.1 (at 0.3 the emulation sits at 1.3 of the bar: one fp32 rounding of softplus2(x_00 = 16)
against a batch whose only terms are two softplus(-1)).
"""
import numpy as np
import pytest

import zzt_ops as Z
from oracle import ref_numpy as R

ALL = Z.CASES + Z.ROWS_CASES
IDS = [c.name for c in ALL]
_clean = {}


def clean(c):
    if c.name not in _clean:
        inp, _ = Z.setup(c)
        _clean[c.name] = Z.emulate(c, *inp)
    return _clean[c.name]


def rel(a, r):
    return float(np.abs(np.asarray(a) - r).max(initial=0.0) / max(np.abs(r).max(initial=0.0), 1e-300))


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_links_compose_to_the_oracle(c):
    (z, rp, ci), _ = Z.setup(c)
    r = Z.reference(c, z, rp, ci, exact=True)
    adj = Z.dense_adj(c, rp, ci)
    z64 = z.astype(np.float64)
    if c.rows:
        ce, dz, correct = R.adj_ce_rows(z64, adj[0], c.n, c.r0, c.r1, pos_weight=c.pw, norm=c.norm)
    else:
        ce, dz, correct = R.adj_ce(z64, adj, c.n, pos_weight=c.pw, norm=c.norm)
    assert rel(r.dz.ref, dz) <= 1e-12
    assert r.s0 == pytest.approx(ce, rel=1e-12)
    assert r.s1 == correct


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_emulation_within_the_bounds(c):
    inp, r = Z.setup(c)
    res = Z.check(c, r, clean(c), strict=True)
    print("ZZT_EMU", c.name, " ".join(f"{k} {v:.4f}" for k, v in res.items()))
    assert res["stats0"] < Z.S0_EMU, (c.name, res["stats0"])


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_ambiguity_cap(c):
    """On the reference alone: the count is exact up to n = 129, within 2e-4 of the pairs beyond."""
    _, r = Z.setup(c)
    assert r.amb <= Z.amb_cap(c), (c.name, r.amb, r.pairs)


# Where a fault is NOT expressible (zzt_ops.expressible); everywhere else it must be rejected.
NOT_EXPRESSIBLE = {
    "drop_last_col": "n1 (row 0's only column is its diagonal); the range (128, 129) of n = 129 (likewise)",
    "diag_in": "nowhere",
    "pad_pair": "n128 (no padding); required up to n = 129 only (beyond, ln 2 is under the bar)",
    "count_off": "nowhere; required up to n = 129 only (beyond, ambiguous pairs may hide one)",
    "no_kinv": "every f32 case, bf16 at d <= 32 (no factor), n1 (dJd = 0)",
    "v_scaled": "every f32 case, bf16 at d >= 64 (the scaled image IS the V role), n1",
    "slab_dropped": "every f32 case and every bf16 launch without column splits (one 128-column tile)",
    "edge_no_sigma": "pos_weight 1 (the coefficient is -1), empty, n1",
    "norm_not_2norm": "n1 (dz = 0)",
    "edge_row0": "whole-graph cases and ranges that begin at row 0",
    "jt_pad": "n128 at d = 32, 64, 128 (the image has no padding)",
}
N_NOT_EXPRESSIBLE = {}      # filled and pinned by test_expressible_table


def required(fault, c, ts):
    if fault in ("pad_pair", "count_off") and c.n > Z.AMB_SMALL_N:
        return False
    return Z.expressible(fault, c, ts)


def test_expressible_table():
    assert set(NOT_EXPRESSIBLE) == set(Z.FAULTS)
    for f in Z.FAULTS:
        N_NOT_EXPRESSIBLE[f] = sum(not Z.expressible(f, c, Z.layout(c)[2]) for c in ALL)
    assert N_NOT_EXPRESSIBLE["diag_in"] == 0 and N_NOT_EXPRESSIBLE["count_off"] == 0
    # n1 x 4 d x 2 dtypes, the (128, 129) range x 4 d x 2 dtypes
    assert N_NOT_EXPRESSIBLE["drop_last_col"] == 16
    assert N_NOT_EXPRESSIBLE["norm_not_2norm"] == 8
    assert N_NOT_EXPRESSIBLE["pad_pair"] == 8 and N_NOT_EXPRESSIBLE["jt_pad"] == 6
    # every case that is meant for splits has them at 256 CUs
    for c in ALL:
        if c.dtype == Z.BF16 and not c.rows and c.id in ("n129", "n300", "n1000", "n1300", "pw129", "pw300"):
            want = {"n129": 2, "pw129": 2, "n300": 3, "pw300": 3, "n1000": 8, "n1300": 8}[c.id]
            assert Z.layout(c)[2] == want, c.name


@pytest.mark.parametrize("fault", Z.FAULTS)
def test_planted_fault_is_rejected(fault):
    seen = 0
    for c in ALL:
        inp, r = Z.setup(c)
        if not required(fault, c, r.ts):
            continue
        res = Z.check(c, r, Z.plant(c, inp, clean(c), fault))
        assert max(res.values()) >= 1.0, f"{fault} passes at {c.name}: {res}"
        seen += 1
    assert seen > 0
