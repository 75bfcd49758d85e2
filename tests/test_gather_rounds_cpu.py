"""The hub graphs of tests/gather_rounds.py on the CPU: the own-operand link references
(tests/own_operands.py) are within their own derived bounds on these inputs.

A NumPy emulation of the bf16 chain (float32 arithmetic, the kernels' bf16 stores) passes
every link check on the hub graphs with nothing excluded at the lrelu kink, so a failure of
test_gpu_gather_rounds.py is the kernels', not the reference's.  Rows of 1, 15, 16, 17, 31,
32, 33, 48, 49 and 65 neighbours are all present.  With isolated nodes added the only
exclusions are the isolated rows' dP0 elements (P0 = 0 exactly, on the kink): that is why the
GPU cases checked against the reference have none (tests/gather_rounds.py).
"""
import numpy as np
import pytest

import gather_rounds as G
import own_operands as O


@pytest.mark.parametrize("name,n,d,B", G.CASES, ids=[c[0] for c in G.CASES])
def test_emulation_passes_every_link_with_nothing_excluded(name, n, d, B):
    cfg, batch, p, eps = G.make_case(n, d, B)
    deg = np.diff(batch.rowptr)
    for k in G.HUB_DEGREES:
        assert (deg == k).any(), k
    for fy3 in (False, True):                        # the fused decoder's links and the row engine's
        plan = O.Plan(cfg, fy3)
        b = O.run_chain(p, batch, eps, cfg, plan, "emulate")
        res = O.check_all(b, p, batch, cfg, plan)
        assert not O.failures(res), {k: res[k] for k in O.failures(res)}
        assert not any(nx for _, nx in res.values()), {k: v for k, v in res.items() if v[1]}


def test_isolated_rows_put_only_their_own_dp0_on_the_kink():
    name, n, d, B = G.CASES[0]
    cfg, batch, p, eps = G.make_case(n, d, B, isolated=G.N_ISOLATED)
    plan = O.Plan(cfg, False)
    b = O.run_chain(p, batch, eps, cfg, plan, "emulate")
    res = O.check_all(b, p, batch, cfg, plan)
    assert all(r <= 1.0 for r, _ in res.values())
    h0 = cfg.g_conv_hidden[0]
    assert {k: nx for k, (_, nx) in res.items() if nx} == {"FDP0": B * G.N_ISOLATED * h0}
