"""The spatial-graph references, bounds and guards of tests/abi_ops_sg.py, without a GPU:

(a) on contiguous inputs the factorised float64 reference equals oracle/ref_sg.py's dense
    restatement (sgconv_grads; sg_encoder's BN + lrelu) to 1e-12, fed in chunks of graphs;
    the prep scalars equal their definitions in the header, written as plain loops;
(b) the float32 emulation (split-K weight gradients included) passes every committed case;
(c) each planted fault fails its case, and the failure names the element or the guard.
"""
import numpy as np
import pytest

import abi_ops_sg as S
from oracle import ref_sg as O
from test_abi_ops_cpu import ELEMENT, close, fails, ids, passes

CHUNK = 256                             # graphs per call of the dense oracle


@pytest.fixture(scope="module")
def setups():
    """One setup per (case, bn_act), shared and left unchanged."""
    cache = {}

    def get(name, bn_act):
        if (name, bn_act) not in cache:
            cache[name, bn_act] = S.sg_setup(S.sg_case(name), bn_act)
        return cache[name, bn_act]
    return get


# ---------------------------------------------------------------- (a) the oracle
def dense_oracle(c, bn_act):
    """y, out, dx and the gradients by the dense oracle (torch autograd), summed over chunks."""
    import torch
    N, F, h2 = c.N, c.F, c.hidden[2]
    p = S.sg_unpack(c.prm.astype(np.float64), F, c.hidden)
    x, dO = c.x.astype(np.float64).reshape(c.B, N, F), c.dout.astype(np.float64).reshape(c.B, N, h2)
    adj, rel = c.adj.astype(np.float64), c.rel.astype(np.float64)
    ys, outs, dxs, grads = [], [], [], {k: 0.0 for k in S.SG_BLOCKS}
    for s in range(0, c.B, CHUNK):
        e = min(c.B, s + CHUNK)
        if not bn_act:
            y, g = O.sgconv_grads(adj[s:e], x[s:e], rel[s:e], p, dO[s:e])
            out = O.sg_encoder(adj[s:e], x[s:e], rel[s:e], [p])
            g["gamma"] = g["beta"] = 0.0
        else:
            t = lambda a, rg=False: torch.tensor(a, requires_grad=rg)
            tp = {k: t(v, True) for k, v in p.items()}
            tx = t(x[s:e], True)
            yt = O.sgconv_torch(t(adj[s:e]), tx, t(rel[s:e]), tp)
            tt = yt * (tp["gamma"] * O.BN_C) + tp["beta"]
            ot = torch.maximum(tt, O.LEAK * tt)
            (ot * t(dO[s:e])).sum().backward()
            y, out = yt.detach().numpy(), ot.detach().numpy()
            g = {k: v.grad.numpy() for k, v in tp.items()}
            g["x"] = tx.grad.numpy()
            close(out, O.sg_encoder(adj[s:e], x[s:e], rel[s:e], [p]))
        ys.append(y), outs.append(out), dxs.append(g["x"])
        for k in S.SG_BLOCKS:
            grads[k] = grads[k] + g[k]
    cat = lambda v: np.concatenate(v).reshape(c.R, -1)
    return cat(ys), cat(outs), cat(dxs), grads


@pytest.mark.parametrize("bn_act", [0, 1])
@pytest.mark.parametrize("case", S.SG_CASES, ids=ids(S.SG_CASES))
def test_sg_reference_is_the_oracle(case, bn_act, setups):
    c = setups(case[0], bn_act)
    r = S.sg_chain(c, c.x, c.prm, np.float64, bn_act, c.dout)
    y, out, dx, g = dense_oracle(c, bn_act)
    close(r.y, y), close(r.out, out), close(r.dx, dx)
    for k in S.SG_BLOCKS[:6] + (S.SG_BLOCKS[6:] if bn_act else ()):
        if np.abs(g[k]).max() == 0.0:
            assert not np.asarray(r.grads[k]).any(), k          # no edges: exactly zero
        else:
            close(r.grads[k], g[k])


def test_sg_prep_reference_is_the_header_definition(setups):
    c = setups("strided", 0)
    lr = lambda v: max(v, 0.2 * v)
    rel = c.rel.astype(np.float64)
    N = c.N
    nbr = [c.ci[c.rp[i]:c.rp[i + 1]] for i in range(c.R)]
    for i in range(c.R):
        b = i // N
        assert c.deg[i] == len(nbr[i])
        assert abs(c.ref.e[i] - sum(lr(rel[b, i - b * N, j - b * N]) for j in nbr[i])) <= 1e-12
        for q in range(c.rp[i], c.rp[i + 1]):
            j = c.ci[q]
            assert abs(c.ref.lr[q] - lr(rel[b, i - b * N, j - b * N])) <= 1e-15
            assert abs(c.ref.Q[q] - sum(lr(rel[b, i - b * N, k - b * N]) for k in nbr[j])) <= 1e-12
            assert c.rp[j] <= c.rev[q] < c.rp[j + 1] and c.ci[c.rev[q]] == i


def test_sg_cases_reach_what_they_claim(setups):
    g = setups("r4105", 0).geo
    assert (g.splits, g.kchunk, g.parts) == (2, 2112, 2) and 4105 - 2112 == 1993 == 31 * 64 + 9
    g = setups("r8225", 0).geo
    assert (g.splits, g.parts) == (3, 3)
    for name in ("r4105", "r8225"):
        c = setups(name, 0)
        assert (c.deg == 0).sum() > 100 and (c.adj.reshape(c.B, -1).sum(1) == 0).sum() >= 1, "isolated nodes, empty graphs"
    c = setups("strided", 0)
    assert c.R == 60 and c.bufs["x"].ld == c.F + 3 and c.bufs["dx"].ld == c.F + 5 and c.bufs["x"].off % 4 == 1
    c = setups("no_edges", 0)
    assert c.nnz == 0 and c.bufs["colidx"].width == 1
    assert "dx" not in setups("no_dx", 0).bufs
    g = setups("h0_65", 0).geo
    assert g.ld2 == 71 and g.ld3 == 10 and setups("h0_65", 0).hidden[2] > 64


# ---------------------------------------------------------------- (b) a correct implementation passes
@pytest.mark.parametrize("bn_act", [0, 1])
@pytest.mark.parametrize("case", S.SG_CASES, ids=ids(S.SG_CASES))
def test_emulated_sg_passes(case, bn_act, setups):
    c = setups(case[0], bn_act)
    passes(S.sg_verify(c, S.sg_emulate(c)))


# ---------------------------------------------------------------- (c) planted faults
@pytest.mark.parametrize("fault,case,pattern", [
    ("wg_full_tiles_only", "r4105", r"snd_sg_layer_bwd grads \w+: " + ELEMENT),   # rows >= 64 floor(R / 64) unsummed
    ("wg_drop_last_part", "r4105", r"snd_sg_layer_bwd grads \w+: " + ELEMENT),
    ("x_ld_f", "strided", r"snd_sg_layer_fwd y: " + ELEMENT + ".*ratio inf"),
    ("dw_own_q", "r4105", r"snd_sg_layer_bwd (grads M1|dx): " + ELEMENT),
    ("deg0_as_1", "r4105", r"snd_sg_prep node_deg: " + ELEMENT),
    ("ws_overrun", "no_dx", r"ws: trailing guard, \(row 1, column 0\) changed"),
    ("grads_accumulate", "no_dx", r"snd_sg_layer_bwd grads M1: " + ELEMENT + ".*ratio inf"),
], ids=["wg_full_tiles_only", "wg_drop_last_part", "x_ld_f", "dw_own_q", "deg0_as_1", "ws_overrun", "grads_accumulate"])
def test_fault_sg(fault, case, pattern, setups):
    c = setups(case, 1)
    fails(lambda: S.sg_verify(c, S.sg_emulate(c, fault)), pattern)


def test_fault_sg_degree_zero_row_changes_the_layer(setups):
    """Past the prep check, a degree-0 row taken as degree 1 changes y itself."""
    c = setups("r4105", 0)
    after = S.sg_emulate(c, "deg0_as_1")
    S.put(c, after, "node_deg", c.deg.astype(np.float32))
    fails(lambda: S.sg_verify(c, after), r"snd_sg_layer_fwd y: " + ELEMENT)
