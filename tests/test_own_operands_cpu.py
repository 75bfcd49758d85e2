"""The own-operand link references (tests/own_operands.py) on the CPU.

* composed in float64 without any rounding they ARE the oracle: every cache entry, loss sum
  and gradient block of oracle/ref_numpy.forward_backward to 1e-12;
* their derived bounds admit a correct implementation: a NumPy emulation of the bf16 chain
  (float32 arithmetic, bf16 round-to-nearest-even stores) passes every link check;
* and reject subtle errors: single perturbations of that emulation, each no larger than the
  bf16 operand gap that the measured oracle bars absorb, fail the link they touch and
  nothing upstream of it;
* the committed seeds of the GPU cases keep the oracle's own pre-activations off the lrelu
  kink (at most 4 elements per buffer may be excluded);
* parity_bars.e32_grads measures the fp32 conditioning, not a kink (C2 bench-batch bars).
"""
import numpy as np
import pytest

import own_operands as O
from oracle import ref_numpy as R
from snd_vae_amd.config import tref, tscale
from snd_vae_amd.data import synthetic_batch
from snd_vae_amd.params import init_blocks


def case(cfg, B, seed=3, init=1):
    batch = synthetic_batch(cfg, B, seed=seed)
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in init_blocks(cfg, init).items()}
    rows = B if cfg.topology == "tref" else B * cfg.n_nodes
    eps = np.random.default_rng(5).standard_normal((rows, cfg.latent)).astype(np.float32)
    return batch, p, eps


def rel(a, r):
    return float(np.abs(np.asarray(a) - r).max() / max(np.abs(r).max(), 1e-300))


_TS, _TR = tscale(25, 16), tref(25, 16, g_hidden=16, latent=8)
TOPO_WEIGHTED = pytest.mark.parametrize("cfg,weighted", [(_TS, False), (_TR, False), (_TS, True), (_TR, True)],
                                        ids=["tscale", "tref", "tscale-weighted", "tref-weighted"])


@TOPO_WEIGHTED
def test_links_compose_to_the_oracle(cfg, weighted):
    B = 2
    batch, p, eps = case(cfg, B)
    if weighted:
        cfg = O.weighted_cfg(cfg, batch)
        assert cfg.pos_weight > 1.0 and cfg.norm != 1.0 and cfg.beta == 4.0
    b = O.run_chain(p, batch, eps, cfg, O.Plan(cfg, True, compose=True), "compose")
    adj = [batch.dense_adj(i) for i in range(B)]
    rl, rg, c = R.forward_backward(p, adj, batch.features, batch.feature_truth, batch.spatial_truth,
                                   eps.astype(np.float64), cfg)
    s1, s2 = cfg.s_d_channel[0], cfg.s_d_channel[1]
    L = cfg.latent
    tr = cfg.topology == "tref"
    pairs = {"P1": b["FP1"], "H1": b["FH1"], "G": b["FG"], "h": b["Hh" if tr else "FHH"],
             "mu": b["MS"][:, :L], "s": b["MS"][:, L:], "z": b["ZL" if tr else "Z"], "J": b["Z"],
             "Y1": b["FY1"], "U1": b["FU1"], "Y2s": b["FY2"][:, :s2], "Y2n": b["FY2"][:, s2:],
             "U2s": b["FU2"][:, :s2], "U2n": b["FU2"][:, s2:], "Y3s": b["FY3"], "U3s": b["FU3"],
             "Shat": b["SHAT"], "Xhat": b["XHAT"]}
    for k, v in pairs.items():
        assert rel(v, c[k]) <= 1e-12, k
    # dJ = adj_scale (dJd + e) + dz_dec: the oracle's cache["dJ"] through the first link it feeds
    R_ = B * cfg.n_nodes
    rows = B if tr else R_
    assert float(b["l:kl_sum"]) == pytest.approx(-2.0 * rl["kl"] * rows * L, rel=1e-12)
    assert float(b["l:sse_s"]) == pytest.approx(rl["spatial_cost"] * R_ * cfg.spatial_dim, rel=1e-12)
    assert float(b["l:sse_n"]) == pytest.approx(rl["node_cost"] * R_ * cfg.num_feature, rel=1e-12)
    assert set(rg) == {k[2:] for k in b if k.startswith("g:")}
    for k, g in rg.items():
        assert rel(b["g:" + k].reshape(g.shape), g) <= 1e-12, k


@TOPO_WEIGHTED
def test_own_structure_ce_sum_composes_to_the_oracle(cfg, weighted):
    """parity_bars.own_structure's CE sum and count on the unrounded operands of the composed
    chain are the oracle's: norm (dense + sum_e[(pw - 1) softplus(L_e) - pw L_e] + B n
    softplus(-1)) == pairs * adj_cost (the oracle's adj_cost is the mean that already carries
    norm), to 1e-12."""
    import parity_bars as PB
    B, n = 2, cfg.n_nodes
    batch, p, eps = case(cfg, B)
    if weighted:
        cfg = O.weighted_cfg(cfg, batch)
    b = O.run_chain(p, batch, eps, cfg, O.Plan(cfg, True, compose=True), "compose")
    rl = R.forward_backward(p, [batch.dense_adj(i) for i in range(B)], batch.features, batch.feature_truth,
                            batch.spatial_truth, eps.astype(np.float64), cfg, want_grads=False)[0]
    ce, absum, correct, amb = PB.own_structure_sums(b["JROW"].reshape(B, n, -1), b["ZB"], batch, cfg, k32=O.ident)
    assert ce == pytest.approx(B * n * n * rl["adj_cost"], rel=1e-12)
    assert absum >= abs(ce) and correct == rl["correct"]
    if weighted:   # the weights matter: the unweighted sum is somewhere else entirely
        ce1 = PB.own_structure_sums(b["JROW"].reshape(B, n, -1), b["ZB"], batch,
                                    cfg.replace(pos_weight=1.0, norm=1.0), k32=O.ident)[0]
        assert abs(ce1 - ce) > 1e-3 * absum


EMU = {"n200_d16": (tscale(200, 16), 3, False), "n130_d64": (tscale(130, 64), 2, True),
       "n140_d128": (tscale(140, 128), 2, False), "tref_n130_d32": (tref(130, 32, g_hidden=16, latent=8), 2, False)}
_emu_cache = {}


def emulation(key, weighted=False):
    """(cfg, batch, p, eps, plan, clean buffers) -- computed once per case.  ``weighted``:
    at the batch's own pos_weight / norm and beta = 4 (own_operands.weighted_cfg)."""
    if (key, weighted) not in _emu_cache:
        cfg, B, fy3 = EMU[key]
        batch, p, eps = case(cfg, B)
        if weighted:
            cfg = O.weighted_cfg(cfg, batch)
        plan = O.Plan(cfg, fy3)
        _emu_cache[key, weighted] = (cfg, batch, p, eps, plan, O.run_chain(p, batch, eps, cfg, plan, "emulate"))
    return _emu_cache[key, weighted]


@pytest.mark.parametrize("key,weighted", [(k, False) for k in EMU] + [(k, True) for k in EMU],
                         ids=list(EMU) + [k + "-weighted" for k in EMU])
def test_bounds_admit_a_correct_implementation(key, weighted):
    cfg, batch, p, eps, plan, b = emulation(key, weighted)
    res = O.check_all(b, p, batch, cfg, plan)
    assert not O.failures(res), {k: res[k] for k in O.failures(res)}
    # the bf16 stores sit at their half ulp: the bound is not slack by more than the factor 2
    # between the low and the high end of a binade
    assert max(r for k, (r, _) in res.items() if k in ("FU1", "FG", "FDY2")) > 0.45


def ulp_bf16(v):
    return 2.0 ** (np.floor(np.log2(abs(v))) - 7)


def perturbed(key, target, fn):
    """The emulation with link ``target``'s stored value replaced by fn(value, bufs): the
    names of the failing links, and the step order of all links."""
    cfg, batch, p, eps, plan, _ = emulation(key)
    order = []

    def hook(name, v, b):
        order.append(name)
        return fn(v.copy(), b) if name == target else None

    b = O.run_chain(p, batch, eps, cfg, plan, "emulate", perturb=hook)
    assert target in order
    return O.failures(O.check_all(b, p, batch, cfg, plan)), order


def assert_caught(fails, order, target):
    assert target in fails, (target, fails)
    up = [k for k in fails if order.index(k) < order.index(target)]
    assert not up, ("a check upstream of the perturbed link failed", up)
    # every link is referred to its own stored operands: nothing else may move
    assert fails == [target], fails


@pytest.mark.parametrize("key", ["n200_d16", "n130_d64"])
def test_two_bf16_ulps_on_one_element(key):
    def fn(v, b):
        r, c_ = 77, 5
        v[r, c_] += 2 * ulp_bf16(v[r, c_])
        return v
    for target in ("FU2", "FXW1", "FDP1"):
        fails, order = perturbed(key, target, fn)
        assert_caught(fails, order, target)


@pytest.mark.parametrize("key", ["n200_d16", "n130_d64"])
@pytest.mark.parametrize("kind", ["dropped", "leaked"])
def test_conv2_halo_tap_at_a_graph_boundary(key, kind):
    """Tap t = +2 of conv2 at the end of a graph: "dropped" -- the tap that reads the graph's
    last row (for row n - 3) is left out; "leaked" -- the graph's last row, whose +2 tap lies
    past the graph and must read zero, reads the next graph's row instead."""
    cfg, batch, p, _, _, _ = emulation(key)
    n, s1 = cfg.n_nodes, cfg.s_d_channel[0]
    s2 = cfg.s_d_channel[1]
    K2s = O.bf16(p["dec.K2s"])

    def fn(v, b):
        if kind == "dropped":
            r = n - 3
            v[r, :s2] -= b["FU1"][r + 2, :s1] @ K2s[4]
        else:
            r = n - 1
            v[r, :s2] += b["FU1"][r + 2, :s1] @ K2s[4]
        return v.astype(np.float32).astype(np.float64)
    fails, order = perturbed(key, "FY2", fn)
    assert_caught(fails, order, "FY2")


@pytest.mark.parametrize("key", ["n200_d16", "n130_d64"])
def test_one_neighbour_skipped_in_one_row_of_fp1(key):
    cfg, batch, p, _, _, _ = emulation(key)
    r = int(np.argmax(np.diff(batch.rowptr)))            # the highest-degree row: its last neighbour
    j = int(batch.colidx[batch.rowptr[r + 1] - 1])

    def fn(v, b):
        v[r] = (v[r] - b["FXW1"][j]).astype(np.float32)
        return v
    fails, order = perturbed(key, "FP1", fn)
    assert_caught(fails, order, "FP1")


@pytest.mark.parametrize("key", ["n200_d16", "n130_d64"])
@pytest.mark.parametrize("block", ["dec.K2s", "enc.W1", "dec.K1"])
def test_last_partial_row_chunk_left_out_of_a_weight_gradient(key, block):
    cfg, batch, p, _, _, _ = emulation(key)
    n, R_ = cfg.n_nodes, cfg.n_nodes * batch.n_graphs
    lo = (R_ // 128) * 128                               # rows of the last partial 128-row chunk
    assert 0 < R_ - lo < 128
    s1, s2 = cfg.s_d_channel[0], cfg.s_d_channel[1]

    def fn(v, b):
        def cut(a):
            a = a.copy()
            a[:lo] = 0.0
            return a
        if block == "dec.K2s":
            part = O.conv_wgrad(b["FU1"][:, :s1], cut(b["FDY2"][:, :s2]), n)
        elif block == "dec.K1":
            part = O.conv_wgrad(b["ZB"], cut(b["FDY1"]), n)
        else:
            part = b["FH1"].T @ cut(b["FDXW1"])
        return (v - part.reshape(v.shape)).astype(np.float32).astype(np.float64)
    fails, order = perturbed(key, "g:" + block, fn)
    assert_caught(fails, order, "g:" + block)


@pytest.mark.parametrize("key", ["n130_d64", "n140_d128"])
def test_feature_column_dropped_from_fhh(key):
    """One of the X columns appended to B1 (at d = 128 a true K tail: fp32 weight rows past
    the packed image) left out of h = G Wh + bh."""
    cfg, batch, p, _, plan, _ = emulation(key)
    h1 = cfg.g_conv_hidden[1]
    k = h1 + cfg.f_in - 1
    assert (plan.kwh <= k) == (key == "n140_d128")
    w = p["enc.Wh"][k] if plan.kwh <= k else O.bf16(p["enc.Wh"])[k]

    def fn(v, b):
        e = O.emulated_fhh(b, p, plan) - np.outer(b["FG"][:, k], w)
        return O.bf16(e)
    fails, order = perturbed(key, "FHH", fn)
    assert_caught(fails, order, "FHH")


@pytest.mark.parametrize("key", ["n200_d16", "n130_d64", "n140_d128"])
def test_one_tile_of_djd_scaled(key):
    def fn(v, b):
        v[32:64, :16] *= 1.0 + 2.0 ** -6
        return v.astype(np.float32).astype(np.float64)
    fails, order = perturbed(key, "DJD", fn)
    assert_caught(fails, order, "DJD")


# ---- planted faults in how the step uses pos_weight / norm / beta: each is ONE change to
# the weighted emulation (own_operands.edge_sigmoid / edge_coef / loss_scales, the three
# places the emulation reads the weights through), run on the chain's own upstream buffers.
def _sig_negated(x):                                  # (a) sigmoid(-L) for sigmoid(L)
    return _EDGE_SIGMOID(-x)


def _sig_no_e(x):                                     # (b) r instead of e r on the negative branch
    e = np.exp(-np.abs(x))
    return 1 / (1 + e)


def _coef_pw(x, pw):                                  # (c) pw instead of pw - 1 on the sigmoid
    return np.full(x.shape, -pw, x.dtype) + pw * O.edge_sigmoid(x)


def _coef_early_out(x, pw):                           # (f) the pw == 1 early-out's coefficient
    return np.full(x.shape, -pw, x.dtype)


def _scales_no_norm(cfg, B, n, RH, L, k32):           # (d) adj_scale without norm
    pw, _, klc = _LOSS_SCALES(cfg, B, n, RH, L, k32)
    return pw, k32(2.0 / (float(B) * n * n)), klc


def _scales_no_beta(cfg, B, n, RH, L, k32):           # (e) kl_scale without beta
    pw, adj, _ = _LOSS_SCALES(cfg, B, n, RH, L, k32)
    return pw, adj, k32(1.0 / (float(RH) * L))


_EDGE_SIGMOID, _LOSS_SCALES = O.edge_sigmoid, O.loss_scales
FAULTS = {"a_sigmoid_of_minus_L": ("edge_sigmoid", _sig_negated), "b_r_for_e_r": ("edge_sigmoid", _sig_no_e),
          "c_pw_for_pw_minus_1": ("edge_coef", _coef_pw), "d_adj_scale_without_norm": ("loss_scales", _scales_no_norm),
          "e_kl_scale_without_beta": ("loss_scales", _scales_no_beta), "f_early_out_coef": ("edge_coef", _coef_early_out)}
# the links that read dJ (and the scales) directly; the first is the one that must fail
FIRST = {False: ("FDMS", "g:enc.bms"), True: ("g:dec.Wp", "g:dec.bp", "DZL", "DMS")}


def planted(key, fault, monkeypatch):
    """The weighted emulation with ``fault`` planted: the links that read dJ / the scales
    directly hold what the faulty step computes from the (clean) upstream buffers, everything
    downstream is computed from those.  Returns (failing links, step order, first targets)."""
    cfg, batch, p, eps, plan, clean = emulation(key, True)
    targets = FIRST[plan.tref]
    with monkeypatch.context() as m:
        m.setattr(O, FAULTS[fault][0], FAULTS[fault][1])
        faulty = O.run_chain(p, batch, eps, cfg, plan, "emulate")
    order = []

    def hook(name, v, b):
        order.append(name)
        return faulty[name] if name in targets else None

    b = O.run_chain(p, batch, eps, cfg, plan, "emulate", perturb=hook)
    up = order[:order.index(targets[0])]
    assert all(np.array_equal(b[k], clean[k]) and np.array_equal(faulty[k], clean[k]) for k in up)
    return O.failures(O.check_all(b, p, batch, cfg, plan)), order, targets


def assert_fault_caught(fails, order, targets):
    assert targets[0] in fails, (targets[0], fails)
    up = [k for k in fails if order.index(k) < order.index(targets[0])]
    assert not up, ("a check upstream of the planted fault failed", up)
    # everything downstream is referred to its own stored operands: nothing else may move
    assert set(fails) <= set(targets), fails


@pytest.mark.parametrize("key", ["n200_d16", "n130_d64"])
@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_in_the_loss_weights_fails_fdms(key, fault, monkeypatch):
    fails, order, targets = planted(key, fault, monkeypatch)
    assert targets[0] == "FDMS"
    assert_fault_caught(fails, order, targets)


@pytest.mark.parametrize("fault", ["a_sigmoid_of_minus_L", "c_pw_for_pw_minus_1"])
def test_planted_fault_on_the_graph_latent(fault, monkeypatch):
    """Graph latent: dJ first feeds the projection's weight gradient g:dec.Wp.  Its edge
    logits at initialisation are small (|L| < 0.1, sigmoid within 0.025 of 1/2), so (a), the
    sign inside the sigmoid, moves a coefficient by at most (pw - 1) 0.05; summed into
    g:dec.Wp that is still thousands of bounds, so (a) fails the link here as well.  (c) --
    pw for pw - 1, which moves every coefficient by sigmoid(L) ~ 1/2 -- is asserted beside
    it, should a case with smaller logits ever let (a) through."""
    fails, order, targets = planted("tref_n130_d32", fault, monkeypatch)
    assert targets[0] == "g:dec.Wp"
    assert_fault_caught(fails, order, targets)


def test_weighted_emulation_takes_both_sigmoid_branches():
    """The planted faults (a) / (b) need edges on both branches of edge_ce_terms, and logits
    large enough for the sigmoid to matter: true at the emulated cases' own operands."""
    for key in ("n200_d16", "n130_d64"):
        cfg, batch, p, eps, plan, b = emulation(key, True)
        rows = np.repeat(np.arange(len(batch.rowptr) - 1), np.diff(batch.rowptr))
        Le = (b["ZB"][rows] * b["ZB"][batch.colidx]).sum(1)
        assert (Le < -1).mean() > 0.02 and (Le > 1).mean() > 0.02, (key, (Le < -1).mean(), (Le > 1).mean())


_SEEDED = sorted({(c[0].replace("_chain", ""),) + c[1:6] + c[7:] for c in O.CASES}, key=lambda c: c[0])


@pytest.mark.parametrize("name,topology,n,d,B,kbar,weighted", _SEEDED,
                         ids=["-".join(str(v) for v in c[:6]) for c in _SEEDED])
def test_committed_seeds_keep_the_oracle_off_the_kink(name, topology, n, d, B, kbar, weighted):
    """(The forward pre-activations do not depend on the loss weights; the "_w" twins are
    asserted all the same.)"""
    cfg, batch, p, eps = O.make_case(topology, n, d, B, kbar, weighted)
    assert (cfg.pos_weight != 1.0 and cfg.norm != 1.0 and cfg.beta == O.WEIGHTED_BETA) == weighted
    adj = [batch.sparse_adj(i) for i in range(B)]
    _, _, c = R.forward_backward(p, adj, batch.features, batch.feature_truth, batch.spatial_truth,
                                 eps.astype(np.float64), cfg, want_grads=False, row_chunk=512)
    k = O.oracle_kinks(c, p)
    assert max(k.values()) <= O.KINK_CAP, k


def test_e32_is_the_conditioning_not_the_kink():
    """C2 bench-batch fp32 bars are max(2e-4, 10 e32).  With the oracle's lrelu' overridden at
    one decoder pre-activation (what the test does where the fp32 step ties at the kink), the
    kink-aligned gradient is 1e-3..1e-2 of a block away from the plain one; e32 is computed
    against the PLAIN gradient and stays at its no-kink value."""
    import parity_bars as PB
    cfg = tscale(25, 16)
    B = 2
    batch, p, eps = case(cfg, B)
    adj = [batch.dense_adj(i) for i in range(B)]
    args = (adj, batch.features, batch.feature_truth, batch.spatial_truth, eps.astype(np.float64), cfg)
    _, rg, c = R.forward_backward(p, *args)
    # a pre-activation at the kink: beta moved so that T1[r, col] = +1e-4 |beta| (fp32 resolves
    # it, so the torch-fp32 run keeps the oracle's side), the step takes the other side
    r, col = 20, 7
    p = {k: v.copy() for k, v in p.items()}
    p["dec.bn1.beta"][col] -= c["T1"][r, col] * (1 - 1e-4)
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    _, rg, c = R.forward_backward(p, *args)
    t = c["T1"][r, col]
    assert 0 < abs(t) < 1e-3 * abs(c["T1"]).max()
    over = np.full(c["T1"].shape, np.nan)
    over[r, col] = 0.2 if t >= 0 else 1.0
    rg_kink = R.forward_backward(p, *args, lrelu_override={"T1": over})[1]
    e_plain = PB.e32_grads(p, adj, *args[1:5], cfg, rg)
    e_kink = PB.e32_grads(p, adj, *args[1:5], cfg, rg_kink)
    assert max(e_plain.values()) < 2e-5, e_plain
    moved = [k for k in rg if e_kink[k] > 10 * max(e_plain[k], 2e-5)]
    assert "dec.K1" in moved and "dec.bn1.beta" in moved, e_kink
