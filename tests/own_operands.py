"""Own-operand references for every link of the bf16 step (plain NumPy, no GPU needed).

The bf16 plan materialises the whole chain of the step in named workspace buffers.  Each
*link* below takes its inputs exactly as they sit in HBM (bf16 / fp32 buffers, the CSR, the
fp32 parameters -- rounded to bf16 where the kernel reads a packed bf16 weight image) and
returns a ``Link``:

* ``ref``  the operation in float64 on those inputs (products of bf16 values are exact in
  float64, so the GPU may differ only by its fp32 arithmetic and one output rounding),
* ``mag``  the sum of the absolute values of the terms added to form each element,
* ``K``    the number of terms summed into an element,
* ``stored``  "bf16" or "f32": the format of the buffer the link writes,
* ``extra``  a derived absolute allowance (transcendentals, roundings before a sum),
* ``excl``  elements on the lrelu kink (see below), not compared.

Bounds, all derived (none comes from a GPU measurement):

* base, every link: ``(K + 4) 2^-23 mag`` -- fp32 accumulation of K terms in any order
  (each partial sum is at most mag, each add rounds by 2^-24 relative; the factor 2 and the
  "+ 4" cover the handful of fp32 multiplies of an epilogue, gamma * c, lrelu's 0.2 x, ...);
* a bf16-stored output adds ``2^-8 |ref|``: one bf16 ulp, half for round-to-nearest-even
  and half for an fp32 value that sits on a rounding boundary;
* a link through exp / sigmoid adds 1e-6 relative of the transcendental's value (v_exp_f32,
  v_rcp_f32: 1 ulp each, plus the argument's scaling to base 2), as
  ``parity_bars.own_structure`` already allows;
* the per-edge coefficient (pw - 1) sigmoid(L) - pw of the weighted CE adds, per edge,
  |pw - 1| (sigmoid' dL + 1e-6 sigmoid) |z_j| with dL the fp32 bound of the d-term logit
  (tests/zzt_ops.py derives the stand-alone op's the same way); exactly zero at pw = 1;
* a sum of values that an upstream link could not pin exactly (an intermediate the plan
  does not materialise, kink elements) carries that upstream bound, propagated.

The lrelu kink: lrelu' is discontinuous at 0, and the GPU evaluates the pre-activation
T = y gamma c + beta in fp32 from the STORED fp32 y (RC_DECBWD / head_rows epilogues), so it
may land on the other side of 0 only where |T| <= 2^-22 (|y gamma c| + |beta|) (two fp32
roundings); such elements are excluded and counted (cap: 4 per buffer and case).  The
encoder's P1 is read back as stored, its sign is exact: nothing is excluded; P0 is
recomputed as AX W0 (f <= 4 terms): excluded where |P0| <= 2^-22 sum |AX W0|.

Rounding points were read from the epilogues (snd_fast.hip rowconv_kernel / head_rows,
snd_fast_enc.hip gcn0_kernel / spmm_row_epilogue / reparam_prep_kernel, snd_common.hpp
reparam_bwd_elem, snd_zzt.hip v7 / v9, snd_tref.hip), not from the oracle; the fused
kernels are bitwise equal to the row-engine chain (tests/test_gpu_step.py), so one
reference per link serves both.

``step_links`` is a generator over all links in step order; it reads its operands from a
dict of buffers lazily, so the same code serves three uses:

* check:     the dict holds the GPU's (or an emulation's) buffers; every link is compared;
* compose:   float64, no rounding, unrounded parameters -- each link's ref is stored as the
             next link's operand; must reproduce oracle/ref_numpy.forward_backward;
* emulate:   float32 arithmetic (np.float32 matmuls) + bf16 round-to-nearest-even stores: a
             correct implementation that the bounds must admit.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, Optional

import numpy as np

U23 = 2.0 ** -23
BF_ULP = 2.0 ** -8
KINK = 2.0 ** -22
TRANS = 1e-6
BN_C = 1.0 / math.sqrt(1.0 + 1e-3)
SQRT_LOG2E = 1.2011224087864498          # reparam_prep_kernel's sc (fp32 constant)
INV_SQRT_LOG2E = 0.8325546111576977      # snd_zzt.hip kInvSqrtLog2e
LN2 = math.log(2.0)
KINK_CAP = 4


def bf16(a):
    """Round to bf16 (nearest even) and back, as float64."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(torch.bfloat16).to(torch.float32).numpy().astype(np.float64)


def ident(a):
    return np.asarray(a, np.float64)


@dataclass
class Link:
    ref: np.ndarray
    mag: np.ndarray
    K: object                 # int or an array broadcastable to ref
    stored: str = "f32"
    extra: object = 0.0
    excl: Optional[np.ndarray] = None

    def bound(self):
        ref = np.asarray(self.ref, np.float64)
        b = (np.asarray(self.K, np.float64) + 4.0) * U23 * np.asarray(self.mag, np.float64) + self.extra
        if self.stored == "bf16":
            b = b + BF_ULP * np.abs(ref)
        return np.broadcast_to(b, ref.shape)

    def ratio(self, got):
        """(worst |got - ref| / bound over the compared elements, #excluded)."""
        ref = np.asarray(self.ref, np.float64)
        got = np.asarray(got, np.float64).reshape(ref.shape)
        err = np.abs(got - ref)
        b = self.bound()
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0.0, 0.0, err / b)
        r = np.where(np.isfinite(got), r, np.inf)
        nex = 0
        if self.excl is not None:
            nex = int(self.excl.sum())
            r = np.where(self.excl, 0.0, r)
        return (float(r.max()) if r.size else 0.0), nex


# ---------------------------------------------------------------- primitives (dtype dt)
def lrelu(x):
    return np.maximum(x, x.dtype.type(0.2) * x)


def lrelu_grad(x):
    return np.where(x >= 0, x.dtype.type(1.0), x.dtype.type(0.2))


def csr(batch, dt):
    import scipy.sparse as sp
    R = len(batch.rowptr) - 1
    return sp.csr_matrix((np.ones(len(batch.colidx), dt), batch.colidx.astype(np.int64),
                          batch.rowptr.astype(np.int64)), shape=(R, R))


def conv_fwd(x, w, n):
    """per graph: out[r] = sum_t x[r + t - 2] @ w[t] (k = 5 SAME, zero outside the graph)."""
    B = x.shape[0] // n
    xp = np.pad(x.reshape(B, n, -1), ((0, 0), (2, 2), (0, 0)))
    out = 0
    for t in range(5):
        out = out + xp[:, t:t + n] @ w[t]
    return out.reshape(B * n, -1)


def conv_bwd_data(dy, w, n):
    """per graph: dx[r] = sum_t dy[r + 2 - t] @ w[t]^T."""
    B = dy.shape[0] // n
    dp = np.pad(dy.reshape(B, n, -1), ((0, 0), (2, 2), (0, 0)))
    out = 0
    for t in range(5):
        out = out + dp[:, 4 - t:4 - t + n] @ w[t].T
    return out.reshape(B * n, -1)


def conv_wgrad(x, dy, n):
    """dW[t] = sum_r x[r + t - 2]^T dy[r] over the rows of every graph."""
    B = x.shape[0] // n
    xp = np.pad(x.reshape(B, n, -1), ((0, 0), (2, 2), (0, 0)))
    d = dy.reshape(B, n, -1)
    return np.stack([np.einsum("bnk,bno->ko", xp[:, t:t + n], d) for t in range(5)])


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def edge_sigmoid(x):
    """sigmoid(x) as edge_ce_terms (snd_common.hpp) orders it, in x's dtype: e = e^-|x|,
    r = 1 / (1 + e), r for x >= 0 and e r below."""
    e = np.exp(-np.abs(x))
    r = 1 / (1 + e)
    return np.where(x >= 0, r, e * r)


def edge_coef(x, pw):
    """The per-edge gradient coefficient of an A = 1 pair with logit x on top of the dense
    kernel's sigmoid(x): -pw + (pw - 1) sigmoid(x); -pw alone at pw == 1 (the early-out)."""
    coef = np.full(x.shape, -pw, x.dtype)
    if pw != 1:
        coef = coef + (pw - 1) * edge_sigmoid(x)
    return coef


def loss_scales(cfg, B, n, RH, L, k32):
    """(pos_weight, adj_scale, kl_scale) as the step forms them (snd_step.hip): the config
    holds pos_weight / norm / beta as floats (``k32``), adj_scale = 2 norm / (B n^2) and
    kl_scale = beta / (RH L) are evaluated in double and passed to the kernels as floats."""
    adj = k32(2.0 * float(k32(cfg.norm)) / (float(B) * n * n))
    klc = k32(float(k32(cfg.beta)) / (float(RH) * L))
    return k32(cfg.pos_weight), adj, klc


def zzt_dp(d):
    """Column padding of the zz^T staging images (snd_zzt.hip zzt_dp)."""
    return 32 if d <= 32 else (64 if d <= 64 else 128)


def djd_graph(Jg, Vg, kinv, d, T, sr, round_s=True, r0=0, r1=None, diag_summed=False):
    """One graph's dJd link (the dense zz^T kernels, snd_zzt.hip), rows [r0, r1): (ref, mag,
    extra).  Jg [n, d] is the K role as stored (log2 units), Vg the V role as stored, kinv the
    factor applied to the sum.  x_ij = J_i . J_j (fp32 MFMA), s_ij = 1 / (1 + 2^-x_ij),
    dJd_i = kinv sum_{j != i} s_ij V_j.  s is within ds of the float64 value (fp32
    accumulation of x, 1e-6 for exp2 / rcp).  ``round_s`` (the bf16 kernels): s is rounded to
    bf16 (``sr``) before the second MFMA; where a rounding boundary lies within ds the term
    may differ by one bf16 ulp of s, and those terms' |V_j| ulp(s) are the extra.  Otherwise
    (the f32 kernels) the extra is ds |V| itself.  ``diag_summed``: the kernel adds s_ii V_i
    with the tile and subtracts it afterwards (v4 / v7 / v9: no mask in the tile loop), so the
    fp32 sum holds that term twice: 2 |s_ii V_i| joins mag (it matters where n is small)."""
    f64 = np.float64
    r1 = Jg.shape[0] if r1 is None else r1
    idx = np.arange(r1 - r0)
    x = Jg[r0:r1] @ Jg.T
    sg = 1.0 / (1.0 + np.exp2(-x))
    sb = T(sr(sg)) if round_s else T(sg)
    sii = sb[idx, r0 + idx].copy()
    sb[idx, r0 + idx] = 0.0
    ref = (sb @ Vg) * kinv
    mag = (sb @ np.abs(Vg)) * kinv
    if diag_summed:
        mag = mag + 2 * sii[:, None] * np.abs(Vg[r0:r1]) * kinv
    s64 = np.asarray(sg, f64)
    aJ = np.abs(Jg).astype(f64)
    dx = (d + 4) * U23 * (aJ[r0:r1] @ aJ.T)
    ds = s64 * (1 - s64) * LN2 * dx + 2 * TRANS * s64
    if round_s:
        ulp = np.exp2(np.floor(np.log2(np.maximum(s64, 1e-300))) - 7)
        fr = s64 / ulp
        w = (np.abs(fr - np.floor(fr) - 0.5) * ulp <= ds) * ulp   # (the diagonal too: s_ii is
        # evaluated twice, in the tile and in the per-row correction that subtracts it)
    else:
        w = ds
        w[idx, r0 + idx] = 0.0                                    # masked, never evaluated
    return ref, mag, (w @ np.abs(Vg).astype(f64)) * float(kinv)


class Plan:
    """What the plan decided and the test asserted: the K tails (columns of the operand past
    the packed bf16 image, multiplied by the fp32 weight rows: rowconv_kernel's ``wtail``)
    and whether conv3's FY3 / FU3 are materialised (row-engine decoder only)."""

    def __init__(self, cfg, fy3: bool, compose: bool = False):
        f, (h0, h1) = cfg.f_in, cfg.g_conv_hidden
        self.kw1 = h0 + f if h0 + f <= 128 else h0           # snd_step.hip: kw1 / kwh
        self.kwh = h1 + f if h1 + f <= 128 else h1
        self.fy3 = fy3
        self.compose = compose
        self.tref = cfg.topology == "tref"


# ---------------------------------------------------------------- the step, link by link
def step_links(b: Dict[str, np.ndarray], p, batch, cfg, plan: Plan, dt=np.float64,
               wr: Callable = bf16, sr: Callable = bf16):
    """Yield (name, Link) for every link in step order.  ``b`` holds the operands (logical
    layouts: no row padding, [s | n] columns adjacent); a link's own output must be in ``b``
    before the generator is resumed.  ``wr`` rounds a weight the kernels read as a packed
    bf16 image, ``sr`` a value the kernel rounds to bf16 in registers (identity to compose).
    Names "g:<block>" are gradient blocks, "l:<term>" loss sums."""
    f64 = np.float64
    T = lambda a: np.asarray(a, dt)
    n, B = cfg.n_nodes, batch.n_graphs
    R = n * B
    L, f = cfg.latent, cfg.f_in
    h0, h1 = cfg.g_conv_hidden
    gh, dj = cfg.g_hidden_size, cfg.node_h_size
    W = h1 + f
    s1, s2, s3 = cfg.s_d_channel
    n1, n2 = cfg.n_d_channel
    sd, nf = cfg.spatial_dim, cfg.num_feature
    c = dt(BN_C)
    A = csr(batch, dt)
    deg = np.diff(batch.rowptr).astype(f64)[:, None]
    X, S, Xf = T(batch.features), T(batch.spatial_truth), T(batch.feature_truth)
    P = {k: T(v) for k, v in p.items()}
    W_ = lambda k: T(wr(p[k]))                       # packed bf16 image of a weight
    ab = np.abs

    def lin(x, w, bias=None):
        ref, mag = x @ w, ab(x) @ ab(w)
        if bias is not None:
            ref, mag = ref + bias, mag + ab(bias)
        return ref, mag

    def tailed(name, k0):
        """weight rows [0, k0) from the bf16 image, the rest (K tail) in fp32."""
        w = P[name]
        return np.concatenate([W_(name)[:k0], w[k0:]], 0) if k0 < w.shape[0] else W_(name)

    # ================= encoder forward (gcn0_kernel / enc_front_kernel)
    yield "AX", Link(A @ X, A @ ab(X), deg)
    AX = T(b["AX"])
    yield "AXB", Link(AX, ab(AX), 0, "bf16")
    g0c, g1c, gec = P["enc.bn0.gamma"] * c, P["enc.bn1.gamma"] * c, P["enc.bne.gamma"] * c
    P0, P0m = lin(AX, P["enc.W0"])                    # W0 in fp32 (f <= 4 terms)
    yield "FH1", Link(np.concatenate([lrelu(P0) * g0c + P["enc.bn0.beta"], X], 1),
                      np.concatenate([P0m * ab(g0c) + ab(P["enc.bn0.beta"]), ab(X)], 1), f + 2, "bf16")
    FH1 = T(b["FH1"])
    ref, mag = lin(FH1, tailed("enc.W1", plan.kw1))
    yield "FXW1", Link(ref, mag, h0 + f, "bf16")
    FXW1 = T(b["FXW1"])
    yield "FP1", Link(A @ FXW1, A @ ab(FXW1), deg)
    P1 = T(b["FP1"])
    a1 = lrelu(P1)
    b1v = a1 * g1c + P["enc.bn1.beta"]
    H2 = np.concatenate([b1v, X], 1)
    H2m = np.concatenate([ab(a1 * g1c) + ab(P["enc.bn1.beta"]), ab(X)], 1)
    yield "FG", Link(H2 * gec + P["enc.bne.beta"], H2m * ab(gec) + ab(P["enc.bne.beta"]), 3, "bf16")
    FG = T(b["FG"])

    if not plan.tref:
        # ============= node-latent heads (RC_LIN x2 / head_fwd_kernel), reparameterisation
        ref, mag = lin(FG, tailed("enc.Wh", plan.kwh), P["enc.bh"])
        yield "FHH", Link(ref, mag, W + 1, "bf16")
        FHH = T(b["FHH"])
        ref, mag = lin(FHH, W_("enc.Wms"), P["enc.bms"])
        yield "MS", Link(ref, mag, gh + 1)
        MS, EPS = T(b["MS"]), T(b["EPS"])
        mu, s = MS[:, :L], MS[:, L:]
        es = np.exp(s)
        yield "Z", Link(mu + EPS * es, ab(mu) + ab(EPS * es), 2, extra=TRANS * ab(EPS * es).astype(f64))
        Z = T(b["Z"])
        yield "ZB", Link(Z, ab(Z), 0, "bf16")
    else:
        # ============= graph-latent heads and projection (snd_tref.hip: fp32 weight streams
        # over the bf16 G; small_head_fwd / gemm + reparam_fwd; all fp32-stored)
        ref, mag = lin(FG.reshape(B, n * W), P["enc.Wh"], P["enc.bh"])
        yield "Hh", Link(ref, mag, n * W + 1)
        Hh = T(b["Hh"])
        ref, mag = lin(Hh, P["enc.Wms"], P["enc.bms"])
        yield "MS", Link(ref, mag, gh + 1)
        MS, EPS = T(b["MS"]), T(b["EPS"])
        mu, s = MS[:, :L], MS[:, L:]
        es = np.exp(s)
        yield "ZL", Link(mu + EPS * es, ab(mu) + ab(EPS * es), 2, extra=TRANS * ab(EPS * es).astype(f64))
        ZL = T(b["ZL"])
        ref, mag = lin(ZL, P["dec.Wp"], P["dec.bp"])
        yield "Z", Link(ref.reshape(R, dj), mag.reshape(R, dj), L + 1)
        Z = T(b["Z"])
        yield "ZB", Link(Z, ab(Z), 0, "bf16")
    # KL sum (kl_elem: -(expm1(2s) - 2s) - mu^2 per element in fp32, fp64 sums): per element
    # ~8 fp32 roundings of terms no larger than |expm1(2s) - 2s| + mu^2, exp where |2s| >= 1/2
    x2 = 2 * s
    if dt is np.float64:
        br = np.expm1(x2) - x2
    else:   # kl_elem's own branches: the Taylor series below |2s| = 1/2, else (e^x - 1) - x
        tl = np.zeros_like(x2) + dt(1.0 / 3628800.0)
        for k in (362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0, 2.0):
            tl = tl * x2 + dt(1.0 / k)
        br = np.where(ab(x2) < 0.5, x2 * x2 * tl, (np.exp(x2) - 1) - x2)
    kle = -br - mu * mu
    klm = ab(br) + mu * mu
    klx = np.where(ab(2 * s) >= 0.5, np.exp(2 * s) + 1.0 + ab(2 * s), 0.0)
    yield "l:kl_sum", Link(np.array(kle.sum(dtype=f64)), np.array(klm.sum(dtype=f64) + klx.sum(dtype=f64)), 4,
                           extra=TRANS * float(klx.sum(dtype=f64)))
    ZB = T(b["ZB"])
    # zz^T staging rows (reparam_prep_kernel): bf16(z * sqrt(log2 e)), one fp32 multiply
    sc = dt(SQRT_LOG2E)
    yield "JROW", Link(Z * sc, ab(Z * sc), 0, "bf16")
    J = T(b["JROW"])

    # ================= structure term: dJd of the dense kernel (snd_zzt.hip v7 / v9)
    # x_ij = J_i . J_j (fp32 MFMA), s_ij = bf16(1 / (1 + 2^-x_ij)) -- the operand of the second
    # MFMA -- dJd_i = (sum_j s_ij J_j - bf16(s_ii) J_i) / sqrt(log2 e).  The fp32 x may move s
    # across a bf16 rounding boundary: s is within ds of the float64 value (fp32 accumulation
    # of x, 1e-6 for exp2 / rcp), and where a boundary lies within ds the term may differ by
    # one bf16 ulp of s: those terms' |J_j| ulp(s) are added to the bound.
    # d <= 32 runs v4: its second MFMA reads the transposed image of the UNSCALED bf16 z (== ZB),
    # and nothing is divided out; v7 / v9 (d = 64, 128) read the scaled rows for both products.
    scaled = zzt_dp(dj) >= 64 or plan.compose
    kinv = dt(INV_SQRT_LOG2E) if scaled else dt(1.0)
    refs, mags, exts = [], [], []
    for g in range(B):
        Jg = J[g * n:(g + 1) * n]
        r, m, e = djd_graph(Jg, Jg if scaled else ZB[g * n:(g + 1) * n], kinv, dj, T, sr)
        refs.append(r), mags.append(m), exts.append(e)
    yield "DJD", Link(np.concatenate(refs), np.concatenate(mags), n + 2, extra=np.concatenate(exts))
    DJD = T(b["DJD"])

    # ================= decoder forward (RC_FWD x3 + head_rows / dec_chain_fwd)
    def bn_lrelu(y, gam, bet):
        gc = gam * c
        return Link(lrelu(y * gc + bet), ab(y * gc) + ab(bet), 2, "bf16")

    def kink(y, gam, bet, dy=0.0):
        gc = np.asarray(gam, f64) * BN_C
        y, bet = np.asarray(y, f64), np.asarray(bet, f64)
        return np.abs(y * gc + bet) <= KINK * (np.abs(y * gc) + np.abs(bet)) + dy * np.abs(gc)

    ref, mag = conv_fwd(ZB, W_("dec.K1"), n), conv_fwd(ab(ZB), ab(W_("dec.K1")), n)
    yield "FY1", Link(ref + P["dec.b1"], mag + ab(P["dec.b1"]), 5 * dj + 1)
    Y1 = T(b["FY1"])
    yield "FU1", bn_lrelu(Y1, P["dec.bn1.gamma"], P["dec.bn1.beta"])
    U1 = T(b["FU1"])
    K2s, K2n, K3s = W_("dec.K2s"), W_("dec.K2n"), W_("dec.K3s")
    b2 = np.concatenate([P["dec.b2s"], P["dec.b2n"]])
    g2 = np.concatenate([P["dec.bn2s.gamma"], P["dec.bn2n.gamma"]])
    be2 = np.concatenate([P["dec.bn2s.beta"], P["dec.bn2n.beta"]])
    ref = np.concatenate([conv_fwd(U1[:, :s1], K2s, n), conv_fwd(U1[:, s1:], K2n, n)], 1)
    mag = np.concatenate([conv_fwd(ab(U1[:, :s1]), ab(K2s), n), conv_fwd(ab(U1[:, s1:]), ab(K2n), n)], 1)
    yield "FY2", Link(ref + b2, mag + ab(b2), 5 * max(s1, n1) + 1)
    Y2 = T(b["FY2"])
    yield "FU2", bn_lrelu(Y2, g2, be2)
    U2 = T(b["FU2"])
    y3 = Link(conv_fwd(U2[:, :s2], K3s, n) + P["dec.b3s"],
              conv_fwd(ab(U2[:, :s2]), ab(K3s), n) + ab(P["dec.b3s"]), 5 * s2 + 1)
    g3c = P["dec.bn3s.gamma"] * c
    if plan.fy3 or plan.compose:
        yield "FY3", y3
        Y3 = T(b["FY3"])
        dY3 = 0.0                                                     # stored: exact operand
        u3 = bn_lrelu(Y3, P["dec.bn3s.gamma"], P["dec.bn3s.beta"])
        u3.stored = "f32"                                             # conv3's U is fp32 (head input)
        yield "FU3", u3
        U3 = T(b["FU3"])
        dU3 = 0.0
    else:
        # the fused decoder keeps conv3's Y / U in LDS: the heads are referred to FU2, with
        # conv3's own derived bound carried through BN / lrelu (slope <= 1) and the head sum
        Y3 = y3.ref
        dY3 = y3.bound()
        U3 = lrelu(Y3 * g3c + P["dec.bn3s.beta"])
        dU3 = dY3 * np.abs(np.asarray(g3c, f64)) + 4 * U23 * (np.abs(Y3 * g3c) + np.abs(P["dec.bn3s.beta"])).astype(f64)

    def head(U, dU, Wn, bn, cout):
        zo, zm = lin(U, P[Wn], P[bn])
        y = sigmoid(zo)
        dz = (U.shape[1] + 5) * U23 * zm.astype(f64) + (dU @ np.abs(P[Wn]).astype(f64) if np.ndim(dU) else 0.0)
        return Link(y, np.zeros_like(y), 0, extra=0.25 * dz + 2 * TRANS * np.asarray(y, f64))

    yield "SHAT", head(U3, dU3, "dec.Ws", "dec.bs", sd)
    SH = T(b["SHAT"])
    yield "XHAT", head(U2[:, s2:], 0.0, "dec.Wn", "dec.bn", nf)
    XH = T(b["XHAT"])
    # SSE sums: fp32 diff (one rounding), squared and summed in fp64
    for nm, Y, Tg in (("l:sse_s", SH, S), ("l:sse_n", XH, Xf)):
        e2 = np.asarray(((Y - Tg) ** 2), f64).sum()
        yield nm, Link(np.array(e2), np.array(e2), 0)

    # ================= decoder backward (head_rows, RC_DECBWD x2, RC_LIN / dec_chain_bwd)
    def head_bwd(Yh, Tg, Wn, U, dU, ypre, dy_pre, gam, bet):
        """dp = 2 (yh - t) / count * yh (1 - yh) from the STORED yhat; du = dp W^T;
        dt = du lrelu'(y gamma c + beta); dy = dt gamma c.  ~6 fp32 roundings in dp."""
        cnt = dt(Yh.size)
        dp = dt(2.0) * (Yh - Tg) / cnt * Yh * (1 - Yh)
        w = P[Wn]
        du, dum = dp @ w.T, ab(dp) @ ab(w.T)
        gc = gam * c
        dtv = du * lrelu_grad(ypre * gc + bet)
        out = Link(dtv * gc, dum * ab(gc), Yh.shape[1] + 6, "bf16", excl=kink(ypre, gam, bet, dy_pre))
        # parameter gradients from the same registers (column sums in fp32, R rows)
        KR = R + Yh.shape[1] + 6
        ex = out.excl
        lost = lambda v: np.where(ex, 0.8 * np.abs(np.asarray(v, f64)), 0.0).sum(0)   # a kink element's term
        dUa = dU if np.ndim(dU) else np.zeros(U.shape)
        dYa = dy_pre if np.ndim(dy_pre) else np.zeros(U.shape)
        grads = {
            "W": Link(U.T @ dp, ab(U.T) @ ab(dp), KR, extra=dUa.T @ np.abs(np.asarray(dp, f64))),
            "b": Link(dp.sum(0), ab(dp).sum(0), KR),
            "gamma": Link((dtv * ypre).sum(0) * c, ab(dum * ypre).sum(0) * c, KR,
                          extra=lost(dum * ypre) + (np.abs(np.asarray(dum, f64)) * dYa).sum(0)),
            "beta": Link(dtv.sum(0), dum.sum(0), KR, extra=lost(dum)),
            "bias": Link((dtv * gc).sum(0), (dum * ab(gc)).sum(0), KR, extra=lost(dum * gc)),
        }
        return out, grads

    dy3, g3 = head_bwd(SH, S, "dec.Ws", U3, dU3, Y3, dY3, P["dec.bn3s.gamma"], P["dec.bn3s.beta"])
    yield "FDY3", dy3
    DY3 = T(b["FDY3"])
    dy2n, g2n = head_bwd(XH, Xf, "dec.Wn", U2[:, s2:], 0.0, Y2[:, s2:], 0.0, P["dec.bn2n.gamma"],
                         P["dec.bn2n.beta"])

    def dec_bwd(acc, accm, ypre, gam, bet, K):
        """RC_DECBWD epilogue: dt = acc lrelu'(y gamma c + beta), o = dt gamma c (bf16);
        column partials {dt y, dt, o} from the fp32 values before that rounding."""
        gc = gam * c
        dtv = acc * lrelu_grad(ypre * gc + bet)
        out = Link(dtv * gc, accm * ab(gc), K + 2, "bf16", excl=kink(ypre, gam, bet))
        ex = out.excl
        lost = lambda v: np.where(ex, 0.8 * np.abs(np.asarray(v, f64)), 0.0).sum(0)
        KR = R + K + 2
        return out, {"gamma": Link((dtv * ypre).sum(0) * c, ab(accm * ypre).sum(0) * c, KR, extra=lost(accm * ypre)),
                     "beta": Link(dtv.sum(0), accm.sum(0), KR, extra=lost(accm)),
                     "bias": Link((dtv * gc).sum(0), (accm * ab(gc)).sum(0), KR, extra=lost(accm * gc))}

    dy2s, g2s = dec_bwd(conv_bwd_data(DY3, K3s, n), conv_bwd_data(ab(DY3), ab(K3s), n), Y2[:, :s2],
                        P["dec.bn2s.gamma"], P["dec.bn2s.beta"], 5 * s3)
    yield "FDY2", Link(np.concatenate([dy2s.ref, dy2n.ref], 1), np.concatenate([dy2s.mag, dy2n.mag], 1),
                       max(dy2s.K, dy2n.K), "bf16", excl=np.concatenate([dy2s.excl, dy2n.excl], 1))
    DY2 = T(b["FDY2"])
    acc = np.concatenate([conv_bwd_data(DY2[:, :s2], K2s, n), conv_bwd_data(DY2[:, s2:], K2n, n)], 1)
    accm = np.concatenate([conv_bwd_data(ab(DY2[:, :s2]), ab(K2s), n),
                           conv_bwd_data(ab(DY2[:, s2:]), ab(K2n), n)], 1)
    dy1, g1 = dec_bwd(acc, accm, Y1, P["dec.bn1.gamma"], P["dec.bn1.beta"], 5 * max(s2, n2))
    yield "FDY1", dy1
    DY1 = T(b["FDY1"])
    K1 = W_("dec.K1")
    yield "DZDEC", Link(conv_bwd_data(DY1, K1, n), conv_bwd_data(ab(DY1), ab(K1), n), 5 * (s1 + n1))
    DZDEC = T(b["DZDEC"])

    # ---- decoder parameter gradients (wgrad_kernel: bf16 x, bf16 dy, fp32 slabs; the
    # column partials above; head_rows' {u dp, dp})
    def wg(x, dy):
        return Link(conv_wgrad(x, dy, n), conv_wgrad(ab(x), ab(dy), n), R)

    yield "g:dec.K3s", wg(U2[:, :s2], DY3)
    yield "g:dec.K2s", wg(U1[:, :s1], DY2[:, :s2])
    yield "g:dec.K2n", wg(U1[:, s1:], DY2[:, s2:])
    yield "g:dec.K1", wg(ZB, DY1)
    for pre, g in (("dec.bn3s", g3), ("dec.bn2n", g2n), ("dec.bn2s", g2s), ("dec.bn1", g1)):
        yield f"g:{pre}.gamma", g["gamma"]
        yield f"g:{pre}.beta", g["beta"]
    yield "g:dec.b3s", g3["bias"]
    yield "g:dec.b2n", g2n["bias"]
    yield "g:dec.b2s", g2s["bias"]
    yield "g:dec.b1", g1["bias"]
    yield "g:dec.Ws", g3["W"]
    yield "g:dec.bs", g3["b"]
    yield "g:dec.Wn", g2n["W"]
    yield "g:dec.bn", g2n["b"]

    # ================= dJ -> d[mu | s]
    # The per-edge terms (edge_ce_terms: head_bwd_kernel, the d = 128 edge + reparam kernel,
    # edge_bf16_kernel), never materialised on the fused paths: L_ij = ZB_i . ZB_j over the
    # stored bf16 z (fp32 sum of d exact products), coef_ij = (pw - 1) sigmoid(L_ij) - pw on
    # top of the dense kernel's sigmoid, e_i = sum_j coef_ij ZB_j over the row's neighbours.
    # The coefficient's own error (the fp32 logit through sigmoid', 1e-6 of the sigmoid for
    # exp / rcp and the two roundings that form coef) times |ZB_j| is the extra; at pw == 1
    # the coefficient is -1, its error exactly zero and e_i = -sum_j z_j.
    k32 = (lambda v: v) if plan.compose else np.float32       # the step passes them as floats
    RH = B if plan.tref else R
    pw, adj, klc = (dt(v) for v in loss_scales(cfg, B, n, RH, L, k32))
    ei = np.repeat(np.arange(R), np.diff(batch.rowptr))
    ej_ = batch.colidx.astype(np.int64)
    Le = (ZB[ei] * ZB[ej_]).sum(1)
    coef = edge_coef(Le, pw)
    if pw != 1:
        L64, pw64 = np.asarray(Le, f64), float(pw)
        dLe = (dj + 4) * U23 * (np.abs(ZB[ei]).astype(f64) * np.abs(ZB[ej_]).astype(f64)).sum(1)
        sg = sigmoid(L64)
        dcoef = abs(pw64 - 1.0) * (sg * (1 - sg) * dLe + TRANS * sg)
    else:
        dcoef = np.zeros(len(ei))
    rp, ci = batch.rowptr.astype(np.int64), batch.colidx.astype(np.int64)
    import scipy.sparse as sp
    C = sp.csr_matrix((coef, ci, rp), shape=(R, R))
    EJ, EJm = C @ ZB, abs(C) @ ab(ZB)
    EJx = float(abs(adj)) * (sp.csr_matrix((dcoef, ci, rp), shape=(R, R)) @ np.abs(ZB).astype(f64))

    def reparam_bwd(dz, dzm, Kz, stored, dzx=0.0):
        """reparam_bwd_elem: dm = kl mu + dz; dl = dz eps e^s + kl (e^2s - 1); ``dzx``: an
        absolute allowance on dz, carried into both halves."""
        dm, dmm = klc * mu + dz, ab(klc * mu) + dzm
        dl = dz * EPS * es + klc * (es * es - 1)
        dlm = dzm * ab(EPS * es) + ab(klc) * (es * es + 1)
        ext = TRANS * np.asarray(ab(dz * EPS * es) + 2 * ab(klc) * es * es, f64)
        return Link(np.concatenate([dm, dl], 1), np.concatenate([dmm, dlm], 1), Kz + 4, stored,
                    extra=np.concatenate([np.zeros(dm.shape) + dzx, ext + dzx * np.asarray(ab(EPS * es), f64)], 1))

    if not plan.tref:
        dz = adj * (DJD + EJ) + DZDEC
        # (the kernel adds the zz^T column-split partials in fp32 first: their |.| sum if given)
        dzm = ab(adj) * (T(b.get("DJD_abs", ab(DJD))) + EJm) + ab(DZDEC)
        dms = reparam_bwd(dz, dzm, deg + 4, "bf16", EJx)
        yield "FDMS", dms
        DMS = T(b["FDMS"])
        # the [mu | s] bias gradient: column sums of the fp32 values before the bf16 rounding
        yield "g:enc.bms", Link(dms.ref.sum(0), dms.mag.sum(0), R + 8, extra=np.asarray(dms.extra, f64).sum(0))
        yield "g:enc.Wms", Link(FHH.T @ DMS, ab(FHH.T) @ ab(DMS), R)
        Wms = W_("enc.Wms")
        dh = Link(DMS @ Wms.T, ab(DMS) @ ab(Wms.T), 2 * L, "bf16")
        yield "FDH", dh
        DH = T(b["FDH"])
        yield "g:enc.bh", Link(dh.ref.sum(0), dh.mag.sum(0), R + 2 * L)
        yield "g:enc.Wh", Link(FG.T @ DH, ab(FG.T) @ ab(DH), R)
        Wh = W_("enc.Wh")                              # the backward image holds all W rows
        dg, dgm, Kg = DH @ Wh.T, ab(DH) @ ab(Wh.T), gh
    else:
        # d_sg_lin1 backward, small_head_bwd / reparam_bwd + gemm, tref_head_bwd: all fp32
        dJ = (adj * (DJD + EJ) + DZDEC).reshape(B, n * dj)
        dJm = (ab(adj) * (ab(DJD) + EJm) + ab(DZDEC)).reshape(B, n * dj)
        Kj = float(deg.max()) + 4
        dJx = EJx.reshape(B, n * dj)                   # the edge coefficients' allowance on dJ
        yield "g:dec.Wp", Link(ZL.T @ dJ, ab(ZL.T) @ dJm, B + Kj, extra=np.abs(np.asarray(ZL, f64)).T @ dJx)
        yield "g:dec.bp", Link(dJ.sum(0), dJm.sum(0), B + Kj, extra=dJx.sum(0))
        Wp = P["dec.Wp"]
        yield "DZL", Link(dJ @ Wp.T, dJm @ ab(Wp.T), n * dj + Kj, extra=dJx @ np.abs(np.asarray(Wp, f64)).T)
        DZL = T(b["DZL"])
        yield "DMS", reparam_bwd(DZL, ab(DZL), 0, "f32")
        DMS = T(b["DMS"])
        yield "g:enc.bms", Link(DMS.sum(0), ab(DMS).sum(0), B)
        yield "g:enc.Wms", Link(Hh.T @ DMS, ab(Hh.T) @ ab(DMS), B)
        Wms = P["enc.Wms"]
        yield "DH", Link(DMS @ Wms.T, ab(DMS) @ ab(Wms.T), 2 * L)
        DH = T(b["DH"])
        yield "g:enc.bh", Link(DH.sum(0), ab(DH).sum(0), B)
        Gf = FG.reshape(B, n * W)
        yield "g:enc.Wh", Link(Gf.T @ DH, ab(Gf.T) @ ab(DH), B)
        Wh = P["enc.Wh"]
        yield "FDG", Link((DH @ Wh.T).reshape(R, W), (ab(DH) @ ab(Wh.T)).reshape(R, W), gh, "bf16")
        dg = T(b["FDG"])                               # RC_ENC1 through an identity image: exact
        dgm, Kg = ab(dg), 0

    # ================= encoder backward tail (RC_ENC1, A @ dP1, RC_ENC0)
    dh2 = dg[:, :h1] * gec[:h1]
    dh2m = dgm[:, :h1] * ab(gec[:h1])
    yield "FDP1", Link(dh2 * g1c * lrelu_grad(P1), dh2m * ab(g1c), Kg + 3, "bf16")
    DP1 = T(b["FDP1"])
    KR = R + Kg + 3
    yield "g:enc.bne.gamma", Link((dg * H2).sum(0) * c, (dgm * H2m).sum(0) * c, KR)
    yield "g:enc.bne.beta", Link(dg.sum(0), dgm.sum(0), KR)
    yield "g:enc.bn1.gamma", Link((dh2 * a1).sum(0) * c, (dh2m * ab(a1)).sum(0) * c, KR)
    yield "g:enc.bn1.beta", Link(dh2.sum(0), dh2m.sum(0), KR)
    yield "FDXW1", Link(A @ DP1, A @ ab(DP1), deg, "bf16")
    DXW1 = T(b["FDXW1"])
    yield "g:enc.W1", Link(FH1.T @ DXW1, ab(FH1.T) @ ab(DXW1), R)
    W1b = W_("enc.W1")[:h0]
    db, dbm = DXW1 @ W1b.T, ab(DXW1) @ ab(W1b.T)
    exc0 = np.abs(np.asarray(P0, f64)) <= KINK * np.asarray(P0m, f64)
    yield "FDP0", Link(db * g0c * lrelu_grad(P0), dbm * ab(g0c), h1 + 2, "bf16", excl=exc0)
    DP0 = T(b["FDP0"])
    yield "g:enc.bn0.gamma", Link((db * lrelu(P0)).sum(0) * c, (dbm * P0m).sum(0) * c, R + h1 + f)
    yield "g:enc.bn0.beta", Link(db.sum(0), dbm.sum(0), R + h1)
    AXB = T(b["AXB"])
    yield "g:enc.W0", Link(AXB.T @ DP0, ab(AXB.T) @ ab(DP0), R)


# ---------------------------------------------------------------- drivers
def store(link: Link, rounding=True):
    """The value a correct implementation leaves in the link's buffer."""
    v = np.asarray(link.ref, np.float64)
    if not rounding:
        return v
    v = v.astype(np.float32).astype(np.float64)
    return bf16(v) if link.stored == "bf16" else v


def run_chain(p, batch, eps, cfg, plan: Plan, mode: str, perturb=None):
    """mode "compose": float64, no rounding anywhere (parameters unrounded); "emulate":
    float32 arithmetic + the kernels' roundings.  ``perturb(name, value, bufs)`` may return
    a replacement for a link's stored value (sensitivity tests).  Returns the buffer dict."""
    comp = mode == "compose"
    b = {"EPS": np.asarray(eps, np.float64)}
    it = step_links(b, p, batch, cfg, plan, np.float64 if comp else np.float32,
                    ident if comp else bf16, ident if comp else bf16)
    for name, link in it:
        v = store(link, rounding=not comp)
        if perturb is not None:
            w = perturb(name, v, b)
            if w is not None:
                v = w
        b[name] = v
    return b


def check_all(b, p, batch, cfg, plan: Plan):
    """Every link of the step against the buffers in ``b``: {name: (ratio, n_excluded)}."""
    out = {}
    for name, link in step_links(b, p, batch, cfg, plan):
        if name not in b:
            raise KeyError(f"own_operands: buffer {name} not provided")
        out[name] = link.ratio(b[name])
    return out


def failures(res):
    return sorted(k for k, (r, nx) in res.items() if not r <= 1.0 or nx > KINK_CAP)


def oracle_kinks(cache, p):
    """#elements of the float64 oracle's own pre-activations on the kink, per layer."""
    out = {}
    for nm, pre in (("T1", "dec.bn1"), ("T2s", "dec.bn2s"), ("T2n", "dec.bn2n"), ("T3s", "dec.bn3s")):
        y = cache["Y" + nm[1:]]
        gc, be = p[pre + ".gamma"] * BN_C, p[pre + ".beta"]
        out[nm] = int((np.abs(cache[nm]) <= KINK * (np.abs(y * gc) + np.abs(be))).sum())
    for nm in ("P0", "P1"):
        out[nm] = int((np.abs(cache[nm]) <= KINK * np.abs(cache[nm]).max()).sum())
    return out


# ---------------------------------------------------------------- reading a plan's buffers
def _split(t, a, bw):
    """[s | n] split layout (ColMap): part A at [0, a), part B at [round_up(a, 8), ...)."""
    o = -(-a // 8) * 8
    return np.concatenate([t[:, :a], t[:, o:o + bw]], 1)


def read_plan(model, opt, batch, cfg, fy3: bool):
    """The plan's buffers after one forward_backward, in logical layouts, as float64."""
    import torch
    n, B = cfg.n_nodes, batch.n_graphs
    R = n * B
    L, f = cfg.latent, cfg.f_in
    h0, h1 = cfg.g_conv_hidden
    gh, dj = cfg.g_hidden_size, cfg.node_h_size
    W = h1 + f
    s1, s2, s3 = cfg.s_d_channel
    n1, n2 = cfg.n_d_channel
    tref = cfg.topology == "tref"
    r8 = lambda v: -(-v // 8) * 8
    ld1, ld2, ld3 = r8(r8(s1) + n1), r8(r8(s2) + n2), r8(s3)
    bf, f32 = torch.bfloat16, torch.float32

    def rd(name, dtp, rows, ld, w=None):
        t = model.buffer(name, dtp)[:rows * ld].view(rows, ld).double().cpu().numpy()
        return t if w is None else t[:, :w]

    b = {}
    b["AX"] = rd("AX", f32, R, 4, f)
    b["AXB"] = rd("AXB", bf, R, 8, f)
    b["FH1"] = rd("FH1", bf, R, r8(h0 + f), h0 + f)
    b["FXW1"] = rd("FXW1", bf, R, h1)
    b["FP1"] = rd("FP1", f32, R, h1)
    b["FG"] = rd("FG", bf, R, r8(W), W)
    RH = B if tref else R
    b["MS"] = rd("MS", f32, RH, 2 * L)
    b["EPS"] = rd("EPS", f32, RH, L)
    b["Z"] = rd("Z", f32, R, dj)
    b["ZB"] = rd("ZB", bf, R, dj)
    if tref:
        b["Hh"] = rd("Hh", f32, B, gh)
        b["ZL"] = rd("ZL", f32, B, L)
        for nm, w in (("DZL", L), ("DMS", 2 * L), ("DH", gh)):
            b[nm] = rd(nm, f32, B, w)
        b["FDG"] = rd("FDG", bf, R, r8(W), W)
    else:
        b["FHH"] = rd("FHH", bf, R, gh)
        b["FDMS"] = rd("FDMS", bf, R, 2 * L)
        b["FDH"] = rd("FDH", bf, R, gh)
    npad, dp = -(-n // 128) * 128, zzt_dp(dj)
    jrow = model.buffer("ZSTAGE", bf)[:B * npad * dp].view(B, npad, dp).double().cpu().numpy()
    b["JROW"] = jrow[:, :n, :dj].reshape(R, dj)
    b["JROW_pad"] = float(np.abs(jrow[:, n:, :]).max(initial=0.0)) + float(np.abs(jrow[:, :, dj:]).max(initial=0.0))
    djd = rd("DJD", f32, R, dj)
    dja = np.abs(djd)
    x = model.buffer("DJDX", f32)
    # node latent: the zz^T column-split partials are summed by the kernel that reads dJd
    # (zero where a split is unused); graph latent: zz^T has summed them into DJD itself
    for k in range(0 if tref else x.numel() // (R * dj)):
        part = x[k * R * dj:(k + 1) * R * dj].view(R, dj).double().cpu().numpy()
        djd, dja = djd + part, dja + np.abs(part)
    b["DJD"], b["DJD_abs"] = djd, dja
    b["FY1"] = _split(rd("FY1", f32, R, ld1), s1, n1)
    b["FU1"] = _split(rd("FU1", bf, R, ld1), s1, n1)
    b["FDY1"] = _split(rd("FDY1", bf, R, ld1), s1, n1)
    b["FY2"] = _split(rd("FY2", f32, R, ld2), s2, n2)
    b["FU2"] = _split(rd("FU2", bf, R, ld2), s2, n2)
    b["FDY2"] = _split(rd("FDY2", bf, R, ld2), s2, n2)
    b["FDY3"] = rd("FDY3", bf, R, ld3, s3)
    if fy3:
        b["FY3"] = rd("FY3", f32, R, ld3, s3)
        b["FU3"] = rd("FU3", f32, R, ld3, s3)
    b["SHAT"] = rd("SHAT", f32, R, cfg.spatial_dim)
    b["XHAT"] = rd("XHAT", f32, R, cfg.num_feature)
    b["DZDEC"] = rd("DZDEC", f32, R, dj)
    b["FDP1"] = rd("FDP1", bf, R, h1)
    b["FDXW1"] = rd("FDXW1", bf, R, h1)
    b["FDP0"] = rd("FDP0", bf, R, h0)
    for k, g in opt.grad_blocks().items():
        b["g:" + k] = np.asarray(g, np.float64)
    ld = opt.loss_dict()
    b["l:kl_sum"] = np.array(-2.0 * ld["kl"] * RH * L)
    b["l:sse_s"] = np.array(ld["spatial_cost"] * R * cfg.spatial_dim)
    b["l:sse_n"] = np.array(ld["node_cost"] * R * cfg.num_feature)
    return b


# ---------------------------------------------------------------- the committed cases
# (name, topology, n, d, B, kbar, chain): the smallest shapes that reach each dispatch
# branch of the bf16 plan, every one with partial tiles (tests/test_gpu_own_operands.py).
# Batch seed, init seed and eps seed are fixed below; the float64 oracle's own
# pre-activations stay off the kink for them (tests/test_own_operands_cpu.py).
# The last field, weighted: every case has a twin "<name>_w" at the loss weights of the
# weighted-BCE run -- pos_weight and norm of main.py:246-247 from the case's own batch
# (rounded to float32, as the config struct holds them) and beta = 4 -- so that the sigmoid
# of the per-edge coefficient, norm in adj_scale and beta in kl_scale are all in play.
_SHAPES = (
    ("tscale_n200_d16", "tscale", 200, 16, 3, None, False),
    ("tscale_n300_d32", "tscale", 300, 32, 3, None, False),
    ("tscale_n512_d64", "tscale", 512, 64, 2, None, False),
    ("tscale_n512_d64_chain", "tscale", 512, 64, 2, None, True),
    ("tscale_n1000_d128", "tscale", 1000, 128, 2, None, False),
    ("tscale_n1000_d128_chain", "tscale", 1000, 128, 2, None, True),
    ("tref_n300_d32", "tref", 300, 32, 2, None, False),
    ("tscale_n256_d64_k40", "tscale", 256, 64, 2, 40.0, False),
)
CASES = tuple(c + (False,) for c in _SHAPES) + tuple((c[0] + "_w",) + c[1:] + (True,) for c in _SHAPES)
BATCH_SEED, INIT_SEED, EPS_SEED = 11, 2, 9
WEIGHTED_BETA = 4.0


def weighted_cfg(cfg, batch):
    """cfg at the batch's own class balance (main.py:246-247, as float32) and beta = 4."""
    from snd_vae_amd.input_data import class_balance
    pw, nm = class_balance(batch.n_graphs, cfg.n_nodes, int(batch.rowptr[-1]))
    return cfg.replace(weighted_bce=True, pos_weight=float(np.float32(pw)), norm=float(np.float32(nm)),
                       beta=WEIGHTED_BETA)


def make_case(topology, n, d, B, kbar, weighted=False):
    """(cfg, batch, fp32-exact parameter blocks, fp32 eps) of a committed case."""
    from snd_vae_amd.config import tref, tscale
    from snd_vae_amd.data import synthetic_batch
    from snd_vae_amd.params import init_blocks
    cfg = tscale(n, d) if topology == "tscale" else tref(n, d, g_hidden=16, latent=8)
    batch = synthetic_batch(cfg, B, seed=BATCH_SEED, kbar=kbar)
    if weighted:
        cfg = weighted_cfg(cfg, batch)
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in init_blocks(cfg, INIT_SEED).items()}
    rows = B if topology == "tref" else B * n
    eps = np.random.default_rng(EPS_SEED).standard_normal((rows, cfg.latent)).astype(np.float32)
    return cfg, batch, p, eps


def emulated_fhh(b, p, plan: Plan):
    """h = G Wh + bh in float32 before its bf16 store (sensitivity tests perturb it there)."""
    f32 = np.float32
    w = p["enc.Wh"]
    wi = np.concatenate([bf16(w)[:plan.kwh], w[plan.kwh:]], 0).astype(f32)
    return (b["FG"].astype(f32) @ wi + p["enc.bh"].astype(f32)).astype(np.float64)
