"""Own-operand references, bounds and a float32 emulation for snd_zzt_ce / snd_zzt_ce_rows
(snd_zzt.hip, edge_kernel of snd_spmm.hip), plain NumPy: importable without a GPU.

The ops are a chain of links, each taken in float64 on its operands AS STORED (the rounding
points were read from zzt_prep_kernel and the dense kernels' header comments, not from the
oracle):

* K role   J = T(fl32(z * 1.2011224087864498f)), T = bf16 round-to-nearest-even or float32
           (``jrow`` [B, npad, dp]; x = J_i . J_j is the logit in log2 units);
* V role   bf16, d <= 32 (v4<32>): T(z), the transposed image ``jt`` [B, dp, npad];
           bf16, d = 64 / 128 (v9 / v7): J, the sum times kInvSqrtLog2e;  f32: z;
* colpart  [B, npad / 64, dp]: 64-term fp32 column sums of the stored J;
* dJd      own_operands.djd_graph (the same function the step's DJD link uses), K = n + 2,
           + the column-split count where a launch has splits; f32 kernels: s is not rounded
           to bf16, the transcendental / fp32-accumulation term ds |V| stays;
* ej       edge_kernel on the UNROUNDED fp32 z (both dtypes): coef = (pw - 1) sigma(L) - pw,
           K = degree, 1e-6 on the transcendental where pw != 1;
* dz       2 norm (dJd + ej): the two links' bounds and three fp32 roundings;
* stats[1] pairs - nnz - #{x_ij > 0, i != j} + 2 #{L_edge > 0}: exact up to the pairs whose
           |x| lies within that pair's own fp32 accumulation bound of zero (counted, capped);
* stats[0] |got - ref| <= 1e-6 sum |terms| -- the bar the step's tests hold the same kernels
           to; NOT a worst case, and therefore conditional on the emulation below staying
           under a quarter of it at every case (tests/test_zzt_ops_cpu.py).

``emulate`` is a float32 implementation with the kernels' summation structure (per-64-row
column sums, sum_j x_ij as the fp32 dot J_i . colsum, one fp32 log2 per quad product or per
eight logits, padded pairs added as x = 0 and subtracted per row block, bf16 s before the
second product, double accumulation above that); ``fault`` plants one error into it.

The workspace layouts mirror zzt_stage / snd_zzt_ce / zrows_layout of snd_zzt.hip.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace as NS

import numpy as np

from own_operands import INV_SQRT_LOG2E, LN2, SQRT_LOG2E, TRANS, U23, Link, bf16, djd_graph, ident, zzt_dp

F32, BF16 = 0, 1
SOFTPLUS_M1 = math.log1p(math.exp(-1.0))
NCU = 256                  # MI355X; the GPU test passes the device's own count
ROWS = TJ2 = 128           # rows per row block, columns per split tile (snd_zzt.hip)
S0_BAR = 1e-6              # stats[0]: of sum |terms|
S0_EMU = 0.25              # the emulation's share of that bar
AMB_SMALL_N = 129          # up to here the seeds leave no ambiguous pair
AMB_CAP = 2e-4             # of the case's pairs, beyond
f32 = np.float32


# ---------------------------------------------------------------- geometry (snd_zzt.hip)
def npad(n):
    return -(-n // ROWS) * ROWS


def r256(b):
    return -(-b // 256) * 256


def tsplit_blocks(wgs, n, dtype, ncu=NCU):
    """zzt_tsplit_blocks: column splits of a launch of ``wgs`` row blocks."""
    if dtype != BF16 or wgs >= ncu:
        return 1
    return max(1, min(-(-ncu // wgs), 8, npad(n) // TJ2))


def wpb(d, dtype):
    return 2 if dtype == BF16 and zzt_dp(d) == 64 else 1


def edge_blocks(rows, d):
    lpr = 16 if d >= 64 else d // 4
    return -(-rows // (256 // lpr))


def kernel(d, dtype):
    dp = zzt_dp(d)
    return f"f32<{dp}>" if dtype == F32 else {32: "v4<32>", 64: "v9", 128: "v7"}[dp]


def _stage(B, n, d, dtype):
    """zzt_stage: [jrow | jt | colpart] -> ({name: (byte offset, bytes)}, total bytes)."""
    dp, es = zzt_dp(d), (2 if dtype == BF16 else 4)
    img = B * npad(n) * dp * es
    cp = B * (npad(n) // 64) * dp * 4
    return {"jrow": (0, img), "jt": (r256(img), img), "colpart": (2 * r256(img), cp)}, 2 * r256(img) + r256(cp)


def ws_layout(B, n, d, dtype, ncu=NCU):
    """snd_zzt_ce's carve of its workspace: ({name: (offset, bytes)}, total, splits)."""
    lay, b = _stage(B, n, d, dtype)
    b = r256(b)
    R = B * n
    ts = tsplit_blocks(B * (npad(n) // ROWS), n, dtype, ncu)
    blocks = B * (npad(n) // ROWS) * ts * wpb(d, dtype)
    for name, size in (("ej", R * d * 4), ("pd", 16 * blocks), ("pe", 16 * edge_blocks(R, d)),
                       ("extra", (ts - 1) * R * d * 4)):
        lay[name] = (b, size)
        b += r256(size)
    return lay, b, ts


def rows_layout(n, d, r0, r1, dtype, ncu=NCU):
    """zrows_layout (snd_zzt_ce_rows)."""
    lay, b = _stage(1, n, d, dtype)
    b = r256(b)
    rows, nrb = r1 - r0, -(-r1 // ROWS) - r0 // ROWS
    ts = tsplit_blocks(nrb, n, dtype, ncu)
    for name, size in (("djd", n * d * 4), ("ej", rows * d * 4), ("pd", 16 * nrb * ts * wpb(d, dtype)),
                       ("pe", 16 * edge_blocks(rows, d)), ("extra", max(0, ts - 1) * n * d * 4)):
        lay[name] = (b, size)
        b += r256(size)
    return lay, b, ts


def layout(c, ncu=NCU):
    return rows_layout(c.n, c.d, c.r0, c.r1, c.dtype, ncu) if c.rows else ws_layout(c.B, c.n, c.d, c.dtype, ncu)


def read_ws(c, raw, ncu=NCU):
    """The staging images, ej (and the range's dJd rows) out of the workspace bytes."""
    lay, _, _ = layout(c, ncu)
    raw = np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
    B, n, d, dp, P = c.B, c.n, c.d, zzt_dp(c.d), npad(c.n)

    def part(name, dt):
        o, s = lay[name]
        return raw[o:o + s].view(dt)

    if c.dtype == BF16:
        img = lambda name: (part(name, np.uint16).astype(np.uint32) << 16).view(f32).astype(np.float64)
    else:
        img = lambda name: part(name, f32).astype(np.float64)
    out = {"jrow": img("jrow").reshape(B, P, dp), "jt": img("jt").reshape(B, dp, P),
           "colpart": part("colpart", f32).astype(np.float64).reshape(B, P // 64, dp),
           "ej": part("ej", f32).astype(np.float64).reshape(c.r1 - c.r0, d)}
    if c.rows:
        out["djd"] = part("djd", f32).astype(np.float64).reshape(n, d)[c.r0:c.r1]
    return out


# ---------------------------------------------------------------- the cases
def case(id, B, n, d, dtype, pw=1.0, norm=1.0, scale=0.3, kind="std", rows=None):
    r0, r1 = rows if rows else (0, B * n)
    name = f"{id}_d{d}_{'bf16' if dtype else 'f32'}" + (f"_r{r0}_{r1}" if rows else "")
    return NS(id=id, name=name, B=B, n=n, d=d, dtype=dtype, pw=pw, norm=norm, scale=scale, kind=kind,
              rows=rows is not None, r0=r0, r1=r1)


def _cases():
    out, ALL = [], (16, 32, 64, 128)
    each = lambda ds, dts=(F32, BF16): [(d, t) for d in ds for t in dts]
    for id, B, n in (("n1", 2, 1), ("n2", 2, 2), ("n31", 2, 31), ("n33", 2, 33), ("n63", 2, 63), ("n64", 2, 64),
                     ("n65", 2, 65), ("n127", 1, 127), ("n128", 1, 128), ("n129", 1, 129), ("b9", 9, 33),
                     ("n200", 2, 200), ("n300", 3, 300)):
        # n1 at d = 128, bf16: |z_0|^2 log2(e) = 16 at scale 0.3, and one fp32 rounding of
        # softplus2(x_00) there is the whole bar of a batch whose terms are 2 softplus(-1)
        out += [case(id, B, n, d, t, scale=0.1 if (n, d, t) == (1, 128, BF16) else 0.3) for d, t in each(ALL)]
    out += [case("n1000", 1, 1000, d, t) for d, t in each((64, 128))]
    out += [case("n1300", 1, 1300, d, t) for d, t in each((32, 64))]
    for n in (65, 129, 300):
        out += [case(f"pw{n}", 2, n, d, t, pw=3.5, norm=0.7) for d, t in each(ALL)]
    out += [case("empty", 2, 65, d, t, kind="empty") for d, t in each(ALL)]
    out += [case("big", 2, 65, d, BF16, kind="big") for d in (32, 64, 128)]
    return tuple(out)


def _rows_cases():
    out = []
    for n, ds, ranges in ((129, (16, 32, 64, 128), ((0, 128), (128, 129))),
                          (300, (16, 32, 64, 128), ((0, 128), (128, 300), (256, 300), (0, 300))),
                          (1000, (64, 128), ((384, 896), (896, 1000))),
                          (1300, (32, 64), ((1280, 1300),))):
        out += [case(f"rows{n}", 1, n, d, t, pw=3.5 if n == 300 else 1.0, norm=0.7 if n == 300 else 1.0, rows=r)
                for d in ds for t in (F32, BF16) for r in ranges]
    return tuple(out)


CASES = _cases()
ROWS_CASES = _rows_cases()
PARTITIONS = {129: ((0, 128), (128, 129)), 300: ((0, 128), (128, 300))}
PLANTED_DEGREES = (0, 1, 3, 4, 5, 9)        # rows 0..5 of every graph with n >= 31


def _graph(rng, n):
    nb = [set() for _ in range(n)]
    lo = 0
    if n >= 31:
        lo = len(PLANTED_DEGREES)
        for i, deg in enumerate(PLANTED_DEGREES):
            for j in rng.choice(np.arange(lo, n), deg, replace=False):
                nb[i].add(int(j)), nb[int(j)].add(i)
    if n == 2:
        nb[0].add(1), nb[1].add(0)
    m = n - lo
    for _ in range(3 * m if m > 8 else m):          # average degree about 6
        i, j = (int(v) for v in rng.integers(lo, n, 2))
        if i != j:
            nb[i].add(j), nb[j].add(i)
    return nb


def _gen(c, seed):
    rng = np.random.default_rng(seed)
    z = (c.scale * rng.standard_normal((c.B * c.n, c.d))).astype(f32)
    if c.kind == "big":                                  # L = +-100 between rows 0-3 and 4-7
        a = np.zeros(c.d, f32)
        a[:4] = 5.0
        for g in range(c.B):
            z[g * c.n:g * c.n + 4], z[g * c.n + 4:g * c.n + 8] = a, -a
    rp, ci = [0], []
    for g in range(c.B):
        for s in (_graph(rng, c.n) if c.kind != "empty" else [()] * c.n):
            ci += [g * c.n + j for j in sorted(s)]
            rp.append(len(ci))
    return z, np.asarray(rp, np.int32), np.asarray(ci, np.int32)


@functools.lru_cache(maxsize=None)
def _setup(key):
    c = _BY_NAME[key]
    if c.rows:                                          # the ranges of one graph share its z and CSR
        w = case(c.id, 1, c.n, c.d, c.dtype, c.pw, c.norm, c.scale)
        _BY_NAME.setdefault(w.name, w)
        inp = _setup(w.name)[0]
        return inp, reference(c, *inp)
    base = 1000 * c.n + 10 * c.d + c.dtype + (7 if c.kind == "big" else 0) + (3 if c.pw != 1.0 else 0)
    for k in range(64):
        inp = _gen(c, base + 100003 * k)
        ref = reference(c, *inp)
        if c.n > AMB_SMALL_N or ref.amb == 0:           # seeds picked on the CPU: no ambiguous pair
            return inp, ref
    raise AssertionError(f"{c.name}: no seed without an ambiguous pair")


def setup(c):
    """((z, rowptr, colidx) of the whole batch, reference), cached per case."""
    return _setup(c.name)


def dense_adj(c, rp, ci):
    out = []
    for g in range(c.B):
        a = np.zeros((c.n, c.n))
        rows = np.repeat(np.arange(c.n), np.diff(rp[g * c.n:(g + 1) * c.n + 1]))
        a[rows, ci[rp[g * c.n]:rp[(g + 1) * c.n]] - g * c.n] = 1.0
        out.append(a)
    return out


# ---------------------------------------------------------------- the operands as stored
def stored(c, z, exact=False):
    """(J, V, kinv) float64 [R, d]; ``exact``: no rounding anywhere (compose)."""
    if exact:
        z = np.asarray(z, np.float64)
        return z * math.sqrt(math.log2(math.e)), z, 1.0
    T = bf16 if c.dtype == BF16 else ident
    J = T(np.asarray(z, f32) * f32(SQRT_LOG2E))
    if c.dtype == F32:
        return J, np.asarray(z, np.float64), 1.0
    if zzt_dp(c.d) == 32:
        return J, bf16(z), 1.0
    return J, J, float(f32(INV_SQRT_LOG2E))


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def reference(c, z, rp, ci, exact=False, ncu=NCU):
    """Every link of the case in float64 on the operands as stored."""
    B, n, d, dp, P = c.B, c.n, c.d, zzt_dp(c.d), npad(c.n)
    z = np.asarray(z, f32)
    z64 = z.astype(np.float64)
    J, V, kinv = stored(c, z, exact)
    T = (lambda a: np.asarray(a, np.float64))
    ts = layout(c, ncu)[2]
    r = NS(ts=ts)
    # ---- prep links: the images bit for bit (padding exactly zero), the 64-row column sums
    r.jrow = np.zeros((B, P, dp))
    r.jrow[:, :n, :d] = J.reshape(B, n, d)
    r.jt = np.zeros((B, dp, P))
    Tz = (bf16(z) if c.dtype == BF16 else z64) if not exact else z64
    r.jt[:, :d, :n] = Tz.reshape(B, n, d).transpose(0, 2, 1)
    blk = r.jrow.reshape(B, P // 64, 64, dp)
    r.colpart = Link(blk.sum(2), np.abs(blk).sum(2), 64)
    # ---- dense: dJd of the rows, loss terms, count, ambiguous pairs
    refs, mags, exts = [], [], []
    dl = dabs = 0.0
    dpos = amb = 0
    for g in range(B):
        lo, hi = (c.r0, c.r1) if c.rows else (0, n)
        Jg = J[g * n:(g + 1) * n]
        a, m, e = djd_graph(Jg, V[g * n:(g + 1) * n], kinv, d, T, ident if exact else bf16,
                            round_s=c.dtype == BF16 and not exact, r0=lo, r1=hi,
                            diag_summed=c.dtype == BF16 and not exact)
        refs.append(a), mags.append(m), exts.append(e)
        x = Jg[lo:hi] @ Jg.T
        off = np.ones(x.shape, bool)
        off[np.arange(hi - lo), np.arange(lo, hi)] = False
        L = x * LN2
        sp = softplus(L)
        dl += float(sp[off].sum())
        # the signed kernels add x and log2(1 + 2^-x): where logits are planted far out
        # ("big") the terms that cancel are the |x|-form's
        dabs += float((np.abs(L) + np.log1p(np.exp(-np.abs(L))))[off].sum()) if c.kind == "big" else float(sp[off].sum())
        dpos += int(((x > 0) & off).sum())
        aJ = np.abs(Jg)
        amb += int(((np.abs(x) <= (d + 4) * U23 * (aJ[lo:hi] @ aJ.T)) & off).sum())
    K = n + 2 + (ts if ts > 1 else 0)
    r.djd = Link(np.concatenate(refs), np.concatenate(mags), K, extra=np.concatenate(exts))
    # ---- edges (fp32 z, unrounded)
    rows = c.r1 - c.r0
    rpl = np.asarray(rp[c.r0:c.r1 + 1], np.int64)
    deg = np.diff(rpl)
    ri = np.repeat(np.arange(rows), deg)
    cj = np.asarray(ci[rpl[0]:rpl[-1]], np.int64)
    zi, zj = z64[c.r0 + ri], z64[cj]
    Le = (zi * zj).sum(1)
    dLe = (d + 4) * U23 * (np.abs(zi) * np.abs(zj)).sum(1)
    sg = sigmoid(Le)
    coef = (c.pw - 1.0) * sg - c.pw
    dcoef = abs(c.pw - 1.0) * (sg * (1 - sg) * dLe + TRANS * sg) if c.pw != 1.0 else np.zeros_like(Le)
    ej, ejm, ejx = np.zeros((rows, d)), np.zeros((rows, d)), np.zeros((rows, d))
    np.add.at(ej, ri, coef[:, None] * zj)
    np.add.at(ejm, ri, np.abs(coef)[:, None] * np.abs(zj))
    np.add.at(ejx, ri, dcoef[:, None] * np.abs(zj))
    r.ej = Link(ej, ejm, deg[:, None], extra=ejx)
    te = (c.pw - 1.0) * softplus(Le) - c.pw * Le
    tp = int((Le > 0).sum())
    amb_e = int((np.abs(Le) <= dLe).sum())
    # ---- dz = 2 norm (dJd + ej): both bounds, three fp32 roundings (2 norm, the add, the product)
    sc = 2.0 * c.norm
    r.dz = Link(sc * (r.djd.ref + ej), 0.0 * ej, 0,
                extra=sc * (r.djd.bound() + r.ej.bound()) * (1 + 3 * 2.0 ** -24) +
                3 * 2.0 ** -24 * sc * (np.abs(r.djd.ref) + np.abs(ej)))
    # ---- stats
    nrows = B * n if not c.rows else rows
    r.s0 = c.norm * (dl + float(te.sum()) + nrows * SOFTPLUS_M1)
    r.s0_abs = abs(c.norm) * (dabs + float(np.abs(te).sum()) + nrows * SOFTPLUS_M1)
    r.s1 = float(nrows * n - int(rpl[-1] - rpl[0]) - dpos + 2 * tp)
    r.amb = amb + amb_e
    r.amb_w = amb + 2 * amb_e                      # an edge pair moves the count by 2
    r.pairs = nrows * n
    return r


def check(c, r, got, strict=False):
    """{link: worst err / bound} of the buffers in ``got`` (emulate's / read_ws's names plus
    "dz" and "stats").  ``strict``: fail at the first link over its bound, naming the element."""
    import abi_ops as A
    B, n, d = c.B, c.n, c.d
    out = {}

    def link(name, lk, v):
        out[name] = A.assert_link(f"{c.name} {name}", lk, v) if strict else float(A.ratios(lk, v)[0].max(initial=0.0))

    for name in ("jrow", "jt"):                    # bitwise the host value, padding exactly zero
        w, g = getattr(r, name), np.asarray(got[name], np.float64)
        same = (w == g) & (np.signbit(w) == np.signbit(g))
        out[name] = 0.0 if same.all() else np.inf
        if strict and not same.all():
            i = tuple(int(k) for k in np.argwhere(~same)[0])
            raise AssertionError(f"{c.name} {name}: element {i} is {g[i]!r}, the host value is {w[i]!r}")
    link("colpart", r.colpart, got["colpart"])
    if "djd" in got:
        link("djd", r.djd, got["djd"])
    link("ej", r.ej, got["ej"])
    link("dz", r.dz, got["dz"])
    s = np.asarray(got["stats"], np.float64)
    out["stats0"] = abs(s[0] - r.s0) / (S0_BAR * r.s0_abs) if np.isfinite(s[0]) else np.inf
    out["stats1"] = abs(s[1] - r.s1) / (r.amb_w + 0.5) if np.isfinite(s[1]) else np.inf
    if strict:
        assert out["stats0"] < 1.0, (c.name, "stats[0]", s[0], r.s0, S0_BAR * r.s0_abs)
        assert out["stats1"] < 1.0, (c.name, "stats[1]", s[1], r.s1, "ambiguous pairs", r.amb)
    return out


def amb_cap(c):
    return 0 if c.n <= AMB_SMALL_N else int(AMB_CAP * (c.r1 - c.r0 if c.rows else c.B * c.n) * c.n)


# ---------------------------------------------------------------- the float32 emulation
FAULTS = ("drop_last_col", "diag_in", "pad_pair", "count_off", "no_kinv", "v_scaled", "slab_dropped",
          "edge_no_sigma", "norm_not_2norm", "edge_row0", "jt_pad")


def expressible(fault, c, ts):
    """Whether the fault changes anything at this case (tests/test_zzt_ops_cpu.py lists why)."""
    first = c.r0 if c.rows else 0
    has_edges = c.kind != "empty" and c.n >= 2
    return {"drop_last_col": c.n >= 2 and first != c.n - 1,
            "diag_in": True,
            "pad_pair": c.n % ROWS != 0,
            "count_off": True,
            "no_kinv": c.dtype == BF16 and c.d >= 64 and c.n >= 2,
            "v_scaled": c.dtype == BF16 and c.d <= 32 and c.n >= 2,
            "slab_dropped": ts > 1,
            "edge_no_sigma": c.pw != 1.0 and has_edges,
            "norm_not_2norm": c.n >= 2,
            "edge_row0": c.rows and c.r0 > 0 and has_edges,
            "jt_pad": c.n % ROWS != 0 or zzt_dp(c.d) != c.d}[fault]


def _bf(a):
    """float32 array rounded to bf16 (nearest even), as float32."""
    return bf16(a).astype(f32)


def emulate(c, z, rp, ci, fault=None, ncu=NCU):
    """What a correct float32 implementation with the kernels' structure leaves: the staging
    images, colpart, ej, (the range's dJd rows,) dz and stats.  ``fault`` plants one of FAULTS."""
    B, n, d, dp, P = c.B, c.n, c.d, zzt_dp(c.d), npad(c.n)
    bf = c.dtype == BF16
    T = _bf if bf else (lambda a: np.asarray(a, f32))
    ts = layout(c, ncu)[2]
    z = np.asarray(z, f32)
    zp = np.zeros((B, P, dp), f32)
    zp[:, :n, :d] = z.reshape(B, n, d)
    Js = T(zp * f32(SQRT_LOG2E))                     # zzt_prep_kernel: (T)(v * sc)
    Zt = T(zp)
    out = {"jrow": Js.astype(np.float64), "jt": Zt.transpose(0, 2, 1).astype(np.float64)}
    if fault == "jt_pad":
        g = out["jt"]
        g[(0, d, 0) if dp != d else (0, 0, n)] = 2.0 ** -10
    blk = Js.reshape(B, P // 64, 64, dp)
    cp = np.zeros((B, P // 64, dp), f32)
    for rr in range(64):                             # fp32, in row order
        cp = cp + blk[:, :, rr, :]
    out["colpart"] = cp.astype(np.float64)
    signed = bf                                      # v4 / v7 / v9; the f32 kernels mask
    scaled_v = bf and dp >= 64
    if fault == "v_scaled":
        scaled_v = True
    Vp = Js if scaled_v else Zt
    kinv = f32(INV_SQRT_LOG2E) if (bf and dp >= 64 and fault != "no_kinv") else f32(1.0)
    # graph column sums: NT / dp strided partial sums over the 64-row partials, then those
    grp = (512 if bf and dp == 64 else 1024) // dp      # v9 runs 512 threads
    cs = np.zeros((B, grp, dp), f32)
    for p in range(P // 64):
        cs[:, p % grp] = cs[:, p % grp] + cp[:, p]
    colsum = np.zeros((B, dp), f32)
    for k in range(grp):
        colsum = colsum + cs[:, k]

    R0, R1 = (c.r0, c.r1) if c.rows else (0, n)
    B0, B1 = R0 // ROWS * ROWS, -(-R1 // ROWS) * ROWS      # the launch's row blocks, padded
    frow = R0                                        # the row the dense faults hit
    djd = np.zeros((B, R1 - R0, d), f32)
    dl, dc = 0.0, 0.0
    ntot = P // TJ2
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        for g in range(B):
            Jg = Js[g]
            x = (Jg[B0:B1] @ Jg.T).astype(f32)       # fp32 MFMA accumulation
            ii = np.arange(B0, B1)
            if signed:
                y = -x
                q = (np.exp2(y) + f32(1.0)).astype(f32)
                s = _bf((f32(1.0) / q).astype(f32))
                q4 = q.reshape(B1 - B0, P // 4, 4)
                lt = np.log2(((q4[..., 0] * q4[..., 1]) * (q4[..., 2] * q4[..., 3])).astype(f32)).astype(f32)
                one = np.where(y > 24.0, y, np.log2(q).astype(f32)).astype(f32).reshape(q4.shape)
                one = ((one[..., 0] + one[..., 1]) + one[..., 2]) + one[..., 3]
                lt = np.where(np.isfinite(lt), lt, one)          # the quad-overflow fallback
                loss2 = float(lt.sum(dtype=np.float64))
                cnt = float((y < 0).sum())
                Ji = Jg[B0:B1]
                xd = np.zeros(B1 - B0, f32)
                xs = np.zeros(B1 - B0, f32)
                for k in range(dp):                              # fp32 dots, in k order
                    xd = xd + Ji[:, k] * Ji[:, k]
                    xs = xs + Ji[:, k] * colsum[g, k]
                valid = ii < n
                if fault == "diag_in":
                    valid = valid & (ii != frow)
                spd = (np.maximum(xd, 0) + np.log2(f32(1.0) + np.exp2(-np.abs(xd)))).astype(f32)
                loss2 += float(xs[ii < n].sum(dtype=np.float64)) - float(spd[valid].sum(dtype=np.float64))
                cnt -= float(((xd > 0) & valid).sum())
                for rb in range(B0 // ROWS, B1 // ROWS):         # zzt_padded_pairs
                    loss2 -= float(ROWS * P - max(0, min(ROWS, n - rb * ROWS)) * n)
                sd = _bf((f32(1.0) / (np.exp2(-xd) + f32(1.0))).astype(f32))
                sd = np.where(valid, sd, f32(0.0)).astype(f32)
                parts = []
                for sp in range(ts):                             # column splits over 128-column tiles
                    c0, c1 = sp * ntot // ts * TJ2, (sp + 1) * ntot // ts * TJ2
                    sl = s[:, c0:c1]
                    if fault == "drop_last_col" and c0 <= n - 1 < c1:
                        sl = sl.copy()
                        sl[frow - B0, n - 1 - c0] = 0.0
                    o = (sl @ Vp[g, c0:c1]).astype(f32)
                    if sp == 0:
                        o = o - sd[:, None] * Vp[g, B0:B1]
                    parts.append((o * kinv).astype(f32))
                acc = parts[0]
                for k, o in enumerate(parts[1:]):                # zzt_split_sum_kernel, in order
                    if not (fault == "slab_dropped" and k == len(parts) - 2):
                        acc = acc + o
            else:
                jj = np.arange(P)
                mask = (ii[:, None] < n) & (jj[None, :] < n) & (ii[:, None] != jj[None, :])
                if fault == "diag_in":
                    mask[frow - B0, frow] = True
                ex = np.exp2(-np.abs(x)).astype(f32)
                qd = (f32(1.0) + ex).astype(f32)
                rc = (f32(1.0) / qd).astype(f32)
                s = np.where(mask, np.where(x > 0, rc, ex * rc), f32(0.0)).astype(f32)
                # eight logits per log2: j = 32 chunk + 16 h + 4 q4 + e over (h, e)
                g8 = lambda a: a.reshape(B1 - B0, P // 32, 2, 4, 4).transpose(0, 1, 3, 2, 4).reshape(B1 - B0, P // 32, 4, 8)
                qm, xm = g8(np.where(mask, qd, f32(1.0))), g8(np.where(mask, np.maximum(x, 0), f32(0.0)))
                prod, csum = np.ones(qm.shape[:3], f32), np.zeros(qm.shape[:3], f32)
                for e in range(8):
                    prod, csum = prod * qm[..., e], csum + xm[..., e]
                loss2 = float((csum + np.log2(prod).astype(f32)).astype(f32).sum(dtype=np.float64))
                cnt = float(((x > 0) & mask).sum())
                if fault == "drop_last_col":
                    s[frow - B0, n - 1] = 0.0
                acc = (s @ Vp[g]).astype(f32)
            dl += loss2 * LN2
            dc += cnt
            djd[g] = acc[R0 - B0:R1 - B0, :d]
    djd = djd.reshape(-1, d)
    # ---- edge_kernel: fp32 dot, fp32 coefficient, neighbours in CSR order
    rows = c.r1 - c.r0
    e0 = 0 if fault == "edge_row0" else c.r0
    rpl = np.asarray(rp[c.r0:c.r1 + 1], np.int64)
    deg = np.diff(rpl)
    ej = np.zeros((rows, d), f32)
    lossr = np.zeros(rows, f32)
    tp = 0
    pw = f32(c.pw)
    for k in range(int(deg.max(initial=0))):
        ri = np.nonzero(deg > k)[0]
        zj = z[np.asarray(ci, np.int64)[rpl[ri] + k]]
        zi = z[e0 + ri]
        dot = np.zeros(len(ri), f32)
        for q in range(d):
            dot = dot + zi[:, q] * zj[:, q]
        coef = np.full(len(ri), -pw, f32)
        if c.pw != 1.0:
            sg = (f32(1.0) / (f32(1.0) + np.exp(-dot).astype(f32))).astype(f32)
            sp = (np.maximum(dot, 0) + np.log1p(np.exp(-np.abs(dot)).astype(f32)).astype(f32)).astype(f32)
            coef = coef + (pw - f32(1.0)) * (f32(1.0) if fault == "edge_no_sigma" else sg)
            lossr[ri] = lossr[ri] + (pw - f32(1.0)) * sp
        lossr[ri] = lossr[ri] - pw * dot
        tp += int((dot > 0).sum())
        ej[ri] = ej[ri] + coef[:, None] * zj
    el = float(lossr.sum(dtype=np.float64))
    out["ej"] = ej.astype(np.float64)
    if c.rows:
        out["djd"] = djd.astype(np.float64)
    sc = f32(1.0 if fault == "norm_not_2norm" else 2.0) * f32(c.norm)
    out["dz"] = (sc * (djd + ej)).astype(f32).astype(np.float64)
    nrows = B * n if not c.rows else rows
    nnz = float(rpl[-1] - rpl[0])
    s0 = float(f32(c.norm)) * (dl + el + nrows * SOFTPLUS_M1)
    s1 = float(nrows) * n - nnz - dc + 2.0 * tp
    if fault == "pad_pair":
        s0 += LN2 * float(f32(c.norm))
    if fault == "count_off":
        s1 += 1.0
    out["stats"] = np.array([s0, s1])
    return out


POST_HOC = ("pad_pair", "count_off", "norm_not_2norm", "jt_pad")     # faults of the last store only


def plant(c, inp, clean, fault):
    """The emulation's buffers with ``fault`` planted (``clean`` = emulate(c, *inp))."""
    if fault not in POST_HOC:
        return emulate(c, *inp, fault=fault)
    out = {k: v.copy() for k, v in clean.items()}
    if fault == "pad_pair":
        out["stats"][0] += LN2 * float(f32(c.norm))
    elif fault == "count_off":
        out["stats"][1] += 1.0
    elif fault == "norm_not_2norm":
        out["dz"] *= 0.5                                # a power of two: exact in fp32
    else:
        out["jt"][(0, c.d, 0) if zzt_dp(c.d) != c.d else (0, 0, c.n)] = 2.0 ** -10
    return out


_BY_NAME = {c.name: c for c in CASES + ROWS_CASES}
assert len(_BY_NAME) == len(CASES) + len(ROWS_CASES)
