"""Constructed inputs, float64 references and plan-level emulations of the two planned bf16
SpMMs, snd_csr_spmm_bf16_window (csrc/snd_spmm_win.hip) and snd_csr_spmm_bf16_tiled
(csrc/snd_fast_enc.hip).  Plain NumPy + scipy: importable without a GPU.

* ``band_batch``: batches whose window-plan beta is prescribed exactly.  In position space
  row q has neighbours at q - beta and q + beta where they exist, the rest of its degree is
  drawn from [q - beta, q + beta]; the degrees sit on the kernel's list boundaries (8-entry
  padding, 32 staged entries, the k >= 32 loop); a random permutation per graph maps
  positions to rows.  ``WINDOW_CASES`` places them on the kernel's limits: the last beta of
  the one-barrier schedule, the first and the last of the two-barrier one, segments of one
  step, of ten steps and mid-graph segments.
* ``TILE_CASES``: CSRs on the row-tile kernel's limits: tile sets of 319 / 320 rows (the LDS
  image cap and the register kernel behind it), degrees on the 16-entry rounds and the 32
  prefetched ids, one and two rows per 8-lane group, a short last tile, runs of tiles.
* the reference: one ``own_operands.Link`` per output (ref = A @ h in float64 on the bf16 h,
  mag = |A| @ |h|, K = the row's degree, stored bf16), bounded per element by that module's
  derived rule (K + 4) 2^-23 mag + 2^-8 |ref|.  Nothing is excluded; an empty row has bound
  0 and must be exactly +0.
* ``window_emulate`` / ``tiles_emulate``: the kernels' walks restated over the PLAN ARRAYS
  alone (they never see the CSR): an explicit ring (slot -> position) filled by the prologue
  and the per-step pieces, list reads of 32 staged entries, wave trip counts; float32 sums
  in list order, rounded to bf16.  They are the vehicle of the planted faults of
  tests/test_spmm_plans_cpu.py.  ``ring_hazards`` is the same walk asking only whether every
  position a step needs is resident and stays so.

The ring model.  While step s sums, the window pieces e(0..s-2) have landed (the step's
vmcnt wait), e(s-1) and e(s) are in flight: each may or may not have landed.  A slot is safe
if the landed content is the wanted position and no piece in flight writes another one
there; the emulation reads the wrong content wherever the schedule allows one.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace as NS

import numpy as np

import abi_ops as A
from own_operands import bf16

RING, STEP, WAVES = 1096, 128, 16
ZSLOT = RING                       # the zero row's slot: list padding
MAX_BETA8, ONE_BARRIER_BETA8 = 352, 288
WIN_WIDTH = 64
DEGREES = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 63)
TILE_CAP, TILE_GROUPS = 319, 64    # LDS image rows; 8-lane groups per workgroup
TILE_DEGREES = (0, 1, 8, 9, 16, 17, 31, 32, 33, 47, 48, 49, 100)


def cdiv(a, b):
    return -(-a // b)


def graph_batch(n, B, rp, ci):
    from snd_vae_amd.data import GraphBatch
    z = np.zeros((n * B, 1), np.float32)
    return GraphBatch(B, n, np.asarray(rp, np.int32), np.asarray(ci, np.int32), z, z, z)


def _csr(n, B, rows, cols):
    """Block-diagonal CSR from (global row, global column) entries; a stable sort keeps the
    entries of a row in the order given."""
    o = np.argsort(rows, kind="stable")
    rp = np.zeros(n * B + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n * B), out=rp[1:])
    ci = cols[o] if len(cols) else np.zeros(1, np.int64)     # an empty CSR keeps one element
    return rp.astype(np.int32), ci.astype(np.int32)


# ================================================================= band batches
def _band_pattern(n, beta, rng):
    """(q, p): the entries of one graph in position space, shuffled within rows."""
    deg = np.where(rng.random(n) < 0.5, rng.choice(DEGREES, n), rng.integers(0, 7, n))
    deg[rng.permutation(n)[:len(DEGREES)]] = DEGREES          # every listed degree occurs
    q = np.repeat(np.arange(n), deg)
    i = np.arange(len(q)) - np.repeat(np.cumsum(deg) - deg, deg)
    p = rng.integers(np.maximum(q - beta, 0), np.minimum(q + beta, n - 1) + 1)
    has_lo, has_hi = q - beta >= 0, q + beta < n
    p = np.where((i == 0) & (has_lo | has_hi), np.where(has_lo, q - beta, q + beta), p)
    p = np.where((i == 1) & has_lo & has_hi, q + beta, p)
    o = np.lexsort((rng.random(len(q)), q))                   # the kernels sum in colidx order
    return q, p[o]


@functools.lru_cache(maxsize=3)
def _band(n, B, beta, seed):
    from snd_vae_amd.data import window_plan
    rng = np.random.default_rng([seed, n, B, beta])
    pats = [_band_pattern(n, beta, rng) for _ in range(min(B, 3))] if beta > 0 else []
    rows, cols, order = [], [], np.empty(n * B, np.int64)
    for b in range(B):
        perm = rng.permutation(n) + b * n                     # position q holds row perm[q]
        order[b * n:(b + 1) * n] = perm
        if pats:
            q, p = pats[b % len(pats)]
            rows.append(perm[q])
            cols.append(perm[p])
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
    rp, ci = _csr(n, B, cat(rows), cat(cols))
    order = order.astype(np.int32)
    wp = window_plan(graph_batch(n, B, rp, ci), order)
    assert wp.beta == beta and wp.max_degree == (63 if beta else 0), (wp.beta, wp.max_degree)
    return rp, ci, order, wp


def band_batch(n, B, beta, seed):
    """(rowptr, colidx, order) of B graphs of n rows whose window plan has exactly this beta
    and largest degree 63 (beta 0: every row empty, colidx of one element)."""
    return _band(n, B, beta, seed)[:3]


def degree64_rejected():
    """A row of degree 64 does not fit the metadata word: window_plan must refuse."""
    from snd_vae_amd.data import window_plan
    n = 80
    rows = np.zeros(64, np.int64)
    rp, ci = _csr(n, 1, rows, np.arange(1, 65))
    try:
        window_plan(graph_batch(n, 1, rp, ci), np.arange(n, dtype=np.int32))
    except ValueError:
        return True
    return False


# ================================================================= window cases
# name: (n, B, beta, workgroups per graph, seg, steps of each segment, rows of the last step)
WINDOW_CASES = {
    "w_one_288": (840, 3, 288, 7, 128, (1,) * 7, 72),
    "w_two_289": (840, 3, 289, 7, 128, (1,) * 7, 72),
    "w_two_345": (840, 3, 345, 7, 128, (1,) * 7, 72),
    "w_two_352": (840, 3, 352, 7, 128, (1,) * 7, 72),
    "w_run_5": (1160, 256, 5, 1, 1280, (10,), 8),
    "w_run_288": (1160, 256, 288, 1, 1280, (10,), 8),
    "w_run_352": (1160, 256, 352, 1, 1280, (10,), 8),
    "w_seg_345": (2312, 86, 345, 3, 896, (7, 7, 5), 8),
    "w_empty": (130, 5, 0, 2, 128, (1, 1), 2),
}
WINDOW_FAULTS = ("ring_1088", "piece_one_step_late", "pad_slot_0", "beta8_floor", "tail_past_32_dropped",
                 "last_step_unclamped", "graph_base_dropped", "prologue_stops_at_hi0")


def segments(n, B):
    """launch_spmm_window's segment rule: (workgroups per graph, positions per segment)."""
    steps = cdiv(n, STEP)
    spg = max(1, min(steps, cdiv(256, B)))
    seg = cdiv(steps, spg) * STEP
    return cdiv(n, seg), seg


def window_path(name):
    """What the case reaches, from the launch arithmetic (asserted against the table)."""
    n, B, beta = WINDOW_CASES[name][:3]
    spg, seg = segments(n, B)
    nsteps = tuple(cdiv(min(n, (g + 1) * seg) - g * seg, STEP) for g in range(spg))
    beta8 = (beta + 7) & ~7
    return NS(spg=spg, seg=seg, nsteps=nsteps, last_rows=n - (spg - 1) * seg - (nsteps[-1] - 1) * STEP, beta8=beta8,
              one_barrier=beta8 <= ONE_BARRIER_BETA8)


def _seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


def _h(rows, width, seed):
    return bf16(np.random.default_rng(seed).standard_normal((rows, width)).astype(np.float32)).astype(np.float32)


def _plan_vec(bufs, name, arr):
    dt = {"int32": "i32", "uint16": "u16"}[arr.dtype.name]
    bufs[name] = A.vec(len(arr), dt, data=arr, name=name)


def _operands(c, plan):
    """h (ldh = width + 8), out (ldo = width + 16), the CSR, the schedule, the plan arrays at
    exactly the planner's lengths, and out_ref for snd_csr_spmm_bf16 on the same operands."""
    w = c.width
    c.bufs = {"h": A.guarded(c.rows, w, w + 8, "bf16", data=c.h, name="h"),
              "out": A.guarded(c.rows, w, w + 16, "bf16", name="out"),
              "out_ref": A.guarded(c.rows, w, w + 16, "bf16", name="out_ref")}
    _plan_vec(c.bufs, "rowptr", c.rp)
    _plan_vec(c.bufs, "colidx", c.ci)
    for k, v in plan.items():
        if v is not None:
            _plan_vec(c.bufs, k, np.ascontiguousarray(v))
    c.inputs = [k for k in c.bufs if k not in ("out", "out_ref")]
    return c


def window_setup(name):
    n, B, beta = WINDOW_CASES[name][:3]
    rp, ci, order, wp = _band(n, B, beta, 1)
    p = window_path(name)
    assert (p.spg, p.seg, p.nsteps, p.last_rows) == WINDOW_CASES[name][3:], (name, p)
    c = NS(name=name, op="window", n=n, B=B, rows=n * B, width=WIN_WIDTH, beta=beta, rp=rp, ci=ci, order=order,
           wp=wp, h=_h(n * B, WIN_WIDTH, _seed(name)))
    return _operands(c, dict(meta=wp.meta, slots=wp.slots, rows=wp.rows, order=wp.order))


# ----------------------------------------------------------------- the ring
def ring_walk(n, P0, seg, beta8, ring=RING, step=STEP, fault=None):
    """Per step s of the segment at P0: (s, landed, flying), slot -> position (-1: never
    written).  ``landed``: the prologue's window [Q0, hi(1)] and the pieces e(0..s-2);
    ``flying``: what e(s-1) and e(s) write.  e(s) is 16 pieces of 8 positions from the first
    8-aligned position past hi(s+1); past the window end the pieces repeat the last row."""
    P1 = min(n, P0 + seg)
    Q0, Q1 = max(0, P0 - beta8), min(n, P1 + beta8)
    hi = lambda s: min(P0 + step * s + step - 1 + beta8, Q1 - 1)

    def piece(s):
        p = ((hi(s + 1) + 8) & ~7) + np.arange(8 * WAVES)
        return p % ring, np.minimum(p, Q1 - 1)

    landed = np.full(RING + 2, -1, np.int64)
    top = hi(0) if fault == "prologue_stops_at_hi0" else hi(1)
    p = Q0 + np.arange(8 * ((top - Q0) // 8 + 1))
    landed[p % ring] = np.minimum(p, Q1 - 1)
    lag = 3 if fault == "piece_one_step_late" else 2          # the fault issues e(s - 1) at step s
    for s in range(cdiv(P1 - P0, step)):
        if s - lag >= 0:
            sl, pos = piece(s - lag)
            landed[sl] = pos
        flying = np.full(RING + 2, -1, np.int64)
        for t in (s - lag + 1, s - lag + 2):
            if t >= 0:
                sl, pos = piece(t)
                flying[sl] = pos
        yield s, landed, flying


def ring_hazards(n, P0, seg, beta8, ring=RING, step=STEP):
    """(step, position, content) of every position a step needs (its rows' positions +- beta8
    inside the graph) that has not landed, or that a piece in flight replaces."""
    P1 = min(n, P0 + seg)
    bad = []
    for s, landed, flying in ring_walk(n, P0, seg, beta8, ring, step):
        lo = max(0, P0 + step * s - beta8)
        hi = min(min(P0 + step * s + step, P1) - 1 + beta8, n - 1)
        p = np.arange(lo, hi + 1)
        sl = p % ring
        missing = landed[sl] != p
        over = ~missing & (flying[sl] != -1) & (flying[sl] != p)
        bad += [(s, int(x), int(landed[x % ring])) for x in p[missing]]
        bad += [(s, int(x), int(flying[x % ring])) for x in p[over]]
    return bad


def _gather(h, order, content, gb):
    """h rows of graph-local ring contents (-1: never written -> NaN)."""
    v = h[order[gb + np.maximum(content, 0)]]
    v[content < 0] = np.nan
    return v


def window_emulate(wp, h, n, B, fault=None, ring=RING, step=STEP, beta8=None):
    """The window kernel's walk over (meta, slots, rows, order) and h [n B, 64] float32.
    Returns (bf16 bits [n B, 64], written [n B])."""
    if fault == "ring_1088":
        ring = 1088
    if beta8 is None:
        beta8 = wp.beta & ~7 if fault == "beta8_floor" else (wp.beta + 7) & ~7
    h = np.asarray(h, np.float32)
    R = n * B
    meta, rows, order = (np.asarray(v, np.int64) for v in (wp.meta, wp.rows, wp.order))
    slots = np.asarray(wp.slots, np.int64)
    if fault == "pad_slot_0":
        slots = np.where(slots == ZSLOT, 0, slots)
    out, written, deferred = np.zeros((R, WIN_WIDTH), np.float32), np.zeros(R, bool), []
    spg, seg = segments(n, B)
    gb = np.repeat(np.arange(B) * n, step)                      # graph base of every (graph, lane row)
    hb = np.zeros_like(gb) if fault == "graph_base_dropped" else gb
    for sg in range(spg):
        P0, P1 = sg * seg, min(n, (sg + 1) * seg)
        for s, landed, flying in ring_walk(n, P0, seg, beta8, ring, step, fault):
            q = P0 + step * s + np.arange(step)
            if fault != "last_step_unclamped":
                q = np.minimum(q, P1 - 1)                       # duplicates are benign
            q = np.tile(q, B)
            inside = gb + q < R
            li = np.minimum(gb + q, R - 1)                      # listing index: meta / rows
            deg, st = meta[li] & 63, (meta[li] >> 6) * 8
            assert st.max() + 32 <= len(slots), "the kernel reads 32 entries from every list start"
            # a wave sums its 8 listed rows in chunks of 4 entries up to their largest degree
            kmax = np.repeat(np.minimum((deg.reshape(-1, 8).max(1) + 3) // 4 * 4, 32), 8)
            acc = np.zeros((len(q), WIN_WIDTH), np.float32)
            for k in range(int(max(kmax.max(), 0 if fault == "tail_past_32_dropped" else deg.max()))):
                act = np.flatnonzero((k < kmax) if k < 32 else (k < deg))
                sl = slots[st[act] + k]
                live = sl != ZSLOT
                act, sl = act[live], sl[live]
                # the position the list means: the one congruent to the slot nearest the row
                want = q[act] + (sl - q[act] + ring // 2) % ring - ring // 2
                la, fl = landed[sl], flying[sl]
                content = np.where(la != want, la, np.where((fl != -1) & (fl != want), fl, want))
                own = k < deg[act]                              # a pad entry has no wanted position
                content = np.where(own, content, np.where(la >= 0, la, fl))
                acc[act] += _gather(h, order, content, hb[act])
            sel = inside & (q < P1)
            out[rows[li[sel]]] = acc[sel]
            written[rows[li[sel]]] = True
            late = inside & (q >= P1)                           # last_step_unclamped only
            if late.any():
                deferred.append((rows[li[late]], acc[late]))
    for r, v in deferred:
        out[r] = v
    return A.bf16_bits(out).reshape(R, WIN_WIDTH), written


# ================================================================= tile cases
# name: (n, B, tile_rows, width, kind)
TILE_CASES = {
    "t_cap319_w64": (384, 1, 64, 64, "cap319"),
    "t_cap319_w128": (384, 1, 64, 128, "cap319"),
    "t_cap320_w64": (384, 1, 64, 64, "cap320"),
    **{f"t_deg_w{w}": (200, 2, 64, w, "deg") for w in (8, 24, 64, 72, 128)},
    "t_tr1": (37, 3, 1, 64, "rand"),
    "t_tr100_tail": (37, 3, 100, 64, "rand"),
    "t_tr65": (130, 2, 65, 64, "rand"),
    "t_tr128": (256, 8, 128, 64, "rand"),
    "t_run3": (520, 24, 8, 64, "rand"),
}
TILE_FAULTS = ("lcol_off_by_one", "rounds_stop_at_32", "trip_from_last_row", "short_last_tile_skipped",
               "second_pass_skipped", "set_cap_off_by_one")


def _tile_csr(n, B, kind, rng):
    rows, cols = [], []
    if kind.startswith("cap"):
        # rows 0..63: 5 neighbours each among rows 64..383, 320 distinct in all (319: row 63
        # shares one with row 62); the other rows keep to their own tile
        pool = 64 + rng.permutation(320)
        nb = pool.reshape(64, 5).copy()
        if kind == "cap319":
            nb[63, 0] = nb[62, 3]
        rows.append(np.repeat(np.arange(64), 5))
        cols.append(nb.ravel())
        for r in range(64, n):
            d = r % 4
            rows.append(np.full(d, r))
            cols.append(r // 64 * 64 + rng.choice(64, d, replace=False))
    else:
        for r in range(n * B):
            # "deg": neighbours among the graph's first 150 rows, so a tile over two graphs
            # keeps its set (<= 300) inside the LDS image
            d, m = (TILE_DEGREES[r % len(TILE_DEGREES)], 150) if kind == "deg" else (int(rng.integers(0, min(n, 40))), n)
            rows.append(np.full(d, r))
            cols.append(r // n * n + rng.choice(m, d, replace=False))     # shuffled, distinct
    return _csr(n, B, np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64))


def tile_path(c):
    """What the case reaches, restating launch_spmm_bf16_epi."""
    T = cdiv(c.rows, c.tile_rows)
    lds = (c.rt.ustride + 1) * 256 * (2 if c.width > 64 else 1)
    tiled = c.rt.ustride <= TILE_CAP
    grid = min(T, 256 * max(1, min(2, (160 * 1024) // lds)))
    return NS(tiled=tiled, tiles=T, lds=lds, grid=grid, rpg=1 if c.tile_rows <= TILE_GROUPS else 2,
              short_last=c.rows % c.tile_rows, xcd_major=c.n % c.tile_rows == 0 and c.B % 8 == 0)


def tile_setup(name, ordered):
    """``ordered``: a per-graph permutation as row_order (the cap cases permute inside each
    tile, so both schedules sit on the cap); else row_order = NULL."""
    from snd_vae_amd.data import row_tiles
    n, B, tr, w, kind = TILE_CASES[name]
    rng = np.random.default_rng([_seed(name.split("_w")[0]), int(ordered)])
    rp, ci = _tile_csr(n, B, kind, np.random.default_rng(_seed(name.split("_w")[0])))
    order = None
    if ordered:
        blk = tr if kind.startswith("cap") else n
        order = np.concatenate([lo + rng.permutation(min(blk, n * B - lo)) for lo in range(0, n * B, blk)]).astype(np.int32)
    rt = row_tiles(graph_batch(n, B, rp, ci), order, tr)
    c = NS(name=name + ("_row_order" if ordered else ""), op="tiled", n=n, B=B, rows=n * B, width=w, tile_rows=tr,
           kind=kind, rp=rp, ci=ci, order=order, rt=rt, h=_h(n * B, w, _seed(name)))
    if kind.startswith("cap"):
        assert rt.ustride == int(kind[3:]), rt.ustride
    assert (rt.ustride <= TILE_CAP) == (kind != "cap320"), (name, rt.ustride)   # else: the register kernel
    return _operands(c, dict(row_order=order, rows=rt.rows, trp=rt.trp, lcol=rt.lcol, ucol=rt.ucol))


def tiles_emulate(rt, h, width, fault=None):
    """The row-tile kernel's walk over (rows, trp, lcol, ucol) and h [R, width] float32: per
    tile an image of the zero row and h[ucol]; every row sums its lcol entries in order up
    to the trip count of its wave's first row (rows are listed by degree, so that is the
    wave's longest).  Returns (bf16 bits [R, width], written [R])."""
    h = np.asarray(h, np.float32)
    R, tr, ust = len(rt.trp) - 1, rt.tile_rows, rt.ustride
    trp, lcol, ucol, rows = (np.asarray(v, np.int64) for v in (rt.trp, rt.lcol, rt.ucol, rt.rows))
    T = cdiv(R, tr)
    if fault == "short_last_tile_skipped" and R % tr:
        T -= 1
    out, written = np.zeros((R, width), np.float32), np.zeros(R, bool)
    for j in range(1 if fault == "second_pass_skipped" else cdiv(tr, TILE_GROUPS)):
        ls = np.tile(np.arange(TILE_GROUPS) + j * TILE_GROUPS, T)            # slot inside the tile
        t = np.repeat(np.arange(T), TILE_GROUPS)
        slot = t * tr + ls
        ok = (ls < tr) & (slot < R)
        sc = np.minimum(slot, R - 1)
        s = np.where(ok, trp[sc], 0)
        deg = np.where(ok, trp[sc + 1], 0) - s
        lead = 7 if fault == "trip_from_last_row" else 0
        dm = np.repeat(deg.reshape(-1, 8)[:, lead], 8)                       # the wave's trip count
        if fault == "rounds_stop_at_32":
            dm = np.minimum(dm, 32)
        acc = np.zeros((len(slot), width), np.float32)
        for k in range(int(dm.max()) if len(dm) else 0):
            act = np.flatnonzero((k < dm) & (k < deg))                       # past its degree: the zero row
            u = lcol[s[act] + k] - (0 if fault == "lcol_off_by_one" else 1)  # image row 1 + u holds set entry u
            staged = (u >= 0) & (u < (min(ust, TILE_CAP - 1) if fault == "set_cap_off_by_one" else ust))
            col = np.where(staged, ucol[np.minimum(t[act] * ust + u, len(ucol) - 1)], -1)
            v = h[np.maximum(col, 0)]
            v[col < 0] = np.nan                                              # never staged
            acc[act] += v
        out[rows[sc[ok]]] = acc[ok]
        written[rows[sc[ok]]] = True
    return A.bf16_bits(out).reshape(R, width), written


# ================================================================= reference, verify
def plain_sum_bits(rp, ci, h):
    """The plain float32 sum of every row's neighbours in colidx order, rounded to bf16."""
    h = np.asarray(h, np.float32)
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    deg = np.diff(rp)
    acc = np.zeros((len(deg), h.shape[1]), np.float32)
    for k in range(int(deg.max()) if len(deg) else 0):
        act = np.flatnonzero(deg > k)
        acc[act] += h[ci[rp[act] + k]]
    return A.bf16_bits(acc).reshape(acc.shape)


def link(c):
    if getattr(c, "_link", None) is None:
        nnz = int(c.rp[-1])
        c._link = A.ref_spmm(c.rp, c.ci[:nnz], c.h, "bf16")
    return c._link


def emulate(c, fault=None):
    """The buffers a correct implementation (or a planted fault) leaves."""
    after = A.initial(c)
    if c.op == "window":
        bits, written = window_emulate(c.wp, c.h, c.n, c.B, fault)
    else:
        bits, written = tiles_emulate(c.rt, c.h, c.width, fault)
    blk = c.bufs["out"].block(after["out"])
    blk[written] = bits[written]
    return after


def verify(c, after, name="out"):
    """Every element within its bound (the failure names it), empty rows exactly +0, no
    element left at the pattern, guards and padding intact, inputs bitwise unchanged."""
    g = c.bufs[name]
    bits = g.block(after[name])
    what = f"{c.op} {c.name} {name}"
    ratio = A.assert_link(what, link(c), g.values(after[name]))
    empty = np.diff(c.rp.astype(np.int64)) == 0
    assert not bits[empty].any(), f"{what}: an empty row is not +0"
    assert not (bits == A.PATTERN["bf16"][2]).any(), f"{what}: an element was never written"
    A.check_guards(c, after)
    for k in c.inputs:
        assert np.array_equal(after[k].view(np.uint8), c.bufs[k].arr.view(np.uint8)), f"{what}: input {k} changed"
    return ratio
