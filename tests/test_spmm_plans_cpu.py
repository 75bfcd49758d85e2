"""The window and row-tile SpMM plans without a GPU (tests/spmm_plans.py): every case is
walked by the plan-level emulation on the plan of data.window_plan / data.row_tiles and must
pass the same ``verify`` the GPU results go through, bitwise the plain float32 colidx-order
sum; every planted fault must fail it; every case must still reach the path it is named for;
and the ring model shows why the window cap is beta8 = 352.
"""
import numpy as np
import pytest

import spmm_plans as P

# the case on which each planted fault is shown to fail (a small one where the fault can show)
WINDOW_FAULT_CASE = {
    "ring_1088": "w_seg_345",               # positions >= 1088 land 8 slots off what the lists name
    "piece_one_step_late": "w_seg_345",     # needs a segment of several steps
    "prologue_stops_at_hi0": "w_seg_345",
    "pad_slot_0": "w_two_345",
    "beta8_floor": "w_two_345",             # beta % 8 != 0: the neighbour at +345 is outside 344
    "tail_past_32_dropped": "w_one_288",
    "last_step_unclamped": "w_one_288",     # 72-row last step: rows 72..127 are the next graph's
    "graph_base_dropped": "w_two_352",
}
TILE_FAULT_CASE = {
    "lcol_off_by_one": "t_tr65",
    "rounds_stop_at_32": "t_deg_w64",
    "trip_from_last_row": "t_deg_w24",
    "short_last_tile_skipped": "t_tr100_tail",
    "second_pass_skipped": "t_tr100_tail",
    "set_cap_off_by_one": "t_cap319_w128",
}


def emulation_passes(c):
    after = P.emulate(c)
    ratio = P.verify(c, after)
    assert ratio < 1.0
    got = c.bufs["out"].block(after["out"])
    assert np.array_equal(got, P.plain_sum_bits(c.rp, c.ci[:int(c.rp[-1])], c.h)), "bitwise the plain float32 sum"
    return after


def fault_fails(c, fault):
    with pytest.raises(AssertionError, match=f"{c.op} {c.name} out"):
        P.verify(c, P.emulate(c, fault))


# ---------------------------------------------------------------- band batches, window plan
def test_window_plan_refuses_degree_64():
    assert P.degree64_rejected()


@pytest.mark.parametrize("n,B,beta", [(840, 3, 352), (840, 3, 289), (300, 2, 7)])
def test_band_batch_has_the_prescribed_beta(n, B, beta):
    """wp.beta and max_degree are asserted inside; here: the neighbours at exactly +-beta exist,
    the listed degrees occur, colidx is not sorted (the kernels sum in colidx order)."""
    from snd_vae_amd.data import window_plan
    rp, ci, order = P.band_batch(n, B, beta, 1)
    wp = window_plan(P.graph_batch(n, B, rp, ci), order)
    assert wp.beta == beta and wp.max_degree == 63
    pos = np.empty(n * B, np.int64)
    pos[order] = np.arange(n * B) % n
    d = pos[ci] - np.repeat(pos, np.diff(rp))
    assert (d == beta).any() and (d == -beta).any() and np.abs(d).max() == beta
    assert set(P.DEGREES) <= set(np.diff(rp).tolist())
    assert any((np.diff(ci[s:e]) < 0).any() for s, e in zip(rp[:-1], rp[1:]))
    assert np.array_equal(np.sort(order.reshape(B, n), 1), np.arange(n * B).reshape(B, n))


def test_slot_array_covers_every_32_entry_read():
    """The kernel reads 32 entries from every list start.  A trailing all-empty group has
    empty lists that start at the array's end: the array must reach 32 entries past it (it
    ended 24 past: the last 16 bytes of the read lay outside)."""
    from snd_vae_amd.data import window_plan
    n = 136
    rows = np.repeat(np.arange(8), 9)                  # rows 0..7: 9 neighbours; the rest empty
    rp, ci = P._csr(n, 1, rows, (rows + 1 + np.tile(np.arange(9), 8)) % n)
    wp = window_plan(P.graph_batch(n, 1, rp, ci), np.arange(n, dtype=np.int32))
    start = (wp.meta.astype(np.int64) >> 6) * 8
    assert (wp.meta[-8:] & 63 == 0).all() and start.max() == 8 * 16      # position 128..135: empty lists at the end
    assert len(wp.slots) == start.max() + 32 and (wp.slots[8 * 16:] == P.ZSLOT).all()
    # a last list of 8 keeps the documented 24 trailing entries, and nothing more
    rp, ci = P._csr(n, 1, np.full(3, n - 1), np.array([5, 6, 7]))
    wp = window_plan(P.graph_batch(n, 1, rp, ci), np.arange(n, dtype=np.int32))
    assert len(wp.slots) == (int(wp.meta.max()) >> 6) * 8 + 8 + 24


# ---------------------------------------------------------------- window cases
@pytest.mark.parametrize("name", list(P.WINDOW_CASES))
def test_window_case(name):
    c = P.window_setup(name)                           # asserts beta, max_degree, the segment table
    p = P.window_path(name)
    # the path the case is named for
    assert p.beta8 <= P.MAX_BETA8
    assert p.one_barrier == (c.beta <= 288), (name, p)
    if name.startswith("w_two") or name in ("w_run_352", "w_seg_345"):
        assert not p.one_barrier
    if name in ("w_two_289", "w_two_345"):
        assert c.beta % 8 and p.beta8 == {289: 296, 345: 352}[c.beta]
    if name.startswith("w_run"):
        assert (p.spg, p.nsteps, p.last_rows) == (1, (10,), 8) and c.n > P.RING    # the ring wraps
    if name == "w_seg_345":
        assert p.spg == 3 and p.nsteps == (7, 7, 5) and p.seg - p.beta8 > 0         # P0 > 0, Q0 = P0 - beta8 > 0
    if name == "w_empty":
        assert c.rp[-1] == 0 and len(c.ci) == 1 and c.wp.max_degree == 0
    else:
        deg = c.wp.meta & 63
        assert deg.max() == 63 and ((deg > 32).sum() > 0) and (deg == 0).any()
    for g in range(p.spg):
        assert P.ring_hazards(c.n, g * p.seg, p.seg, p.beta8) == [], (name, g)
    emulation_passes(c)


def test_ring_cap_is_352():
    """beta8 = 360 on the ten-step segment: e(3) lands positions 1120.. on the slots of
    positions 24.. that step 3 still reads.  352 is the last clean beta8, for every segment
    shape of the cases; the one-step segments never recycle a slot."""
    bad = P.ring_hazards(1160, 0, 1280, 360)
    assert bad and bad[0] == (3, 24, 1120)
    for n, seg in ((1160, 1280), (2312, 896), (840, 128), (4096, 4096)):
        for P0 in range(0, n, seg):
            for beta8 in (8, 288, 296, 344, 352):
                assert P.ring_hazards(n, P0, seg, beta8) == [], (n, P0, beta8)
    assert P.ring_hazards(4096, 0, 4096, 360)


@pytest.mark.parametrize("fault", P.WINDOW_FAULTS)
def test_window_fault_fails(fault):
    fault_fails(P.window_setup(WINDOW_FAULT_CASE[fault]), fault)


# ---------------------------------------------------------------- tile cases
@pytest.mark.parametrize("ordered", [False, True], ids=["natural", "row_order"])
@pytest.mark.parametrize("name", list(P.TILE_CASES))
def test_tile_case(lib_built, name, ordered):
    c = P.tile_setup(name, ordered)                    # asserts ustride 319 / 320, tiled or not
    p = P.tile_path(c)
    n, B, tr, w, kind = P.TILE_CASES[name]
    deg = np.diff(c.rp)
    if kind == "cap319":
        assert c.rt.ustride == 319 and p.tiled and p.lds == (160 if w == 128 else 80) * 1024
    if kind == "cap320":
        assert c.rt.ustride == 320 and not p.tiled
    if kind == "deg":
        assert set(deg.tolist()) == set(P.TILE_DEGREES) and p.tiled
    if name == "t_tr1":
        assert p.tiles == c.rows and p.rpg == 1
    if name == "t_tr100_tail":
        assert p.rpg == 2 and p.short_last == 11 and p.tiles == 2
    if name == "t_tr65":
        assert p.rpg == 2 and p.short_last == 0
    if name == "t_tr128":
        assert p.rpg == 2 and p.xcd_major and p.grid % 8 == 0
    if name == "t_run3":
        assert p.tiles == 1560 and p.grid == 512 and p.xcd_major and deg.max() > 32
    assert len(c.rt.rows) == c.rows and len(c.rt.trp) == c.rows + 1 and len(c.rt.lcol) == c.rp[-1]
    assert len(c.rt.ucol) == p.tiles * c.rt.ustride
    emulation_passes(c)


@pytest.mark.parametrize("fault", P.TILE_FAULTS)
def test_tile_fault_fails(lib_built, fault):
    fault_fails(P.tile_setup(TILE_FAULT_CASE[fault], False), fault)
