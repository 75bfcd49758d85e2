"""snd_csr_spmm_bf16_window and snd_csr_spmm_bf16_tiled at their plan limits, through the raw
entry points on the guarded operands of tests/spmm_plans.py: h with ldh = width + 8, out with
ldo = width + 16, every plan array a guarded vector of exactly the planner's length (slots:
the documented trailing entries and nothing more).

One call per case; afterwards every output element is within its derived bound of the float64
reference (the failure names the element), empty rows are +0, no element is left at the
pattern, every guard and padding element is intact, every input is bitwise unchanged, and out
is bitwise what snd_csr_spmm_bf16 leaves on the same operands and schedule (the header's
contract).  The ratios are printed ("ABI_RATIO <op> <case> out <ratio>"; run with -s):
DESIGN.md §3 records them, the bars stay the derived bounds.
"""
import ctypes

import numpy as np
import pytest
import torch

import abi_ops as A
import spmm_plans as P

pytestmark = pytest.mark.gpu

ERR_ARG = -1
_VIEW = {"bf16": np.int16, "u16": np.int16}


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def lib():
    from snd_vae_amd import _lib
    return _lib.lib(), _lib.stream_ptr(), _lib


class Device:
    """The guarded buffers of a context on the device."""

    def __init__(self, c):
        self.c = c
        self.t = {k: torch.from_numpy(g.arr.view(_VIEW.get(g.dtype, g.arr.dtype))).cuda() for k, g in c.bufs.items()}

    def p(self, name):
        g = self.c.bufs.get(name)
        return 0 if g is None else self.t[name].data_ptr() + g.off * g.arr.itemsize

    def back(self):
        torch.cuda.synchronize()
        return {k: t.cpu().numpy().view(self.c.bufs[k].arr.dtype) for k, t in self.t.items()}


def call_window(c, d, **over):
    L, S, _ = lib()
    a = dict(meta=d.p("meta"), slots=d.p("slots"), rows=d.p("rows"), order=d.p("order"), n_rows=c.rows,
             n_per_graph=c.n, n_graphs=c.B, beta=c.beta, h=d.p("h"), ldh=c.bufs["h"].ld, width=c.width,
             out=d.p("out"), ldo=c.bufs["out"].ld)
    a.update(over)
    return L.snd_csr_spmm_bf16_window(*a.values(), S)


def call_tiled(c, d, **over):
    L, S, _lib = lib()
    a = dict(rowptr=d.p("rowptr"), colidx=d.p("colidx"), n_rows=c.rows, tiles=True, h=d.p("h"), ldh=c.bufs["h"].ld,
             width=c.width, out=d.p("out"), ldo=c.bufs["out"].ld, n_per_graph=c.n, n_graphs=c.B,
             row_order=d.p("row_order"), tile_rows=c.tile_rows)
    a.update(over)
    tr = a.pop("tile_rows")
    t = _lib.RowTiles(d.p("rows"), d.p("trp"), d.p("lcol"), d.p("ucol"), tr, c.rt.ustride)
    a["tiles"] = ctypes.byref(t) if a["tiles"] else None
    return L.snd_csr_spmm_bf16_tiled(*a.values(), S)


def call_ref(c, d):
    """snd_csr_spmm_bf16 on the same h, CSR and schedule, into out_ref."""
    L, S, _lib = lib()
    _lib.check(L.snd_csr_spmm_bf16(d.p("rowptr"), d.p("colidx"), c.rows, d.p("h"), c.bufs["h"].ld, c.width,
                                   d.p("out_ref"), c.bufs["out_ref"].ld, c.n, c.B,
                                   d.p("order" if c.op == "window" else "row_order"), S), "snd_csr_spmm_bf16")


def run(c, call, op, flag=0, ref=True):
    """One call on fresh device buffers; everything the module text lists.  Returns out's bits."""
    _, _, _lib = lib()
    d = Device(c)
    _lib.check(_lib.lib().snd_debug_set(flag))
    try:
        rc = call(c, d)
        torch.cuda.synchronize()
    finally:
        _lib.check(_lib.lib().snd_debug_set(0))
    _lib.check(rc, op)
    if ref:
        call_ref(c, d)
    after = d.back()
    ratio = P.verify(c, after)
    print(f"ABI_RATIO {op} {c.name}{'_dbg%d' % (flag >> 24) if flag else ''} out {ratio:.4f}")
    out = c.bufs["out"].block(after["out"]).copy()
    if ref:
        assert np.array_equal(out, c.bufs["out_ref"].block(after["out_ref"])), f"{op} {c.name}: not bitwise snd_csr_spmm_bf16"
    return out


# ---------------------------------------------------------------- the window kernel
@pytest.mark.parametrize("name", list(P.WINDOW_CASES))
def test_window(name):
    c = P.window_setup(name)
    assert len(c.bufs["slots"].arr) == len(c.wp.slots) + 2 * A.G           # the planner's length between the guards
    out = run(c, call_window, "csr_spmm_bf16_window")
    if name == "w_run_288":
        # the two-barrier schedule forced at the one-barrier limit, and wave w summing group w
        for flag in (32 << 24, 64 << 24):
            assert np.array_equal(run(c, call_window, "csr_spmm_bf16_window", flag, ref=False), out), flag >> 24


# ---------------------------------------------------------------- the row-tile kernel
@pytest.mark.parametrize("ordered", [False, True], ids=["natural", "row_order"])
@pytest.mark.parametrize("name", list(P.TILE_CASES))
def test_tiled(name, ordered):
    c = P.tile_setup(name, ordered)
    run(c, call_tiled, "csr_spmm_bf16_tiled")


# ---------------------------------------------------------------- rejected calls
def rejected(c, d, rc, entry, what):
    """SND_ERR_ARG, a message naming the entry point, every buffer as it was."""
    _, _, _lib = lib()
    assert rc == ERR_ARG, (what, rc)
    assert entry in _lib.last_error(), (what, _lib.last_error())
    after = d.back()
    for k, g in c.bufs.items():
        assert np.array_equal(after[k].view(np.uint8), g.arr.view(np.uint8)), f"{what}: {k} changed by a rejected call"


def test_window_rejects():
    c = P.window_setup("w_one_288")
    d = Device(c)
    bad = [dict(beta=353), dict(beta=-1), dict(width=48), dict(width=128), dict(ldh=68), dict(ldo=56),
           dict(n_rows=c.rows + 1), dict(n_per_graph=c.n + 1)]
    bad += [{k: 0} for k in ("meta", "slots", "rows", "order", "h", "out")]
    for over in bad:
        rejected(c, d, call_window(c, d, **over), "snd_csr_spmm_bf16_window", over)
    run(c, call_window, "csr_spmm_bf16_window")                             # and an accepted one


def test_tiled_rejects():
    c = P.tile_setup("t_tr65", True)
    d = Device(c)
    bad = [dict(tile_rows=0), dict(tile_rows=129), dict(width=4), dict(width=136), dict(ldh=c.width + 4),
           dict(tiles=False), dict(h=0), dict(out=0)]
    for over in bad:
        rejected(c, d, call_tiled(c, d, **over), "snd_csr_spmm_bf16_tiled", over)
    run(c, call_tiled, "csr_spmm_bf16_tiled")
