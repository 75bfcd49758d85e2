"""snd_zzt_ce and snd_zzt_ce_rows at the C ABI, every link on its own operands.

Raw ctypes on guarded operands (tests/abi_ops.py): z, rowptr (a slice for _rows), colidx,
stats, dz and a workspace of EXACTLY the queried bytes, every one between guard bands, the
outputs and the whole workspace pre-filled with the NaN pattern -- a partial that the stats
kernel sums but no block wrote, or a slab row the split sum reads unwritten, poisons the
result.  Two pointer placements: on a 256-byte boundary, and 16 bytes past one (the ABI
promises the kernels no more than 16 bytes).

Each case asserts every link of tests/zzt_ops.py (the staging images bit for bit, their
padding exactly zero, colpart, ej and -- for a row range -- dJd read from the workspace; dz per
element, no exclusions; stats[1] exact up to the counted ambiguous pairs; stats[0] at
1e-6 of sum |terms|), every guard, a second call bitwise equal in stats and dz, and the
column-split count the case is there for (zzt_tsplit_blocks' formula with the device's CU
count).  One line per case is printed ("ZZT_ABI <id> <link> <ratio> ...") and appended to
zzt_abi_errors.jsonl beside own_operand_errors.jsonl.
"""
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import abi_ops as A
import own_operands as O
import parity_bars as PB
import zzt_ops as Z
from test_gpu_abi_ops import Device, ids, lib, ok  # noqa: F401
from test_gpu_abi_ops_sg import rejected

pytestmark = pytest.mark.gpu
LOG = os.path.join(os.path.dirname(PB.LOG), "zzt_abi_errors.jsonl")
SPLIT_CASES = ("n129", "n300", "n1000", "n1300", "pw129", "pw300")     # bf16: column splits expected


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def operands(c, place, ws_bytes, z, rp, ci):
    """The guarded operands; place 0: every pointer on a 256-byte boundary, 1: 16 bytes past."""
    bf = c.dtype == Z.BF16
    o4, o8 = (4 * place), (64 + 8 * place)             # f32 / i32 elements; bf16 elements (G is 128 bytes there)
    rows = c.r1 - c.r0
    bufs = {"z": A.guarded(c.B * c.n, c.d, offset=o4, data=z, name="z"),
            "rowptr": A.vec(rows + 1, "i32", offset=o4, data=rp[c.r0:c.r1 + 1], name="rowptr"),
            "stats": A.vec(2, "f64", offset=2 * place, name="stats"),
            "dz": A.guarded(rows, c.d, offset=o4, name="dz"),
            "ws": A.vec(ws_bytes // 2, "bf16", offset=o8, name="ws") if bf else
                  A.vec(ws_bytes // 4, "f32", offset=o4, name="ws")}
    if len(ci):
        bufs["colidx"] = A.vec(len(ci), "i32", offset=o4, data=ci, name="colidx")
    return NS(bufs=bufs)


def call(L, S, c, dev, need, **over):
    a = dict(z=dev.p("z"), dz=dev.p("dz"), ws=dev.p("ws"), ws_bytes=need, d=c.d, n=c.n, r0=c.r0, r1=c.r1, dtype=c.dtype)
    a.update(over)
    rp, ci, st = dev.p("rowptr"), dev.p("colidx"), dev.p("stats")
    if c.rows:
        return L.snd_zzt_ce_rows(a["z"], a["n"], a["d"], a["r0"], a["r1"], rp, ci, c.pw, c.norm, st, a["dz"], a["ws"],
                                 a["ws_bytes"], a["dtype"], S)
    return L.snd_zzt_ce(a["z"], c.B, a["n"], a["d"], rp, ci, c.pw, c.norm, st, a["dz"], a["ws"], a["ws_bytes"],
                        a["dtype"], S)


def query(L, c, **over):
    a = dict(d=c.d, n=c.n, r0=c.r0, r1=c.r1, dtype=c.dtype)
    a.update(over)
    if c.rows:
        return L.snd_zzt_ce_rows_workspace(a["n"], a["d"], a["r0"], a["r1"], a["dtype"])
    return L.snd_zzt_ce_workspace(c.B, a["n"], a["d"], a["dtype"])


def run(c, place):
    """One case: both calls, every link, guards; returns (ratios, stats of the first call)."""
    L, S, _ = lib()
    (z, rp, ci), _ = Z.setup(c)
    cu = ncu()
    r = Z.reference(c, z, rp, ci, ncu=cu) if cu != Z.NCU else Z.setup(c)[1]
    need = query(L, c)
    lay, total, ts = Z.layout(c, cu)
    # ---- the path: the workspace holds exactly the mirrored carve, with the expected splits
    assert need == total, (c.name, need, total, ts)
    wgs = (-(-c.r1 // 128) - c.r0 // 128) if c.rows else c.B * (Z.npad(c.n) // 128)
    assert ts == Z.tsplit_blocks(wgs, c.n, c.dtype, cu) <= min(8, Z.npad(c.n) // 128)
    if c.dtype == Z.BF16 and c.id in SPLIT_CASES:
        assert ts >= 2, f"{c.name}: meant for column splits, gets none at {cu} CUs"
    ctx = operands(c, place, need, z, rp, ci)
    d = Device(ctx)
    for k in ("z", "dz", "ws"):
        assert d.p(k) % 256 == 16 * place, (k, d.p(k) % 256)
    ok(call(L, S, c, d, need), "snd_zzt_ce")
    a1 = d.back()
    ok(call(L, S, c, d, need), "snd_zzt_ce")
    a2 = d.back()
    A.check_guards(ctx, a1)
    A.check_guards(ctx, a2)
    got = Z.read_ws(c, ctx.bufs["ws"].block(a1["ws"]), cu)
    got["dz"] = ctx.bufs["dz"].values(a1["dz"])
    got["stats"] = ctx.bufs["stats"].values(a1["stats"]).reshape(2)
    res = Z.check(c, r, got, strict=False)
    print("ZZT_ABI", f"{c.name}_p{place}", " ".join(f"{k} {v:.4f}" for k, v in res.items()), "amb", r.amb, "ts", ts)
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(json.dumps({"case": c.name, "place": place, "kernel": Z.kernel(c.d, c.dtype), "splits": ts,
                            "ambiguous": r.amb, "links": {k: float(v) for k, v in res.items()}}) + "\n")
    assert r.amb <= Z.amb_cap(c), (c.name, r.amb)
    Z.check(c, r, got, strict=True)                       # fails naming the link and the element
    for k in ("stats", "dz"):
        assert np.array_equal(a1[k].view(np.uint8), a2[k].view(np.uint8)), f"{c.name}: {k} differs in a second call"
    return res, got["stats"], r


@pytest.mark.parametrize("place", [0, 1], ids=["aligned256", "plus16"])
@pytest.mark.parametrize("c", Z.CASES, ids=[c.name for c in Z.CASES])
def test_zzt_ce(c, place):
    run(c, place)


@pytest.mark.parametrize("place", [0, 1], ids=["aligned256", "plus16"])
@pytest.mark.parametrize("c", Z.ROWS_CASES, ids=[c.name for c in Z.ROWS_CASES])
def test_zzt_ce_rows(c, place):
    run(c, place)


@pytest.mark.parametrize("dtype", [Z.F32, Z.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,d", [(129, 16), (129, 32), (129, 64), (129, 128), (300, 16), (300, 32), (300, 64), (300, 128)])
def test_zzt_ce_rows_partition_sums_to_the_graph(n, d, dtype):
    """The stats of a partition of [0, n) sum to the whole-graph reference (same z, same CSR)."""
    parts = [c for c in Z.ROWS_CASES if (c.n, c.d, c.dtype) == (n, d, dtype) and (c.r0, c.r1) in Z.PARTITIONS[n]]
    assert [(c.r0, c.r1) for c in parts] == list(Z.PARTITIONS[n])
    whole = Z.case(parts[0].id, 1, n, d, dtype, pw=parts[0].pw, norm=parts[0].norm)
    (z, rp, ci), _ = Z.setup(parts[0])
    for c in parts[1:]:
        assert np.array_equal(Z.setup(c)[0][0], z), "the ranges of one n share z"
    r = Z.reference(whole, z, rp, ci, ncu=ncu())
    s = sum(run(c, 0)[1] for c in parts)
    assert abs(s[0] - r.s0) <= Z.S0_BAR * r.s0_abs, (s[0], r.s0)
    assert abs(s[1] - r.s1) <= r.amb_w, (s[1], r.s1, r.amb)


# ---------------------------------------------------------------- rejections
def _reject_ctx(rows=False):
    c = [k for k in (Z.ROWS_CASES if rows else Z.CASES) if (k.n, k.d, k.dtype) == (300, 32, Z.BF16)][0]
    L, S, _ = lib()
    (z, rp, ci), _ = Z.setup(c)
    need = query(L, c)
    d = Device(operands(c, 0, need, z, rp, ci))
    return L, S, c, d, need


@pytest.mark.parametrize("rows", [False, True], ids=["ce", "rows"])
@pytest.mark.parametrize("what", ["ws_short", "d48", "n0", "dtype", "z_misaligned", "dz_misaligned", "ws_misaligned"])
def test_rejects(what, rows):
    L, S, c, d, need = _reject_ctx(rows)
    over = {"ws_short": dict(ws_bytes=need - 1), "d48": dict(d=48), "n0": dict(n=0), "dtype": dict(dtype=7),
            "z_misaligned": dict(z=d.p("z") + 4), "dz_misaligned": dict(dz=d.p("dz") + 8),
            "ws_misaligned": dict(ws=d.p("ws") + 2, ws_bytes=need)}[what]
    # (nothing launches: a misaligned pointer is only compared, never dereferenced)
    rejected(call(L, S, c, d, need, **over), d, "snd_zzt_ce_rows" if rows else "snd_zzt_ce")


@pytest.mark.parametrize("what", ["row0_64", "row1_off_block"])
def test_rows_rejects_a_range_off_the_row_blocks(what):
    L, S, c, d, need = _reject_ctx(True)
    over = dict(r0=64, r1=128) if what == "row0_64" else dict(r0=0, r1=200)      # n = 300
    rejected(call(L, S, c, d, need, **over), d, "snd_zzt_ce_rows")


# ---------------------------------------------------------------- v1 on its own operands
V1_CASES = tuple(k[:7] for k in O.CASES if k[1] == "tscale" and k[5] is None and not k[6] and not k[7])   # default weights


@pytest.mark.parametrize("name,topology,n,d,B,kbar,chain", V1_CASES, ids=[k[0] for k in V1_CASES])
def test_v1_on_its_own_operands(name, topology, n, d, B, kbar, chain):
    """zzt_dense_bf16<DP> (variant 1, bench.py's previous_variant) launched on the step's staged
    operands: dJd per element with the step's own dJd link (K role the staged rows, V role the
    unscaled transposed image, s rounded to bf16, the diagonal masked, no splits), the loss
    partials against the dense part of parity_bars.own_structure at its 1e-6 bar, the count
    exact up to the ambiguous pairs."""
    from snd_vae_amd import _lib
    from snd_vae_amd.model import DeviceBatch, SGCNModelVAE
    from snd_vae_amd.optimizer import OptimizerVAE
    assert len(V1_CASES) == 4
    cfg, batch, p, eps = O.make_case(topology, n, d, B, kbar)
    model = SGCNModelVAE(cfg, B, dtype="bf16", blocks=p)
    opt = OptimizerVAE(model, fuse_adam=False)
    db = DeviceBatch(batch)
    opt.forward_backward(db, torch.from_numpy(eps).cuda())
    torch.cuda.synchronize()
    pz = model.buffer("PZZT", torch.float64)
    pz.zero_()
    model.buffer("DJD").fill_(float("nan"))
    _lib.check(_lib.lib().snd_plan_launch(model.plan, db.c_struct(), model.workspace.data_ptr(), b"zzt_dense_v1",
                                          _lib.stream_ptr()))
    torch.cuda.synchronize()
    R, P, dp = B * n, Z.npad(n), O.zzt_dp(d)
    st = model.buffer("ZSTAGE", torch.bfloat16)
    img = B * P * dp
    jt0 = Z.r256(img * 2) // 2                               # zzt_stage: [jrow | jt | colpart]
    jrow = st[:img].view(B, P, dp).double().cpu().numpy()
    jt = st[jt0:jt0 + img].view(B, dp, P).double().cpu().numpy()
    assert not jrow[:, n:].any() and not jrow[:, :, d:].any() and not jt[:, d:].any() and not jt[:, :, n:].any()
    parts = [O.djd_graph(jrow[g, :n, :d], jt[g, :d, :n].T.copy(), 1.0, d, lambda a: np.asarray(a, np.float64), O.bf16)
             for g in range(B)]
    link = O.Link(*(np.concatenate([q[k] for q in parts]) for k in (0, 1)), n + 2,
                  extra=np.concatenate([q[2] for q in parts]))
    got = model.buffer("DJD")[:R * d].view(R, d).double().cpu().numpy()
    ratio = A.assert_link(f"v1 {name} DJD", link, got)
    ce, pos, amb = PB.own_structure_dense(jrow[:, :n, :d])
    s = pz.view(-1, 2).sum(0).cpu().numpy()
    print("ZZT_ABI", f"v1_{name}", f"djd {ratio:.4f} stats0 {abs(s[0] - ce) / (1e-6 * ce):.4f} count_diff {s[1] - pos:.0f} amb {amb}")
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(json.dumps({"case": "v1_" + name, "kernel": f"v1<{dp}>", "ambiguous": amb,
                            "links": {"djd": ratio, "stats0": abs(s[0] - ce) / (1e-6 * ce), "count_diff": float(s[1] - pos)}}) + "\n")
    assert abs(s[0] - ce) <= 1e-6 * ce, (s[0], ce)
    assert abs(s[1] - pos) <= amb, (s[1], pos, amb)
