"""Inference of the disentangled model without a GPU: the references of
tests/disent_infer_ref.py against each other and the oracle, the traverse rows of
snd_vae_amd/disent_model.py against the literal transcription of model.py:232-358, and the
host side of ``snd_e2e_decode`` (ABI 22): the header, the exports, and every SND_ERR_ARG
rule, which the entry point checks before anything touches the device.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import disent_infer_ref as IR
from oracle import ref_disent as RD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def operands(N, seed, B=2, Dz=3, hidden=(5, 4)):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, N, Dz))
    layers, cin = [], 2 * Dz
    for co in hidden:
        layers.append({"gamma": rng.standard_normal(cin), "beta": 0.3 * rng.standard_normal(cin),
                       "w": rng.standard_normal((N, cin, co)) / np.sqrt(2 * N * cin), "b": 0.3 * rng.standard_normal(co)})
        cin = co
    head = {"gamma": rng.standard_normal(cin), "beta": 0.3 * rng.standard_normal(cin),
            "w": rng.standard_normal((cin, 2)), "b": rng.standard_normal(2)}
    return z, layers, head


@pytest.mark.parametrize("N,hidden", [(7, (5, 4)), (8, (5, 4)), (25, (6, 3)), (8, (6,)), (1, (4, 3))])
def test_factorised_layer0_is_the_literal_decoder(N, hidden):
    """Odd and even N (asymmetric SAME padding), one layer, a lone node."""
    z, layers, head = operands(N, N, hidden=hidden)
    lit = IR.structure_literal(z, layers, head)[0].numpy()
    fac = IR.structure_factorised(z, layers, head)
    assert np.abs(lit - fac).max() <= 1e-12 * max(1.0, np.abs(lit).max())
    assert (lit[:, np.arange(N), np.arange(N)] == -1).all()
    bound = IR.margin_bound(z, layers, head)
    assert np.abs(bound.margin - lit).max() <= 1e-12 * max(1.0, np.abs(lit).max())


@pytest.mark.parametrize("N", [7, 8])
def test_margin_sign_counts_what_structure_decoder_counts(N):
    z, layers, head = operands(N, 10 + N)
    rng = np.random.default_rng(N)
    adj = (rng.random((2, N, N)) < 0.4).astype(np.float64)
    t = lambda a: torch.tensor(a)
    lt = [{k: t(v) for k, v in l.items()} for l in layers]
    ht = {k: t(v) for k, v in head.items()}
    correct = RD.structure_decoder_torch(t(z), adj, lt, ht)[1]
    margin, a = IR.structure_literal(z, layers, head)
    assert ((margin.numpy() > 0) == adj).sum() == correct
    assert (a.numpy() == (margin.numpy() > 0)).all()


def test_the_margin_bars_admit_the_float32_reference():
    """Both bars hold for a correct fp32 implementation: the literal decoder run in
    torch.float32 (another summation order than the kernel's) stays inside the derived rule
    and inside the bar of the C ABI test, which is never the looser of the two."""
    for case in IR.DECODE_CASES[:2] + IR.DECODE_CASES[3:5]:
        c = IR.decode_operands(case, 0)
        r = IR.margin_bar(c.z, c.layers, c.head)
        m32 = IR.structure_literal(c.z, c.layers, c.head, torch.float32)[0].double().numpy()
        offd = ~np.eye(c.N, dtype=bool)
        err = np.abs(m32 - r.margin)[:, offd]
        assert (err < r.rule[:, offd]).all() and (err < r.bound[:, offd]).all()
        assert (r.bound <= r.rule).all() and r.e32 < 1e-5


def bases(M, Ls, Lg, Lsg, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((M, Ls)).astype(np.float32), rng.standard_normal((M, Lg)).astype(np.float32),
            rng.standard_normal((M, Lsg)).astype(np.float32))


@pytest.mark.parametrize("per_block", [False, True])
def test_traverse_rows_are_the_reference_construction(per_block):
    from snd_vae_amd.disent_model import traverse_all_rows, traverse_rows
    Ls, Lg, Lsg, V = 3, 2, 4, 5
    length = Ls + Lg + Lsg
    zs, zg, zsg = bases(length if per_block else 1, Ls, Lg, Lsg)
    rang = np.arange(-10, 10, 2)[:V]                             # model.py:341
    tile = lambda a: a if per_block else np.repeat(a, length, axis=0)
    ref = IR.traverse_all_rows_literal(tile(zs), tile(zg), tile(zsg), rang, V)
    got = traverse_all_rows(zs, zg, zsg, rang)
    for g, r in zip(got, ref):
        assert g.dtype == np.float32 and g.shape == r.shape == (length * V, r.shape[1])
        assert np.array_equal(g, r)
    for group, n in (("s", Ls), ("g", Lg), ("sg", Lsg)):
        for dim in range(n):
            ref1 = IR.traverse_rows_literal(group, dim, tile(zs), tile(zg), tile(zsg), rang, V)
            got1 = traverse_rows(group, dim, zs, zg, zsg, rang)
            for g, r in zip(got1, ref1):
                assert np.array_equal(g, r), (group, dim)
    # per-group values
    got = traverse_all_rows(zs, zg, zsg, {"s": rang, "g": rang + 1, "sg": rang + 2})
    assert np.array_equal(got[1][Ls * V:(Ls + 1) * V, 0], rang + 1)
    assert np.array_equal(got[2][(Ls + Lg) * V:(Ls + Lg + 1) * V, 0], rang + 2)


def test_traverse_rows_reject_bad_shapes():
    from snd_vae_amd.disent_model import mean_over_copies, traverse_all_rows, traverse_rows
    zs, zg, zsg = bases(2, 3, 2, 4)                              # 2 rows: neither 1 nor 9
    with pytest.raises(ValueError):
        traverse_all_rows(zs, zg, zsg, [0.0, 1.0])
    zs, zg, zsg = bases(1, 3, 2, 4)
    with pytest.raises(ValueError):
        traverse_all_rows(zs, zg, zsg, [])
    with pytest.raises(ValueError):
        traverse_rows("s", 3, zs, zg, zsg, [0.0])
    with pytest.raises(ValueError):
        traverse_rows("x", 0, zs, zg, zsg, [0.0])
    z = np.arange(24, dtype=np.float32).reshape(6, 4)
    assert np.array_equal(mean_over_copies(z, 3), z.reshape(2, 3, 4).mean(1))   # main.py:407
    with pytest.raises(ValueError):
        mean_over_copies(z, 4)


# ---------------------------------------------------------------- the C ABI, host side
def test_header_and_library_declare_the_decoder(lib_built):
    from snd_vae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snd_vae.h")).read()
    so = ctypes.CDLL(lib_built)
    for name in ("snd_e2e_decode", "snd_e2e_decode_workspace"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert hasattr(so, name), name
    assert "snd_e2e_layer_t" in hdr and "model.py:193-208" in hdr
    assert int(re.search(r"#define\s+SND_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 22
    assert _lib.ABI_VERSION >= 22


class HostArgs:
    """A well-formed argument list over host memory.  No rule below reaches a launch, so
    nothing dereferences these pointers."""

    def __init__(self, _lib, B=2, N=7, Dz=3, hidden=(5, 4)):
        self.L = _lib.lib()
        self._lib = _lib
        self.B, self.N, self.D, self.hidden = B, N, Dz, hidden
        f = lambda n: np.zeros(max(n, 1), np.float32)
        self.keep = {"z": f(B * N * Dz), "hg": f(hidden[-1]), "hb": f(hidden[-1]), "hw": f(2 * hidden[-1]), "hbias": f(2),
                     "adj": np.zeros(B * N * N, np.uint8), "margin": f(B * N * N)}
        cin = 2 * Dz
        self.layers = (_lib.E2ELayer * len(hidden))()
        for i, co in enumerate(hidden):
            for k, n in (("gamma", cin), ("beta", cin), ("w", N * cin * co), ("b", co)):
                self.keep[f"l{i}{k}"] = f(n)
                setattr(self.layers[i], k, self.keep[f"l{i}{k}"].ctypes.data)
            self.layers[i].cout = co
            cin = co
        self.couts = (ctypes.c_int * len(hidden))(*hidden)
        self.need = self.L.snd_e2e_decode_workspace(B, N, Dz, self.couts, len(hidden))
        self.keep["ws"] = np.zeros(self.need, np.uint8)

    def call(self, **kw):
        p = lambda k: self.keep[k].ctypes.data
        a = dict(z=p("z"), ldz=self.D, B=self.B, N=self.N, D=self.D, layers=self.layers, n_layers=len(self.hidden),
                 hg=p("hg"), hb=p("hb"), hw=p("hw"), hbias=p("hbias"), adj=p("adj"), margin=p("margin"),
                 ws=p("ws"), ws_bytes=self.need)
        a.update(kw)
        rc = self.L.snd_e2e_decode(a["z"], a["ldz"], a["B"], a["N"], a["D"], a["layers"], a["n_layers"], a["hg"],
                                   a["hb"], a["hw"], a["hbias"], a["adj"], a["margin"], a["ws"], a["ws_bytes"], None)
        return rc, self._lib.last_error()


def test_decode_rejects_bad_arguments_before_any_launch(lib_built):
    from snd_vae_amd import _lib
    h = HostArgs(_lib)
    assert h.need > 0
    bad = [dict(z=None), dict(layers=None), dict(hg=None), dict(hb=None), dict(hw=None), dict(hbias=None),
           dict(adj=None), dict(ws=None), dict(n_layers=0), dict(n_layers=-1), dict(B=0), dict(N=0), dict(D=0),
           dict(ldz=h.D - 1), dict(ws_bytes=h.need - 1)]
    for kw in bad:
        rc, msg = h.call(**kw)
        assert rc == -1, (kw, rc)
        assert msg.startswith("snd_e2e_decode:"), (kw, msg)
    assert "workspace" in h.call(ws_bytes=h.need - 1)[1]
    assert "ldz" in h.call(ldz=h.D - 1)[1]
    assert "n_layers" in h.call(n_layers=0)[1]
    # a null operand inside a layer, a width below 1
    for field in ("gamma", "beta", "w", "b"):
        g = HostArgs(_lib)
        setattr(g.layers[1], field, None)
        rc, msg = g.call()
        assert rc == -1 and "null operand" in msg, (field, msg)
    g = HostArgs(_lib)
    g.layers[0].cout = 0
    rc, msg = g.call()
    assert rc == -1 and "width" in msg, msg
    # the head's 32-channel limit (snd_e2e_head_ce's); 32 itself and a wider middle layer are fine shapes
    g = HostArgs(_lib, hidden=(5, 33))
    rc, msg = g.call()
    assert rc == -1 and "32" in msg, msg
    assert HostArgs(_lib, hidden=(33, 32)).need > 0
    # a bad shape has no workspace size
    assert h.L.snd_e2e_decode_workspace(0, 7, 3, h.couts, 2) == 0
    assert h.L.snd_e2e_decode_workspace(2, 7, 3, h.couts, 0) == 0
    assert h.L.snd_e2e_decode_workspace(2, 7, 3, None, 2) == 0


@pytest.mark.parametrize("case", IR.DECODE_CASES, ids=[c[0] for c in IR.DECODE_CASES])
def test_decode_workspace_is_within_the_cap(lib_built, case):
    """At most two activations of the widest layer plus the weight image.  A lone node
    (N = 1) has no pair structure to save on: its per-node terms are as large as an
    activation, and the cap is not claimed there."""
    from snd_vae_amd import _lib
    _, B, N, Dz, hidden, _, _ = case
    couts = (ctypes.c_int * len(hidden))(*hidden)
    need = _lib.lib().snd_e2e_decode_workspace(B, N, Dz, couts, len(hidden))
    assert need > 0 and need % 4 == 0
    if N > 1:
        assert need <= IR.workspace_limit(B, N, Dz, hidden), (need, IR.workspace_limit(B, N, Dz, hidden))
    # no pair tensor: far below [B, N, N, 2D] + an activation once N is not tiny
    if case[0] == "ref":
        assert need < B * N * N * (2 * Dz + 2 * max(hidden)) * 4
