"""The factorised training engine of the e2e structure decoder (``snd_e2e_train``, ABI 24)
without a GPU: the float64 restatement of its formulas (tests/e2e_train_ref.py) against
autograd on the literal pair-tensor model (``oracle.ref_disent.structure_decoder_grads``),
every SND_ERR_ARG rule through ctypes (they return before the device is touched), and the
header, the exports and the ABI number."""
import ctypes
import os
import re

import numpy as np
import pytest

import e2e_train_ref as TR
from oracle import ref_disent as RD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", TR.CPU_SHAPES, ids=[f"b{s[0]}_n{s[1]}_d{s[2]}_" + "x".join(map(str, s[3]))
                                                      for s in TR.CPU_SHAPES])
def test_the_factorised_formulas_equal_autograd_on_the_pair_tensor(shape):
    c = TR.operands(*shape, seed=0)
    ce, correct, dz, lg, hg = TR.train_ref(c.z, c.adj, c.layers, c.head)
    rce, rcorrect, rdz, rlg, rhg = RD.structure_decoder_grads(c.z, c.adj, c.layers, c.head)
    assert abs(ce - rce) <= 1e-12 * abs(rce)
    assert correct == rcorrect
    errs = TR.block_errors((dz, lg, hg), (rdz, rlg, rhg))
    assert len(errs) == 1 + 4 * len(shape[3]) + 4
    for k, e in errs.items():
        assert e <= 1e-12, (k, e)


def test_the_v_t_form_of_a_general_layer_is_the_e2e_filter():
    rng = np.random.default_rng(5)
    for N in (1, 2, 5, 8):
        x, w, b = rng.standard_normal((2, N, N, 3)), rng.standard_normal((N, 3, 4)), rng.standard_normal(4)
        g = rng.standard_normal((2, N, N, 4))
        assert np.allclose(TR.layer_fwd(x, w, b), RD.e2e(x, w, b), rtol=0, atol=1e-12)
        for got, ref in zip(TR.layer_bwd(x, w, g), RD.e2e_grads(x, w, b, g)):
            assert np.allclose(got, ref, rtol=0, atol=1e-12)


def test_header_and_library_declare_the_training_engine(lib_built):
    from snd_vae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snd_vae.h")).read()
    so = ctypes.CDLL(lib_built)
    for name in ("snd_e2e_train", "snd_e2e_train_workspace"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert hasattr(so, name), name
    assert "snd_e2e_layer_grad_t" in hdr
    abi = int(re.search(r"#define\s+SND_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert abi == _lib.ABI_VERSION == so.snd_abi_version() and abi >= 24      # 24 introduced the entry points
    assert [f[0] for f in _lib.E2ELayerGrad._fields_] == ["dgamma", "dbeta", "dw", "db"]


class HostArgs:
    """A well-formed argument list over host memory.  No rule below reaches a launch, so
    nothing dereferences these pointers."""

    def __init__(self, _lib, B=2, N=7, Dz=3, hidden=(5, 4)):
        self.L = _lib.lib()
        self._lib = _lib
        self.B, self.N, self.D, self.hidden = B, N, Dz, hidden
        f = lambda n: np.zeros(max(n, 1), np.float32)
        c = hidden[-1]
        self.keep = {"z": f(B * N * Dz), "adj": f(B * N * N), "dz": f(B * N * Dz), "out": np.zeros(2, np.float64)}
        for k, n in (("hg", c), ("hb", c), ("hw", 2 * c), ("hbias", 2)):
            self.keep[k], self.keep["d" + k] = f(n), f(n)
        cin = 2 * Dz
        self.layers = (_lib.E2ELayer * len(hidden))()
        self.grads = (_lib.E2ELayerGrad * len(hidden))()
        for i, co in enumerate(hidden):
            for k, n in (("gamma", cin), ("beta", cin), ("w", N * cin * co), ("b", co)):
                self.keep[f"l{i}{k}"], self.keep[f"g{i}{k}"] = f(n), f(n)
                setattr(self.layers[i], k, self.keep[f"l{i}{k}"].ctypes.data)
                setattr(self.grads[i], "d" + k, self.keep[f"g{i}{k}"].ctypes.data)
            self.layers[i].cout = co
            cin = co
        self.couts = (ctypes.c_int * len(hidden))(*hidden)
        self.need = self.L.snd_e2e_train_workspace(B, N, Dz, self.couts, len(hidden))
        self.keep["ws"] = np.zeros(max(self.need, 1), np.uint8)

    def call(self, **kw):
        p = lambda k: self.keep[k].ctypes.data
        a = dict(z=p("z"), ldz=self.D, adj=p("adj"), B=self.B, N=self.N, D=self.D, layers=self.layers,
                 n_layers=len(self.hidden), hg=p("hg"), hb=p("hb"), hw=p("hw"), hbias=p("hbias"), dz=p("dz"),
                 lddz=self.D, grads=self.grads, dhg=p("dhg"), dhb=p("dhb"), dhw=p("dhw"), dhbias=p("dhbias"),
                 out=p("out"), ws=p("ws"), ws_bytes=self.need)
        a.update(kw)
        rc = self.L.snd_e2e_train(a["z"], a["ldz"], a["adj"], a["B"], a["N"], a["D"], a["layers"], a["n_layers"],
                                  a["hg"], a["hb"], a["hw"], a["hbias"], a["dz"], a["lddz"], a["grads"], a["dhg"],
                                  a["dhb"], a["dhw"], a["dhbias"], a["out"], a["ws"], a["ws_bytes"], None)
        return rc, self._lib.last_error()


def test_train_rejects_bad_arguments_before_any_launch(lib_built):
    from snd_vae_amd import _lib
    h = HostArgs(_lib)
    assert h.need > 0 and h.need % 4 == 0
    nulls = ("z", "adj", "layers", "hg", "hb", "hw", "hbias", "dz", "grads", "dhg", "dhb", "dhw", "dhbias", "out", "ws")
    bad = [{k: None} for k in nulls] + [dict(n_layers=0), dict(n_layers=-1), dict(n_layers=17), dict(B=0), dict(B=-1),
                                       dict(B=262141), dict(N=0), dict(D=0), dict(N=513), dict(ldz=h.D - 1),
                                       dict(lddz=h.D - 1), dict(ws_bytes=h.need - 1)]
    for kw in bad:
        rc, msg = h.call(**kw)
        assert rc == -1, (kw, rc)
        assert msg.startswith("snd_e2e_train:"), (kw, msg)
    for k in nulls:
        assert "null operand" in h.call(**{k: None})[1], k
    assert "workspace" in h.call(ws_bytes=h.need - 1)[1]
    assert "ldz" in h.call(ldz=h.D - 1)[1]
    assert "lddz" in h.call(lddz=h.D - 1)[1]
    assert "n_layers" in h.call(n_layers=0)[1] and "n_layers" in h.call(n_layers=17)[1]
    assert "n_graphs" in h.call(B=262141)[1]
    # d has no bound of its own: only that the launches of layer 0 fit a grid
    for big in ((1 << 24) + 1, 1 << 24):                   # over the cap; n_graphs n 2 d over 2^31 x 256 threads
        rc, msg = h.call(D=big, ldz=big, lddz=big, B=2 if big > 1 << 24 else 262140, N=7 if big > 1 << 24 else 512,
                         ws_bytes=1 << 62)
        assert rc == -1 and msg.startswith("snd_e2e_train: d "), (big, msg)
    assert h.L.snd_e2e_train_workspace(2, 7, (1 << 24) + 1, h.couts, 2) == 0
    # a null operand or gradient inside a layer, a width below 1 or over 512
    for field in ("gamma", "beta", "w", "b"):
        g = HostArgs(_lib)
        setattr(g.layers[1], field, None)
        rc, msg = g.call()
        assert rc == -1 and "null operand" in msg, (field, msg)
        g = HostArgs(_lib)
        setattr(g.grads[0], "d" + field, None)
        rc, msg = g.call()
        assert rc == -1 and "null operand" in msg, (field, msg)
    for width in (0, 513):
        g = HostArgs(_lib)
        g.layers[0].cout = width
        rc, msg = g.call()
        assert rc == -1 and "width" in msg, (width, msg)
    # the head's 32-channel limit; 32 itself and a wider middle layer are fine shapes
    g = HostArgs(_lib, hidden=(5, 33))
    assert g.need == 0
    rc, msg = g.call(ws_bytes=1 << 30)
    assert rc == -1 and "32" in msg, msg
    assert HostArgs(_lib, hidden=(33, 32)).need > 0
    # a bad shape has no workspace size
    W = h.L.snd_e2e_train_workspace
    assert W(0, 7, 3, h.couts, 2) == 0 and W(262141, 7, 3, h.couts, 2) == 0
    assert W(2, 0, 3, h.couts, 2) == 0 and W(2, 513, 3, h.couts, 2) == 0 and W(2, 7, 0, h.couts, 2) == 0
    assert W(2, 7, 3, h.couts, 0) == 0 and W(2, 7, 3, h.couts, 17) == 0 and W(2, 7, 3, None, 2) == 0
    assert W(2, 7, 3, (ctypes.c_int * 2)(5, 0), 2) == 0 and W(2, 7, 3, (ctypes.c_int * 2)(513, 4), 2) == 0


def test_the_host_op_rejects_an_unknown_engine():
    from snd_vae_amd import disent
    assert disent.ENGINES == ("direct", "factorised")
    with pytest.raises(ValueError, match="engine"):
        disent.structure_decoder(np.zeros((1, 2, 3)), None, [], {}, engine="fused")
