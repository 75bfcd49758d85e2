"""snd_graph_spectrum without a GPU (ABI 28): the reference's closed forms against its own
eigvalsh route, the device's doubled recurrence against both, metrics.SpectrumStats (the
Jackson-kernel density and its resolution), the header / library / binding / stub agreement and
every SND_ERR_ARG rule (none reaches a launch).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import graph_motifs_ref as M
import graph_spectrum_ref as S
import graph_stats_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("name", list(S.NAMED))
def test_closed_forms_equal_the_eigvalsh_route(name):
    c, lam = S.named_case(name)
    got = S.laplacian_spectrum(c, 0)
    assert np.abs(got - lam).max() <= 1e-12, name
    K = 128
    assert np.abs(S.exact_moments(c, K)[0] - S.moments_of_spectrum(lam, K)).max() <= 1e-9 * c.n
    padded, lam_p = S.named_case(name, pad=5)                                # isolated nodes: eigenvalue 0 of L
    assert np.abs(S.laplacian_spectrum(padded, 0) - lam_p).max() <= 1e-12
    assert S.info(padded)[0, 1] == 5 + (c.n if name == "empty25" else 0)


def test_the_empty_graph_alternates():
    c, _ = S.named_case("empty25")
    assert np.array_equal(S.exact_moments(c, 9)[0], 25.0 * (-1.0) ** np.arange(9))
    assert S.info(c).tolist() == [[0, 25, 0, 25]]


def test_the_table_of_the_issue():
    lam = lambda name: S.named_case(name)[1]
    assert np.allclose(lam("K40"), [0.0] + [40.0 / 39.0] * 39, atol=0, rtol=1e-15)
    assert np.allclose(np.sort(lam("C30")), np.sort(1 - np.cos(2 * np.pi * np.arange(30) / 30)), atol=1e-15)
    assert np.allclose(np.sort(lam("P33")), np.sort(1 - np.cos(np.pi * np.arange(33) / 32)), atol=1e-15)
    for name, n in (("star50", 50), ("K8_12", 20)):
        assert np.array_equal(lam(name), [0.0] + [1.0] * (n - 2) + [2.0])


@pytest.mark.parametrize("name", ["b70_mixed", "n64", "k64", "n65", "r257", "k200"])
def test_the_doubled_recurrence_equals_the_eigvalsh_route(name):
    """The device's route (K / 2 applications of M, doubling identities) in float64 against the
    reference's, exact and probe mode: 2e-11 at most on these cases, the bar of the GPU test is
    1e-9 N."""
    c = S.build_case(name)
    K = S.CASES[name]
    want = S.reference(name)[0]
    worst = 0.0
    for g in range(0, c.B, 7):
        Mm = S.operator(c, g)[0]
        got = S.doubled_moments(Mm, np.eye(c.n), K)
        worst = max(worst, np.abs(got - want[g]).max())
        assert got[0] == c.n and got[1] == -S.info(c)[g, 1]
        V = S.probe_signs(c.n, 40, g, 9)
        assert np.abs(S.doubled_moments(Mm, V, K) - S.plain_moments(Mm, V, K)).max() / 40 <= 1e-9 * c.n
    print(f"GSPECTRUM doubled vs eigvalsh {name}: {worst:.3g}")
    assert worst <= 1e-9 * c.n
    for g, lam in S.known_spectra(name).items():                              # the closed forms inside the cases
        assert np.abs(want[g] - S.moments_of_spectrum(lam, K)).max() <= 1e-9 * c.n, (name, g)


def test_odd_and_smallest_moment_counts():
    c = S.build_case("n65")
    Mm = S.operator(c, 1)[0]
    full = S.exact_moments(c, 9)[1]
    for K in (2, 3, 4, 9):
        assert np.abs(S.doubled_moments(Mm, np.eye(c.n), K) - full[:K]).max() <= 1e-9 * c.n


def test_probe_signs_are_the_philox_stream():
    from oracle import ref_rng
    s = S.probe_signs(5, 3, 2, (7 << 32) | 11)
    for i in range(5):
        for r in range(3):
            w = ref_rng.philox4x32_10([i], [r], [2], [S.PHILOX_TAG], 11, 7)[0][0]
            assert s[i, r] == (-1.0 if int(w) & 1 else 1.0)
    big = S.probe_signs(64, 64, 0, 1)
    assert abs(big.mean()) < 0.1 and set(np.unique(big)) == {-1.0, 1.0}


# ---------------------------------------------------------------- metrics.SpectrumStats
def _stats(cases, K=128):
    from snd_vae_amd.metrics import SpectrumStats
    return SpectrumStats(np.concatenate([S.exact_moments(c, K) for c in cases]),
                         np.concatenate([S.info(c) for c in cases]), cases[0].n)


def _resolution_cases():
    out = [G.Case("g25", 1, 25, *M.random_csr(1, 25, 0.16, seed=1, extras=False)),
           G.Case("g64", 1, 64, *M.random_csr(1, 64, 0.1, seed=2, extras=False)),
           G.Case("g257", 1, 257, *M.random_csr(1, 257, 0.03, seed=3, extras=False)),
           S.named_case("K40")[0], S.named_case("empty25")[0]]
    return out


@pytest.mark.parametrize("K", [128, 64])
def test_the_density_resolves_the_spectrum_to_pi_over_k(K):
    """Per graph the EMD in lambda units between density(200) from exact moments and the 200-bin
    eigenvalue histogram is at most pi / K, the Jackson kernel's width (0.012-0.018 at K = 128
    and 0.018 at K = 64 when this was written, against 0.0245 and 0.049)."""
    from snd_vae_amd.metrics import emd
    for c in _resolution_cases():
        st = _stats([c], K)
        d = st.density(200)
        assert d.shape == (1, 200) and (d >= 0).all() and abs(d.sum() - 1.0) <= 1e-12
        dist = emd(d[0], S.eigen_histogram(S.laplacian_spectrum(c, 0), 200), 2.0 / 200)
        print(f"GSPECTRUM resolution {c.name} K {K}: emd {dist:.4f} bar {np.pi / K:.4f}")
        assert dist <= np.pi / K, (c.name, K, dist)


def test_density_rows_are_a_distribution():
    from snd_vae_amd.metrics import SpectrumStats, jackson_weights
    c = S.build_case("b70_mixed")
    st = _stats([c])
    for bins in (200, 64, 1):
        d = st.density(bins)
        assert d.shape == (70, bins) and (d >= 0).all() and np.abs(d.sum(axis=1) - 1.0).max() <= 1e-12
    g = jackson_weights(128)
    assert g[0] == 1.0 and (np.diff(g) < 0).all() and g[-1] > 0
    pm = SpectrumStats(S.probe_moments(c, 128, 40, 3), S.info(c, 40), 25).density(200)    # estimates too
    assert (pm >= 0).all() and np.abs(pm.sum(axis=1) - 1.0).max() <= 1e-12
    with pytest.raises(ValueError):
        st.density(0)


def test_spectrum_stats_concat_eq_and_two_sample_statistics():
    from snd_vae_amd.metrics import SpectrumStats
    c = S.build_case("b70_mixed")
    m, i = S.exact_moments(c, 64), S.info(c)
    whole = SpectrumStats(m, i, 25)
    a, b = SpectrumStats(m[:30], i[:30], 25), SpectrumStats(m[30:], i[30:], 25)
    assert whole.n_graphs == 70 and whole.n_moments == 64 and whole.tensors is None
    assert SpectrumStats.concat([a, b]) == whole and a != b and a != SpectrumStats(m[:30], i[:30], 26)
    with pytest.raises(ValueError):
        SpectrumStats.concat([a, SpectrumStats(m[:30, :32], i[:30], 25)])
    with pytest.raises(ValueError):
        SpectrumStats.concat([])
    assert whole.mmd(whole) == 0.0 and abs(whole.kld(whole)) <= 1e-15
    dense = SpectrumStats(m[4::6][:10], i[4::6][:10], 25)                     # G(25, 0.3)
    sparse = SpectrumStats(m[1::6][:10], i[1::6][:10], 25)                    # G(25, 0.04)
    assert dense.mmd(sparse) > 10 * dense.mmd(SpectrumStats(m[10::6][:10], i[10::6][:10], 25)) > 0
    assert dense.kld(sparse) > 0
    cmp = dense.compare(sparse)
    assert set(cmp) == {"mmd_spectrum", "kld_spectrum", "self", "other"}
    assert cmp["mmd_spectrum"] == dense.mmd(sparse, sigma=1.0) and cmp["self"] == dense.summary()
    s = sparse.summary()
    assert set(s) == {"n_graphs", "n_moments", "mean_isolated_share", "mean_one_way", "mean_second_moment"}
    assert s["mean_isolated_share"] == float(np.mean(sparse.info[:, 1] / 25.0)) > 0
    assert s["mean_one_way"] == float(np.mean(sparse.info[:, 2]))
    # tr(M^2) / N from mu_2 against the dense operator
    for g in (3, 64):
        Mm = S.operator(c, g)[0]
        assert abs(whole.second_moment()[g] - np.trace(Mm @ Mm) / 25.0) <= 1e-12
    with pytest.raises(ValueError):
        dense.mmd(sparse, sigma=0.0)
    with pytest.raises(ValueError):
        dense.compare(3)


# ---------------------------------------------------------------- the C ABI without a device
def test_header_library_and_integration_agree_on_abi_28(lib_built):
    from snd_vae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snd_vae.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    so = ctypes.CDLL(lib_built)
    for name in ("snd_graph_spectrum", "snd_graph_spectrum_workspace"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(so, name) and name in doc, name
    abi = int(re.search(r"#define\s+SND_ABI_VERSION\s+(\d+)", hdr).group(1))
    stub = int(re.search(r"SND_ABI_VERSION\s*=\s*(\d+)", doc).group(1))
    assert abi == _lib.ABI_VERSION == so.snd_abi_version() == stub and abi >= 28
    assert re.search(r"SND_SPECTRUM_FORCE_GLOBAL\s*=\s*1\b", hdr)


def test_no_spill_or_scratch_in_the_new_kernels(lib_built):
    from snd_vae_amd.build import build_info, kernel_resources
    names = ("gs_prep_kernel", "gs_weight_kernel", "gs_init_kernel", "gs_step_kernel", "gs_reduce_kernel",
             "gs_lds_kernel", "gs_final_kernel")
    res = {k: v for k, v in kernel_resources().items() if any(s in k for s in names)}
    assert len(res) == 7, sorted(res)
    for k, v in res.items():
        assert v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0 and v.get("scratch", 0) == 0, (k, v)
    assert not any("gs_" in k for k in build_info().get("spills", {}))


class HostArgs:
    """A well-formed argument list over host memory.  No rule below reaches a launch, so nothing
    dereferences these pointers."""

    def __init__(self, _lib, B=2, n=10, cap=40, K=16):
        self.L = _lib.lib()
        self._lib = _lib
        self.need = self.L.snd_graph_spectrum_workspace(B, n, cap)
        self.bufs = {"rowptr": np.zeros(B * n + 1, np.int32), "colidx": np.zeros(cap, np.int32),
                     "moments": np.full(B * K, 7.0, np.float64), "info": np.full(B * 4, 7, np.int64),
                     "ws": np.full(self.need // 8 + 1, 7, np.int64)}
        self.args = dict(rowptr=self.bufs["rowptr"].ctypes.data, colidx=self.bufs["colidx"].ctypes.data,
                         nnz_cap=cap, n_graphs=B, n=n, n_moments=K, n_probes=0, seed=0, flags=0,
                         moments=self.bufs["moments"].ctypes.data, info=self.bufs["info"].ctypes.data,
                         ws=self.bufs["ws"].ctypes.data, ws_bytes=self.need)

    def call(self, **kw):
        a = dict(self.args)
        a.update(kw)
        rc = self.L.snd_graph_spectrum(*a.values(), None)
        msg = self._lib.last_error() if rc else ""
        for k in ("moments", "info", "ws"):
            assert (self.bufs[k] == 7).all(), (kw, k)
        return rc, msg


def test_the_op_rejects_bad_arguments_before_any_launch(lib_built):
    from snd_vae_amd import _lib
    h = HostArgs(_lib)
    # 32 B per graph, 8 B per entry, two state buffers of 256 B per row, 16 B per 8-row tile, 4 B per row
    assert h.need == 64 + 320 + 2 * 20 * 256 + 2 * 2 * 16 + 80 and h.need % 16 == 0
    bad = [dict(n_graphs=0), dict(n_graphs=-1), dict(n=0), dict(n=S.MAX_N + 1), dict(n=S.MAX_N, n_graphs=1 << 17),
           dict(nnz_cap=-1), dict(n_moments=1), dict(n_moments=S.MAX_MOMENTS + 1), dict(n_probes=-1), dict(flags=2),
           dict(flags=-1), dict(rowptr=None), dict(moments=None), dict(info=None), dict(colidx=None),
           dict(ws_bytes=h.need - 1), dict(ws=None), dict(ws=h.args["ws"] + 4)]
    for kw in bad:
        rc, msg = h.call(**kw)
        assert rc == -1, (kw, rc)
        assert msg.startswith("snd_graph_spectrum:"), (kw, msg)
    assert "workspace" in h.call(ws_bytes=h.need - 1)[1] and "n_moments" in h.call(n_moments=1)[1]
    assert "colidx" in h.call(colidx=None)[1] and "n=" in h.call(n=0)[1] and "flags" in h.call(flags=4)[1]
    assert "n_probes" in h.call(n_probes=-3)[1]
    L = h.L
    assert L.snd_graph_spectrum_workspace(0, 10, 40) == 0 and L.snd_graph_spectrum_workspace(2, S.MAX_N + 1, 40) == 0
    assert L.snd_graph_spectrum_workspace(2, 10, -1) == 0 and L.snd_graph_spectrum_workspace(1 << 17, S.MAX_N, 0) == 0
    for B, n, cap in ((1, 1, 0), (3, 65, 1001), (7, 16384, 5)):
        assert L.snd_graph_spectrum_workspace(B, n, cap) % 16 == 0


def test_layers_checks_without_a_device():
    import torch
    from snd_vae_amd import layers
    rp, ci = torch.zeros(21, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    assert layers.SPECTRUM_MAX_N == S.MAX_N and layers.SPECTRUM_MAX_MOMENTS == S.MAX_MOMENTS
    assert layers.SPECTRUM_EXACT_MAX_N == 256 and layers.SPECTRUM_PROBES == 32
    for kw, match in ((dict(n_graphs=0), "n_graphs"), (dict(n=S.MAX_N + 1), "16384"), (dict(n_moments=1), "n_moments"),
                      (dict(n_moments=513), "n_moments"), (dict(n_probes=-1), "n_probes"), (dict(seed=-1), "seed"),
                      (dict(), "device tensor")):
        a = dict(rowptr=rp, colidx=ci, n_graphs=2, n=10)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            layers.graph_spectrum(**a)
