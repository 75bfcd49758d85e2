"""``snd_latent_mi`` (ABI 25) at the C ABI on guarded operands (tests/abi_ops.py) against the
NumPy restatement (tests/latent_mi_ref.py): the joint counts exactly, the ranges by value, mi,
hz and hf to 1e-11 absolute, every guard band intact, every output fully written, two runs and
a captured-graph replay bitwise equal, and mi unchanged without the optional outputs.

The 1e-11: the weights c / rows of a block sum to 1, so the terms' magnitudes sum to at most
log(rows) <= 17 wherever rows fit an int; at most 1024 terms are added in double and the
device log is within a few ulp, so the error is about 1024 * 1.1e-16 * 17 = 2e-12; the bar is
five times that.

Shapes: rows 1, 2, 63, 64, 65, 257 (two row slices of the count kernel, the second of one
row), 1000 (four slices, a tail of 232; eight chunks of 128 rows with tails); n_lat 1, 3, 64,
65 (the range kernel's second column tile holds one latent and the factors), 400 (the
reference's; at 20 x 20 bins and 3 factors a tile is 8 columns), 13 at 32 x 32 bins and 7
factors (a tile of one column), and 7 factors at 32 x 32 bins with 13 latents; bins 1, 2, 20,
32 with nbz != nbf.
"""
import numpy as np
import pytest
import torch

import latent_mi_ref as MR
from abi_ops import check_guards, guarded
from types import SimpleNamespace as NS

pytestmark = pytest.mark.gpu
TOL = 1e-11


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def lib():
    from snd_vae_amd import _lib
    return _lib.lib(), _lib.stream_ptr(), _lib


class Case:
    """Guarded operands and outputs of one call: z with ldz = L + 3, f with ldf = K + 1, NaN
    padding, every pointer ``offset`` elements past a 16-byte boundary."""

    def __init__(self, z, f, nbz, nbf, offset=1, optional=True):
        self.z, self.f, self.nbz, self.nbf = z, f, nbz, nbf
        rows, L = z.shape
        K = f.shape[1]
        self.rows, self.L, self.K = rows, L, K
        b = {"z": guarded(rows, L, L + 3, "f32", offset, z, "z"), "f": guarded(rows, K, K + 1, "f32", offset, f, "f"),
             "mi": guarded(L, K, K, "f64", 0, None, "mi"), "hz": guarded(1, L, L, "f64", 0, None, "hz"),
             "hf": guarded(1, K, K, "f64", 0, None, "hf")}
        if optional:
            b["range"] = guarded(L + K, 2, 2, "f32", offset, None, "range")
            b["joint"] = guarded(L * K, nbz * nbf, nbz * nbf, "i32", offset, None, "joint")
        L_, _, _ = lib()
        self.need = L_.snd_latent_mi_workspace(rows, L, K, nbz, nbf)
        assert self.need > 0
        # the workspace 4 bytes off 16-byte alignment as well, with a guard of its own behind it
        self.ws = torch.full((self.need + 4 + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        self.c = NS(bufs=b)
        self.t = {k: torch.from_numpy(g.arr.copy()).cuda() for k, g in b.items()}

    def ptr(self, k):
        if k not in self.t:
            return None
        g = self.c.bufs[k]
        return self.t[k].data_ptr() + g.off * self.t[k].element_size()

    def call(self):
        L_, S, _lib = lib()
        _lib.check(L_.snd_latent_mi(self.ptr("z"), self.L + 3, self.ptr("f"), self.K + 1, self.rows, self.L, self.K,
                                    self.nbz, self.nbf, self.ptr("mi"), self.ptr("hz"), self.ptr("hf"),
                                    self.ptr("range"), self.ptr("joint"), self.ws.data_ptr() + 4, self.need, S),
                   "snd_latent_mi")

    def read(self):
        """Synchronise, check every guard and the inputs, return the logical outputs."""
        torch.cuda.synchronize()
        after = {k: t.cpu().numpy() for k, t in self.t.items()}
        check_guards(self.c, after)
        b = self.c.bufs
        assert np.array_equal(b["z"].block(after["z"]), self.z, equal_nan=True)
        assert np.array_equal(b["f"].block(after["f"]), self.f, equal_nan=True)
        assert np.all(self.ws[self.need + 4:].cpu().numpy() == 0xA5), "a byte past the workspace was written"
        assert np.all(self.ws[:4].cpu().numpy() == 0xA5), "a byte before the workspace was written"
        out = {k: b[k].block(after[k]).copy() for k in b if k not in ("z", "f")}
        out["hz"], out["hf"] = out["hz"].reshape(-1), out["hf"].reshape(-1)
        if "joint" in out:
            out["joint"] = out["joint"].reshape(self.L, self.K, self.nbz, self.nbf)
        return out


def check(z, f, nbz, nbf, offset=1):
    """One call against the restatement; returns (case, outputs, reference)."""
    c = Case(z, f, nbz, nbf, offset)
    c.call()
    got = c.read()
    ref = MR.latent_mi_ref(z, f, nbz, nbf)
    L, K = c.L, c.K
    assert np.array_equal(got["joint"], ref["joint"]), "joint counts differ"
    assert np.all(got["joint"].sum((2, 3)) == c.rows)
    assert np.array_equal(got["range"], ref["range"])                     # by value: -0 == +0
    for k in ("mi", "hz", "hf"):
        assert np.all(np.isfinite(got[k])), (k, "an element was not written")
        err = float(np.max(np.abs(got[k] - ref[k])))
        print(f"{k}: max abs err {err:.3e} (rows {c.rows}, L {L}, K {K}, bins {nbz} x {nbf})")
        assert err <= TOL, (k, err)
    return c, got, ref


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 257, 1000])
def test_rows(rows):
    check(*MR.random_case(rows, 5, 3, seed=rows), 20, 20)


@pytest.mark.parametrize("L", [1, 3, 64, 65, 400])
def test_latent_columns_with_a_tile_tail(L):
    check(*MR.random_case(257, L, 3, seed=L), 20, 20)                    # 400, 65, 3, 1: no multiple of 8


@pytest.mark.parametrize("K", [1, 3, 7])
def test_factor_columns(K):
    check(*MR.random_case(129, 13, K, seed=K), 20, 5)


@pytest.mark.parametrize("nbz,nbf", [(1, 1), (2, 2), (20, 20), (32, 32), (20, 5), (2, 32), (32, 1)])
def test_bins(nbz, nbf):
    check(*MR.random_case(300, 13, 7, seed=nbz * 33 + nbf, levels=32), nbz, nbf)


def test_more_factors_than_one_tile_holds():
    # 32 x 32 bins: 12 factors' counters fill the 48 KiB, so 13 factors are two factor tiles (12 + 1)
    check(*MR.random_case(130, 3, 13, seed=30, levels=32), 32, 32)


def test_more_rows_than_the_range_kernel_has_slices():
    # past 1024 x 256 rows a range slice grows beyond 256 rows (293 here, the last one shorter)
    check(*MR.random_case(300001, 2, 1, seed=31), 20, 5)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_any_pointer_alignment(offset):
    check(*MR.random_case(65, 7, 3, seed=40 + offset), 20, 20, offset=offset)


def test_a_constant_column():
    z, f = MR.random_case(100, 4, 2, seed=50)
    z[:, 2] = 1.5
    f[:, 1] = -2.0
    _, got, _ = check(z, f, 20, 5)
    assert got["hz"][2] == 0.0 and got["hf"][1] == 0.0
    assert np.all(got["mi"][2] == 0.0) and np.all(got["mi"][:, 1] == 0.0)
    assert np.all(got["joint"][2, :, 1:] == 0) and np.all(got["joint"][:, 1, :, 1:] == 0)


def test_integer_valued_data_on_the_bin_edges():
    nb = 20
    rng = np.random.default_rng(51)
    z = rng.integers(0, nb + 1, size=(500, 3)).astype(np.float32)       # lo = 0, hi = nb: every value is an edge
    z[0], z[1] = 0.0, float(nb)
    f = rng.integers(0, 5, size=(500, 2)).astype(np.float32)             # 5 levels in 5 bins
    f[0], f[1] = 0.0, 4.0
    _, got, _ = check(z, f, nb, 5)
    for l in range(3):
        want = np.bincount(np.minimum(z[:, l].astype(np.int64), nb - 1), minlength=nb)
        assert np.array_equal(got["joint"][l, 0].sum(axis=1), want)
    for k in range(2):
        assert np.array_equal(got["joint"][0, k].sum(axis=0), np.bincount(f[:, k].astype(np.int64), minlength=5))


def test_magnitudes_of_1e30_beside_1e_minus_30():
    z, f = MR.random_case(200, 4, 2, seed=52)
    z[:, 0] = np.where(np.arange(200) % 2, 1e30, 1e-30).astype(np.float32) * z[:, 0]
    z[:, 1] *= np.float32(1e-30)
    z[:, 2] *= np.float32(1e30)
    f[:, 1] = np.where(f[:, 1] > 2, 1e30, 1e-30).astype(np.float32)
    check(z, f, 20, 20)


def test_two_runs_and_a_graph_replay_are_bitwise_equal():
    z, f = MR.random_case(1000, 65, 3, seed=53)
    c, first, _ = check(z, f, 20, 20)
    c.call()
    second = c.read()
    for k in first:
        assert np.array_equal(first[k].view(np.uint8), second[k].view(np.uint8)), k
    r = Case(z, f, 20, 20)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r.call()                                                         # module load outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for k in ("mi", "hz", "hf", "range", "joint"):                       # back to the pattern: the replay must write
        r.t[k].copy_(torch.from_numpy(r.c.bufs[k].arr))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r.call()
    g.replay()
    replayed = r.read()
    for k in first:
        assert np.array_equal(first[k].view(np.uint8), replayed[k].view(np.uint8)), k


def test_without_the_optional_outputs_mi_is_unchanged():
    z, f = MR.random_case(257, 13, 3, seed=54)
    _, full, _ = check(z, f, 20, 5)
    c = Case(z, f, 20, 5, optional=False)
    c.call()
    got = c.read()
    for k in ("mi", "hz", "hf"):
        assert np.array_equal(full[k].view(np.uint8), got[k].view(np.uint8)), k


def test_nan_inputs_stay_inside_the_outputs():
    z, f = MR.random_case(130, 5, 2, seed=55)
    z[3, 1] = z[77, 4] = f[5, 0] = np.nan
    z[:, 2] = np.nan                                                     # a column without a range
    z[9, 0], z[10, 0] = np.inf, -np.inf
    c = Case(z, f, 20, 5)
    c.call()
    got = c.read()                                                       # the guards are checked in read()
    assert np.all(got["joint"] >= 0) and np.all(got["joint"].sum((2, 3)) == 130)


def test_layers_latent_mi_and_the_metric_object():
    from snd_vae_amd import layers
    from snd_vae_amd.metrics import LatentMI
    z, f = MR.random_case(300, 12, 3, seed=56)
    ref = MR.latent_mi_ref(z, f, 20, 5)
    big = torch.full((300, 16), float("nan"), device="cuda")
    big[:, 2:14] = torch.from_numpy(z).cuda()                            # a column block: ldz = 16
    fd = torch.from_numpy(f).cuda()
    mi, hz, hf, joint, rng = layers.latent_mi(big[:, 2:14], fd, n_bins=20, factor_bins=5, want_joint=True)
    assert mi.dtype == torch.float64 and tuple(mi.shape) == (12, 3) and joint.dtype == torch.int32
    assert np.array_equal(joint.cpu().numpy(), ref["joint"]) and np.array_equal(rng.cpu().numpy(), ref["range"])
    groups = {"s": slice(0, 4), "g": slice(4, 8), "sg": slice(8, 12)}
    m = LatentMI(mi, hz, hf, groups)
    assert m.tensors is not None and m.n_latents == 12 and m.n_factors == 3
    want = LatentMI(ref["mi"], ref["hz"], ref["hf"], groups)
    assert np.max(np.abs(m.mi - want.mi)) <= TOL and np.max(np.abs(m.hf - want.hf)) <= TOL
    assert abs(m.mig() - want.mig()) <= 1e-9 and m.best_latent() == want.best_latent()
    mi.zero_()
    assert m.mi.any()                                                    # the host copy, until ...
    m.invalidate()
    assert not m.mi.any()
    same = layers.latent_mi(big[:, 2:14], fd, n_bins=20, factor_bins=5)
    assert len(same) == 3 and np.max(np.abs(same[0].cpu().numpy() - ref["mi"])) <= TOL
    default = layers.latent_mi(big[:, 2:14], fd)                         # factor_bins defaults to n_bins
    assert np.max(np.abs(default[2].cpu().numpy() - MR.latent_mi_ref(z, f, 20, 20)["hf"])) <= TOL
    for bad in (dict(n_bins=0), dict(n_bins=33), dict(factor_bins=0), dict(n_bins=2.5)):
        with pytest.raises(ValueError):
            layers.latent_mi(big[:, 2:14], fd, **bad)
    with pytest.raises(ValueError):
        layers.latent_mi(big[:, 2:14], fd[:299])
    with pytest.raises(ValueError):
        layers.latent_mi(big[:, 2:14].double(), fd)
    with pytest.raises(ValueError):
        layers.latent_mi(big.t()[2:14].t()[:, ::2], fd)                  # a column stride of 2
