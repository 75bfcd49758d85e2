"""``snd_latent_reg``'s total-correlation gradient where it is hard: a small batch.

The gradient weight of the TC term is softmax_i S[j, i] - softmax_i lqp[j, i, l] with
S = sum_l lqp.  Right after initialisation the encoder's mu and logstd are close to zero, so the
rows of S (about -L in magnitude) differ by little between the samples i, both softmaxes are
close to 1 / B, and their difference, the gradient, is small against them.  An fp32 running sum
over L = 100 terms, S stored at its full magnitude (an ulp of 3e-5 in an exponent) and fp32
softmaxes then leave 1e-4 of the gradient's max-abs as noise, which the encoder's bias and BN
sums amplify further (tests/test_gpu_disent_train_engine.py: the first beta-TCVAE step at
B = 2).  The block therefore runs in double on the fp32 operands and stores S relative to its
row max.

Bar: dmu / dlogstd within 1e-5 of their max-abs of the float64 oracle
(``oracle.ref_disent.group_reg_torch`` on the sample exactly as the kernel sees it), the bar
tests/test_gpu_disent.py::test_latent_reg sets for this op; the values to 1e-5 relative.
Cases: the model's state at initialisation (B = 2, L = 100, |mu|, |logstd| ~ 0.02), the same
with the two samples swapped (the row max of S is then off the diagonal), a lone sample (every
weight is zero), three samples, and means far apart (rows of S hundreds apart: the softmax of S
underflows to one sample).  The figures are printed as "LATENT_TC <case> dmu <rel> dlogstd <rel>".
"""
import numpy as np
import pytest
import torch

from oracle import ref_disent as RD

pytestmark = pytest.mark.gpu

# (id, B, L, scale of mu and logstd, swap the samples)
CASES = (("init_b2", 2, 100, 0.02, False), ("init_b2_swapped", 2, 100, 0.02, True), ("lone", 1, 7, 0.5, False),
         ("b3", 3, 5, 0.5, False), ("init_b10", 10, 100, 0.02, False), ("far_apart", 4, 100, 3.0, False))
KW = {"w_kl": 1.0, "w_tc": 10.0}                 # beta-TCVAE (optimizer.py:175-183)


@pytest.fixture(scope="module", autouse=True)
def _gpu(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


def rel(got, ref):
    scale = np.abs(ref).max()
    err = np.abs(np.asarray(got, np.float64) - ref).max()
    return 0.0 if err == 0 else err / scale


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_total_correlation_gradient_at_a_small_batch(case):
    from snd_vae_amd import disent
    name, B, L, scale, swap = case
    rng = np.random.default_rng([B, L, int(100 * scale), int(swap)])
    mu = (scale * rng.standard_normal((B, L))).astype(np.float32)
    s = (min(scale, 0.5) * rng.standard_normal((B, L))).astype(np.float32)
    z = (mu + rng.standard_normal((B, L)).astype(np.float32) * np.exp(s)).astype(np.float32)
    if swap:
        z = np.ascontiguousarray(z[::-1])
    cu = lambda a: torch.from_numpy(a).cuda()
    v, dmu, ds = disent.latent_reg(cu(mu), cu(s), cu(z), **KW)
    # the oracle with the sample exactly as the kernel sees it: eps' = (z - mu) e^-s
    eps64 = (z.astype(np.float64) - mu) * np.exp(-s.astype(np.float64))
    val, rdmu, rds = RD.group_reg_torch(mu, s, eps64, **KW)
    ref = RD.group_reg(mu, s, z, **KW)
    e_mu, e_s = rel(dmu.cpu().numpy(), rdmu), rel(ds.cpu().numpy(), rds)
    print(f"LATENT_TC {name} dmu {e_mu:.3e} dlogstd {e_s:.3e} tc {v['tc']!r} ref {ref['tc']!r}")
    assert v["term"] == pytest.approx(val, rel=1e-5, abs=1e-7)
    assert v["tc"] == pytest.approx(ref["tc"], rel=1e-5, abs=1e-7)
    assert e_mu < 1e-5 and e_s < 1e-5, (name, e_mu, e_s)
