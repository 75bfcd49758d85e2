"""The d = 64 zz^T kernel's registers and LDS from the compiler's resource remarks (no GPU).

zzt_dense_bf16_v9 runs two 512-thread workgroups per CU at 4 waves per SIMD: that holds
only while every instantiation stays within 128 VGPRs without spilling, and while the
shipped one's static LDS leaves room for two workgroups in the CU's 160 KB."""
from snd_vae_amd.build import kernel_resources

SHIPPED = "zzt_dense_bf16_v9ILb0EE"   # <MEAS = false>
MEASURE = "zzt_dense_bf16_v9ILb1EE"   # <MEAS = true>


def _v9():
    return {k: v for k, v in kernel_resources().items() if "zzt_dense_bf16_v9" in k}


def test_v9_instantiations_fit_four_waves_per_simd(lib_built):
    res = _v9()
    # exactly the shipped kernel and its measurement build: no A/B instantiation beside them
    assert len(res) == 2 and sum(SHIPPED in k for k in res) == 1 and sum(MEASURE in k for k in res) == 1, sorted(res)
    for k, v in res.items():
        assert v["vgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["vgprs"] + v.get("agprs", 0) <= 128, (k, v)
        assert v["occupancy"] >= 4, (k, v)


def test_shipped_v9_lds_lets_two_workgroups_share_a_cu(lib_built):
    (v,) = [v for k, v in _v9().items() if SHIPPED in k]
    assert v["lds"] <= 80 * 1024, v
