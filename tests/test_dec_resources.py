"""The fused decoder kernels' registers from the compiler's resource remarks (no GPU).

dec_fwd_kernel and dec_bwd_kernel run one 1024-thread workgroup per CU: 16 waves, four per
SIMD, which holds only within 128 VGPRs.  They sit at 114 - 122, and a spill in dec_bwd_kernel
once cost 26 us per C2 step: every instantiation must stay without spill or scratch, within
128 VGPRs and at occupancy 4 or more."""
from snd_vae_amd.build import kernel_resources


def test_dec_kernels_fit_four_waves_per_simd(lib_built):
    res = {k: v for k, v in kernel_resources().items() if "dec_fwd_kernel" in k or "dec_bwd_kernel" in k}
    # the fused chains: 128-, 64- and 32-row tiles and the streamed 64-row ones, forward and backward
    chains = [k for k in res if "DecChainFwdArgs" in k or "DecChainBwdArgs" in k]
    assert len(chains) >= 8, sorted(res)
    for k, v in res.items():
        assert v["vgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["vgprs"] + v.get("agprs", 0) <= 128, (k, v)
        assert v["occupancy"] >= 4, (k, v)
