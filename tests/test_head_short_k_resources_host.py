"""The short-reduction head kernels (csrc/lin_f32.hip) are built for two 8-wave workgroups per CU and keep their B look-ahead
only without scratch (a reload from scratch waits with vmcnt(0) and drains it, as in s6_main_loop).  Like
test_head_kernel_resources_host.py this reads hipcc's per-kernel resource report only -- no assembly text is searched."""
from test_head_kernel_resources_host import _report

# kernel (substring of the mangled name) -> waves per SIMD it must reach: 8-wave workgroups, two per CU
KERNELS = {
    "24lin_s6_lnf_shared_kernelE": 4,
    "23lin_s6_lnb_short_kernelE": 4,
}


def test_short_k_kernels_compile_without_scratch_at_two_workgroups_per_cu():
    rep = _report()
    for sub, waves in KERNELS.items():
        names = [n for n in rep if sub in n]
        assert len(names) == 1, (sub, sorted(rep))
        r = rep[names[0]]
        print(names[0], r)
        assert r["ScratchSize"] == 0, (names[0], r)
        assert r["VGPRs Spill"] == 0, (names[0], r)
        assert r["Occupancy"] >= waves, (names[0], r)
