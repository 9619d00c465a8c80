"""The split-arithmetic head kernels keep their k-loop look-ahead only if they compile without scratch: a reload from scratch
is a vector-memory operation, its wait is vmcnt(0), and that drains every load s6_main_loop (csrc/lin_f32.hip) has in
flight.  This reads hipcc's own per-kernel resource report (-Rpass-analysis=kernel-resource-usage, kept by build.py next
to the object) -- no assembly text is searched."""
import os
import re
import tempfile

from artspeech_amd import build as B

# kernel (substring of the mangled name) -> waves per SIMD it must reach:
#   lin_s6_kernel<EPI>: 8-wave workgroups, two per CU = 4 waves per SIMD
#   lin_out_s6_kernel: 4-wave workgroups; LOUT_WPS = 3 of them per CU are what the kernel is built for (its tile list keeps
#     4 x 256 slots on measurement, see as_lin_out_try: a list of 3 x 256 was no faster than the spilling kernel)
#   lin_s6_plain_kernel<4, 2>: the heads' dx1 (<= 512 workgroups of 4 waves on 256 CUs: two per CU at most)
KERNELS = {
    "13lin_s6_kernelILi1EE": 4,
    "13lin_s6_kernelILi2EE": 4,
    "17lin_out_s6_kernelE": 3,
    "19lin_s6_plain_kernelILi4ELi2EE": 2,
}


def _report():
    path = B.resources_path("lin_f32.hip")
    src = os.path.join(B.CSRC, "lin_f32.hip")
    headers = [os.path.join(B.CSRC, f) for f in os.listdir(B.CSRC) if f.endswith(".h")]
    if B._newer(src, path, headers):   # not built yet (or stale): this one device compile, its object thrown away
        os.makedirs(B.OBJ, exist_ok=True)
        with tempfile.TemporaryDirectory() as tmp:
            B.compile_one("lin_f32.hip", B.SOURCES["lin_f32.hip"], os.path.join(tmp, "lin_f32.o"),
                          os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), verbose=False)
    kernels, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+([A-Za-z][^:\[]*?)(?: \[[^\]]*\])?: (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = kernels.setdefault(val, {})
        elif cur is not None and val.lstrip("-").isdigit():
            cur[key] = int(val)
    return kernels


def test_head_kernels_compile_without_scratch_at_their_occupancy():
    rep = _report()
    for sub, waves in KERNELS.items():
        names = [n for n in rep if sub in n]
        assert len(names) == 1, (sub, sorted(rep))
        r = rep[names[0]]
        print(names[0], r)
        assert r["ScratchSize"] == 0, (names[0], r)
        assert r["VGPRs Spill"] == 0, (names[0], r)
        assert r["Occupancy"] >= waves, (names[0], r)
