"""fe::rows_claim, fe::rows_append and fe::rows_combine (the merge of saved rows, csrc/hip/frontend.hip.h) are streaming kernels with
a handful of live values per lane — rows_combine holds one entry's ten moment words at most: they must use no scratch memory and
spill nothing.  hipcc cross-compiles for gfx950 without a GPU; this test reads its kernel-resource-usage remarks, as
tests/test_map_score_resources.py does for the scoring kernels."""
import os
import re
import subprocess

from mad_icp_amd import _build

KERNELS = ("rows_claim", "rows_append", "rows_combine")


def test_merge_kernels_use_no_scratch(tmp_path):
    src = os.path.join(_build.CSRC, "hip", "madicp_capi.hip")
    cmd = [_build.HIPCC] + [f for f in _build.HIP_FLAGS if f != "-shared"] + ["-c", "-I" + _build.INC, "-I" + os.path.join(_build.CSRC, "hip"),
                                                                               src, "-o", str(tmp_path / "capi.o"),
                                                                               "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    seen = {}
    for block in out.split("Function Name: ")[1:]:
        name = block.split()[0]
        for kernel in KERNELS:
            if re.search(r"2fe\d+%sE" % kernel, name):  # (madicp::fe::<kernel>, mangled)
                seen[kernel] = dict(vgprs=int(re.search(r"VGPRs: (\d+)", block).group(1)),
                                    scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)),
                                    vgpr_spill=int(re.search(r"VGPRs Spill: (\d+)", block).group(1)),
                                    sgpr_spill=int(re.search(r"SGPRs Spill: (\d+)", block).group(1)),
                                    lds=int(re.search(r"LDS Size \[bytes/block\]: (\d+)", block).group(1)))
    print(seen)
    assert set(seen) == set(KERNELS), seen
    for kernel in KERNELS:
        assert seen[kernel]["scratch"] == 0 and seen[kernel]["vgpr_spill"] == 0 and seen[kernel]["sgpr_spill"] == 0 and seen[kernel]["lds"] == 0, seen
