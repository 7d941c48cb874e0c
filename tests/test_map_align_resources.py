"""fe::map_align_terms keeps one point's 28 terms in registers from the linearisation to the end of the wavefront butterfly, beside
the query's state: it must spill nothing (a spilled term is a scratch round trip per butterfly step).  hipcc cross-compiles for
gfx950 without a GPU; this test reads its kernel-resource-usage remarks, as tests/test_kernel_resources.py does for the round kernel."""
import os
import re
import subprocess

from mad_icp_amd import _build


def test_align_terms_kernel_spills_nothing(tmp_path):
    src = os.path.join(_build.CSRC, "hip", "madicp_capi.hip")
    cmd = [_build.HIPCC] + [f for f in _build.HIP_FLAGS if f != "-shared"] + ["-c", "-I" + _build.INC, "-I" + os.path.join(_build.CSRC, "hip"),
                                                                               src, "-o", str(tmp_path / "capi.o"),
                                                                               "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    seen = {}
    for block in out.split("Function Name: ")[1:]:
        name = block.split()[0]
        for kernel in ("map_align_terms", "map_align_join", "map_align_step"):
            if kernel in name:
                seen[kernel] = (int(re.search(r"VGPRs: (\d+)", block).group(1)),
                                int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)),
                                int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", block).group(1)))
    print(seen)
    assert set(seen) == {"map_align_terms", "map_align_join", "map_align_step"}, seen
    assert seen["map_align_terms"][1] == 0, seen
    assert seen["map_align_join"][1] == 0, seen
