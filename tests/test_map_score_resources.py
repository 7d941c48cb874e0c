"""fe::map_score_poses keeps the keys, slots and rows of every gather chain of a step in registers (9 cells of 2 poses at reach 1,
8 poses at reach 0): it must spill nothing to scratch memory.  hipcc cross-compiles for gfx950 without a GPU; this test reads its
kernel-resource-usage remarks, as tests/test_map_align_resources.py does for the registration's kernels."""
import os
import re
import subprocess

from mad_icp_amd import _build


def test_score_kernels_use_no_scratch(tmp_path):
    src = os.path.join(_build.CSRC, "hip", "madicp_capi.hip")
    cmd = [_build.HIPCC] + [f for f in _build.HIP_FLAGS if f != "-shared"] + ["-c", "-I" + _build.INC, "-I" + os.path.join(_build.CSRC, "hip"),
                                                                               src, "-o", str(tmp_path / "capi.o"),
                                                                               "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    seen = {}
    for block in out.split("Function Name: ")[1:]:
        name = block.split()[0]
        reach = re.search(r"map_score_posesILi([01])E", name)
        if reach:
            seen[int(reach.group(1))] = dict(vgprs=int(re.search(r"VGPRs: (\d+)", block).group(1)),
                                             scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)),
                                             vgpr_spill=int(re.search(r"VGPRs Spill: (\d+)", block).group(1)),
                                             lds=int(re.search(r"LDS Size \[bytes/block\]: (\d+)", block).group(1)))
    print(seen)
    assert set(seen) == {0, 1}, seen
    for reach in (0, 1):
        assert seen[reach]["scratch"] == 0 and seen[reach]["vgpr_spill"] == 0, seen
        assert seen[reach]["lds"] == 64 * 96 + 64 * 3 * 8, seen  # the chunk's poses and its 64-bit counters
