"""Where a device voxel map's columns lie is decided on the host alone (mad_icp_amd/csrc/common/map_layout.h): for all eight
column combinations and capacities 1..70, 4095, 4096, 4097, 2^18 and 2^24 the offsets are those of the allocation code the header
replaced, the columns are ascending, disjoint and aligned, the block is the documented bytes per row of capacity, and the scratch
of a prune and of a clearing stays within the 24 cap bytes of the fresh block's table region for every row count
(tests/cpp/map_layout_check.cpp).  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_map_layout_matches_the_allocation_it_replaced(tmp_path):
    exe = str(tmp_path / "map_layout_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-I" + os.path.join(ROOT, "mad_icp_amd", "csrc", "common"),
                           os.path.join(ROOT, "tests", "cpp", "map_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "map layout ok" in out.stdout
