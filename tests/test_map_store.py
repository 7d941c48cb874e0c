"""HostMapStore (mad_icp_amd/csrc/host/map_store.h), the host half of the one map store behind Pipeline, is VoxelMap and nothing
else: tests/cpp/map_store_check.cpp — a stand-alone program with its own main that links csrc/host/voxel_map.cpp and the header
alone, nothing of HIP — drives one scripted sequence (three folds with duplicates, points on cell faces and an empty cloud; a clearing
and a prune with a watermark inside the map, tracking on; a removal refused because the log is full; every column of the window
download at first_row 0, in the middle and at size(); a buffer one row short; takeRemoved; a query at reach 0 and at reach 1; clear)
through a HostMapStore and through a VoxelMap called directly, for all eight combinations of attribute, evidence and moments, and
holds every return code and every output byte equal.  Once plain, once under AddressSanitizer + UndefinedBehaviorSanitizer with every
output buffer sized exactly (skipped where the sanitizer runtime does not link).  Nothing is loaded into Python.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_and_run(tmp_path, extra):
    cxx = os.environ.get("CXX", "g++")
    exe = tmp_path / "map_store_check"
    csrc = os.path.join(ROOT, "mad_icp_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + extra + [
        "-I" + os.path.join(csrc, "host"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "map_store_check.cpp"), os.path.join(csrc, "host", "voxel_map.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "8 sets equal" in run.stdout


def test_host_map_store_is_the_voxel_map(tmp_path):
    build_and_run(tmp_path, [])


def test_host_map_store_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    trial = tmp_path / "trial.cpp"
    trial.write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx] + SAN + [str(trial), "-o", str(tmp_path / "trial")], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime does not link here: " + probe.stderr[-300:])
    build_and_run(tmp_path, SAN)
