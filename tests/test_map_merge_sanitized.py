"""The host voxel map's merge of saved rows under AddressSanitizer + UndefinedBehaviorSanitizer: tests/cpp/map_merge_check.cpp — a
stand-alone program with its own main that links csrc/host/voxel_map.cpp directly — is compiled here and run.  Every column of a
batch lives in a buffer of exactly n entries, so a read past any of them is reported; after every merge every column of the map is
held to a restatement kept in the program.  Nothing is loaded into Python; skipped where the sanitizer runtime does not link."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_map_merge_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    trial = tmp_path / "trial.cpp"
    trial.write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx] + SAN + [str(trial), "-o", str(tmp_path / "trial")], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime does not link here: " + probe.stderr[-300:])
    exe = tmp_path / "map_merge_check"
    csrc = os.path.join(ROOT, "mad_icp_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra"] + SAN + [
        "-I" + os.path.join(csrc, "host"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "map_merge_check.cpp"), os.path.join(csrc, "host", "voxel_map.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "48 sets clean" in run.stdout
