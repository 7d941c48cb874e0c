"""The voxel map's surfel and its gate under AddressSanitizer + UndefinedBehaviorSanitizer: tests/cpp/map_surfel_check.cpp — a
stand-alone program with its own main that includes csrc/common/voxel_moments.h and map_align.h directly — is compiled here and
run over the degenerate populations of tests/surfel_exact_ref.py's catalogue, rebuilt there from integers.  The ten words and the
three outputs live in heap blocks of exactly their size, so a read or write past any of them is reported; points and lines are
never inliers, exact planes always.  Nothing is loaded into Python; skipped where the sanitizer runtime does not link."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_map_surfel_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    trial = tmp_path / "trial.cpp"
    trial.write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx] + SAN + [str(trial), "-o", str(tmp_path / "trial")], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime does not link here: " + probe.stderr[-300:])
    exe = tmp_path / "map_surfel_check"
    csrc = os.path.join(ROOT, "mad_icp_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra"] + SAN + [
        "-I" + os.path.join(csrc, "host"), os.path.join(ROOT, "tests", "cpp", "map_surfel_check.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    print(run.stdout)  # (with what the zero rule's coefficients stand on, measured again on the solve without the rule)
    assert "684 surfels clean" in run.stdout and "without the zero rule:" in run.stdout
