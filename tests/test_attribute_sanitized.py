"""The host twins of the per-point attribute under AddressSanitizer + UndefinedBehaviorSanitizer: tests/cpp/attribute_check.cpp — a
stand-alone program with its own main that links csrc/host/ingest_records.cpp, cloud_export.cpp and voxel_map.cpp directly — is
compiled here and run.  Every record buffer holds exactly n * step bytes and every output buffer exactly the rows asked for, so an
attribute field read past the last record or a word written past the last row is reported.  Nothing is loaded into Python; skipped
where the sanitizer runtime does not link."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_attribute_twins_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    trial = tmp_path / "trial.cpp"
    trial.write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx] + SAN + [str(trial), "-o", str(tmp_path / "trial")], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime does not link here: " + probe.stderr[-300:])
    exe = tmp_path / "attribute_check"
    csrc = os.path.join(ROOT, "mad_icp_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra"] + SAN + [
        "-I" + os.path.join(csrc, "host"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "attribute_check.cpp")] + [
        os.path.join(csrc, "host", f) for f in ("ingest_records.cpp", "cloud_export.cpp", "voxel_map.cpp")] + ["-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "89 sets clean" in run.stdout
