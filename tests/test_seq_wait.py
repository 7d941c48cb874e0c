"""The host's wait for a sequence number that a kernel publishes is written down once (mad_icp_amd/csrc/common/seq_wait.h) and
checked here on the CPU with a scripted stream probe, a fake clock and a counting pause (tests/cpp/seq_wait_check.cpp): the
outcome of every branch — the number there, the stream drained without it, a stream error, the communicator's and the caller's
bound — and the exact number of probes, clock reads and pauses.  No GPU test may provoke a failed stream, a lost rank or a
timeout of work in flight, so these branches are held here alone.  Built a second time as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer; nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "seq_wait_check.cpp")
INC = "-I" + os.path.join(ROOT, "mad_icp_amd", "csrc", "common")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "seq wait ok: 75 cases" in out.stdout


def test_seq_wait_outcomes_and_poll_counts(tmp_path):
    exe = str(tmp_path / "seq_wait_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", INC, SRC, "-o", exe])
    _run(exe)


def test_seq_wait_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    trial = tmp_path / "trial.cpp"
    trial.write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx] + SAN + [str(trial), "-o", str(tmp_path / "trial")], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime does not link here: " + probe.stderr[-300:])
    exe = str(tmp_path / "seq_wait_check_san")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + SAN + [INC, SRC, "-o", exe], capture_output=True,
                           text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    _run(exe)
