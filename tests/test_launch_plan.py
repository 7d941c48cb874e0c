"""How a registration becomes launches is decided on the host alone (mad_icp_amd/csrc/common/launch_plan.h): the launch
geometry and route of every recorded case (tests/golden/launch_plan/cases.json, recorded from the code the header replaced),
the graph key, and the option table against the accepted ranges, stored values and messages of the if-chains it replaced
(tests/cpp/launch_plan_check.cpp).  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_matches_the_recorded_decisions(tmp_path):
    exe = str(tmp_path / "launch_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "mad_icp_amd", "csrc", "common"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "launch_plan_check.cpp"),
                           "-o", exe])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "launch_plan", "cases.json")], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "launch plan ok" in out.stdout
