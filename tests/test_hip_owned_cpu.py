"""CPU test: the owning types of oat_amd/csrc/hip_owned.h (device block, pinned block, event) against a fake runtime --
tests/host/hip_owned_test.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers linked in."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_release_exactly_what_they_hold(tmp_path):
    exe = tmp_path / "hip_owned_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "host", "hip_owned_test.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
