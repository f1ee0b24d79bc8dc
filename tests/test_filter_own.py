"""FirSet::reserve (csrc/gpsiq_filter.h), the first-use routine of the filter stage's member of the device context, and
PieceRing::reserve (csrc/gpsiq_stage_batch.h), that of the staging ring its batch call works through its pieces with, on the CPU:
tests/filter_own.cpp defines the HIP entry points csrc/gpsiq_own.h calls as counting fakes over malloc / free and is built with the
address and undefined-behaviour sanitizers; no HIP runtime is linked.  It checks that gpsiq_filter's share is six resources, neither a
stream nor a staging buffer among them, that what the batch call reserves (ring and set) completes on the attempt after a failure at any one of its sixteen resources
with nothing made twice, that a grow step of the staging pairs which failed at any member is completed by a later, smaller request,
and that nothing is released twice or left alive."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")


def test_filter_set_first_use_and_growth(tmp_path):
    exe = str(tmp_path / "filter_own")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "filter_own.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr       # both sanitizers are silent
    assert run.stdout.splitlines()[-1] == "filter own ok"
