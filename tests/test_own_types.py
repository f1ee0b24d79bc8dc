"""The owning types the device context is made of (csrc/gpsiq_own.h: DevBuf, PinnedBuf, Event, Stream), the one rule its groups of
buffers grow by (reserve_together, ibid.) and the first-use routines built from them: the carrier chain's and the device
evaluation's (csrc/gpsiq_ctx.h), those of the four stream stages (csrc/gpsiq_despread.h, gpsiq_pack.h, gpsiq_acquire.h,
gpsiq_follow.h) and that of the staged batch calls' staging ring (csrc/gpsiq_stage_batch.h), on the CPU.  tests/own_types.cpp defines the HIP entry points the headers call as counting fakes over malloc /
free, each with a "fail the k-th call" switch, and is built with the address and undefined-behaviour sanitizers; no HIP runtime is
linked.  It checks that a reserve at or below the capacity makes no call, that growing is one free and one allocation of exactly
the count given, that a failed allocation or a failed free leaves the buffer empty, reported and usable again, that ensure() is
idempotent, that a group grows only when its smallest member lacks room and then in the order given, that every first-use set --
chain, device evaluation, repair, despread, pack, the piece ring, acquire, follow -- completes on the attempt after a failure at any one of its
resources, that a grow step which failed at any member is completed by a later, smaller request, that every stage set ends at the
sizes its site's slack gives, and that nothing is ever released twice or left alive."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")


def test_owning_types_and_first_use_sets(tmp_path):
    exe = str(tmp_path / "own_types")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "own_types.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr       # both sanitizers are silent
    assert run.stdout.splitlines()[-1] == "own types ok"
