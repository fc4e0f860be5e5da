"""The engine's host C++ (plan cache, per-thread staging, batching queue,
dispatcher lanes, knob setter) under AddressSanitizer + UndefinedBehavior-
Sanitizer and ThreadSanitizer, on the CPU: tests/host_sanitize builds
engine.cpp / hostq.cpp / capi.cpp / codes.cpp / knobs.cpp with g++ against a
CPU stand-in for the HIP runtime (asynchronous in-order streams with random
delays, events, pinned vs pageable copies, two devices) and CPU kernels, and
host_stress.cpp drives the C ABI from many threads, comparing every result
with the oracle.  The stand-in models HIP's per-thread sticky last-error slot
and injects allocation failures: every call must leave the slot clean, also
after a failure the engine recovered from (host_stress.cpp phase 2c).  Round
3's verdict asked for this in place of re-running the GPU suite to reproduce
round 2's silent host-side abort ("The round-2 abort")."""
import os
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sanitize")


@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-s", "-j4", "-C", HERE], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return os.path.join(HERE, "_build")


@pytest.mark.parametrize("binary,threads,rounds", [
    ("stress_asan", 16, 8), ("stress_asan_measure", 16, 8),
    ("stress_tsan", 12, 4), ("stress_tsan_measure", 12, 4)])
def test_host_side_under_sanitizers(built, binary, threads, rounds):
    env = dict(os.environ,
               ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1:exitcode=66:second_deadlock_stack=1")
    r = subprocess.run([os.path.join(built, binary), str(threads), str(rounds)],
                       capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "host_stress: all results bit-exact" in r.stdout
    assert "recovered HIP failures: ok" in r.stdout  # phase 2c ran (injected allocation failures)
    assert "WARNING: ThreadSanitizer" not in out and "runtime error" not in out, out[-6000:]
