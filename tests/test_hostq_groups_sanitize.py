"""Group-wise completion of the batching queue (hostq.cpp,
Knobs::hostq_done_groups) under AddressSanitizer + UndefinedBehaviorSanitizer
and under ThreadSanitizer, on the CPU: tests/host_sanitize/hostq_groups.cpp
(its own main) with the engine's host C++, the CPU stand-in for the HIP
runtime and the CPU kernels of that directory, built as an executable and run
as one.  32 threads, G = 4 in every waiting form, an injected failure of one
group's output copy, and no slot left busy: see the program's header."""
import os
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sanitize")
CSRC = os.path.join("..", "..", "leo_erasure_amd", "csrc")
ORACLE = os.path.join("..", "..", "oracle", "leoec_oracle.c")
SRCS = [os.path.join(CSRC, f) for f in ("engine.cpp", "hostq.cpp", "codes.cpp", "knobs.cpp", "capi.cpp")] + \
    ["fake_kernels.cpp", "tls_teardown.cpp", "hostq_groups.cpp"]
COMMON = ["-std=c++17", "-g", "-O1", "-pthread", "-I.", "-fno-omit-frame-pointer", "-DLEOEC_MEASURE",
          "-DLEOEC_HOSTQ_GROUP_MIN_OUT=65536", "-Wall", "-Wno-unused-function"]
SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
              "tsan": ["-fsanitize=thread"]}


def _build(kind):
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    obj = os.path.join(out, f"groups_oracle_{kind}.o")
    exe = os.path.join(out, f"groups_{kind}")
    flags = SANITIZERS[kind]
    for cmd in (["gcc", "-std=c11", "-g", "-O2", "-pthread", "-fPIC", flags[0], "-c", ORACLE, "-o", obj],
                ["g++"] + COMMON + flags + ["-o", exe] + SRCS + [obj, "-ldl"]):
        r = subprocess.run(cmd, cwd=HERE, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("kind", ["asan", "tsan"])
def test_hostq_groups_under_sanitizers(kind):
    exe = _build(kind)
    env = dict(os.environ,
               ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1:exitcode=66:second_deadlock_stack=1")
    r = subprocess.run([exe, "32", "6" if kind == "asan" else "4"], capture_output=True, text=True,
                       timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "hostq_groups: all checks held" in r.stdout
    assert "WARNING: ThreadSanitizer" not in out and "runtime error" not in out, out[-6000:]
