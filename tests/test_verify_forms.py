"""leoec_verify_dev, form parity: the two-pass form (LEOEC_VERIFY_FORM=1:
encode into a workspace, then compare) on the configurations gf8_check
serves must give the fused form's flags, word for word.

The measure_gpu tests need the measurement build's knob and run in a process
of their own that loads libleoec_measure.so alone (LEOEC_LIBRARY=measure),
started by test_verify_forms_in_own_process below; in the product tests'
process they skip (the `measure` fixture).
Run directly: LEOEC_LIBRARY=measure python -m pytest tests/test_verify_forms.py -m measure_gpu
"""
import os
import subprocess
import sys

import pytest

import gpu_helpers as H
import verify_helpers as V


@pytest.mark.gpu
@pytest.mark.measure_gpu
@pytest.mark.parametrize("family", V.GF8_FAMILIES, ids=V.family_id)
def test_two_pass_form_matches_fused(gpu, le, oracle, family, measure):
    cls, k, m, w, B = family
    errors = []
    for size in H.edge_sizes(k, w, B):
        case = H.edge_case(le, oracle, family[:4], size)
        measure.delenv("LEOEC_VERIFY_FORM")
        assert le.device.verify_workspace(cls, (k, m, w), size, case.n) == 0
        fused = [V.run_verify(gpu, le, case, V.damage(case, s)) for s in (False, True)]
        measure.setenv("LEOEC_VERIFY_FORM", "1")
        assert le.device.verify_workspace(cls, (k, m, w), size, case.n) == case.n * m * case.bs
        for s in (False, True):
            got, err = V.run_verify(gpu, le, case, V.damage(case, s))
            if err or fused[s][1]:
                errors.append(err or fused[s][1])
            if got != fused[s][0] or got != V.expected_flags(oracle, case, s):
                errors.append(f"{case.ident()} call {1 + s}: two-pass {[hex(x) for x in got]}, "
                              f"fused {[hex(x) for x in fused[s][0]]}")
        # one object per chunk
        ws = gpu.empty(m * case.bs, dtype=gpu.uint8, device="cuda")
        got, err = V.run_verify(gpu, le, case, V.damage(case, True), workspace=ws)
        if err or got != fused[True][0]:
            errors.append(err or f"{case.ident()} chunked: {[hex(x) for x in got]}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_verify_forms_in_own_process(gpu, tmp_path):
    """The measure_gpu tests of this file in a child process that loads
    libleoec_measure.so alone (as test_gpu_parity.py's
    test_measurement_forms_in_own_process does for test_measure_forms.py).
    The child's output goes to verify_forms.log in the test's temporary
    directory; a failure shows its tail."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "leo_erasure_amd", "libleoec_measure.so")):
        pytest.skip("measurement build absent (make -C leo_erasure_amd/csrc measure)")
    log = str(tmp_path / "verify_forms.log")
    env = dict(os.environ, LEOEC_LIBRARY="measure", LIBC_FATAL_STDERR_="1")
    cmd = [sys.executable, "-u", "-m", "pytest", os.path.abspath(__file__),
           "-m", "measure_gpu", "-x", "-q", "-p", "no:cacheprovider",
           "--timeout", "120", "--timeout-method", "thread"]
    with open(log, "w") as fh:
        rc = subprocess.call(cmd, cwd=root, env=env, stdout=fh, stderr=subprocess.STDOUT,
                             timeout=280)
    with open(log) as fh:
        tail = fh.read()[-4000:]
    assert rc == 0, f"verify form tests failed (rc {rc}), {log}:\n{tail}"
    summary = tail.strip().splitlines()[-1]
    assert "passed" in summary and "skipped" not in summary, summary
