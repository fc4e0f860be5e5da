"""leoec_heal_dev, form parity: the generic form (LEOEC_HEAL_FORM=1: masks
copied back, one plan launch per run of equal masks) on the configurations
gf8_heal serves must leave the arenas and the unhealed words the fused form
leaves, byte for byte.

The measure_gpu tests need the measurement build's knob and run in a process
of their own that loads libleoec_measure.so alone (LEOEC_LIBRARY=measure),
started by test_heal_forms_in_own_process below; in the product tests'
process they skip (the `measure` fixture).
Run directly: LEOEC_LIBRARY=measure python -m pytest tests/test_heal_forms.py -m measure_gpu
"""
import os
import subprocess
import sys

import pytest

import gpu_helpers as H
import heal_helpers as P


@pytest.mark.gpu
@pytest.mark.measure_gpu
@pytest.mark.parametrize("family", P.GF8_FAMILIES, ids=P.family_id)
def test_generic_form_matches_fused(gpu, le, oracle, family, measure):
    """run_heal compares every byte of both arenas and every unhealed word
    with the one expectation (the oracle's blocks), so two forms that both
    pass it left identical arenas."""
    cls, k, m, w, B = family
    em = P.edge_masks(k, m)
    runs = [em[1]] * 3 + em[:1] * 2 + [em[2]] * 2 + em[7:]  # runs of equal masks, as a scrub finds them
    errors = []
    for size in H.edge_sizes(k, w, B):
        case = H.edge_case(le, oracle, family[:4], size, n=P.EDGE_N)
        for form in (None, "1"):
            if form is None:
                measure.delenv("LEOEC_HEAL_FORM")
            else:
                measure.setenv("LEOEC_HEAL_FORM", form)
            for masks in (em, runs):
                errors += [f"LEOEC_HEAL_FORM={form}: {e}" for e in P.run_heal(gpu, le, case, masks)]
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_heal_forms_in_own_process(gpu, tmp_path):
    """The measure_gpu tests of this file in a child process that loads
    libleoec_measure.so alone (as test_verify_forms.py's
    test_verify_forms_in_own_process).  The child's output goes to
    heal_forms.log in the test's temporary directory; a failure shows its
    tail."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "leo_erasure_amd", "libleoec_measure.so")):
        pytest.skip("measurement build absent (make -C leo_erasure_amd/csrc measure)")
    log = str(tmp_path / "heal_forms.log")
    env = dict(os.environ, LEOEC_LIBRARY="measure", LIBC_FATAL_STDERR_="1")
    cmd = [sys.executable, "-u", "-m", "pytest", os.path.abspath(__file__),
           "-m", "measure_gpu", "-x", "-q", "-p", "no:cacheprovider",
           "--timeout", "120", "--timeout-method", "thread"]
    with open(log, "w") as fh:
        rc = subprocess.call(cmd, cwd=root, env=env, stdout=fh, stderr=subprocess.STDOUT,
                             timeout=280)
    with open(log) as fh:
        tail = fh.read()[-4000:]
    assert rc == 0, f"heal form tests failed (rc {rc}), {log}:\n{tail}"
    summary = tail.strip().splitlines()[-1]
    assert "passed" in summary and "skipped" not in summary, summary
