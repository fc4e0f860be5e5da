"""leoec_heal_ws_dev's persistent loop and chunk seam at test-sized batches:
the rebuild grid capped with LEOEC_SCRUB_GRID and the batch cut into chunks of
LEOEC_HEAL_WS_CHUNK objects (measurement build).

The product grid is min(objects x m x tiles, resident workgroups of the
device) and the product chunk holds any batch a device can hold: on a
test-sized batch every workgroup gets one item and there is one chunk
(test_device_heal_ws.py's batch of twice the grid aside).  With
LEOEC_SCRUB_GRID=1 one workgroup walks every item of the list; with 7 a
workgroup's successive items change object, mask, slot and tile.  With
LEOEC_HEAL_WS_CHUNK=2 the edge-mask batch of 9 objects takes five chunks: the
list and its count are rewritten per chunk, the indices are the chunk's own,
the totals add up across chunks, and the last chunk holds one object.  The
batches and expectations are test_device_heal_ws.py's edge masks, byte for
byte, for one family per rebuild kernel and width.

The measure_gpu tests need the measurement build's knobs and run in a process
of their own that loads libleoec_measure.so alone (LEOEC_LIBRARY=measure),
started by test_heal_ws_forms_in_own_process below; in the product tests'
process they skip (the `measure` fixture).
Run directly: LEOEC_LIBRARY=measure python -m pytest tests/test_heal_ws_forms.py -m measure_gpu
"""
import os
import subprocess
import sys

import pytest

import gpu_helpers as H
import heal_helpers as HH
import heal_ws_helpers as X

FAMILIES = [("vandrs", 10, 4, 8, 8704), ("vandrs", 20, 4, 8, 8704), ("vandrs", 10, 4, 16, 8704),
            ("vandrs", 6, 3, 32, 8704), ("cauchyrs", 6, 3, 4, 4352 * 4), ("liberation", 4, 2, 7, 2176 * 7)]
FORMS = (("LEOEC_SCRUB_GRID", "1"), ("LEOEC_SCRUB_GRID", "7"), ("LEOEC_HEAL_WS_CHUNK", "2"), (None, None))


def test_families(le):
    assert all(f in HH.FAMILIES for f in FAMILIES)
    assert HH.EDGE_N % 2 == 1  # the last chunk of two holds one object


@pytest.mark.gpu
@pytest.mark.measure_gpu
@pytest.mark.parametrize("family", FAMILIES, ids=HH.family_id)
def test_heal_ws_forms(gpu, le, oracle, family, measure):
    cls, k, m, w, B = family
    masks = HH.edge_masks(k, m)
    errors = []
    for knob, value in FORMS:
        measure.delenv("LEOEC_SCRUB_GRID")
        measure.delenv("LEOEC_HEAL_WS_CHUNK")
        if knob:
            measure.setenv(knob, value)
        for size in X.sizes(family):
            case = H.edge_case(le, oracle, family[:4], size, n=HH.EDGE_N)
            errors += [f"{knob}={value}: {e}" for e in X.run_heal_ws(gpu, le, case, masks)]
            errors += [f"{knob}={value} reversed: {e}"
                       for e in X.run_heal_ws(gpu, le, case, list(reversed(masks)))]
    assert not errors, "\n".join(e[:1500] for e in errors[:12])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_heal_ws_forms_in_own_process(gpu, tmp_path):
    """The measure_gpu tests of this file in a child process that loads
    libleoec_measure.so alone (as test_scrub_gfw_forms.py's).  The child's
    output goes to heal_ws_forms.log in the test's temporary directory; a
    failure shows its tail."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "leo_erasure_amd", "libleoec_measure.so")):
        pytest.skip("measurement build absent (make -C leo_erasure_amd/csrc measure)")
    log = str(tmp_path / "heal_ws_forms.log")
    env = dict(os.environ, LEOEC_LIBRARY="measure", LIBC_FATAL_STDERR_="1")
    cmd = [sys.executable, "-u", "-m", "pytest", os.path.abspath(__file__),
           "-m", "measure_gpu", "-x", "-q", "-p", "no:cacheprovider",
           "--timeout", "120", "--timeout-method", "thread"]
    with open(log, "w") as fh:
        rc = subprocess.call(cmd, cwd=root, env=env, stdout=fh, stderr=subprocess.STDOUT,
                             timeout=280)
    with open(log) as fh:
        tail = fh.read()[-4000:]
    assert rc == 0, f"heal_ws form tests failed (rc {rc}), {log}:\n{tail}"
    summary = tail.strip().splitlines()[-1]
    assert "passed" in summary and "skipped" not in summary, summary
