"""leoec_read_dev's chunk seam at test-sized batches: the batch cut into chunks
of LEOEC_READ_CHUNK objects (measurement build).

The product chunk only keeps a launch's grid below 2^31 workgroups and holds
any batch a device can hold, so on a test-sized batch there is one chunk.  With
LEOEC_READ_CHUNK=2 the five objects take three chunks, the last of one object:
every chunk's objs, parity and out rows start at its own first object, and
every group of the range and every launch of survivors runs once per chunk.
Ranges, erased sets and expectations are test_device_read.py's, byte for byte,
for one family per kernel: gf_read in two launches, bit_read in one and in two.

The measure_gpu test needs the measurement build's knobs and runs in a process
of its own that loads libleoec_measure.so alone (LEOEC_LIBRARY=measure),
started by test_read_forms_in_own_process below; in the product tests' process
it skips (the `measure` fixture).
Run directly: LEOEC_LIBRARY=measure python -m pytest tests/test_read_forms.py -m measure_gpu
"""
import os
import subprocess
import sys

import pytest

import gpu_helpers as H
import read_helpers as R

FAMILIES = [("vandrs", 20, 4, 8, 8704), ("cauchyrs", 6, 3, 4, 4352 * 4), R.LIBERATION_WIDE]
CHUNKS = ("2", "1", None)


def test_families(le):
    assert all(f in R.FAMILIES for f in FAMILIES)
    assert R.N % 2 == 1  # the last chunk of two holds one object


@pytest.mark.gpu
@pytest.mark.measure_gpu
@pytest.mark.parametrize("family", FAMILIES, ids=R.family_id)
def test_read_chunks(gpu, le, oracle, family, measure):
    errors = []
    size = R.sizes(family)[0]
    case = H.edge_case(le, oracle, family[:4], size)
    rs = R.ranges(family, size, case.bs)
    for chunk in CHUNKS:
        measure.delenv("LEOEC_READ_CHUNK")
        if chunk:
            measure.setenv("LEOEC_READ_CHUNK", chunk)
        for off, length in (rs[0], rs[8], rs[11]):  # the object, across a block boundary, 3 1/2 blocks
            for name, erased in R.erased_sets(family, off, length, case.bs).items():
                errors += R.run_read(gpu, le, case, erased, off, length, name,
                                     knob=f"LEOEC_READ_CHUNK={chunk} ")
    assert not errors, "\n".join(e[:800] for e in errors[:8])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_read_forms_in_own_process(gpu, tmp_path):
    """The measure_gpu test of this file in a child process that loads
    libleoec_measure.so alone.  The child's output goes to read_forms.log in
    the test's temporary directory; a failure shows its tail."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "leo_erasure_amd", "libleoec_measure.so")):
        pytest.skip("measurement build absent (make -C leo_erasure_amd/csrc measure)")
    log = str(tmp_path / "read_forms.log")
    env = dict(os.environ, LEOEC_LIBRARY="measure", LIBC_FATAL_STDERR_="1")
    cmd = [sys.executable, "-u", "-m", "pytest", os.path.abspath(__file__),
           "-m", "measure_gpu", "-x", "-q", "-p", "no:cacheprovider",
           "--timeout", "120", "--timeout-method", "thread"]
    with open(log, "w") as fh:
        rc = subprocess.call(cmd, cwd=root, env=env, stdout=fh, stderr=subprocess.STDOUT,
                             timeout=280)
    with open(log) as fh:
        tail = fh.read()[-4000:]
    assert rc == 0, f"read form tests failed (rc {rc}), {log}:\n{tail}"
    summary = tail.strip().splitlines()[-1]
    assert "passed" in summary and "skipped" not in summary, summary
